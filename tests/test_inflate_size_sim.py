"""The sizing mode of the one inflate decoder (IM_SIZE: zipc_amd/csrc/inflate_lane.h, inflate_span.h) and the close rule
of zipc_hip_zlib_size_batch (zlib_container.h zlib_close_size), compiled with g++ (tests/size_sim/sim_size.cpp) and held
against the oracle: a stream's status and decompressed size from a walk that stores nothing.  No GPU; the kernel that
runs the mode is checked in tests/test_gpu_inflate_size.py."""
import collections
import ctypes as C
import os
import sys

import pytest

import mutation
import size_cases
import util
from host_sim import HERE as HOST_SIM_DIR, lib as host_sim_lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, util.GOLDEN)
import inflate_rules  # noqa: E402

POISON = 0xEE
ROOM = 1 << 20  # a destination no case needs more than: every rule case writes less, the golden streams too
# the forms the sim has: (span, budget) -- the plain step alone at two budgets of turns between refills of the input ring,
# the span decoder with the emulated wave's lanes resumed in ascending and in descending order
FORMS = {"plain-512": (0, 512), "plain-7": (0, 7), "span-a": (1, 24), "span-d": (2, 24)}


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    L = C.CDLL(mutation.gxx(tmp_path_factory.mktemp("size_sim") / "libsize_sim.so", [os.path.join(HERE, "size_sim", "sim_size.cpp")],
                            include=[HOST_SIM_DIR], extra=["-Wall", "-Wno-unknown-pragmas"]))
    L.sim_size.restype = C.c_int
    L.sim_size.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, C.c_uint32, C.c_int,
                           C.c_int, C.POINTER(C.c_uint64)]
    L.sim_zlib_close_size.restype = None
    L.sim_zlib_close_size.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_ulonglong, C.POINTER(C.c_ulonglong)]
    L.sim_zlib_open_status.restype = C.c_uint
    L.sim_zlib_open_status.argtypes = [C.c_ulonglong, C.c_uint, C.c_uint]
    return L


@pytest.fixture(scope="module")
def inflate_sim():
    return host_sim_lib()


class Dest:
    """the poisoned buffer handed to the sim as its destination; `untouched` after every call"""

    def __init__(self, n=ROOM + 64):
        self.image = bytes([POISON]) * n
        self.buf = C.create_string_buffer(self.image, n)

    def untouched(self):
        return self.buf.raw == self.image


def size(sim, dest, stream, limit=None, form="plain-512", dst_off=0, dst_cap=0, flags_extra=0):
    span, budget = FORMS[form]
    ol = C.c_uint64(0xEEEEEEEE)
    st = sim.sim_size(stream, len(stream), dest.buf, dst_off, dst_cap, int(limit is not None), limit or 0, flags_extra, span, budget,
                      C.byref(ol))
    return st, ol.value


def test_the_rule_table_is_the_one_these_tests_were_written_for():
    """486 cases, 413 short ones and 73 inside streams of 600 KB and more.  By status the table holds 151 accepted,
    304 CORRUPTED and 31 SIZE_EXCEEDED cases, the last always with a limit; 11 of the accepted ones have a limit.  (The
    issue behind these tests gave 196 / 250 / 40 and 10 for that split; the table as it stands counts as asserted here,
    and every test below runs all 486 whatever their split.)"""
    cases = inflate_rules.wrapped_cases()
    assert len(cases) == 486
    assert sum(not n.endswith("/e") for n in cases) == 413 and sum(n.endswith("/e") for n in cases) == 73
    assert all(len(c.plain) >= 600000 for n, c in cases.items() if n.endswith("/e") and c.status == 0)
    by = collections.Counter(c.status for c in cases.values())
    assert (by[0], by[1], by[2]) == (151, 304, 31) and sum(by.values()) == 486
    assert all(c.limit is not None for c in cases.values() if c.status == 2)
    assert sum(c.status == 0 and c.limit is not None for c in cases.values()) == 11


@pytest.mark.parametrize("form", ["plain-512", "plain-7", "span-a"])
def test_rule_cases_size_as_the_oracle_says(sim, oracle, form):
    """all 486 cases of tests/golden/inflate_rules.py, each with its own limit or none: the oracle holds the case
    (size_cases.rule_cases), and the mode's (status, out_len) is (the case's status, the length of its bytes when
    accepted); the destination stays as it was.  No case is left out: every form runs every one -- the plain step at two
    budgets, and the span decoder."""
    dest = Dest()
    cases = size_cases.rule_cases()
    for c in cases:
        got = size(sim, dest, c.stream, c.limit, form)
        assert got == c.want, (form, c.name, got, c.want)
    assert len(cases) == 486 and dest.untouched()
    if form.startswith("span"):  # (the long cases went through the span decoder, not round it)
        spans = (C.c_uint64 * 2).in_dll(sim, "sim_size_spans")
        assert spans[0] > 73 and spans[1] > 73 * 300000, list(spans)


def test_the_descriptors_destination_is_not_looked_at(sim, oracle):
    """dst_off and dst_cap of the descriptor are ignored, whatever they hold; a flag bit other than HAS_LIMIT and a
    src_len above the limit are the stream's own INVALID_ARG; an empty source is what the oracle says of it"""
    dest = Dest()
    data = util.text(5000, 3)
    s = oracle.deflate(data, level=2)[1]
    for dst_off, dst_cap in ((0, 0), (1 << 63, 1 << 40), (12345, 7), (0, 0xFFFF0001)):
        for form in FORMS:
            assert size(sim, dest, s, None, form, dst_off, dst_cap) == (0, len(data))
            assert size(sim, dest, s, len(data) - 1, form, dst_off, dst_cap) == (2, 0)
    for bit in (2, 1 << 31):
        assert size(sim, dest, s, None, flags_extra=bit) == (18, 0)
        assert size(sim, dest, s, len(data), flags_extra=bit) == (18, 0)
    ol = C.c_uint64()
    assert sim.sim_size(s, 0xFFFF0001, dest.buf, 0, 0, 0, 0, 0, 0, 512, C.byref(ol)) == 18 and ol.value == 0  # (nothing is read of it)
    st0, d0, _ = oracle.inflate(b"")
    assert size(sim, dest, b"") == (st0, len(d0) if st0 == 0 else 0) and st0 == 1
    assert dest.untouched()


def _inflate_model(inflate_sim, stream, limit, cap=ROOM):
    dst = C.create_string_buffer(cap + 64)
    ol, ck = C.c_uint64(), C.c_uint32()
    st = inflate_sim.sim_inflate(stream, len(stream), dst, cap, int(limit is not None), limit or 0, 0, C.byref(ol), C.byref(ck), 512)
    assert st != 16, "the buffer was to be large enough"
    return st, ol.value


def test_the_mode_equals_the_decoding_mode(sim, inflate_sim, monkeypatch):
    """Two modes of one decoder, compared with each other on purpose: on the golden streams (with no limit, the exact
    one, one more and one less) and on the header fuzz of test_inflate_models_header_fuzz, the sizing mode's
    (status, out_len) is the decoding model's, which gets a buffer large enough and the same limit."""
    monkeypatch.delenv("SIM_INFLATE_WIDE", raising=False)
    monkeypatch.delenv("SIM_INFLATE_SPAN", raising=False)
    dest = Dest()
    seen = collections.Counter()
    for s in util.zlib_streams():
        n = s["plain_len"]
        assert n <= ROOM
        for limit in (None, n, n + 1, max(0, n - 1)):
            want = _inflate_model(inflate_sim, s["raw"], limit)
            for form in ("plain-512", "span-a", "span-d"):
                assert size(sim, dest, s["raw"], limit, form) == want, (s["name"], limit, form)
            seen[want[0]] += 1
    assert seen[0] > 0 and seen[2] > 0
    fuzz = collections.Counter()
    for k, s in enumerate(util.header_fuzz_streams(78, 150, 450)):
        for limit in (1 << 16, None):
            want = _inflate_model(inflate_sim, s, limit)
            for form in ("plain-7", "span-a"):
                assert size(sim, dest, s, limit, form) == want, (k, limit, form)
            fuzz[want[0]] += 1
    assert fuzz[0] > 20 and fuzz[1] > 20, fuzz
    assert dest.untouched()


def test_zlib_close_rule(sim, oracle):
    """zlib_close_size over zlib_cases.decompress_cases(): the container's verdict (zlib_open_status, or INVALID_ARG for
    a stray flag bit, as zlib_open_kernel says) over the sizing mode's verdict of the body -- of nothing, for a stream
    that failed its check, as zlib.hip's zlib_no_stream hands it over -- against size_cases.expect_zlib_size (the oracle)."""
    dest = Dest()
    out = (C.c_ulonglong * 3)()
    for c, want, _ in size_cases.zlib_expectations():
        z = c.stream
        if c.flags:
            pre = 18
        else:
            pre = sim.sim_zlib_open_status(len(z), z[0] if len(z) >= 6 else 0, z[1] if len(z) >= 6 else 0)
        if pre == 0:
            inner = size(sim, dest, z[2:len(z) - 2], c.limit, "span-a", dst_cap=c.cap)
        else:
            inner = size(sim, dest, b"", None)
        sim.sim_zlib_close_size(pre, inner[0], 0xABCD, inner[1], out)
        assert (out[0], out[2]) == want and out[1] == 0, (c.name, tuple(out), want)
    assert dest.untouched()
    # the rule itself: the check's verdict first, the checksum always 0, nothing compared
    for pre in (1, 3, 4, 5, 18):
        sim.sim_zlib_close_size(pre, 0, 7, 99, out)
        assert tuple(out) == (pre, 0, 0)
    sim.sim_zlib_close_size(0, 0, 7, 99, out)
    assert tuple(out) == (0, 0, 99)
    sim.sim_zlib_close_size(0, 2, 7, 0, out)
    assert tuple(out) == (2, 0, 0)
