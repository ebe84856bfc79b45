"""zipc_amd/csrc/packed_layout.h -- the rules of the packed decode forms (zipc_hip_inflate_packed_batch), one header for the
kernels of packed.hip, their launcher and this test -- compiled with g++ into a host model (tests/packed_sim/sim_packed.cpp)
that runs the layout kernel's tiles and waves as loops and checks every index before it is used.  The expected values are
the few lines of `expect` below, not the header; a mutation table over the header.  No GPU; the kernels are checked in
tests/test_gpu_inflate_packed.py."""
import ctypes as C
import os

import numpy as np
import pytest

import mutation
import util  # noqa: F401  (sets sys.path through conftest)

HERE = os.path.dirname(os.path.abspath(__file__))
SIM = os.path.join(HERE, "packed_sim", "sim_packed.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "zipc_amd", "csrc")
HEADER = os.path.join(CSRC, "packed_layout.h")
DESC = np.dtype([("src_off", "<u8"), ("src_len", "<u8"), ("dst_off", "<u8"), ("dst_cap", "<u8"), ("limit", "<u8"), ("flags", "<u4"),
                 ("reserved", "<u4")])
RESULT = np.dtype([("status", "<u4"), ("checksum", "<u4"), ("out_len", "<u8")])
VERDICT = np.dtype([("status", "<u4"), ("roomed", "<u4"), ("dst_off", "<u8")])
PACKED = np.dtype([("status", "<u4"), ("checksum", "<u4"), ("out_len", "<u8"), ("dst_off", "<u8"), ("reserved", "<u8")])
OK, CORRUPTED, SIZE_EXCEEDED, DST_TOO_SMALL, INVALID_ARG = 0, 1, 2, 16, 18
MAX_STREAM_LEN = 0xFFFF0000
ALIGNS = (1, 2, 16, 4096)


FLAGS = dict(include=[CSRC], extra=["-Wall", "-Wno-unknown-pragmas"])


def _bind(so):
    L = C.CDLL(so)
    L.sim_packed_run.restype = C.c_uint64
    L.sim_packed_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p]
    L.sim_packed_call_status.restype = C.c_uint32
    L.sim_packed_call_status.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int]
    L.sim_packed_size_form.restype = C.c_int
    L.sim_packed_size_form.argtypes = [C.c_uint64]
    L.sim_packed_tile.restype = L.sim_packed_wave.restype = C.c_uint32
    return L


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return _bind(mutation.gxx(tmp_path_factory.mktemp("packed_sim") / "libpacked_sim.so", [SIM], **FLAGS))


def _descs(n):
    d = np.zeros(n, DESC)
    d["src_off"] = np.arange(n, dtype=np.uint64) * 100
    d["src_len"] = 50 + np.arange(n, dtype=np.uint64) % 7
    d["dst_off"], d["dst_cap"] = 0xDEAD, 0xBEEF  # (not to be looked at)
    d["limit"] = np.arange(n, dtype=np.uint64) % 3 * 1000
    d["flags"] = np.arange(n, dtype=np.uint32) % 3 != 0
    return d


def _would_decode(sized):
    """what the stub's inflate says of a stream that reaches it: OK with the size and a checksum of its own; every 5th a failure
    of the decoder's own (the close hands it on as it is)"""
    w = np.zeros(len(sized), RESULT)
    for i, (_, ol) in enumerate(sized):
        w[i] = (CORRUPTED, 0, 0) if i % 5 == 4 else (OK, 0x1000 + i, ol)
    return w


def run(L, sized, max_out_len, align, arena_len):
    """-> (verdicts, inner descriptors, results, need, stats)"""
    n = len(sized)
    m = max(n, 1)
    descs = _descs(m)
    s = np.zeros(m, RESULT)
    for i, (st, ol) in enumerate(sized):
        s[i] = (st, 0, ol)
    would = _would_decode(sized) if n else np.zeros(1, RESULT)
    verdicts, inner, results = np.full(m, 0xEE, "u1").repeat(16).view(VERDICT), np.zeros(m, DESC), np.zeros(m, PACKED)
    need, stats = np.full(1, 0xEEEE, np.uint64), np.zeros(3, np.uint64)
    L.sim_packed_run(descs.ctypes.data, s.ctypes.data, would.ctypes.data, n, max_out_len, align, arena_len, verdicts.ctypes.data,
                     inner.ctypes.data, results.ctypes.data, need.ctypes.data, stats.ctypes.data)
    return verdicts[:n], inner[:n], results[:n], int(need[0]), tuple(int(v) for v in stats)


def expect(sized, max_out_len, align, arena_len):
    """the rule of include/zipc_hip.h, serially: per stream (status, roomed, dst_off), and need"""
    off = need = 0
    out = []
    for st, ol in sized:
        if st == OK and ol <= max_out_len:
            out.append((OK if off + ol <= arena_len else DST_TOO_SMALL, 1, off))
            need = off + ol
            off += (ol + align - 1) // align * align
        else:
            out.append((st if st != OK else INVALID_ARG, 0, 0))
    return out, need


def _pattern(n, seed, bad_every=7):
    """n tiny streams: sizes 0..40 in a fixed pseudo-random pattern, every bad_every-th corrupted"""
    x, out = seed, []
    for i in range(n):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out.append((CORRUPTED, 0) if i % bad_every == bad_every - 1 else (OK, (x >> 8) % 41))
    return out


HAND = [(OK, 10), (CORRUPTED, 0), (OK, 33), (SIZE_EXCEEDED, 0), (DST_TOO_SMALL, 0), (INVALID_ARG, 0), (OK, 0), (OK, 300), (OK, 7),
        (CORRUPTED, 9), (OK, 256), (OK, 0), (OK, 5), (OK, 257), (SIZE_EXCEEDED, 40)]  # max_out_len 256: 300 and 257 are above it
# (name, sized, max_out_len, arena lengths beside `need`, `need - 1` and 0)
CASES = [
    ("hand-made verdicts", HAND, 256, (10 ** 6,)),
    ("nothing takes room", [(CORRUPTED, 0), (OK, 9), (INVALID_ARG, 3)], 8, (100,)),
    ("zero-length streams at the end", [(OK, 10), (OK, 20), (OK, 0), (OK, 0)], 64, (29, 30, 31)),
    ("zero-length streams behind one that did not fit, a good one in front", [(OK, 4096), (OK, 1), (OK, 0), (OK, 0), (CORRUPTED, 0)], 4096, (4096,)),
    ("the last streams take no room", [(OK, 3), (OK, 5), (CORRUPTED, 0), (OK, 99), (SIZE_EXCEEDED, 0)], 50, (8, 7)),
    ("sums beyond 2^32", [(OK, MAX_STREAM_LEN)] * 3 + [(OK, 1), (OK, MAX_STREAM_LEN + 1)], MAX_STREAM_LEN, (3 * MAX_STREAM_LEN, 1 << 40)),
    ("one stream", [(OK, 17)], 17, (17,)),
    ("no stream", [], 10, (5,)),
] + [("n = %d" % n, _pattern(n, n), 40, ()) for n in (63, 64, 65, 1023, 1024, 1025, 2048, 2049, 3100)] + [
    ("a wave and a tile of streams without room at the end", _pattern(70, 3) + [(CORRUPTED, 0)] * 1100 + [(OK, 50)] * 3, 40, ()),
]


def _arenas(sized, max_out_len, align, extra):
    need = expect(sized, max_out_len, align, 0)[1]
    return [a for a in dict.fromkeys((need, need - 1, 0) + tuple(extra)) if a >= 0]


def test_constants(sim):
    assert (sim.sim_packed_tile(), sim.sim_packed_wave()) == (1024, 64)
    # sizing by one wave below the capacity from which inflate_batch enters its block path, by blocks from there on
    assert sim.sim_packed_size_form(0) == 0 and sim.sim_packed_size_form((256 << 10) - 1) == 0
    assert sim.sim_packed_size_form(256 << 10) == 1 and sim.sim_packed_size_form(MAX_STREAM_LEN) == 1


def test_call_rules(sim):
    ok = dict(dst_null=0, arena=100, n=5, max_out=1000, align=16, crc_op=0)

    def st(**kw):
        a = dict(ok, **kw)
        return sim.sim_packed_call_status(a["dst_null"], a["arena"], a["n"], a["max_out"], a["align"], a["crc_op"])

    assert st() == OK
    assert st(dst_null=1) == INVALID_ARG and st(dst_null=1, arena=0) == OK
    assert st(n=0x7FFFFFFF) == OK and st(n=0x80000000) == INVALID_ARG
    for a in range(0, 8200):
        assert st(align=a) == (OK if a in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096) else INVALID_ARG), a
    assert st(align=1 << 13) == INVALID_ARG and st(align=1 << 63) == INVALID_ARG
    assert st(max_out=MAX_STREAM_LEN) == OK and st(max_out=MAX_STREAM_LEN + 1) == INVALID_ARG
    assert [st(crc_op=c) for c in (-1, 0, 1, 2, 3, 4)] == [INVALID_ARG, OK, OK, OK, OK, INVALID_ARG]


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_model_follows_the_rule(sim, name):
    """every case, every align, the arena exactly `need`, one byte short, empty and more: verdicts, `need`, the descriptors
    inflate ran with and the results are the rule's; no index left its array and no stream reached inflate with room outside
    the arena"""
    _, sized, max_out_len, extra = next(c for c in CASES if c[0] == name)
    descs, would = _descs(max(len(sized), 1)), _would_decode(sized)
    for align in ALIGNS:
        needs = set()
        for arena in _arenas(sized, max_out_len, align, extra):
            want, need = expect(sized, max_out_len, align, arena)
            v, inner, res, got_need, stats = run(sim, sized, max_out_len, align, arena)
            what = (name, align, arena)
            if not sized:
                assert stats == (0, 0, 0) and got_need == 0
                continue
            assert got_need == need, what
            needs.add(got_need)
            assert stats[0] == 0 and stats[1] == (len(sized) + 1023) // 1024, what
            assert stats[2] == sum(w[0] == OK for w in want), what
            for i, (st, roomed, off) in enumerate(want):
                assert (int(v["status"][i]), int(v["roomed"][i]), int(v["dst_off"][i])) == (st, roomed, off), (what, i)
                if roomed:
                    assert off % align == 0, (what, i)
                d, r = inner[i], res[i]
                if st == OK:
                    assert (int(d["src_off"]), int(d["src_len"]), int(d["dst_off"]), int(d["dst_cap"]), int(d["limit"]), int(d["flags"])) == \
                        (int(descs["src_off"][i]), int(descs["src_len"][i]), off, sized[i][1], int(descs["limit"][i]), int(descs["flags"][i])), (what, i)
                    assert (int(r["status"]), int(r["checksum"]), int(r["out_len"]), int(r["dst_off"]), int(r["reserved"])) == \
                        (int(would["status"][i]), int(would["checksum"][i]), int(would["out_len"][i]), off, 0), (what, i)
                else:
                    assert (int(d["src_len"]), int(d["dst_cap"]), int(d["flags"])) == (0, 0, 0), (what, i)
                    assert (int(r["status"]), int(r["checksum"]), int(r["out_len"]), int(r["dst_off"]), int(r["reserved"])) == (st, 0, 0, off, 0), (what, i)
        assert len(needs) <= 1, (name, align, "need depends on the arena")


def test_what_the_cases_hold():
    """the cases meet what they are named for"""
    want, need = expect(HAND, 256, 16, 10 ** 6)
    assert {w[0] for w in want} == {OK, CORRUPTED, SIZE_EXCEEDED, DST_TOO_SMALL, INVALID_ARG}
    sized = dict((c[0], c[1]) for c in CASES)["zero-length streams at the end"]
    assert [w[0] for w in expect(sized, 64, 1, 30)[0]] == [OK] * 4                                  # ends exactly at dst_arena_len
    assert [w[0] for w in expect(sized, 64, 1, 29)[0]] == [OK, DST_TOO_SMALL, DST_TOO_SMALL, DST_TOO_SMALL]  # one byte past it
    assert [w[2] for w in expect(sized, 64, 1, 29)[0]] == [0, 10, 30, 30]
    big = dict((c[0], c[1]) for c in CASES)["sums beyond 2^32"]
    want, need = expect(big, MAX_STREAM_LEN, 1, 1 << 40)
    assert want[3] == (OK, 1, 3 * MAX_STREAM_LEN) and need == 3 * MAX_STREAM_LEN + 1 > 1 << 33 and want[4][0] == INVALID_ARG


# ---- the mutation table: (name, the line as it stands, the line mutated) ---------------------------------------------
MUTANTS = (
    ("align_up off by one", "return (len + align - 1) & ~(align - 1);", "return (len + align) & ~(align - 1);"),
    ("padding the offset instead of the length", "return packed_add(off, packed_align_up(len, align)); }",
     "return packed_add(packed_align_up(off, align), len); }"),
    ("fit by < instead of <=", "return packed_add(off, len) <= dst_arena_len; }", "return packed_add(off, len) < dst_arena_len; }"),
    ("a non-OK stream taking room", "{ return sized.status == ST_OK && sized.out_len <= max_out_len; }", "{ return sized.out_len <= max_out_len; }"),
    ("a stream above max_out_len taking room", "{ return sized.status == ST_OK && sized.out_len <= max_out_len; }", "{ return sized.status == ST_OK; }"),
    ("the carried base dropped at a tile boundary", "{ return packed_add(carried, tile_total); }", "{ return tile_total; }"),
    ("d_need taken from the last stream instead of the last roomed one", "{ return roomed ? packed_add(off, len) : 0; }", "{ return packed_add(off, len); }"),
    ("32-bit sums", "ZD_HD uint64_t packed_add(uint64_t a, uint64_t b) { return a + b; }",
     "ZD_HD uint64_t packed_add(uint64_t a, uint64_t b) { return (uint32_t)(a + b); }"),
    ("the scan's upper half taken a bit low", "{ return (uint32_t)(room >> 16); }", "{ return (uint32_t)(room >> 15); }"),
    ("a stream that does not fit handed to inflate", "if (v.roomed && !packed_fits(off, sized.out_len, dst_arena_len)) v.status = ST_DST_TOO_SMALL;", ""),
    ("a stream that does not fit forgets its offset", "v.dst_off = v.roomed ? off : 0;", "v.dst_off = v.roomed && packed_fits(off, sized.out_len, dst_arena_len) ? off : 0;"),
    ("a size above max_out_len reported as OK", "return sized.out_len > max_out_len ? (uint32_t)ST_INVALID_ARG : (uint32_t)ST_OK;", "return (uint32_t)ST_OK;"),
    ("need joined by the smaller end", "{ return a > b ? a : b; }", "{ return a < b ? a : b; }"),
    ("room as large as the call allows, not the stream's size", "in.dst_cap = out_len;", "in.dst_cap = out_len + 1;"),
    ("the close drops the decoder's checksum", "r.checksum = decoded.checksum;", "r.checksum = 0;"),
)


def _observe(L):
    """everything the model says about every case at every align with the arena exactly need, one byte short and empty"""
    out = []
    for name, sized, max_out_len, extra in CASES:
        for align in ALIGNS:
            for arena in _arenas(sized, max_out_len, align, extra):
                v, inner, res, need, stats = run(L, sized, max_out_len, align, arena)
                out.append((name, align, arena, v.tobytes(), inner.tobytes(), res.tobytes(), need, stats))
    return out


def test_mutants_of_the_header_are_killed(sim, tmp_path):
    """each one-line mutant of packed_layout.h, built into a model of its own, changes what the model says of at least one
    case (a verdict, a descriptor, a result, need, or room handed to inflate outside the arena, which the model counts)"""
    base = _observe(sim)
    assert all(row[7][0] == 0 for row in base)
    alive = []
    for k, (name, line, mutated) in enumerate(MUTANTS):
        so = mutation.header_model(SIM, "PACKED_HEADER", HEADER, line, mutated, str(tmp_path / ("mutant%d" % k) / "libmutant.so"), **FLAGS)
        if _observe(_bind(so)) == base:
            alive.append(name)
    assert alive == []
