"""The gzip forms on the CPU (include/zipc_hip.h at zipc_hip_gzip_decompress_batch): RFC 1952's container around the extent
decoder.  The host model is tests/gzip_sim/sim_gzip.cpp -- gzip_container.h's rules (the text the kernels and the host forms
compile) around inflate_lane.h's plain lane step run serially.  What is expected comes from the catalogue
(tests/gzip_cases.py): the header's verdict from a second writing of RFC 1952 in Python, the body from the oracle, extent and
CRC-32 from Python's zlib, and zlib's own verdict of every whole member beside it.  This file holds

  - the catalogue against zlib (wbits=31) and the coverage it claims;
  - the model in the decode and size forms at two budgets of turns, guard bytes around every room, src_used <= src_len;
  - compress: header + the oracle's deflate + trailer, read back by Python's gzip and zlib; the header against Python's gzip;
    BGZF's BSIZE;
  - gzip_next over the files: members, runs, end of members, the lying BSIZE;
  - GZIP_MUTANTS, each built into a model of its own and run in a child process: no survivor;
  - the model as a stand-alone program under the address sanitizer, every source a heap block of exactly src_len bytes;
  - the ABI: every new symbol exported, the C struct's layout equal to GZIP_RESULT_DTYPE."""
import ctypes as C
import gzip
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import gzip_cases as GC
import mutation

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SIM_CPP = os.path.join(HERE, "gzip_sim", "sim_gzip.cpp")
FORMS = {"decode": 0, "size": 1}
BUDGETS = (512, 7)
GUARD, POISON = 64, 0xA5


def bind(so):
    L = C.CDLL(so)
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    L.sim_gzip.restype = None
    L.sim_gzip.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, C.c_int, u64p]
    L.sim_gzip_header.restype = None
    L.sim_gzip_header.argtypes = [C.c_char_p, C.c_uint64, u32p]
    L.sim_gzip_open_compress.restype = None
    L.sim_gzip_open_compress.argtypes = [C.c_uint64, C.c_int, u64p]
    L.sim_gzip_close_compress.restype = None
    L.sim_gzip_close_compress.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_void_p, u64p]
    L.sim_gzip_overhead.restype = C.c_ulonglong
    L.sim_gzip_overhead.argtypes = [C.c_int]
    L.sim_gzip_next.restype = None
    L.sim_gzip_next.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, u32p]
    return L


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return bind(mutation.gxx(tmp_path_factory.mktemp("gzip_sim") / "libgzip_sim.so", [SIM_CPP], extra=["-Wall", "-Wno-unknown-pragmas"]))


@pytest.fixture(scope="module")
def wants(oracle):
    """what every case must give, decode and size: computed once"""
    return {c.name: (GC.want(oracle, c), GC.want(oracle, c, size=True)) for c in GC.cases()}


def run(sim, c, form, budget, crc):
    """the model over one case, its source with what lies behind it in the arena, its room between guard bytes -> (the six
    fields of the record, the room's first out_len bytes, the guards untouched)"""
    size = form == "size"
    cap = 0 if size else c.cap
    buf = (C.c_ubyte * (GUARD + cap + GUARD))()
    C.memset(buf, POISON, len(buf))
    out = (C.c_uint64 * 6)(*[0xEE] * 6)
    arena = C.create_string_buffer(c.src + c.behind, len(c.src) + len(c.behind) + 1)
    sim.sim_gzip(arena, len(c.src), None if size else C.byref(buf, GUARD), cap, int(c.limit is not None), c.limit or 0, c.flags, FORMS[form],
                 crc, budget, out)
    got = np.frombuffer(buf, np.uint8)
    rec = tuple(int(x) for x in out)
    clean = bool((got[:GUARD] == POISON).all() and (got[GUARD + cap:] == POISON).all())
    return rec, got[GUARD:GUARD + min(rec[2], cap)].tobytes(), clean


def body_crc(oracle, c):
    """the CRC-32 the model is handed: of the bytes the oracle inflates the body to (0 where there is no body to inflate)"""
    h = GC.parse_header(c.src)
    if c.flags or h.status != 0:
        return 0
    st, data, _ = oracle.inflate(c.src[h.hdr_len:], decompressed_size=c.limit)
    return zlib.crc32(data) if st == 0 else 0


def failures(sim, oracle, cases, forms, budgets=BUDGETS, wants=None):
    """-> [(case, form, budget, what)]: every case against what the catalogue says of it"""
    bad = []
    for c in cases:
        crc = body_crc(oracle, c)
        for form in forms:
            size = form == "size"
            w = wants[c.name][int(size)] if wants else GC.want(oracle, c, size=size)
            for budget in budgets:
                rec, got, clean = run(sim, c, form, budget, crc)
                what = []
                if rec != tuple(w[:6]):
                    what.append("%r, not %r" % (rec, tuple(w[:6])))
                elif got != w.data:
                    what.append("bytes")
                if not clean:
                    what.append("wrote outside its room")
                if rec[3] > len(c.src):
                    what.append("src_used beyond src_len")
                if what:
                    bad.append((c.name, form, budget, "; ".join(what)))
    return bad


# ---- the catalogue --------------------------------------------------------------------------------------------------

def test_the_catalogue_agrees_with_zlib_and_covers_what_it_claims(oracle, wants):
    # all 32 flag values: zlib accepts each with unused_data of exactly the two bytes behind it
    for c in GC.flag_cases():
        d = zlib.decompressobj(31)
        assert d.decompress(c.src) == GC.flag_member(int(c.name[-2:]))[1] and d.eof and d.unused_data == b"\x1f\x8b", c.name
        w = wants[c.name][0]
        assert (w.status, w.src_used, w.flg, w.out_len) == (0, len(c.src) - 2, int(c.name[-2:]), 150), c.name
    # every proper prefix: zlib leaves it unfinished, the catalogue says CORRUPTED
    cuts = GC.cut_cases()
    assert len(cuts) == sum(len(GC.flag_member(f)[0]) for f in range(32)) > 3000
    for c in cuts:
        d = zlib.decompressobj(31)
        d.decompress(c.src)
        assert not d.eof, c.name
        assert wants[c.name][0].status == wants[c.name][1].status == GC.CORRUPTED, c.name
    # zlib's verdict of every whole member whose verdict is the container's to give (no limit, no flag bit, room enough)
    compared = 0
    for c in GC.flag_cases() + GC.other_cases():
        if c.limit is not None or c.flags or c.name == "body/room_too_small":
            continue
        st, used = GC.zlib_verdict(c.src)
        w = wants[c.name][0]
        if c.name in GC.DIFFERS:
            assert (st, used) != (w.status, w.src_used), c.name
            continue
        if st is None:  # (inflate's own messages are the oracle's)
            assert w.status == GC.CORRUPTED and c.name == "body/corrupted"
            continue
        assert (st, used) == (w.status, w.src_used), (c.name, (st, used), w[:4])
        compared += 1
    assert compared >= 65, compared
    got = {c.name: wants[c.name][0].status for c in GC.other_cases()}
    for name, st in (("small/empty_fixed", 0), ("small/empty_stored", 0), ("small/one_byte", 0), ("short/len0", 1), ("short/len9", 1), ("short/len10", 1),
                     ("short/len17", 1), ("short/len17_cm7", 1), ("header/magic0", 1), ("header/magic1", 1), ("header/cm7", 3), ("header/cm0", 3),
                     ("header/reserved20", 1), ("header/reserved40", 1), ("header/reserved80", 1), ("header/fhcrc_bit0", 1), ("header/fhcrc_bit9", 1),
                     ("header/fhcrc_all_fields", 0), ("header/subfield_overruns_xlen", 0), ("text/name65535", 0), ("text/name65536", 1),
                     ("text/zero_at_src_len_minus_1", 1), ("text/zero_at_src_len", 1), ("trailer/crc_wrong", 6), ("trailer/isize_wrong", 1),
                     ("trailer/both_wrong", 6), ("trailer/wrong_but_right_at_the_end", 6), ("trailer/cut1", 1), ("body/220", 0), ("body/bgzf65280", 0),
                     ("body/fixed", 0), ("body/stored", 0), ("body/dynamic", 0), ("body/corrupted", 1), ("body/room_too_small", 16), ("body/text300k", 0),
                     ("limit/below", 2), ("limit/at", 0), ("limit/above", 0), ("limit/bad_flag", 18)):
        assert got[name] == st, (name, got[name])
    # the sizing form compares no CRC-32 but does compare ISIZE
    assert [wants[n][1].status for n in ("trailer/crc_wrong", "trailer/isize_wrong", "trailer/both_wrong")] == [0, 1, 1]
    assert wants["trailer/crc_wrong"][0].checksum == zlib.crc32(GC._letters(150, 100))
    c = GC.by_name("trailer/cut1")
    assert GC.want(oracle, c._replace(src=c.src + c.behind)).src_used == len(c.src) + 1  # (src_len = src_used - 1)
    assert wants["body/bgzf65280"][0].src_used == len(GC.by_name("body/bgzf65280").src) - 28
    assert GC.parse_header(GC.by_name("body/bgzf65280").src).bsize == wants["body/bgzf65280"][0].src_used
    assert len(GC.by_name("small/empty_fixed").src) == 20
    # the long member's body is one the blocks path PICKS in a call with all the others (forms.h size_blocks_pick's model and
    # constants: fixed 0.8 ms, 0.36 + 0.067 ms a MiB taken, the one wave's 13.2 ms a MiB of the longest stream left)
    bodies = sorted((len(c.src) - w[0].hdr_len for c in GC.flag_cases() + GC.other_cases() for w in [wants[c.name]] if w[0].hdr_len), reverse=True)
    s, o = bodies[0] / 2.0 ** 20, bodies[1] / 2.0 ** 20
    assert bodies[0] == len(GC.by_name("body/text300k").src) - 10 >= 40 << 10 and 0.8 + (0.36 + 0.067) * s + 13.2 * o < 13.2 * s, bodies[:2]


def test_the_header_parse_is_the_second_writing(sim):
    """gzip_parse_header against gzip_cases.parse_header on every case: status, hdr_len, flg, bsize"""
    for c in GC.cases():
        out = (C.c_uint32 * 4)()
        sim.sim_gzip_header(c.src, len(c.src), out)
        assert tuple(out) == tuple(GC.parse_header(c.src)), c.name
    out = (C.c_uint32 * 4)()
    m = GC.flag_member(4)[0]
    sim.sim_gzip_header(m, len(m), out)
    assert out[3] == len(m)  # the BC subfield behind another subfield


# ---- the model ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", sorted(FORMS))
def test_the_model_gives_what_the_references_say(sim, oracle, wants, form):
    bad = failures(sim, oracle, GC.cases(), [form], wants=wants)
    assert not bad, (len(bad), bad[:5])


# ---- compress -------------------------------------------------------------------------------------------------------

def model_compress(sim, name, level, flavour, dst_cap):
    """the rules around deflate's bytes: gzip's open, deflate by its own capacity rule over the room the open gave it (the
    oracle's bytes), gzip's close -> (status, checksum, the member)"""
    import deflate_fit as F

    data = dict(GC.sources())[name]
    o = (C.c_uint64 * 3)()
    sim.sim_gzip_open_compress(dst_cap, flavour, o)
    pre, cap = int(o[0]), int(o[2])
    st, body = (GC.DST_TOO_SMALL, b"") if pre else F.expect(data, level, cap)[:2]
    room = (C.c_ubyte * (dst_cap + GUARD))()
    C.memset(room, POISON, len(room))
    out = (C.c_uint64 * 3)()
    sim.sim_gzip_close_compress(pre, st, zlib.crc32(data), body, len(body), len(data), level, flavour, room, out)
    assert all(b == POISON for b in room[dst_cap:]), "wrote behind its room"
    return int(out[0]), int(out[1]), bytes(room[:int(out[2])])


def compress_failures(sim, picks):
    bad = []
    for name, level, flavour in picks:
        n = len(dict(GC.sources())[name])
        bound = n + 6 * (n // 65534 + 1) + 8 + GC.overhead(flavour)
        for cap in (bound, GC.overhead(flavour) - 1):
            got, want = model_compress(sim, name, level, flavour, cap), GC.compress_want(name, level, flavour, cap)
            if got != want:
                bad.append(("compress:%s:%d:%d" % (name, level, flavour), "compress", cap, "%r, not %r" % (got[:2] + (len(got[2]),), want[:2] + (len(want[2]),))))
    return bad


def all_compress_picks():
    return [(name, level, flavour) for name, _ in GC.sources() for level in GC.LEVELS for flavour in GC.FLAVOURS]


def test_compress_is_header_oracle_deflate_trailer(sim, oracle):
    assert not compress_failures(sim, all_compress_picks())
    n_ok = n_small = 0
    for name, data in GC.sources():
        for level in GC.LEVELS:
            for flavour in GC.FLAVOURS:
                st, crc, m = GC.compress_want(name, level, flavour, 1 << 20)
                if st:
                    assert flavour == GC.BGZF and st == GC.DST_TOO_SMALL and len(data) > 65280, (name, level)
                    n_small += 1
                    continue
                n_ok += 1
                body = oracle.deflate(data, level=level)[1]
                hdr = 18 if flavour == GC.BGZF else 10
                assert m[hdr:-8] == body and gzip.decompress(m) == data, (name, level, flavour)
                d = zlib.decompressobj(31)
                assert d.decompress(m) == data and d.eof and not d.unused_data
                if flavour == GC.BGZF:
                    assert len(m) <= 65536 and struct.unpack("<H", m[16:18])[0] == len(m) - 1 and GC.parse_header(m).bsize == len(m)
    assert n_ok > 100 and n_small >= 12, (n_ok, n_small)
    # every BGZF source of 65 280 bytes fits, whatever it holds
    assert all(GC.compress_want("random65280", level, GC.BGZF, 1 << 20)[0] == 0 for level in GC.LEVELS)


def test_the_header_is_pythons_gzip_header(sim):
    """MTIME 0, XFL 2 at Best and 4 at Fast, OS 255: the ten bytes Python's gzip writes for mtime=0"""
    for level, py in ((3, 9), (1, 1)):
        assert model_compress(sim, "text1", level, GC.PLAIN, 64)[2][:10] == gzip.compress(b"x", py, mtime=0)[:10], level
    assert model_compress(sim, "text1", 2, GC.PLAIN, 64)[2][:10] == bytes.fromhex("1f8b08000000000000ff")
    assert sim.sim_gzip_overhead(GC.PLAIN) == 18 and sim.sim_gzip_overhead(GC.BGZF) == 26


# ---- the host plan --------------------------------------------------------------------------------------------------

def walk(sim, data):
    """gzip_next over a file as the host forms walk it, every member taken at the length the references give it -> [(off,
    known, bsize, isize)], the status the walk ends with, where it ends"""
    off, seen = 0, []
    while True:
        o = (C.c_uint32 * 8)()
        sim.sim_gzip_next(data, len(data), off, o)
        st, end, known, hdr_len, flg, bsize, isize = [int(x) for x in o[:7]]
        if end:
            return seen, 0, off
        if st:
            return seen, st, off
        used = bsize if known else GC.zlib_verdict(data[off:])[1]
        if not used:
            return seen, -1, off
        seen.append((off, known, bsize, isize))
        off += used


def test_gzip_next_plans_the_files(sim):
    for f in GC.files():
        seen, st, end = walk(sim, f.data)
        if f.status == 0:
            assert (st, end, len(seen)) == (0, f.src_used, f.members), f.name
            runs = sum(1 for i, s in enumerate(seen) if s[1] and (i == 0 or not seen[i - 1][1]))
            assert runs == f.runs, (f.name, runs)
            assert sum(s[3] for s in seen if s[1]) == sum(len(zlib.decompress(f.data[s[0]:s[0] + s[2]], 31)) for s in seen if s[1])
    seen, st, end = walk(sim, GC.file_by_name("bgzf_run").data)
    assert all(s[1] for s in seen) and len(seen) == 101 and seen[-1][2] == 28 and seen[-1][3] == 0
    # the lying BSIZE: member 57 is planned one byte too long, and what stands behind it begins no member
    f = GC.file_by_name("bgzf_bsize_lies")
    seen, st, end = walk(sim, f.data)
    true_len = GC.zlib_verdict(f.data[seen[57][0]:])[1]
    assert len(seen) == 58 and st == 0 and seen[57][2] == true_len + 1
    # a BSIZE that reaches beyond the file is not known; the first member's failure is its own; nothing at all is corrupted
    o = (C.c_uint32 * 8)()
    m = GC.bgzf_member(b"reaches beyond")
    sim.sim_gzip_next(m[:-1], len(m) - 1, 0, o)
    assert (o[0], o[1], o[2]) == (0, 0, 0)
    sim.sim_gzip_next(m, len(m), 0, o)
    assert (o[0], o[1], o[2], o[5], o[6]) == (0, 0, 1, len(m), 14)
    assert walk(sim, GC.file_by_name("first_member_bad_method").data)[1] == GC.METHOD and walk(sim, b"")[1] == GC.CORRUPTED
    sim.sim_gzip_next(m + b"\x1f", len(m) + 1, len(m), o)
    assert o[1] == 1  # (one byte behind the last member begins none)


# ---- the mutants ----------------------------------------------------------------------------------------------------
# (name, [(text, replacement), ...] of gzip_container.h, (form, the case that must fail)): one-rule mutants.  Host-model
# mutants: built with g++ and run in child processes, never built into a GPU library.
H = "gzip_container.h"
GZIP_MUTANTS = [
    ("min_length_10", [("GZIP_MIN_LEN = 18;", "GZIP_MIN_LEN = 10;")], ("decode", "short/len17_cm7")),
    ("magic_check_dropped", [("  if (s[0] != 0x1Fu || s[1] != 0x8Bu) return h;\n", "")], ("decode", "header/magic1")),
    ("cm_check_dropped", [("  if (s[2] != 8u) { h.status = ST_ZLIB_METHOD; return h; }\n", "")], ("decode", "header/cm7")),
    ("reserved_mask_c0", [("if ((flg & 0xE0u) != 0) return h;", "if ((flg & 0xC0u) != 0) return h;")], ("decode", "header/reserved20")),
    ("xlen_big_endian", [("(uint64_t)s[pos] | ((uint64_t)s[pos + 1] << 8);", "(uint64_t)s[pos + 1] | ((uint64_t)s[pos] << 8);")], ("decode", "flags/04")),
    ("fname_taken_for_fcomment", [("if (flg & GZIP_FNAME) {", "if (flg & GZIP_FCOMMENT) {")], ("decode", "flags/08")),
    # (a pure swap of the two is no rule change: both are zero-terminated fields skipped one after the other, whichever bit asks first)
    ("fname_and_fcomment_swapped", [("if (flg & GZIP_FNAME) {", "if (flg & GZIP_FCOMMENT_) {"), ("if (flg & GZIP_FCOMMENT) {", "if (flg & GZIP_FNAME) {"),
                                    ("if (flg & GZIP_FCOMMENT_) {", "if (flg & GZIP_FCOMMENT) {")],
     ("decode-flags", ("equivalent", "the fields are skipped in the same order with the same rule"))),
    ("text_cap_65536", [("GZIP_MAX_TEXT = 65535;", "GZIP_MAX_TEXT = 65536;")], ("decode", "text/name65536")),
    ("zero_searched_to_len_inclusive", [("if (pos + n >= len) return 0;", "if (pos + n > len) return 0;")], ("decode", "text/zero_at_src_len")),
    ("fhcrc_mask_ff", [("gzip_u16(s + pos)) & 0xFFFFu) != 0", "gzip_u16(s + pos)) & 0xFFu) != 0")], ("decode", "header/fhcrc_bit9")),
    ("fhcrc_over_itself", [("gzip_header_crc(s, pos) ^", "gzip_header_crc(s, pos + 2) ^")], ("decode", "header/fhcrc_all_fields")),
    ("trailer_at_src_len_minus_8", [("const uint8_t *trailer = stream + hdr_len + u;", "const uint8_t *trailer = stream + src_len - 8u;")],
     ("decode", "flags/00")),
    ("trailer_at_src_len_minus_8_passes_a_wrong_one", [("const uint8_t *trailer = stream + hdr_len + u;", "const uint8_t *trailer = stream + src_len - 8u;")],
     ("decode", "trailer/wrong_but_right_at_the_end")),
    ("trailer_bound_refuses_the_exact_fit", [("if (hdr_len + u + 8u > src_len) return", "if (hdr_len + u + 8u >= src_len) return")],
     ("decode", "small/empty_fixed")),
    ("crc_and_isize_order_swapped", [("  if (crc_bad) return gzip_refusal(ST_CHECKSUM, inner.checksum);\n  if (isize_bad) return gzip_refusal(ST_CORRUPTED, 0);\n",
                                      "  if (isize_bad) return gzip_refusal(ST_CORRUPTED, 0);\n  if (crc_bad) return gzip_refusal(ST_CHECKSUM, inner.checksum);\n")],
     ("decode", "trailer/both_wrong")),
    ("isize_compare_dropped_in_the_sizing_close", [("const bool isize_bad = isize !=", "const bool isize_bad = compare_crc && isize !=")],
     ("size", "trailer/isize_wrong")),
    ("src_used_plus_4", [("r.src_used = hdr_len + u + 8u;", "r.src_used = hdr_len + u + 4u;")], ("size", "small/empty_fixed/ff5")),
    ("xfl_mapping_swapped", [("level == LEVEL_BEST ? 2u : level == LEVEL_FAST ? 4u : 0u", "level == LEVEL_BEST ? 4u : level == LEVEL_FAST ? 2u : 0u")],
     ("compress", "compress:text1:3:0")),
    ("bsize_not_reduced_by_one", [("const uint64_t bsize = member_len - 1u;", "const uint64_t bsize = member_len;")], ("compress", "compress:text65280:2:1")),
    ("bgzf_room_not_clipped", [("return flavour == GZIP_BGZF && cap > GZIP_BGZF_MAX ? GZIP_BGZF_MAX : cap; }", "return cap; }")],
     ("compress", "compress:random65536:2:1")),
]

_CHILD = r"""
import json, os, sys
root, so, form, name = sys.argv[1:5]
sys.path.insert(0, os.path.join(root, "tests")); sys.path.insert(0, root)
import gzip_cases as GC
import oracle
import test_gzip_rules as T
oracle.lib()
if form == "compress":
    _, src, level, flavour = name.split(":")
    bad = T.compress_failures(T.bind(so), [(src, int(level), int(flavour))])
elif form == "decode-flags":
    bad = T.failures(T.bind(so), oracle, GC.flag_cases() + GC.other_cases(), ["decode"])
else:
    bad = T.failures(T.bind(so), oracle, [GC.by_name(name)], [form])
print(json.dumps(sorted({b[0] for b in bad})))
"""


def mutant_model(m, into):
    """the model over a copy of zipc_amd/csrc with one rule changed -> its shared library"""
    name, edits = m[:2]
    csrc, tests = os.path.join(str(into), "zipc_amd", "csrc"), os.path.join(str(into), "tests")
    shutil.copytree(os.path.join(ROOT, "zipc_amd", "csrc"), csrc, ignore=shutil.ignore_patterns("build", "*.hip"))
    for d in ("gzip_sim", "extent_sim"):
        shutil.copytree(os.path.join(HERE, d), os.path.join(tests, d), ignore=shutil.ignore_patterns("*main.cpp"))
    path = os.path.join(csrc, H)
    text = open(path).read()
    for old, new in edits:
        text = mutation.patched(text, old, new, name)
    with open(path, "w") as f:
        f.write(text)
    return mutation.gxx(os.path.join(tests, "gzip_sim", "libgzip_sim.so"), [os.path.join(tests, "gzip_sim", "sim_gzip.cpp")], extra=["-Wno-unknown-pragmas"])


def test_gzip_mutants_are_killed(tmp_path, capsys):
    import concurrent.futures

    sos = mutation.build_all(lambda m: mutant_model(m, tmp_path / m[0]), GZIP_MUTANTS)
    with concurrent.futures.ThreadPoolExecutor(max_workers=mutation.workers()) as ex:
        jobs = [ex.submit(mutation.run_child, _CHILD, ROOT, so, m[2][0], m[2][1]) for m, so in zip(GZIP_MUTANTS, sos)]
        rows = []
        for m, job in zip(GZIP_MUTANTS, jobs):
            rc, failed, err = job.result()
            crashed = rc != 0 or failed is None
            rows.append((m[0], m[2][1], crashed, mutation.verdict(m[2][1], failed or [], crashed), err[-300:] if crashed else ""))
    with capsys.disabled():
        print("\ngzip mutants in the host model")
        for name, killer, crashed, ok, _ in rows:
            print("  %-48s %s%s %s" % (name, killer, " (child crashed)" if crashed else "", "" if ok else "-- SURVIVED"))
    assert all(r[3] and not r[2] for r in rows), [r for r in rows if not r[3] or r[2]]
    assert len(GZIP_MUTANTS) >= 18


def test_the_unmutated_model_fails_none_of_the_killers(sim, oracle):
    for m in GZIP_MUTANTS:
        form, name = m[2]
        if form == "compress":
            _, src, level, flavour = name.split(":")
            assert not compress_failures(sim, [(src, int(level), int(flavour))]), m[0]
        elif form != "decode-flags":
            assert not failures(sim, oracle, [GC.by_name(name)], [form]), m[0]


# ---- the audit program ----------------------------------------------------------------------------------------------

def test_audit_program_under_the_address_sanitizer(tmp_path, oracle, wants):
    """the model as a stand-alone program with its own main, built with -fsanitize=address,undefined and run as a process
    over the whole catalogue, truncations included: every source a heap block of exactly src_len bytes and every room one of
    exactly dst_cap, so a load behind the declared source or a store behind the room trips the sanitizer; it aborts on any
    record that differs from what is expected"""
    rows = []
    for c in GC.cases():
        crc = body_crc(oracle, c)
        for form in ("decode", "size"):
            size = form == "size"
            w = wants[c.name][int(size)]
            rows.append(struct.pack("<13I", len(c.src), 0 if size else c.cap, int(c.limit is not None), c.limit or 0, c.flags, FORMS[form], crc, *w[:6]) + c.src)
    path = tmp_path / "cases.bin"
    path.write_bytes(struct.pack("<I", len(rows)) + b"".join(rows))
    exe = str(tmp_path / "gzip_audit")
    mutation.gxx(exe, [os.path.join(HERE, "gzip_sim", "audit_main.cpp")], shared=False,
                 extra=["-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert b"nothing outside a source or a room" in r.stdout and ("%d cases" % len(rows)).encode() in r.stdout


# ---- the ABI --------------------------------------------------------------------------------------------------------

NEW_SYMBOLS = ("zipc_hip_gzip_decompress_batch", "zipc_hip_gzip_size_batch", "zipc_hip_gzip_size_blocks_batch", "zipc_hip_gzip_bound",
               "zipc_hip_gzip_compress_batch", "zipc_hip_gzip_compress", "zipc_hip_gzip_size", "zipc_hip_gzip_decompress")


def test_every_new_symbol_is_exported_and_bound():
    from zipc_amd import _lib

    L = _lib.lib()
    bound = {s[0] for s in _lib.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert name in bound and getattr(L, name) is not None, name
    assert L.zipc_hip_abi_version() == 1
    for n in (0, 1, 65280, 1 << 20):
        assert L.zipc_hip_gzip_bound(n, 0) == L.zipc_hip_deflate_bound(n) + 18 and L.zipc_hip_gzip_bound(n, 1) == L.zipc_hip_deflate_bound(n) + 26


def test_the_result_record_is_the_dtype(tmp_path):
    from zipc_amd import _lib
    from zipc_amd.batch import GZIP_RESULT_DTYPE as D

    fields = ("status", "checksum", "out_len", "src_used", "hdr_len", "flg")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "zipc_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %d %d\\n", '
                   "sizeof(zipc_hip_gzip_result), " + ", ".join("offsetof(zipc_hip_gzip_result, %s)" % f for f in fields) +
                   ", ZIPC_HIP_GZIP_PLAIN, ZIPC_HIP_GZIP_BGZF); return 0; }\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    got = [int(x) for x in subprocess.run([exe], stdout=subprocess.PIPE, check=True).stdout.split()]
    assert got[:7] == [D.itemsize] + [D.fields[f][1] for f in fields] == [32, 0, 4, 8, 16, 24, 28]
    assert got[7:] == [_lib.GZIP_PLAIN, _lib.GZIP_BGZF] == [0, 1]
    assert C.sizeof(_lib.GzipResult) == 32 and [getattr(_lib.GzipResult, f).offset for f in fields] == got[1:7]
