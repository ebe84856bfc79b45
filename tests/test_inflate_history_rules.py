"""The history forms on the CPU (include/zipc_hip.h at zipc_hip_inflate_history_batch; csrc/inflate_history.h has the rule): a
decode that starts at a bit of a byte with bytes in front of its output, and zlib streams with a preset dictionary.
The host model is tests/history_sim/sim_history.cpp -- inflate_lane.h's plain step and inflate_span.h on an emulated wave,
started and finished through inflate_history.h as inflate.hip's HISTORY wave does it -- in the prefix model's four forms and
the kernels' three modes.  What is expected comes from the catalogue (tests/inflate_history_cases.py), which is checked
here against Python's zlib, and from tests/inflate_room_cases.py; never from the model.  This file holds

  - the catalogue against zlib, item for item;
  - every case in all four forms and three modes, the room at dst_off 1..16 mod 16 between guard bytes, the history
    unchanged afterwards, RFC 1950's Adler-32 of the output alone;
  - the null record over the room catalogue's SIM_FAMILIES: the plain forms, result for result;
  - the dictionary forms' open, seed and close as tables, and end to end over every zlib case;
  - HISTORY_MUTANTS, each built into a model of its own and run in a child process;
  - the model as a stand-alone program under the address sanitizer, every [history | room] a heap block of exactly
    hist_len + dst_cap bytes and every source one of exactly src_len."""
import ctypes as C
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import inflate_history_cases as HC
import inflate_room_cases as RC
import mutation
from host_sim import HERE as HOST_SIM_DIR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SIM_CPP = os.path.join(HERE, "history_sim", "sim_history.cpp")
FORMS = {"plain-512": (0, 512), "plain-7": (0, 7), "span-a": (1, 24), "span-d": (2, 24)}
REAL, PREFIX, SIZE = 0, 1, 2
MODES = {"history": REAL, "prefix": PREFIX, "size": SIZE}
GUARD, POISON = RC.GUARD, RC.POISON
ROOM_MAX = 1 << 20  # a declared room above this is one the case's record or descriptor is refused for: none is allocated


def bind(so):
    L = C.CDLL(so)
    L.sim_history.restype = None
    L.sim_history.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_uint64,
                              C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
    L.sim_dict_adler.restype = C.c_uint
    L.sim_dict_adler.argtypes = [C.c_char_p, C.c_ulonglong]
    L.sim_zlib_open_dict.restype = None
    L.sim_zlib_open_dict.argtypes = [C.c_char_p, C.c_ulonglong, C.c_char_p, C.c_ulonglong, C.POINTER(C.c_ulonglong)]
    L.sim_zlib_dict_seeds.restype = C.c_int
    L.sim_zlib_dict_seeds.argtypes = [C.c_uint, C.c_uint, C.c_ulonglong]
    L.sim_zlib_close_dict.restype = None
    L.sim_zlib_close_dict.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_ulonglong, C.c_int, C.POINTER(C.c_ulonglong)]
    return L


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return bind(mutation.gxx(tmp_path_factory.mktemp("history_sim") / "libhistory_sim.so", [SIM_CPP], include=[HOST_SIM_DIR],
                             extra=["-Wall", "-Wno-unknown-pragmas"]))


def run(sim, c, mode, form, off_mod, adler=0):
    """the model over one case: [guard | arena: pad, history, room | guard], the room at off_mod (mod 16) of the arena
    -> ((status, checksum or ended, out_len), the room's first out_len bytes, what is wrong around the room or None)"""
    span, budget = FORMS[form]
    room = c.cap if c.cap <= ROOM_MAX else 0
    if c.dst_off is not None:
        off = c.dst_off
        assert not c.hist
    else:
        off = len(c.hist) + (off_mod - len(c.hist)) % 16
    buf = (C.c_ubyte * (GUARD + off + room + GUARD))()
    C.memset(buf, POISON, len(buf))
    at = GUARD + off
    C.memmove(C.byref(buf, at - len(c.hist)), c.hist, len(c.hist))
    out = (C.c_uint64 * 3)(0xEE, 0xEE, 0xEE)
    arena = None if mode == SIZE else C.byref(buf, GUARD)
    sim.sim_history(c.raw, len(c.raw), c.rec[0], c.rec[1], arena, off, c.cap, int(c.limit is not None), c.limit or 0, c.flags_extra,
                    mode, adler, span, budget, out)
    got = np.frombuffer(buf, np.uint8)
    rec = (int(out[0]), int(out[1]), int(out[2]))
    wrong = None
    if not (got[:at - len(c.hist)] == POISON).all():
        wrong = "wrote in front of its history"
    elif got[at - len(c.hist):at].tobytes() != c.hist:
        wrong = "changed its history"
    elif not (got[at + room:] == POISON).all():
        wrong = "wrote behind its room"
    elif mode == SIZE and not (got[at:] == POISON).all():
        wrong = "the sizing form wrote"
    return rec, got[at:at + min(rec[2], room)].tobytes(), wrong


def want_of(c, mode, adler=0):
    """-> ((status, checksum or ended, out_len), the bytes or None)"""
    if mode == PREFIX:
        w = HC.expect_prefix(c)
        return w, (c.plain[:w[2]] if w[0] == 0 else None)
    if mode == SIZE:
        st, n = HC.expect_size(c)
        return (st, 0, n), None
    st, n = HC.expect_history(c)
    return (st, zlib.adler32(c.plain) if adler and st == 0 else 0, n), (c.plain if st == 0 else None)


def failures(sim, cases, forms, modes=(REAL, PREFIX, SIZE), adler=1):
    """cases: [(case, off_mod)] -> [(name, mode, form, what)]"""
    bad = []
    for c, off_mod in cases:
        for mode in modes:
            for form in forms:
                rec, data, wrong = run(sim, c, mode, form, off_mod, adler)
                want, plain = want_of(c, mode, adler)
                what = []
                if rec != want:
                    what.append("%r, not %r" % (rec, want))
                elif plain is not None and data != plain:
                    what.append("bytes")
                if wrong:
                    what.append(wrong)
                if what:
                    bad.append((c.name, mode, form, "; ".join(what)))
    return bad


def laid_out():
    return [(c, HC.ROOM_MODS[i % 16]) for i, c in enumerate(HC.cases())]


# ---- the catalogue ------------------------------------------------------------------------------------------------

def _from_bit(raw, bit):
    """the bits of `raw` from `bit` on, as bytes"""
    return (int.from_bytes(raw, "little") >> bit).to_bytes(len(raw), "little")


def test_the_catalogue_is_what_it_claims():
    """every piece against Python's zlib (raw deflate with zdict = the history, read from its start bit): the declared
    bytes, or for a piece declared CORRUPTED zlib's own 'invalid distance too far back'; the record cases are refused for
    what their names say; no family is missing"""
    cases = HC.cases()
    fams = {}
    for c in cases:
        fams[c.name.split("/")[0]] = fams.get(c.name.split("/")[0], 0) + 1
    assert set(fams) == {"fixed", "boundary", "record", "rooms"} and len(cases) == 126, (fams, len(cases))
    n_bad = 0
    for c in cases:
        if c.status == HC.INVALID_ARG:
            assert c.rec[0] > HC.HIST_MAX or c.rec[1] > 7 or (c.dst_off is not None and c.rec[0] > c.dst_off) or c.flags_extra or \
                c.cap > HC.MAX_STREAM_LEN, c.name
            continue
        assert c.rec == (len(c.hist), c.start_bit) and len(c.hist) <= HC.HIST_MAX and c.start_bit <= 7, c.name
        do = zlib.decompressobj(-15, zdict=c.hist) if c.hist else zlib.decompressobj(-15)
        aligned = _from_bit(c.raw, c.start_bit)
        if c.name.startswith("boundary/stored_first"):  # (a stored block's bytes lie on byte boundaries: no shift of the bits keeps them)
            aligned = HC.stored_behind_bit(0)[0]        # the same blocks written from bit 0: equal behind the header's three bits
            assert c.raw[-(len(aligned) - 1):] == aligned[1:] and (int.from_bytes(c.raw[:2], "little") >> c.start_bit) & 7 == aligned[0] & 7 == 0
        try:
            got = do.decompress(aligned)
        except zlib.error as e:
            assert c.status == HC.CORRUPTED and c.plain is None and "distance too far back" in str(e), (c.name, e)
            n_bad += 1
            continue
        assert c.status == HC.OK and do.eof and got == c.plain, c.name
    assert n_bad == sum(c.status == HC.CORRUPTED for c in cases) == 13 + 7 + 2, n_bad
    mods = {(HC.ROOM_MODS[i % 16], len(c.hist) & 1) for i, c in enumerate(cases) if c.name.startswith("rooms/")}
    assert len(mods) == 32  # dst_off 1..16 mod 16, each with an odd and an even history


def test_the_zlib_cases_are_what_they_claim(oracle):
    """every zlib case against Python's zlib with its call's dictionary; the big dictionary's two Adler-32 flavours differ"""
    D = HC.dicts()
    assert zlib.adler32(D["big"]) != oracle.adler32(D["big"]) and [len(D[k]) for k in ("one", "mid", "big")] == [1, 257, 32768]
    zs = HC.zcases()
    assert len(zs) == 58 and {z.dict for z in zs} == set(HC.ZDICT_CALLS)
    for z in zs:
        d = HC.zdict_of(z)
        do = zlib.decompressobj(15, zdict=d) if d else zlib.decompressobj(15)
        try:
            got = do.decompress(z.raw)
            ok = do.eof
        except zlib.error:
            ok = False
        if z.status == HC.OK:
            assert ok and got == z.plain and z.checksum == zlib.adler32(got), z.name
        elif z.status == HC.DST_TOO_SMALL:
            assert ok and len(got) == z.cap + 1, z.name
        else:
            assert not ok, z.name
        if z.status == HC.ZLIB_DICT:
            assert z.checksum == int.from_bytes(z.raw[2:6], "big") != zlib.adler32(d), z.name


@pytest.mark.parametrize("form", sorted(FORMS))
def test_every_case_in_every_mode(sim, form):
    """the whole catalogue: results, bytes, guards, the history unchanged, the Adler-32 of the output alone"""
    bad = failures(sim, laid_out(), [form])
    assert not bad, (len(bad), bad[:5])
    if form.startswith("span"):
        spans = (C.c_uint64 * 2).in_dll(sim, "sim_history_spans")
        assert spans[0] > 0  # (fixed/span_dense and the long text went through the span decoder)


def test_a_record_of_zeros_is_the_plain_form(sim):
    """hist_len 0 and start_bit 0 over the room catalogue: what its items declare of zipc_hip_inflate_batch, the prefix form
    and sizing -- every fourth item of every family in plain-512, every sixteenth in the other three forms (the prefix
    and room models run every item through the same step; what is new here is the start and the result store)"""
    def as_case(it):
        s = RC.stream_of(it)
        return HC.Case(RC.item_id(it), s.raw, 0, b"", (0, 0), it.cap, it.limit, 0, None, s.plain, 0)

    n = 0
    for f in RC.SIM_FAMILIES:
        its = RC.items(f)
        for every, forms in ((4, ["plain-512"]), (16, ["plain-7", "span-a", "span-d"])):
            for it in its[::every]:
                c = as_case(it)
                size_st = 2 if it.limit is not None and len(c.plain) > it.limit else 0
                wants = {REAL: ((it.want, 0, len(c.plain) if it.want == 0 else 0), c.plain if it.want == 0 else None),
                         PREFIX: ({0: (0, 1, len(c.plain)), 16: (0, 0, it.R), 2: (2, 0, 0)}[it.want], c.plain),
                         SIZE: ((size_st, 0, 0 if size_st else len(c.plain)), None)}
                for mode, (want, plain) in wants.items():
                    for form in forms:
                        rec, data, wrong = run(sim, c, mode, form, it.off_mod or 16)
                        assert rec == want and wrong is None, (c.name, mode, form, rec, want, wrong)
                        assert plain is None or data == plain[:rec[2]], (c.name, mode, form)
                        n += 1
    assert n > 3 * 7818 // 4 + 9 * 7818 // 16


# ---- the dictionary forms ---------------------------------------------------------------------------------------------

def dict_model(sim, z, size=False, form="plain-512", gap=True):
    """zipc_hip_zlib_decompress_dict_batch (size: zipc_hip_zlib_size_dict_batch) of one stream as api.hip puts it together:
    open, seed, the history wave over the body, close -> ((status, checksum, out_len), bytes, what is wrong around the room)"""
    d = HC.zdict_of(z)
    o = (C.c_ulonglong * 5)()
    sim.sim_zlib_open_dict(z.raw, len(z.raw), d, len(d), o)
    pre, expect, body_off, body_len, hist_len = (int(x) for x in o)
    off = len(d) + (5 - len(d)) % 16 if gap else 5  # (gap False: dst_off 5, no room for a dictionary of more bytes in front of it)
    buf = (C.c_ubyte * (GUARD + off + z.cap + GUARD))()
    C.memset(buf, POISON, len(buf))
    at = GUARD + off
    seeded = bool(sim.sim_zlib_dict_seeds(pre, hist_len, off)) and not size
    if seeded and hist_len > off:
        return (0xEE, 0xEE, 0xEE), b"", "seeded over the arena's start"
    if seeded:
        C.memmove(C.byref(buf, at - hist_len), d, hist_len)
    inner = (C.c_uint64 * 3)()
    body = z.raw[body_off:body_off + body_len] if pre == 0 else b""
    span, budget = FORMS[form]
    sim.sim_history(body, len(body), hist_len, 0, None if size else C.byref(buf, GUARD), off, z.cap if pre == 0 else 0, 0, 0, 0,
                    SIZE if size else REAL, 1, span, budget, inner)
    out = (C.c_ulonglong * 3)()
    sim.sim_zlib_close_dict(pre, expect, int(inner[0]), int(inner[1]), int(inner[2]), int(size), out)
    got = np.frombuffer(buf, np.uint8)
    front = min(len(d), off)
    gap = got[at - front:at]
    wrong = None
    if not (got[:at - front] == POISON).all() or not (got[at + z.cap:] == POISON).all():
        wrong = "wrote outside the gap and the room"
    elif seeded != (z.seeded and not size and len(d) <= off):
        wrong = "seeded %r" % seeded
    elif not seeded and not (gap == POISON).all():
        wrong = "the gap of a stream that is not seeded was written"
    elif seeded and gap.tobytes() != d:
        wrong = "the gap does not hold the dictionary"
    return tuple(int(x) for x in out), got[at:at + min(int(out[2]), z.cap)].tobytes(), wrong


def zlib_failures(sim, zs, forms=("plain-512",)):
    bad = []
    for z in zs:
        for form, size, gap in [(f, s, True) for f in forms for s in (False, True)] + [(forms[0], s, False) for s in (False, True)]:
            if not gap and len(HC.zdict_of(z)) <= 5:
                continue
            rec, data, wrong = dict_model(sim, z, size, form, gap)
            if size:  # no trailer is compared and there is no room, nor a gap
                st = HC.OK if z.status in (HC.CHECKSUM, HC.DST_TOO_SMALL) else z.status
                want = (st, z.checksum if st == HC.ZLIB_DICT else 0, len(z.plain) if st == HC.OK else 0)
            elif not gap and z.seeded:
                want = (HC.INVALID_ARG, 0, 0)  # (inflate_history.h: hist_len > dst_off)
            else:
                want = (z.status, z.checksum, len(z.plain) if z.status == HC.OK else 0)
            what = []
            if rec != want:
                what.append("%r, not %r" % (rec, want))
            elif not size and want[0] == HC.OK and data != z.plain:
                what.append("bytes")
            if wrong:
                what.append(wrong)
            if what:
                bad.append((z.name, SIZE if size else REAL, form, "; ".join(what)))
    return bad


def test_zlib_cases_through_open_seed_wave_and_close(sim):
    bad = zlib_failures(sim, HC.zcases(), sorted(FORMS))
    assert not bad, (len(bad), bad[:5])


def test_zlib_open_dict_table(sim):
    """the checks in their order: length, FCHECK, method, window, then FDICT's own"""
    d = HC.dicts()["mid"]
    good = HC.zdeflate(b"hello hello hello", 9, d)
    plain = HC.zdeflate(b"hello hello hello", 9)

    def opened(stream, dic=d):
        o = (C.c_ulonglong * 5)()
        sim.sim_zlib_open_dict(stream, len(stream), dic, len(dic), o)
        return tuple(int(x) for x in o)

    trailer = int.from_bytes(good[-4:], "big")
    assert opened(good) == (0, trailer, 6, len(good) - 10, len(d))
    assert opened(plain) == (0, int.from_bytes(plain[-4:], "big"), 2, len(plain) - 4, 0)  # (the reference's body: [2, len - 2))
    assert opened(good[:5])[0] == 1 and opened(b"")[0] == 1
    bad_check = bytes([good[0], good[1] ^ 1]) + good[2:]
    assert opened(bad_check)[0] == 1
    fix = lambda cmf, flg: bytes([cmf, (flg & 0xE0) + (31 - (cmf * 256 + (flg & 0xE0)) % 31) % 31])
    assert opened(fix(0x79, good[1]) + good[2:])[0] == 3      # method 9, with FDICT set: the method comes first
    assert opened(fix(0x88, good[1]) + good[2:])[0] == 4      # window 8
    assert opened(good[:9]) == (1, 0, 0, 0, 0)                # FDICT in 9 bytes
    assert opened(good[:10])[0] == 0 and opened(good[:10])[3] == 0
    assert opened(good, b"") == (5, zlib.adler32(d), 0, 0, 0)  # no dictionary: the DICTID it asks for
    assert opened(good, d[1:]) == (5, zlib.adler32(d), 0, 0, 0)
    for pre, hist_len, dst_off, want in ((0, 257, 257, 1), (0, 257, 256, 0), (0, 0, 0, 0), (5, 0, 1000, 0), (18, 0, 1000, 0), (0, 1, 1, 1)):
        assert sim.sim_zlib_dict_seeds(pre, hist_len, dst_off) == want


def test_zlib_close_dict_table(sim):
    def close(pre, expect, inner, size):
        out = (C.c_ulonglong * 3)()
        sim.sim_zlib_close_dict(pre, expect, inner[0], inner[1], inner[2], size, out)
        return tuple(int(x) for x in out)

    A, B = 0x11E60398, 0x00620062
    for size in (0, 1):
        assert close(5, A, (1, 0, 0), size) == (5, A, 0)       # the DICTID found, in both forms
        for pre in (1, 3, 4, 18):
            assert close(pre, 0, (1, 0, 0), size) == (pre, 0, 0)
        assert close(0, A, (1, 0, 0), size) == (1, 0, 0) and close(0, A, (18, 0, 0), size) == (18, 0, 0)
    assert close(0, A, (0, A, 500), 0) == (0, A, 500) and close(0, A, (0, B, 500), 0) == (6, B, 0)
    assert close(0, A, (0, 0, 500), 1) == (0, 0, 500)          # sizing compares nothing


# ---- the mutants ----------------------------------------------------------------------------------------------------
# (name, file, text, replacement, killer): one-line mutants of inflate_history.h, of zlib_container.h's dictionary rules, of
# the distance test of inflate_lane.h and of the model's dictionary checksum.  killer: (mode, form, the case that must
# fail), mode "zlib" for a case of zcases(); or ("equivalent", why): nothing of the whole catalogue in plain-512 may fail.
# SOME OF THESE READ OR WRITE A BYTE OUT OF THEIR ROOM BY DESIGN (the 64-byte guards hold it inside the child's buffer): they
# are host-model mutants, built with g++ and run in child processes, never built into a GPU library.
_H, _Z = "inflate_history.h", "zlib_container.h"
HISTORY_MUTANTS = [
    ("limit_not_biased", _H, "  d.limit = history_limit(d.limit, hist_len);", "  d.limit = history_limit(d.limit, 0);",
     ("history", "plain-512", "record/limit_counts_the_streams_own_bytes")),
    ("limit_bias_wraps", _H, "return limit > 0xFFFFFFFFu - hist_len ? 0xFFFFFFFFu : limit + hist_len; }", "return limit + hist_len; }",
     ("history", "plain-512", "fixed/match_at_0")),
    ("out_len_keeps_the_history", _H, "r.out_len = status == ST_OK ? history_out_len(out_pos, hist_len) : 0u;",
     "r.out_len = status == ST_OK ? out_pos : 0u;", ("history", "plain-512", "fixed/match_at_0")),
    ("cut_out_len_keeps_the_history", _H, "if (r.status == ST_OK) r.out_len = history_out_len(",
     "if (r.status == ST_OK && r.ended) r.out_len = history_out_len(", ("prefix", "plain-512", "record/room_one_short")),
    ("ended_out_len_keeps_the_history", _H, "if (r.status == ST_OK) r.out_len = history_out_len(",
     "if (r.status == ST_OK && !r.ended) r.out_len = history_out_len(", ("prefix", "plain-512", "fixed/match_at_0")),
    ("distance_test_strict", "inflate_lane.h", "  if (dist > d.out_pos) { d.fail(ST_CORRUPTED); return SYM_STOP; }  // zd.ml:614",
     "  if (dist >= d.out_pos) { d.fail(ST_CORRUPTED); return SYM_STOP; }  // zd.ml:614", ("history", "plain-512", "fixed/dist_exact/h16_p1")),
    ("history_not_counted_as_written", _H, "  d.out_pos = history_out_pos(hist_len);", "  d.out_pos = 0;", ("size", "plain-512", "fixed/match_at_0")),
    ("room_not_widened", _H, "  d.hard_cap = history_cap(d.hard_cap, hist_len);", "  d.hard_cap = history_cap(d.hard_cap, 0);",
     ("history", "plain-512", "fixed/match_at_0")),
    ("start_bit_dropped", _H, "  d.boff = history_bit(start_bit) & 31u;", "  d.boff = 0;", ("history", "plain-512", "fixed/match_at_0_bit5")),
    ("block_start_left_at_0", _H, "  d.blk_out_start = d.out_pos;", "  d.blk_out_start = 0;",
     ("equivalent", "every block header sets blk_out_start to the position it is read at (inflate_lane.h lane_block_header) before anything "
                    "is summed from it: the line keeps the lane's state whole, as the by-blocks start of inflate_wave does")),
    ("adler_over_the_history", "sim_history.cpp", "d.adler = adler_rfc_update(d.adler, dst + d.blk_out_start, d.out_pos - d.blk_out_start);",
     "d.adler = adler_rfc_update(1u, dst, d.out_pos);", ("history", "plain-512", "fixed/match_at_0")),
    ("hist_len_verdict_removed", _H, "  if (hist_len > HISTORY_MAX_LEN) return ST_INVALID_ARG;\n", "", ("size", "plain-512", "record/hist_len_32769")),
    ("start_bit_verdict_removed", _H, "  if (start_bit > HISTORY_MAX_BIT) return ST_INVALID_ARG;\n", "", ("history", "plain-512", "record/start_bit_8")),
    ("gap_verdict_removed", _H, "  if (has_dst && (uint64_t)hist_len > dst_off) return ST_INVALID_ARG;\n", "",
     ("history", "plain-512", "record/hist_len_above_dst_off")),
    ("gap_verdict_in_the_sizing_form", _H, "  if (has_dst && (uint64_t)hist_len > dst_off) return ST_INVALID_ARG;\n",
     "  if ((uint64_t)hist_len > dst_off) return ST_INVALID_ARG;\n", ("size", "plain-512", "record/hist_len_above_dst_off")),
    ("verdicts_reordered", _H, "  if (hist_len > HISTORY_MAX_LEN) return ST_INVALID_ARG;\n  if (start_bit > HISTORY_MAX_BIT) return ST_INVALID_ARG;\n",
     "  if (start_bit > HISTORY_MAX_BIT) return ST_INVALID_ARG;\n  if (hist_len > HISTORY_MAX_LEN) return ST_INVALID_ARG;\n",
     ("equivalent", "every verdict of a record, and of the descriptor behind it, is the one status ST_INVALID_ARG with no bytes: their order "
                    "cannot be seen in a result (the cases with two faults at once pin that)")),
    ("dictid_little_endian", _Z, "return ((uint32_t)at2[0] << 24) | ((uint32_t)at2[1] << 16) | ((uint32_t)at2[2] << 8) | (uint32_t)at2[3];",
     "return ((uint32_t)at2[3] << 24) | ((uint32_t)at2[2] << 16) | ((uint32_t)at2[1] << 8) | (uint32_t)at2[0];",
     ("zlib", "plain-512", "zlib/mid/rec50_l9_dict")),
    ("body_from_byte_2", _Z, "o.status = ST_OK; o.body_off = 6;", "o.status = ST_OK; o.body_off = 2;", ("zlib", "plain-512", "zlib/mid/rec50_l9_dict")),
    ("body_to_the_trailers_middle", _Z, "o.body_len = len - ZLIB_DICT_MIN_LEN;", "o.body_len = len - ZLIB_DICT_MIN_LEN + 2;",
     ("zlib", "plain-512", "zlib/mid/fdict_two_bytes_short")),
    ("fdict_length_not_tested", _Z, "  if (len < ZLIB_DICT_MIN_LEN) { o.status = ST_CORRUPTED; return o; }\n", "",
     ("zlib", "plain-512", "zlib/mid/fdict_in_9_bytes")),
    ("dictid_not_reported", _Z, "if (dict_len == 0 || dictid != dict_adler) { o.dictid = dictid; return o; }",
     "if (dict_len == 0 || dictid != dict_adler) { return o; }", ("zlib", "plain-512", "zlib/mid/wrong_dictid")),
    ("no_dictionary_not_tested", _Z, "if (dict_len == 0 || dictid != dict_adler) {", "if (dictid != dict_adler) {",
     ("equivalent", "without a dictionary the comparison is with 0, the open kernel's and the model's stand-in: only a stream that asks "
                    "for DICTID 0, which is no Adler-32 of anything, would pass -- and decode with no history, as one without FDICT")),
    ("dictionary_adler_in_the_other_flavour", "sim_history.cpp", "adler_chunk_step(s1, s2, n, S1, S2, true);", "adler_chunk_step(s1, s2, n, S1, S2, false);",
     ("zlib", "plain-512", "zlib/big/rec50_l9_dict")),
    ("gap_seeded_without_fdict", _Z, "o.body_len = zlib_body_len(len); return o; }", "o.body_len = zlib_body_len(len); o.hist_len = (uint32_t)dict_len; return o; }",
     ("zlib", "plain-512", "zlib/mid/rec50_l9_plain")),
    ("gap_seeded_over_the_arenas_start", _Z, "return pre == ST_OK && hist_len != 0 && dst_off >= hist_len; }", "return pre == ST_OK && hist_len != 0; }",
     ("zlib", "plain-512", "zlib/mid/rec50_l9_dict")),
    ("dictid_dropped_at_the_close", _Z, "if (pre == ST_ZLIB_DICT) { inner.status = pre; inner.checksum = expect;", "if (pre == ST_ZLIB_DICT) { inner.status = pre; inner.checksum = 0;",
     ("zlib", "plain-512", "zlib/none/fdict_without_a_dictionary")),
]

_CHILD = r"""
import json, os, sys
root, so, mode, form, names = sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4], sys.argv[5].split("|")
sys.path.insert(0, os.path.join(root, "tests")); sys.path.insert(0, root)
import inflate_history_cases as HC
import test_inflate_history_rules as T
sim = T.bind(so)
if names == ["all"]:
    bad = T.failures(sim, T.laid_out(), ["plain-512"]) + T.zlib_failures(sim, HC.zcases())
elif mode == "zlib":
    bad = T.zlib_failures(sim, [z for z in HC.zcases() if z.name in names], [form])
else:
    bad = T.failures(sim, [lc for lc in T.laid_out() if lc[0].name in names], [form], [T.MODES[mode]])
print(json.dumps(sorted({b[0] for b in bad})))
"""


def mutant_model(m, into):
    """the model over a copy of zipc_amd/csrc (and of itself) with one text changed -> its shared library"""
    name, fname, old, new = m[:4]
    csrc, sim_dir = os.path.join(str(into), "zipc_amd", "csrc"), os.path.join(str(into), "tests", "history_sim")
    shutil.copytree(os.path.join(ROOT, "zipc_amd", "csrc"), csrc, ignore=shutil.ignore_patterns("build", "*.hip"))
    os.makedirs(sim_dir)
    shutil.copy(SIM_CPP, sim_dir)
    path = os.path.join(sim_dir if fname == "sim_history.cpp" else csrc, fname)
    text = mutation.patched(open(path).read(), old, new, name)
    with open(path, "w") as f:
        f.write(text)
    return mutation.gxx(os.path.join(sim_dir, "libhistory_sim.so"), [os.path.join(sim_dir, "sim_history.cpp")], include=[HOST_SIM_DIR],
                        extra=["-Wno-unknown-pragmas"])


def test_history_mutants_are_killed(tmp_path, capsys):
    import concurrent.futures

    known = {c.name for c in HC.cases()} | {z.name for z in HC.zcases()}
    sos = mutation.build_all(lambda m: mutant_model(m, tmp_path / m[0]), HISTORY_MUTANTS)
    with concurrent.futures.ThreadPoolExecutor(max_workers=mutation.workers()) as ex:
        jobs = []
        for m, so in zip(HISTORY_MUTANTS, sos):
            killer = m[4]
            if killer[0] == "equivalent":
                jobs.append(ex.submit(mutation.run_child, _CHILD, ROOT, so, "history", "plain-512", "all"))
            else:
                assert killer[2] in known, (m[0], killer[2])
                jobs.append(ex.submit(mutation.run_child, _CHILD, ROOT, so, killer[0], killer[1], killer[2]))
        rows = []
        for m, job in zip(HISTORY_MUTANTS, jobs):
            rc, failed, err = job.result()
            killer = m[4]
            crashed = rc != 0 or failed is None
            ok = mutation.verdict(killer if killer[0] == "equivalent" else killer[2], failed or [], crashed)
            rows.append((m[0], "equivalent" if killer[0] == "equivalent" else killer[2], len(failed or []), crashed, ok, err[-300:] if crashed else ""))
    with capsys.disabled():
        print("\nhistory mutants in the host model")
        for name, killer, n, crashed, ok, _ in rows:
            print("  %-40s %4d cases fail%s  %s %s" % (name, n, " (child crashed)" if crashed else "", killer, "" if ok else "-- NOT AS EXPECTED"))
    assert all(r[4] and not r[3] for r in rows), [r for r in rows if not r[4] or r[3]]


def test_the_unmutated_model_fails_none_of_the_killers(sim):
    names = {m[4][2] for m in HISTORY_MUTANTS if m[4][0] != "equivalent"}
    assert not failures(sim, [lc for lc in laid_out() if lc[0].name in names], sorted(FORMS))
    assert not zlib_failures(sim, [z for z in HC.zcases() if z.name in names], sorted(FORMS))


# ---- the audit program ----------------------------------------------------------------------------------------------

def test_audit_program_under_the_address_sanitizer(tmp_path):
    """the model as a stand-alone program with its own main, built with -fsanitize=address,undefined and run as a process over
    every case whose record and descriptor are accepted, in four forms and three modes: every [history | room] a heap block
    of exactly hist_len + dst_cap bytes and every source one of exactly src_len, so a load in front of the history, a store
    behind the room or a read past the input trips the sanitizer; it aborts on any result or byte that differs"""
    cases = [c for c in HC.cases() if c.status != HC.INVALID_ARG]
    blob = [struct.pack("<I", len(cases))]
    for c in cases:
        blob.append(struct.pack("<6I", len(c.raw), len(c.hist), c.start_bit, c.cap, int(c.limit is not None), c.limit or 0))
        for mode in (REAL, PREFIX, SIZE):
            want, plain = want_of(c, mode, 1)
            blob.append(struct.pack("<4I", want[0], want[1], want[2], int(plain is not None)))
        blob += [c.raw, c.hist, struct.pack("<I", len(c.plain or b"")), c.plain or b""]
    path = tmp_path / "cases.bin"
    path.write_bytes(b"".join(blob))
    exe = str(tmp_path / "history_audit")
    mutation.gxx(exe, [os.path.join(HERE, "history_sim", "audit_main.cpp")], shared=False, include=[HOST_SIM_DIR],
                 extra=["-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert b"nothing outside a block" in r.stdout and ("%d cases" % len(cases)).encode() in r.stdout
