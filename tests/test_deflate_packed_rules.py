"""zipc_amd/csrc/deflate_packed.h -- the rules of the packed encode forms (zipc_hip_deflate_packed_batch), one header for the
kernels of deflate_packed.hip, their launcher, the bound helpers and this test -- compiled with g++ into a host model
(tests/deflate_packed_sim/sim_deflate_packed.cpp) that runs the stage's and the layout's tiles and waves as loops and the copy
per (workgroup, thread) over real byte arrays, with every index checked before it is used and every destination byte's
writers recorded.  The expected values are the few lines of `expect` below, not the header; a mutation table over the
header (and over the two functions of packed_layout.h it takes the layout rule from); the same model as a stand-alone
program under the address sanitizer (audit_main.cpp).  No GPU; the kernels are checked in tests/test_gpu_deflate_packed.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mutation
import util  # noqa: F401  (sets sys.path through conftest)

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "deflate_packed_sim")
SIM = os.path.join(SIM_DIR, "sim_deflate_packed.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "zipc_amd", "csrc")
HEADER = os.path.join(CSRC, "deflate_packed.h")
LAYOUT_HEADER = os.path.join(CSRC, "packed_layout.h")
DESC = np.dtype([("src_off", "<u8"), ("src_len", "<u8"), ("dst_off", "<u8"), ("dst_cap", "<u8"), ("limit", "<u8"), ("flags", "<u4"),
                 ("reserved", "<u4")])
RESULT = np.dtype([("status", "<u4"), ("checksum", "<u4"), ("out_len", "<u8")])
VERDICT = np.dtype([("status", "<u4"), ("roomed", "<u4"), ("dst_off", "<u8")])
PACKED = np.dtype([("status", "<u4"), ("checksum", "<u4"), ("out_len", "<u8"), ("dst_off", "<u8"), ("reserved", "<u8")])
OK, DST_TOO_SMALL, HIP, INVALID_ARG = 0, 16, 17, 18
CRC_NOP, CRC_CRC32, CRC_ADLER32, CRC_ADLER32_RFC = 0, 1, 2, 3
MAX_STREAM_LEN = 0xFFFF0000
ALIGNS = (1, 2, 16, 4096)
SEG = 32768
GUARD = 4096
POISON = 0xEE
# (zlib, crc_op, the arena's address modulo 16)
FLAVOURS = ((0, CRC_NOP, 0), (0, CRC_CRC32, 5), (1, CRC_ADLER32, 11))


FLAGS = dict(include=[CSRC], extra=["-Wall", "-Wno-unknown-pragmas"])


def _bind(so):
    L = C.CDLL(so)
    u64, u32, p = C.c_uint64, C.c_uint32, C.c_void_p
    L.sim_dpacked_run.restype = u64
    L.sim_dpacked_run.argtypes = [p, p, u32, u64, u64, C.c_int, C.c_int, u64, u64, u32, p, u64, p, p, p, p, p, p, p, p, p]
    L.sim_dpacked_call_status.restype = u32
    L.sim_dpacked_call_status.argtypes = [C.c_int, u64, u64, u64, u64, C.c_int, C.c_int, u64, C.c_int]
    for name, args in (("slot_bytes", [u64, C.c_int]), ("arena_bound", [u64, u64, u64, C.c_int]), ("staging_bound", [u64, u64, C.c_int]),
                       ("copy_grid", [u64, u64, C.c_int]), ("slot_align", [])):
        f = getattr(L, "sim_dpacked_" + name)
        f.restype, f.argtypes = u64, args
    L.sim_dpacked_tile.restype = L.sim_dpacked_wave.restype = L.sim_dpacked_seg_bytes.restype = u32
    L.sim_dpacked_staged_byte.restype, L.sim_dpacked_staged_byte.argtypes = C.c_uint8, [u64, u64]
    return L


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return _bind(mutation.gxx(tmp_path_factory.mktemp("deflate_packed_sim") / "libdeflate_packed_sim.so", [SIM], **FLAGS))


def bound(src_len, zlib):
    """zipc_hip_deflate_bound / zipc_hip_zlib_bound, as include/zipc_hip.h states them"""
    return src_len + 6 * (src_len // 65534 + 1) + 8 + (6 if zlib else 0)


def _descs(src_lens):
    n = len(src_lens)
    d = np.zeros(max(n, 1), DESC)
    d["src_off"][:n] = np.arange(n, dtype=np.uint64) * 100
    d["src_len"][:n] = np.array(src_lens, dtype=np.uint64)
    d["dst_off"], d["dst_cap"] = 0xDEAD, 0xBEEF  # (not to be looked at)
    d["flags"][:n] = np.arange(n, dtype=np.uint32) % 2
    return d


def staged_bytes(i, n):
    """the stub's deflate output of stream i (sim_deflate_packed.cpp staged_byte)"""
    j = np.arange(n, dtype=np.uint64)
    return ((np.uint64(i) * np.uint64(167) + j * np.uint64(13) + (j >> np.uint64(8)) + np.uint64(1)) & np.uint64(0xFF)).astype(np.uint8)


def run(L, case, flavour, align, arena, declared=None):
    """-> dict of everything the model says"""
    src_lens, would = case
    zlib, crc_op, base_mis = flavour
    n = len(src_lens)
    m = max(n, 1)
    in_range = [l for l in src_lens if l <= MAX_STREAM_LEN]
    max_src, total = declared if declared else (max(in_range, default=0), sum(in_range))
    descs = _descs(src_lens)
    w = np.zeros(m, RESULT)
    for i, (st, ol, ck) in enumerate(would):
        w[i] = (st, ck, ol + (6 if zlib and st == OK else 0))
    alloc = arena + GUARD
    dst, written, owner = np.full(alloc, POISON, np.uint8), np.zeros(alloc, np.uint8), np.zeros(alloc, np.uint32)
    inner, stage, verdicts = np.zeros(m, DESC), np.full(m, 0xEEEE, np.uint32), np.full(m, 0xEE, "u1").repeat(16).view(VERDICT)
    seg_base, results = np.full(m, 0xEEEE, np.uint32), np.zeros(m, PACKED)
    need, stats = np.full(1, 0xEEEE, np.uint64), np.zeros(12, np.uint64)
    L.sim_dpacked_run(descs.ctypes.data, w.ctypes.data, n, max_src, total, zlib, crc_op, align, arena, base_mis, dst.ctypes.data, alloc,
                      written.ctypes.data, owner.ctypes.data, inner.ctypes.data, stage.ctypes.data, verdicts.ctypes.data,
                      seg_base.ctypes.data, results.ctypes.data, need.ctypes.data, stats.ctypes.data)
    return dict(dst=dst, written=written, owner=owner, inner=inner[:n], stage=stage[:n], verdicts=verdicts[:n], seg_base=seg_base[:n],
                results=results[:n], need=int(need[0]), stats=tuple(int(v) for v in stats), descs=descs[:n], would=w[:n])


def expect(case, flavour, align, arena, declared=None):
    """the rule of include/zipc_hip.h, serially: per stream (status, checksum, out_len, dst_off), its slot offset (None: it
    has none), and need"""
    src_lens, would = case
    zlib, crc_op, _ = flavour
    in_range = [l for l in src_lens if l <= MAX_STREAM_LEN]
    max_src, total = declared if declared else (max(in_range, default=0), sum(in_range))
    bad = any(l > max_src for l in in_range) or sum(in_range) > total
    off = need = slot = 0
    out, slots = [], []
    for l, (st, ol, ck) in zip(src_lens, would):
        if bad or l > MAX_STREAM_LEN:
            out.append((INVALID_ARG, 0, 0, 0))
            slots.append(None)
            continue
        slots.append(slot)
        slot += (bound(l, zlib) + 15) // 16 * 16
        if st != OK:
            out.append((st, ck, 0, 0))
            continue
        ol += 6 if zlib else 0
        if off + ol <= arena:
            out.append((OK, ck, ol, off))
        else:
            out.append((DST_TOO_SMALL, ck if crc_op == CRC_CRC32 else 0, 0, off))
        need = off + ol
        off += (ol + align - 1) // align * align
    return out, slots, need, bad


def _stored(out_lens):
    """streams whose output length is known: ZIPC_HIP_LEVEL_NONE's len + 5 below 65 535 bytes of source, + 10 from there"""
    return [ol - 5 if ol - 5 < 65535 else ol - 10 for ol in out_lens], [(OK, ol, 0xC0DE0000 + i) for i, ol in enumerate(out_lens)]


def _pattern(n, seed, bad_every=7):
    """n tiny streams: sources of 0..40 bytes in a fixed pseudo-random pattern that deflate to a little less or more, every
    bad_every-th refused by deflate itself"""
    x, lens, would = seed, [], []
    for i in range(n):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        l = (x >> 8) % 41
        lens.append(l)
        would.append((HIP, 0, 0) if i % bad_every == bad_every - 1 else (OK, 2 + (x >> 16) % (l + 12), 0x1000 + i))
    return lens, would


# every residue of dst_off modulo 16 at align 1, two streams in one 16-byte unit (5 and 15), the named lengths around a
# unit and around a segment, an exact multiple of the segment, two segments and five bytes
EXACT = [5, 15, 16, 17, 31, 33] + [17] * 16 + [32767, 32768, 32769, 2 * 32768 + 5, 3 * 32768, 7]
_L, _W = _stored([40, 9, 300, 5, 64, 33000, 21])
MIXED = (_L, [_W[0], (DST_TOO_SMALL, 0, 0xCCCC0001), _W[2], (INVALID_ARG, 0, 0), (HIP, 0, 0), _W[5], _W[6]])
_L, _W = _stored([40, 9, 300, 5, 64])
TOO_LONG = (_L[:2] + [MAX_STREAM_LEN + 1] + _L[2:], _W[:2] + [(OK, 77, 0xBAD)] + _W[2:])
# (name, (src_lens, would), arena lengths beside need, need - 1, 0 and the bound)
CASES = [
    ("exact lengths", _stored(EXACT), (40, 5 + 15 + 16 + 9, 70000)),
    ("mixed verdicts", MIXED, (339, 340)),
    ("a descriptor beyond the format's range in the middle", TOO_LONG, (60,)),
    ("nothing takes room", ([3, 4], [(HIP, 0, 0), (DST_TOO_SMALL, 0, 5)]), (100,)),
    ("one stream", _stored([17]), ()),
    ("one empty stream", _stored([5]), ()),
    ("no stream", ([], []), (5,)),
] + [("n = %d" % n, _pattern(n, n), ()) for n in (63, 64, 65, 1023, 1024, 1025, 2049)] + [
    ("a wave and a tile of streams without room at the end", (lambda a, b: (a[0] + [1] * 1100 + b[0], a[1] + [(HIP, 0, 0)] * 1100 + b[1]))(
        _pattern(70, 3), _stored([50, 51, 52])), ()),
]


def _arenas(case, flavour, align, extra):
    need = expect(case, flavour, align, 0)[2]
    n, total = len(case[0]), sum(l for l in case[0] if l <= MAX_STREAM_LEN)
    full = total + 6 * (total // 65534) + 14 * n + (align - 1) * n + (6 * n if flavour[0] else 0)  # the bound helpers' formula
    return [a for a in dict.fromkeys((need, need - 1, 0, need // 2, full) + tuple(extra)) if a >= 0], full


def _check(L, name, case, flavour, align, arena, declared=None):
    src_lens, _ = case
    zlib, crc_op, base_mis = flavour
    n = len(src_lens)
    want, slots, need, bad = expect(case, flavour, align, arena, declared)
    got = run(L, case, flavour, align, arena, declared)
    what = (name, flavour, align, arena, declared)
    st = got["stats"]
    assert st[0] == 0 and st[1] == 0 and st[2] == 0, what  # no index left its array, no vector store off its boundary, no byte twice
    assert got["need"] == need, what
    if n == 0:
        assert st[3:6] == (0, 0, 0) and not got["written"].any(), what
        return need
    assert st[4] == int(bad) and st[10] == (n + 1023) // 1024, what
    assert st[5] == sum(s is not None for s in slots), what
    dst = np.full(arena + GUARD, POISON, np.uint8)
    mask = np.zeros(arena + GUARD, np.uint8)
    segs, prev_owner = 0, 0
    for i, (w, slot) in enumerate(zip(want, slots)):
        r, d = got["results"][i], got["inner"][i]
        assert (int(r["status"]), int(r["checksum"]), int(r["out_len"]), int(r["dst_off"]), int(r["reserved"])) == w + (0,), (what, i)
        if slot is None:
            assert (int(d["src_len"]), int(d["dst_cap"]), int(d["flags"])) == (0, 0, 0), (what, i)
        else:
            assert slot % 16 == 0 and (int(d["src_off"]), int(d["src_len"]), int(d["dst_off"]), int(d["dst_cap"]), int(d["flags"])) == \
                (i * 100, src_lens[i], slot, bound(src_lens[i], zlib), i % 2), (what, i)
        if w[0] == OK:
            off, ol = w[3], w[2]
            assert off % align == 0 and off + ol <= arena, (what, i)
            dst[off:off + ol] = staged_bytes(i, ol)
            mask[off:off + ol] = 1
            for k in range(0, ol, SEG):  # a segment's bytes: one workgroup's, the workgroups in the order of the segments
                own = got["owner"][off + k:off + min(k + SEG, ol)]
                assert own.min() == own.max() == int(got["seg_base"][i]) + k // SEG + 1 > prev_owner, (what, i, k)
                prev_owner = int(own[0])
            segs += (ol + SEG - 1) // SEG
    assert st[3] == segs == st[11], what
    assert np.array_equal(got["written"], mask), what  # every byte of a fitting stream once, no other byte at all
    assert np.array_equal(got["dst"], dst), what
    # the suffix property: the roomed streams that do not fit are those from the first one that does not fit onwards
    roomed = [w for (w, (s, _, _)) in zip(want, case[1]) if s == OK and w[0] in (OK, DST_TOO_SMALL)]
    fits = [w[0] == OK for w in roomed]
    assert fits == sorted(fits, reverse=True), what
    assert [w[3] for w in roomed] == sorted(w[3] for w in roomed), what
    return need


def test_constants_and_bounds(sim):
    assert (sim.sim_dpacked_tile(), sim.sim_dpacked_wave(), sim.sim_dpacked_seg_bytes(), sim.sim_dpacked_slot_align()) == (1024, 64, 32768, 16)
    for l in (0, 1, 65533, 65534, 65535, 2 * 65534 - 1, 2 * 65534, 1 << 20, MAX_STREAM_LEN):
        assert sim.sim_dpacked_slot_bytes(l, 0) == bound(l, 0) and sim.sim_dpacked_slot_bytes(l, 1) == bound(l, 1) == bound(l, 0) + 6
    for n, total in ((1, 0), (1, 65534), (3, 3 * 65534 - 1), (1000, 12345678), (1 << 20, 1 << 36)):
        for align in (1, 2, 16, 4096):
            want = total + 6 * (total // 65534) + 14 * n + (align - 1) * n
            assert sim.sim_dpacked_arena_bound(n, total, align, 0) == want and sim.sim_dpacked_arena_bound(n, total, align, 1) == want + 6 * n
        assert sim.sim_dpacked_staging_bound(n, total, 0) == total + 6 * (total // 65534) + 29 * n
        assert sim.sim_dpacked_copy_grid(n, total, 1) == (total + 6 * (total // 65534) + 35 * n) // 32768 + n
    # the bound covers n slots, each padded, however the total is spread: equal streams, one long and the rest empty
    for n, each in ((7, 65534), (7, 65533), (5, 100), (3, 0)):
        for zlib in (0, 1):
            for lens in ([each] * n, [each * n] + [0] * (n - 1)):
                for align in (1, 16, 4096):
                    assert sum((bound(l, zlib) + align - 1) // align * align for l in lens) <= sim.sim_dpacked_arena_bound(n, each * n, align, zlib)


def test_call_rules(sim):
    ok = dict(dst_null=0, arena=100, n=5, max_src=1000, total=5000, level=2, crc_op=0, align=16, zlib=0)

    def st(**kw):
        a = dict(ok, **kw)
        return sim.sim_dpacked_call_status(a["dst_null"], a["arena"], a["n"], a["max_src"], a["total"], a["level"], a["crc_op"], a["align"], a["zlib"])

    assert st() == OK
    assert st(dst_null=1) == INVALID_ARG and st(dst_null=1, arena=0) == OK
    assert st(n=0x7FFFFFFF, total=0) == INVALID_ARG and st(n=0x80000000) == INVALID_ARG  # (the former: its copy grid is above the limit)
    assert st(n=1 << 30, total=0) == OK
    for a in range(0, 8200):
        assert st(align=a) == (OK if a in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096) else INVALID_ARG), a
    assert st(align=1 << 13) == INVALID_ARG and st(align=1 << 63) == INVALID_ARG
    assert st(max_src=MAX_STREAM_LEN) == OK and st(max_src=MAX_STREAM_LEN + 1) == INVALID_ARG
    assert [st(crc_op=c) for c in (-1, 0, 1, 2, 3, 4)] == [INVALID_ARG, OK, OK, OK, OK, INVALID_ARG]
    assert [st(level=v) for v in (-1, 0, 1, 2, 3, 4)] == [INVALID_ARG, OK, OK, OK, OK, INVALID_ARG]
    # the copy's grid bound: staging bytes / 32 KiB + n_streams at most 0x7FFFFFFF
    lo, hi = 0, 1 << 48
    while lo < hi:  # the largest total whose grid is allowed, by bisection over the model's own bound
        mid = (lo + hi + 1) // 2
        if sim.sim_dpacked_copy_grid(5, mid, 0) <= 0x7FFFFFFF:
            lo = mid
        else:
            hi = mid - 1
    assert (lo + 6 * (lo // 65534) + 29 * 5) // 32768 + 5 == 0x7FFFFFFF
    assert st(total=lo) == OK and st(total=lo + 1) == INVALID_ARG and st(total=1 << 63) == INVALID_ARG and st(total=(1 << 64) - 1) == INVALID_ARG


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_model_follows_the_rule(sim, name):
    """every case, every flavour and align, the arena exactly `need`, one byte short, empty, cut in the middle, the bound and
    more: the slots, the descriptors deflate ran with, the results, `need` and every byte of the arena and of the guard
    behind it are the rule's; no index left its array, no destination byte was written twice or outside a fitting stream"""
    _, case, extra = next(c for c in CASES if c[0] == name)
    for flavour in FLAVOURS:
        for align in ALIGNS:
            arenas, full = _arenas(case, flavour, align, extra)
            needs = {_check(sim, name, case, flavour, align, arena) for arena in arenas}
            assert len(needs) == 1 and needs.pop() <= full, (name, flavour, align, "need depends on the arena, or the bound does not hold")
            assert all(w[0] != DST_TOO_SMALL or s != OK for w, (s, _, _) in zip(expect(case, flavour, align, full)[0], case[1])), (name, "the bound fits")


def test_declared_sizes(sim):
    """max_src_len or total_src_len one too small: every result INVALID_ARG, need 0, no stream reaches deflate, no byte written"""
    for name in ("exact lengths", "mixed verdicts", "a descriptor beyond the format's range in the middle", "n = 1025"):
        _, case, _ = next(c for c in CASES if c[0] == name)
        in_range = [l for l in case[0] if l <= MAX_STREAM_LEN]
        mx, total = max(in_range), sum(in_range)
        for flavour in FLAVOURS:
            for declared, bad in (((mx, total), False), ((mx - 1, total), True), ((mx, total - 1), True), ((mx, total + 1000), False),
                                  ((MAX_STREAM_LEN, total), False), ((0, 0), True)):
                assert expect(case, flavour, 16, 1 << 20, declared)[3] == bad
                _check(sim, name, case, flavour, 16, 1 << 20, declared)
                got = run(sim, case, flavour, 16, 1 << 20, declared)
                if bad:
                    assert got["need"] == 0 and got["stats"][5] == 0 and got["stats"][3] == 0 and not got["written"].any()
                    assert (got["results"]["status"] == INVALID_ARG).all() and not got["results"]["dst_off"].any()


def test_what_the_cases_hold():
    """the cases meet what they are named for"""
    case = dict((c[0], c[1]) for c in CASES)["exact lengths"]
    want = expect(case, FLAVOURS[0], 1, 1 << 20)[0]
    assert {w[3] % 16 for w in want} == set(range(16))                         # every residue of dst_off modulo 16
    assert want[0][3] // 16 == want[1][3] // 16 and want[0][2] == 5            # two streams in one 16-byte unit
    assert {w[2] for w in want} >= {5, 15, 16, 17, 31, 33, 32767, 32768, 32769, 2 * 32768 + 5, 3 * 32768}
    mixed = dict((c[0], c[1]) for c in CASES)["mixed verdicts"]
    assert {w[0] for w in expect(mixed, FLAVOURS[1], 1, 339)[0]} == {OK, DST_TOO_SMALL, HIP, INVALID_ARG}
    short = expect(mixed, FLAVOURS[1], 1, 339)[0]
    assert short[1] == (DST_TOO_SMALL, 0xCCCC0001, 0, 0)                        # deflate's own: no room, its checksum handed on
    assert short[2] == (DST_TOO_SMALL, 0xC0DE0002, 0, 40)                       # the arena's: the offset kept, the CRC-32 of the source
    assert expect(mixed, FLAVOURS[0], 1, 339)[0][2] == (DST_TOO_SMALL, 0, 0, 40)  # ... and 0 with no CRC-32 asked for
    assert expect(mixed, FLAVOURS[1], 1, 340)[0][2] == (OK, 0xC0DE0002, 300, 40)   # ends exactly at dst_arena_len
    long_ = dict((c[0], c[1]) for c in CASES)["a descriptor beyond the format's range in the middle"]
    a, b = expect(long_, FLAVOURS[0], 16, 1 << 20), expect((long_[0][:2] + long_[0][3:], long_[1][:2] + long_[1][3:]), FLAVOURS[0], 16, 1 << 20)
    assert a[0][2] == (INVALID_ARG, 0, 0, 0) and a[0][:2] + a[0][3:] == b[0] and a[2] == b[2]  # the others as if it were absent


# ---- the mutation table: (name, header, the line as it stands, the line mutated) -------------------------------------------
MUTANTS = (
    ("padding the offset instead of the length", LAYOUT_HEADER, "return packed_add(off, packed_align_up(len, align)); }",
     "return packed_add(packed_align_up(off, align), len); }"),
    ("fit by < instead of <=", LAYOUT_HEADER, "return packed_add(off, len) <= dst_arena_len; }", "return packed_add(off, len) < dst_arena_len; }"),
    ("need with padding", HEADER, "{ return packed_end(v.roomed != 0, v.dst_off, out_len); }",
     "{ return packed_end(v.roomed != 0, v.dst_off, packed_align_up(out_len, 16)); }"),
    ("a slot that is not 16-byte aligned", HEADER, "? packed_align_up(dpacked_slot_bytes(src_len, zlib), DPACKED_SLOT_ALIGN) : 0;",
     "? dpacked_slot_bytes(src_len, zlib) : 0;"),
    ("the head one byte long", HEADER, "(DPACKED_UNIT - (uint32_t)((dst_at + s.lo) & (DPACKED_UNIT - 1))) & (DPACKED_UNIT - 1);",
     "(DPACKED_UNIT + 1 - (uint32_t)((dst_at + s.lo) & (DPACKED_UNIT - 1))) & (DPACKED_UNIT - 1);"),
    ("the head one byte short", HEADER, "(DPACKED_UNIT - (uint32_t)((dst_at + s.lo) & (DPACKED_UNIT - 1))) & (DPACKED_UNIT - 1);",
     "(DPACKED_UNIT - 1 - (uint32_t)((dst_at + s.lo) & (DPACKED_UNIT - 1))) & (DPACKED_UNIT - 1);"),
    ("the segment count of an exact multiple", HEADER, "return (len - 1) / DPACKED_SEG_BYTES + 1;", "return len / DPACKED_SEG_BYTES + 1;"),
    ("the declared-size check dropped", HEADER, "return (any_over_max || sum_len > total_src_len) ? 1u : 0u;", "return 0u;"),
    ("only the sum checked, not the longest stream", HEADER, "return (any_over_max || sum_len > total_src_len) ? 1u : 0u;",
     "return sum_len > total_src_len ? 1u : 0u;"),
    ("a stream deflate refused taking room", HEADER, "{ return stage_status == ST_OK && staged.status == ST_OK; }", "{ return stage_status == ST_OK; }"),
    ("a stream that does not fit copied", HEADER, "{ return v.roomed && v.status == ST_OK ? dpacked_segs(out_len) : 0; }",
     "{ return v.roomed ? dpacked_segs(out_len) : 0; }"),
    ("a stream that does not fit forgets its offset", HEADER, "v.dst_off = v.roomed ? off : 0;",
     "v.dst_off = v.roomed && packed_fits(off, staged.out_len, dst_arena_len) ? off : 0;"),
    ("the CRC-32 of a stream that does not fit dropped", HEADER, "{ return crc_op == CRC_CRC32 ? staged_checksum : 0u; }", "{ return 0u; }"),
    ("the tail taken from the head's place", HEADER, "{ return s.head + s.units * DPACKED_UNIT; }", "{ return s.units * DPACKED_UNIT; }"),
    ("a slot of the raw bound under a zlib stream", HEADER, "+ 8 + (zlib ? ZLIB_OVERHEAD : 0); }", "+ 8; }"),
    ("a descriptor beyond the format's range given a slot", HEADER, "ZD_HD bool dpacked_in_range(uint64_t src_len) { return src_len <= MAX_STREAM_LEN; }",
     "ZD_HD bool dpacked_in_range(uint64_t src_len) { return true; }"),
)


def _observe(L):
    """everything the model says about every case at every align with the arena exactly need, one byte short, empty and cut in
    the middle, and with the declared sizes one too small"""
    out = []
    for name, case, extra in CASES:
        for flavour in FLAVOURS[1:]:
            for align in ALIGNS:
                for arena in _arenas(case, flavour, align, extra)[0][:4]:
                    g = run(L, case, flavour, align, arena)
                    out.append((name, flavour, align, arena) + tuple(g[k].tobytes() for k in ("dst", "written", "inner", "results", "seg_base")) +
                               (g["need"], g["stats"]))
    for name in ("exact lengths", "n = 1025"):
        case = dict((c[0], c[1]) for c in CASES)[name]
        mx, total = max(case[0]), sum(case[0])
        for declared in ((mx - 1, total), (mx, total - 1)):
            g = run(L, case, FLAVOURS[1], 16, 1 << 20, declared)
            out.append((name, declared, g["results"].tobytes(), g["written"].tobytes(), g["need"], g["stats"]))
    return out


def test_mutants_of_the_header_are_killed(sim, tmp_path):
    """each one-line mutant of deflate_packed.h (or of the layout rule it takes from packed_layout.h), built into a model of
    its own, changes what the model says of at least one case: a result, a descriptor, a byte of the arena, need, a byte
    written twice or outside a fitting stream, a vector store off its boundary, an index that left its array"""
    base = _observe(sim)
    assert all(row[-1][0] == 0 and row[-1][1] == 0 and row[-1][2] == 0 for row in base)
    alive = []
    for k, (name, header, line, mutated) in enumerate(MUTANTS):
        # (the mutated header's quoted includes look beside it first: a mutated packed_layout.h lies there under its own name)
        so = mutation.header_model(SIM, "DPACKED_HEADER", header, line, mutated, str(tmp_path / ("mutant%d" % k) / "libmutant.so"),
                                   top=HEADER, **FLAGS)
        if _observe(_bind(so)) == base:
            alive.append(name)
    assert alive == []


def test_audit_program_under_the_address_sanitizer(tmp_path):
    """the model as a stand-alone program with its own main, built with -fsanitize=address,undefined and run as a process:
    the cases' seams and a few thousand random ragged batches; it aborts on any index that leaves its array, any byte
    written twice or outside a fitting stream, and any result or byte that differs from a serial restatement of the rule"""
    exe = str(tmp_path / "deflate_packed_audit")
    mutation.gxx(exe, [os.path.join(SIM_DIR, "audit_main.cpp")], shared=False, include=[CSRC],
                 extra=["-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert b"no index left its array" in r.stdout
