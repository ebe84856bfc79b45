"""Inputs of the ragged checksum pass (zipc_hip_checksum_batch), shared by tests/test_checksum_ranges_rules.py (CPU: the
host model of zipc_amd/csrc/checksum_ranges.h) and tests/test_gpu_checksum_batch.py (the kernels): the smallest batches
at which each seam of the pass exists.  numpy only.

A case is an arena (uint8 array), its ranges [(off, len)], the total the call declares, and the indices of the ranges
that must report INVALID_ARG.  Cases are built once per process (case(name)) and must not be written to."""
import numpy as np

import checksum_cases as CC

SEG = 32768            # a workgroup's segment
CHUNK = CC.N           # 5552
PLAN_TILE = 1024       # ranges checksum_plan scans at a time (checksum_ranges.h RANGES_PLAN_TILE)
HORNER_MAX = 16        # segments one lane folds (adler_chain.h CRC_FINISH_HORNER_MAX)
FINISH_LANES = 64      # columns of the finish beyond that (checksum_ranges.h RANGES_FINISH_LANES)
INVALID_ARG = 18
OFFSETS = (3, 21)      # where ranges start within 32 bytes: never a multiple of 16

# lengths on both sides of a 16-byte unit, an Adler chunk, a segment, and of the finish's thresholds:
FINISH_THRESHOLDS = {
    "one lane | columns": (HORNER_MAX * SEG, HORNER_MAX * SEG + 1),         # 16 | 17 segments
    "one row | two rows": (FINISH_LANES * SEG, FINISH_LANES * SEG + 1),     # 64 | 65 segments
}
LENGTHS = (0, 1, 15, 16, 17, 5551, 5552, 5553, 32767, 32768, 32769, 16 * SEG - 1, 16 * SEG + 1) + tuple(
    n for pair in FINISH_THRESHOLDS.values() for n in pair)
LONG = 17 * (1 << 20) + 4321   # "about 17 MiB": 545 segments, 9 rows of the finish


def finish_shape(length):
    """(nseg, by one lane, rows) of crc32_finish_ranges for a range, restated"""
    nseg = -(-length // SEG)
    if nseg <= HORNER_MAX:
        return nseg, True, 0
    return nseg, False, -(-nseg // FINISH_LANES)


def _layout(lengths, start=0):
    """ranges of those lengths one behind the other, each starting 3 or 21 bytes behind a multiple of 32, with a gap"""
    ranges, at = [], start
    for k, n in enumerate(lengths):
        at = (at + 31) // 32 * 32 + OFFSETS[k % 2]
        ranges.append((at, n))
        at += n + 5
    return ranges, at


def _fill(kind, n, seed):
    if kind == "ff":
        return np.full(n, 0xFF, np.uint8)
    if kind == "zero":
        return np.zeros(n, np.uint8)
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _case(arena, ranges, bad=(), total=None):
    ok_sum = sum(n for i, (_, n) in enumerate(ranges) if i not in bad)
    arena.setflags(write=False)
    return dict(arena=arena, ranges=ranges, bad=tuple(bad), total=ok_sum if total is None else total)


def _lengths_case(kind, seed):
    ranges, end = _layout(LENGTHS)
    return _case(_fill(kind, end + 7, seed), ranges)


def _small_batch(n, seed):
    rng = np.random.default_rng(seed)
    ranges, end = _layout(rng.integers(0, 301, n).tolist())
    return _case(_fill("rand", end + 1, seed + 1), ranges)


def _ragged(where, seed=77):
    """one range of about 17 MiB first, in the middle or last among 1000 ranges of 1 to 3000 bytes"""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(1, 3001, 1000).tolist()
    lengths.insert({"first": 0, "middle": 500, "last": 1000}[where], LONG)
    ranges, end = _layout(lengths)
    return _case(_fill("rand", end + 3, seed + 1), ranges)


def _shapes():
    """the same range twice, overlapping ranges, empty ranges between full ones, two bad ranges among good ones (one
    past the arena by a byte, one whose end overflows), a range that ends exactly with the arena"""
    arena = _fill("rand", 100003, 5)
    A = len(arena)
    ranges = [(3, 40000), (3, 40000), (21, 70000), (30021, 33000), (50, 0), (A - 7000, 7000), (A, 0), (A - 6999, 7000),
              (77, 5553), (2 ** 64 - 10, 11), (0, 0), (A - 1, 1)]
    return _case(arena, ranges, bad=(7, 9))


_BUILDERS = {
    "lengths_rand": lambda: _lengths_case("rand", 11),
    "lengths_ff": lambda: _lengths_case("ff", 0),      # the signed remainder bites from 6 KB of 0xFF on
    "lengths_zero": lambda: _lengths_case("zero", 0),
    "p600": lambda: _case(np.concatenate([np.zeros(3, np.uint8), CC.plan("p600").data]), [(3, CC.plan("p600").length)]),
    "n1": lambda: _case(_fill("rand", 1100, 3), [(21, 1000)]),
    "shapes": _shapes,
    "ragged_first": lambda: _ragged("first"),
    "ragged_middle": lambda: _ragged("middle"),
    "ragged_last": lambda: _ragged("last"),
}
for _k, _n in enumerate((PLAN_TILE - 1, PLAN_TILE, PLAN_TILE + 1, 2 * PLAN_TILE - 1, 2 * PLAN_TILE, 2 * PLAN_TILE + 1)):
    _BUILDERS["n%d" % _n] = (lambda n, k: lambda: _small_batch(n, 100 + k))(_n, _k)

NAMES = tuple(_BUILDERS)
SMALL = tuple(n for n in NAMES if not n.startswith(("ragged", "lengths", "p600")))  # cheap enough for every mutant
MAX_ARENA = 48 << 20
_cases = {}


def case(name):
    if name not in _cases:
        c = _BUILDERS[name]()
        assert len(c["arena"]) <= MAX_ARENA
        _cases[name] = c
    return _cases[name]


def ranges_array(ranges):
    """zipc_hip_range records"""
    a = np.zeros(len(ranges), dtype=np.dtype([("off", "<u8"), ("len", "<u8")]))
    a["off"] = [r[0] for r in ranges]
    a["len"] = [r[1] for r in ranges]
    return a


_refs = {}


def reference(name, oracle):
    """[(crc32, adler32 of the reference, adler32 of RFC 1950)] per range of a case, (0, 0, 0) for a bad one: the
    oracle's values, computed once per distinct (off, len) and held against zlib's"""
    import zlib

    if name not in _refs:
        c, seen, out = case(name), {}, []
        for i, (off, n) in enumerate(c["ranges"]):
            if i in c["bad"]:
                out.append((0, 0, 0))
                continue
            if (off, n) not in seen:
                b = c["arena"][off:off + n]
                crc = oracle.crc32(b)
                assert crc == zlib.crc32(b)
                seen[(off, n)] = (crc, oracle.adler32(b), zlib.adler32(b))
            out.append(seen[(off, n)])
        _refs[name] = out
    return _refs[name]
