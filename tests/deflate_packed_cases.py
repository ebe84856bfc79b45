"""The inputs of tests/test_gpu_deflate_packed.py: the plain bytes of every batch, made once per process, shared, never
changed.  Nothing here calls the code under test; where a case needs an output of a known length it says how it gets it."""
import functools

import packed_cases as PC
import util

SEG = 32768
# ZIPC_HIP_LEVEL_NONE: a source of len bytes below 65 535 becomes one stored block, len + 5 bytes.  The output lengths the copy
# can go wrong at: around a 16-byte unit, around a 32 KiB segment, two segments exactly (an exact multiple), and, at align 1,
# an order in which dst_off modulo 16 takes every residue (the sixteen streams of 17) and two streams share one 16-byte
# unit (5, then 15)
EXACT_OUT_LENS = (5, 15, 16, 17, 31, 33) + (17,) * 16 + (SEG - 1, SEG, SEG + 1, 2 * SEG, 7)


@functools.lru_cache(maxsize=None)
def exact_lengths():
    """plains for ZIPC_HIP_LEVEL_NONE whose outputs are EXACT_OUT_LENS long"""
    return tuple(util.rand_bytes(ol - 5, 40 + i) if i % 2 else util.text(ol - 5, 40 + i) for i, ol in enumerate(EXACT_OUT_LENS))


# Two segments and five bytes is no length of stored blocks (65 534 bytes of source and fewer give at most 65 539, more give
# 65 545 and up); at `Fast this input -- random bytes no match is found in, then a run -- comes to it: the oracle says so
# where the case is made
TWO_SEGMENTS_AND_FIVE = 2 * SEG + 5


@functools.lru_cache(maxsize=None)
def two_segments_and_five():
    """(plains, level, the index of the stream whose output is TWO_SEGMENTS_AND_FIVE long): that stream between short ones
    of odd lengths"""
    import oracle

    long_ = util.rand_bytes(65530, 11) + b"\0" * 300
    st, s, _ = oracle.deflate(long_, level=1)
    assert st == 0 and len(s) == TWO_SEGMENTS_AND_FIVE
    return (util.text(33, 1), util.rand_bytes(7, 2), long_, util.text(100, 3), b""), 1, 2


@functools.lru_cache(maxsize=None)
def tiny(n=2049):
    """n tiny plains of 0..40 bytes in a fixed pseudo-random pattern"""
    g = PC._lcg(4099)
    return tuple(bytes((next(g) % 7 + 97) for _ in range(next(g) % 41)) for _ in range(n))


@functools.lru_cache(maxsize=None)
def mixed():
    """the mixed inputs of tests/packed_cases.py: about 200 ragged plains of 1 B .. 70 KiB -- text, random bytes, runs, bytes
    above 0x7F"""
    return tuple(it.plain for it in PC.ragged_batch())


LONG_RUNS_LEN = 300 << 10


@functools.lru_cache(maxsize=None)
def long_runs_among_short():
    """one stream of 300 KiB of runs -- long enough for deflate to parse it by segments -- among short ones"""
    runs = b"".join(bytes([65 + k % 26]) * (50 + 37 * (k % 11)) for k in range(4000))[:LONG_RUNS_LEN]
    assert len(runs) == LONG_RUNS_LEN
    shorts = [util.text(200 + 97 * i, 100 + i) for i in range(12)]
    return tuple(shorts[:5] + [runs] + shorts[5:])
