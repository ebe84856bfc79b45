"""Inputs for the steady form of lz_match's first walk (deflate_lane.h lz_match_runs_pool, zipc_amd/csrc/match_pool.h):
streams of 4-bit symbols -- the data the first form is chosen for -- at the smallest lengths where that loop's entry, its
handouts and its exit can go wrong.  No GPU, no library: tests/test_match_pool_form.py walks them through a model of the
pool, tests/test_gpu_match_steady.py holds the kernel's records of them to the reference.

A wave's loop is steady while every position of its chunk of 256 is 258 or more from the stream's end: the last steady
chunk ends at the largest multiple of 256 (counted from its tile's start) that is at most len - 257.  A tile's positions
end at len - 3."""
import numpy as np

import match_cases as mc

T0 = mc.T0          # positions of a stream's first tile
CHUNK = 256         # match_pool.h POOL_CHUNK
MAXLEN = mc.MAXLEN


def lengths():
    out = []
    # the steady bound falls on a chunk edge (d = 0), a byte before and behind it; j chunks are steady: fewer than the 16 waves,
    # one a wave, one wave gets two, two each
    out += [CHUNK * j + 257 + d for j in (1, 2, 16, 17, 32, 33) for d in (-1, 0, 1)]
    # the same behind the first tile
    out += [T0 + CHUNK * j + 257 + d for j in (0, 1, 16, 17) for d in (-1, 0, 1)]
    # the tile's last chunk holds 256, 1 or 255 positions
    out += [CHUNK * j + 3 + e for j in (2, 17) for e in (0, 1, 255)]
    # a second tile of one or two positions; never steady; the benchmark's length
    out += [T0 + 3, T0 + 4, 300, 65536]
    return out


def symbols(n, seed):
    return np.random.default_rng(seed).integers(0, 16, n, dtype=np.uint8).tobytes()


def streams():
    """-> [match_cases.Stream]: one of every length, and two with planted walks, cut to lengths whose planted part lies in
    steady chunks"""
    out = [mc.Stream("sym4_%d" % n, symbols(n, 1000 + n)) for n in lengths()]
    # a run of one byte: l == 258 ends a walk at its first candidate, inside the steady loop
    d, props = bytearray(symbols(CHUNK * 40 + 257, 7)), []
    mc._periodic(d, props, 1, 2000, 4000, 0xAA)
    out.append(mc.Stream("run_of_one_byte", d, props))
    # chains of Kq, Kq + 1, K and K + 1 candidates for `Fast and `Default: K and K / 4 are reached inside the steady loop
    d, props = bytearray(symbols(CHUNK * 80 + 257, 8)), []
    end = mc._k_low(d, props, 1000)
    assert end + MAXLEN <= CHUNK * 79
    out.append(mc.Stream("k_groups", d, props))
    return out


def tiles(n):
    """[(first position, one past the last)] of the tiles of a stream of n bytes, as lz_match_window_kernel cuts it"""
    out, t = [], 0
    while t < n - 3:
        t1 = T0 if t == 0 else t + mc.TILE
        out.append((t, min(t1, n - 3)))
        t = t1
    return out


def steady_chunks(n):
    """the chunks [lo, hi) of a stream of n bytes in which a wave may be steady, by the arithmetic of the docstring"""
    return [(lo, lo + CHUNK) for t0, t1 in tiles(n) for lo in range(t0, t1, CHUNK) if lo + CHUNK <= t1 and lo + CHUNK - 1 + MAXLEN <= n]
