"""The span decoder's steps (zipc_amd/csrc/inflate_span.h: span_walk_loop, the decode loop of span_decode, span_advance)
through the C ABI batch form on the MI355X: bytes, lengths, status and CRC-32 of every stream against the oracle, against
the plain bytes as built where the stream was assembled here, and against zlib.decompress where zlib made it.  Every
destination is exactly as large as its output: nothing a step reads or writes has slack behind it.

Each case is one call of 64 to 256 streams (inflate_batch_few_kernel); test_mixed_batch puts all of them and sixteen
64 KiB streams of the benchmark's symbols into one call of more than 256 streams (inflate_batch_kernel), slow and fast
lanes side by side.  A span needs eight regions of four granules, 1 KiB of input, so no stream is smaller than 16 KiB
of output.  What is aimed at:

  literals only   every lane of every step holds a literal or two: zlib's Z_HUFFMAN_ONLY over 16 symbols (4-bit codes
                  and skewed ones: two literals per table entry, odd counts at a granule's and a tile's end -- the
                  lengths are odd and all different) and over 200 symbols (8-bit codes: one literal per entry).
  fly matches     matches of 4, 5, 7, 8 and 9 bytes (9 is not requested from memory, it leaves a hole) in blocks
                  assembled here: a sweep of sources that end from 4 bytes before to 8 bytes behind the first byte of
                  the tile the match lies in (the block's first 4096 symbols are 4-bit literals: a granule is 64 bytes
                  and the tiles begin at multiples of 4096, give or take what the wide turns took first -- the sweep
                  covers it); sources that begin at the stream's first byte, and one byte before it, which the oracle
                  refuses; outputs that end 1 to 7 bytes behind a multiple of 4096.
  long symbol     a 15-bit length code + 5 extra bits + a 15-bit distance code + 13 extra bits, 48 bits, starting at
                  every bit 0..31 of an input word: the second word shift of span_advance.
  ring wrap       48 KiB of barely compressible bytes with short repeats, 40 KiB of input and more: regions of the
                  largest size, the ring of 8 words wraps 18 times a region.  zlib levels 1, 6 and 9, and this library's
                  own `Default bytes (the oracle's deflate: tests/test_gpu_parity.py holds the kernels to them).

How many streams take the span path: the library has no counter of it to read back (last_inflate_blocks counts the
waves of a one-stream call), so the cases were run through the host model (tests/host_sim/sim_inflate.cpp, the kernel's
own span code on an emulated wave; tools/exp_span_stats.py's counters) when this file was written.  Every sampled stream
ran spans; the share of its output that spans committed:
  literals only   12 streams sampled.  The 48 of skewed codes and of 200 symbols: 98 to 100 %, one or two spans.  The 16
                  of sixteen 4-bit codes (every fourth stream): 21 to 56 % in 4 to 7 spans -- walks over symbols of one
                  length do not fall into step (inflate_span.h, span_after), the wide turns take the rest.
  fly matches     4 sampled, 2 spans each, 99.6 % and more (all but the last 50 to 64 bytes).
  long symbol     4 sampled, 1 or 2 spans, 99.5 % and more: the 48-bit symbol lies inside a span's tile.
  ring wrap       4 sampled, 4 spans each, 98.8 % and more.
  benchmark's     4 sampled, 1 span each, 99.8 %."""
import functools
import random
import sys
import zlib

import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu
sys.path.insert(0, util.GOLDEN)
import inflate_rules as R  # noqa: E402

# a case's items: (name, stream, the plain bytes or None for a stream that is not valid, whether zlib made it)
# (the 4-bit-letter code and the block writer live in tests/inflate_room_cases.py, which builds on them too)
from inflate_room_cases import DL_LONG, LETTERS, LL, Block as _Block  # noqa: E402,F401


def _letters(r, n):
    return bytes(r.choice(LETTERS) for _ in range(n))


@functools.lru_cache(maxsize=None)
def literal_streams():
    out = []
    for i in range(64):
        r = np.random.RandomState(7000 + i)
        n = 16384 + 2 * 257 * i + 1
        if i % 2 == 0:  # 16 symbols: flat (4-bit codes), or skewed (2 .. 7 bits)
            p = None if i % 4 == 0 else np.array([2.0 ** -(1 + k // 2) for k in range(16)]) / sum(2.0 ** -(1 + k // 2) for k in range(16))
            plain = (r.choice(16, n, p=p) * 11 + 5).astype(np.uint8).tobytes()
        else:
            plain = (r.randint(0, 200, n) + 20).astype(np.uint8).tobytes()
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
        out.append(("literals%d" % i, c.compress(plain) + c.flush(), plain, True))
    return out


@functools.lru_cache(maxsize=None)
def fly_streams():
    out = []
    r = random.Random(41)

    def one(name, q, length, dist, total):
        b = _Block(R.FULL_DL)
        b.lits(_letters(r, q))
        b.match(length, dist)
        b.lits(_letters(r, total - q - length))
        stream, plain = b.done()
        out.append((name, stream, plain, False))

    for length in (4, 5, 7, 8, 9):
        for k in range(13):  # the source ends at 4096 - 4 + k; the match lies in the tile that begins at 4096 or so
            q, end = 4096 + 1500 + 3 * k, 4096 - 4 + k
            one("edge%d_%d" % (length, k), q, length, q - (end - length), 16384 + 64 * k)
        for q in (5000, 9001):  # the source begins at the stream's first byte, and one before it
            one("first%d_%d" % (length, q), q, length, q, 16500)
            one("before%d_%d" % (length, q), q, length, q + 1, 16500)
    for base in (16384, 20480):  # the output ends 1 .. 7 bytes behind a multiple of the tile
        for k in range(1, 8):
            one("tail%d_%d" % (base, k), 6000 + k, (4, 5, 7, 8, 9)[k % 5], 5000, base + k)
    return out


@functools.lru_cache(maxsize=None)
def long_symbol_streams():
    out, offsets = [], set()
    for seed in (0, 1):
        r = random.Random(90 + seed)
        head, tail = _letters(r, 17000 + 3 * seed), _letters(r, 3000)
        for v in range(32):  # v literals of 15 bits move the match through every bit of a word
            b = _Block(DL_LONG)
            b.lits(head)
            b.lits(b"s" * v)
            at = b.match(227 + (v + seed) % 31, 16385 + 19 * v)
            b.lits(tail)
            stream, plain = b.done()
            assert plain is not None
            if seed == 0:
                offsets.add(at % 32)
            out.append(("long%d_%d" % (seed, at % 32), stream, plain, False))
    assert offsets == set(range(32))
    return out


@functools.lru_cache(maxsize=None)
def ring_streams():
    import oracle

    out = []
    for i in range(16):
        r = np.random.RandomState(300 + i)
        a = (r.randint(0, 200, 49152) + 30).astype(np.uint8)
        for at in range(64, 49152 - 16, 41):  # a short repeat every 41 bytes, from up to 20 000 bytes back
            n, back = 3 + int(r.randint(0, 10)), 1 + int(r.randint(0, min(at - 16, 20000)))
            a[at:at + n] = a[at - back:at - back + n].copy()
        plain = a.tobytes()
        for level in (1, 6, 9):
            c = zlib.compressobj(level, zlib.DEFLATED, -15)
            out.append(("ring%d_zlib%d" % (i, level), c.compress(plain) + c.flush(), plain, True))
        st, own, _ = oracle.deflate(plain, level=2)
        assert st == 0
        out.append(("ring%d_default" % i, own, plain, False))
    assert min(len(s[1]) for s in out) > 36 << 10
    return out


@functools.lru_cache(maxsize=None)
def symbol_streams():
    import oracle

    from zipc_amd import synth

    out = []
    for j in range(16):
        plain = synth.stream_bytes_np(2, j, 65536, 4).tobytes()
        st, own, _ = oracle.deflate(plain, level=2)
        assert st == 0
        out.append(("c2_%d" % j, own, plain, False))
    return out


@functools.lru_cache(maxsize=None)
def _wanted(stream):
    """the oracle's (status, bytes, CRC-32): once per stream, shared by the case's own test and the mixed batch"""
    import oracle

    return oracle.inflate(stream, crc_op=oracle.CRC_CRC32)


def _run(gpu_ctx, items):
    caps = [len(_wanted(s)[1]) if _wanted(s)[0] == 0 else 32768 for _, s, _, _ in items]
    got = util.gpu_inflate_batch(gpu_ctx, [s for _, s, _, _ in items], caps, [False] * len(items), [0] * len(items), 1)
    for (name, stream, plain, by_zlib), (st, data, crc) in zip(items, got):
        st0, d0, k0 = _wanted(stream)
        assert (st0 == 0) == (plain is not None), (name, "the oracle and the stream as built part", st0)
        assert st == st0, (name, "status", st, st0)
        if st0 != 0:
            continue
        assert d0 == plain, (name, "the oracle's bytes are not the plain bytes")
        assert len(data) == len(d0), (name, "length", len(data), len(d0))
        assert data == d0, (name, "bytes", next(i for i in range(len(d0)) if data[i] != d0[i]))
        assert crc == k0 == zlib.crc32(plain), (name, "CRC-32", hex(crc), hex(k0))
        if by_zlib:
            assert zlib.decompress(stream, -15) == data, (name, "zlib.decompress")


CASES = {"literals": literal_streams, "fly": fly_streams, "long_symbol": long_symbol_streams, "ring": ring_streams}


@pytest.mark.parametrize("case", sorted(CASES))
def test_case(gpu_ctx, case):
    items = CASES[case]()
    assert 64 <= len(items) <= 256 and all(p is None or 16384 <= len(p) <= 49152 for _, _, p, _ in items)
    _run(gpu_ctx, items)


def test_mixed_batch(gpu_ctx):
    items = [it for case in sorted(CASES) for it in CASES[case]()] + symbol_streams()
    random.Random(5).shuffle(items)
    assert len(items) > 256
    _run(gpu_ctx, items)
