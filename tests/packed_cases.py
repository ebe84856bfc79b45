"""The inputs of tests/test_gpu_inflate_packed.py: raw deflate and zlib streams with the bytes they were made from, made once
per process, shared, never changed.  Streams come from Python's zlib (raw deflate, wbits=-15) and from the project's own
deflate as the oracle computes it (the GPU's deflate gives the same bytes: tests/test_gpu_parity.py); the mixed-verdict
batch takes its good streams from the GPU's deflate itself.  Nothing here calls the code under test."""
import collections
import functools
import zlib

import util

# stream: the source bytes; plain: what it was made from (None: it does not inflate); limit: ?decompressed_size or None;
# flags: the descriptor's flags where they are not what the limit makes them
Item = collections.namedtuple("Item", "name stream plain limit flags")
Item.__new__.__defaults__ = (None, None)

RESERVED_BLOCK = b"\x07\x5a\xc3"  # BFINAL = 1, BTYPE = 3: corrupted at the first three bits


def raw_zlib(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def raw_own(data, level=2):
    import oracle

    st, s, _ = oracle.deflate(data, level=level)
    assert st == 0
    return s


def _lcg(seed):
    x = seed
    while True:
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        yield x >> 8


@functools.lru_cache(maxsize=None)
def tiny_pool(n=2049):
    """n tiny streams: outputs of 0..40 bytes in a fixed pseudo-random pattern, every 7th corrupted; zlib's and the
    project's own deflate in turn"""
    g = _lcg(2049)
    out = []
    for i in range(n):
        size = next(g) % 41
        plain = bytes((next(g) % 7 + 97) for _ in range(size))
        if i % 7 == 6:
            out.append(Item("tiny%d_corrupted" % i, RESERVED_BLOCK, None))
        else:
            out.append(Item("tiny%d" % i, raw_zlib(plain) if i % 2 else raw_own(plain, 1 + i % 3), plain))
    return tuple(out)


HIGH_BYTES = 6 * 1024 + 333  # bytes above 0x7F: from 6 KB on the reference's Adler-32 and RFC 1950's differ (include/zipc_hip.h)


@functools.lru_cache(maxsize=None)
def ragged_batch(n=200):
    """about 200 streams of 1 B .. 70 KiB, ragged: text, random bytes, runs and bytes above 0x7F"""
    g = _lcg(7)
    out = []
    for i in range(n):
        k = next(g) % 100
        size = 1 + (next(g) % 300 if k < 50 else next(g) % 6000 if k < 85 else next(g) % (70 << 10))
        if i == 0:
            size = 1
        if i == 1:
            size = 70 << 10
        kind = i % 4
        plain = (util.text(size, i) if kind == 0 else util.rand_bytes(size, i) if kind == 1 else bytes([65 + i % 26]) * size if kind == 2
                 else bytes(128 + (b & 127) for b in util.text(size, i)))
        out.append(Item("ragged%d_%d" % (i, size), raw_zlib(plain, 1 + i % 9) if i % 2 else raw_own(plain, i % 4), plain))
    for name, plain in (("high_ff", b"\xff" * HIGH_BYTES), ("high_rand", bytes(128 + (b & 127) for b in util.rand_bytes(3 * HIGH_BYTES, 5)))):
        out.append(Item(name, raw_own(plain, 2), plain))
    return tuple(out)


LONG_PLAIN_LEN = 500000
MAX_OUT_BLOCKS = 512 << 10


@functools.lru_cache(maxsize=None)
def long_among_short():
    """one stream of text that inflates to more than 256 KiB -- a chain of dynamic blocks, at least 40 KiB of source -- among
    50 short ones"""
    plain = util.text(LONG_PLAIN_LEN, 6)
    long_ = Item("text_long", raw_own(plain, 2), plain)
    assert len(long_.stream) >= 40 << 10 and 256 << 10 <= len(plain) <= MAX_OUT_BLOCKS
    shorts = [Item("short%d" % i, raw_zlib(p) if i % 2 else raw_own(p, 2), p)
              for i, p in enumerate(util.text(200 + 97 * i, 100 + i) for i in range(50))]
    return tuple(shorts[:20] + [long_] + shorts[20:])


def mixed_verdicts(gpu_deflate):
    """the batch of 9: (items, max_out_len, the statuses the rule's reading of the sizes must come to).  gpu_deflate: bytes ->
    the GPU's own deflate of them"""
    a, b, big = util.text(3000, 1), util.rand_bytes(777, 2), util.text(6000, 3)
    damaged = bytearray(raw_zlib(a))
    damaged[0] = (damaged[0] & 0xF9) | 0x06  # BTYPE = 3
    items = (
        Item("good_own", gpu_deflate(a), a),
        Item("good_zlib", raw_zlib(b), b),
        Item("empty_source", b"", None),
        Item("corrupted", bytes(damaged), None),
        Item("limit_exceeded", raw_zlib(a), None, len(a) - 1),
        Item("limit_met_exactly", raw_own(a, 3), a, len(a)),
        Item("unknown_flag", raw_zlib(b), None, None, 2),
        Item("inflates_to_nothing", raw_zlib(b""), b""),
        Item("above_max_out_len", raw_zlib(big), None),
    )
    return items, 5000, (0, 0, 1, 1, 2, 0, 18, 0, 18)


@functools.lru_cache(maxsize=None)
def zlib_batch():
    """whole zlib streams: good ones, every header failure of tests/zlib_cases.py, one wrong trailer, lengths under 6"""
    import zlib_cases

    picks = []
    for c in zlib_cases.decompress_cases():
        if c.name.startswith(("good_text3000", "good_rand20000", "good_empty", "good_trip0", "len", "fcheck", "method", "window", "dict")) \
                or c.name in ("trailer_byte_-1", "body_damaged_0", "cut4"):
            picks.append(c)
    names = {c.name for c in picks}
    assert {"len0", "len5", "fcheck_off_by_one", "method7", "method7_fcheck", "window8_fcheck", "dict_fcheck", "trailer_byte_-1"} <= names
    return tuple(picks)
