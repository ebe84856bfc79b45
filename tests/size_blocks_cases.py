"""The streams tests/test_gpu_inflate_size_blocks.py sizes by blocks: inputs only, made once per process, shared, never
changed.  Nothing here calls the code under test, and nothing here says what a call is to report: that is the oracle's
word (and, for lengths, the plain bytes as built), taken in the test."""
import collections
import functools
import os
import sys
import zlib

import numpy as np

import util

sys.path.insert(0, util.GOLDEN)
import inflate_rules as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKS_MIN_SRC = 40 << 10
N = 400000  # bytes of every encoder stream's plain text

# a stream and, where the builder knows them, its plain bytes (None: the stream is not a valid one)
Stream = collections.namedtuple("Stream", "name stream plain")


@functools.lru_cache(maxsize=None)
def head_cases():
    """Streams whose FIRST blocks hold the one thing a chain of dry runs cannot see: a match distance against the true
    output position below 32768.  Each is the named first blocks followed by the big valid part of the rule cases'
    wrapper e (320 KB of zlib's dynamic blocks), so that the input passes BLOCKS_MIN_SRC and the blocks chain up."""
    post = R.big_parts()[1]
    lits = list(b"rule cases ")
    out = []

    def add(name, blocks, tail=post):
        stream, plain, _, _ = R.assemble(blocks, post=tail)
        assert len(stream) >= BLOCKS_MIN_SRC, name
        out.append(Stream(name, stream, plain))

    for kind, blk in (("dynamic", R.dynamic), ("fixed", R.fixed)):
        add(kind + "_dist_out_plus1", [blk(lits + [("m", 10, lambda o: o + 1)])])
        add(kind + "_dist_eq_out", [blk(lits + [("m", 10, lambda o: o)])])
    ramp = bytes(range(256)) * 128
    add("stored_32767_then_dist_32768", [R.stored(ramp[:32767]), R.dynamic([("m", 3, 32768)])])
    add("stored_32768_then_dist_32768", [R.stored(ramp), R.dynamic([("m", 3, 32768), 7])])
    # a dynamic block that begins at position 100, runs on literals to 32760 and then reaches 32768 back
    add("literals_to_32760_then_dist_32768", [R.stored(ramp[:100]), R.dynamic([(i * 7) & 255 for i in range(32660)] + [("m", 3, 32768)])])
    # the head sees the final block: two dynamic blocks of rare long codes -- every literal used is 15 bits long -- that
    # inflate to 24 000 bytes from 45 KB of input (end of block 1 bit, literals 0..12 2..14 bits, 13 and 14 15 bits)
    ll = [0] * 257
    ll[256] = 1
    for s in range(13):
        ll[s] = s + 2
    ll[13] = ll[14] = 15
    long_codes = [13 + (i * i // 3) % 2 for i in range(12000)]
    add("head_sees_the_final_block", [R.dynamic(long_codes, ll=ll), R.dynamic(long_codes[::-1], ll=ll)], tail=None)
    assert len(out[-1].plain) == 24000
    return tuple(out)


def _sources(n):
    """the three sources of tests/test_gpu_parity.py's one-stream tests, built again here"""
    text = open(os.path.join(ROOT, "SURVEY.md"), "rb").read() + open(os.path.join(ROOT, "BASELINE.md"), "rb").read()
    rng = np.random.default_rng(21)
    yield "text", (text * (n // len(text) + 1))[:n]
    yield "symbols", (rng.integers(0, 16, n, dtype=np.uint8) * 17).astype(np.uint8).tobytes()
    yield "records", (rng.integers(0, 1 << 14, n // 4 + 1, dtype=np.uint32) * np.uint32(0x10001)).tobytes()[:n]


def _raw_zlib(data, level, flush_every=0, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    if not flush_every:
        return c.compress(data) + c.flush()
    out = b""  # (a full flush ends the block and puts an empty stored block behind it: stored blocks inside the chain)
    for i in range(0, len(data), flush_every):
        out += c.compress(data[i:i + flush_every]) + c.flush(zlib.Z_FULL_FLUSH)
    return out + c.flush()


# the encodings whose streams of text must go by blocks (the others may fall to the one wave, and must still be right)
BY_BLOCKS = ("oracle-default", "oracle-fast", "zlib-1-flushes", "zlib-6-flushes", "zlib-9-flushes")


@functools.lru_cache(maxsize=None)
def encoder_streams():
    """400 000 bytes of each source as the oracle codes them at `Default and `Fast (fixed and dynamic blocks mixed: the
    explorers, the followers, the chain's own walks), as zlib does at 1, 6 and 9 with a full flush every 100 000 bytes
    (empty stored blocks in the chain), with the fixed code only, stored only; and 400 000 zero bytes at zlib 9 (runs)"""
    import oracle

    out = []
    for name, data in _sources(N):
        assert len(data) == N
        encs = [("oracle-default", oracle.deflate(data, level=2)[1]), ("oracle-fast", oracle.deflate(data, level=1)[1])]
        encs += [("zlib-%d-flushes" % lv, _raw_zlib(data, lv, 100000)) for lv in (1, 6, 9)]
        encs += [("zlib-fixed", _raw_zlib(data, 6, strategy=zlib.Z_FIXED)), ("zlib-stored", _raw_zlib(data, 0))]
        for enc, raw in encs:
            out.append(Stream("%s/%s" % (name, enc), raw, data))
    out.append(Stream("zeros/zlib-9", _raw_zlib(bytes(N), 9), bytes(N)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def damaged_streams():
    """a long stream cut in the middle, and one with a damaged byte in a middle block"""
    s = next(x for x in encoder_streams() if x.name == "text/zlib-6-flushes")
    cut = s.stream[:len(s.stream) // 2]
    # (a damaged symbol of a complete code mostly decodes to other bytes; a damaged HEADER is refused: the first byte behind
    # the second full flush is a block's header -- its type made 3)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    at = sum(len(c.compress(s.plain[i:i + 100000]) + c.flush(zlib.Z_FULL_FLUSH)) for i in (0, 100000))
    assert s.stream[:at].endswith(b"\x00\x00\xff\xff") and at < len(s.stream) // 2 + 20000
    b = bytearray(s.stream)
    b[at] |= 0x06
    return (Stream("text_cut_in_the_middle", cut, None), Stream("text_damaged_in_a_middle_block", bytes(b), None))


def zlib_wrap(raw, plain):
    """the stream in a zlib container (RFC 1950: CMF / FLG, the body, an Adler-32 -- of the plain bytes where there are
    any; the sizing forms have no bytes to compare it with)"""
    return b"\x78\x9c" + raw + (zlib.adler32(plain) if plain is not None else 1).to_bytes(4, "big")
