"""The catalogue of streams for the tokens of inflate by blocks: INPUTS ONLY (tests/test_token_rules.py asserts every planted
property from tests/token_ref.py alone; tests/test_gpu_inflate_tokens.py holds the device's tokens to that reference).

Made streams come from the builders of tests/golden/inflate_rules.py (assemble, dynamic, fixed, stored, ("m", len, dist));
encoder streams from zlib and the oracle.  Every stream meant for the block path has at least BLOCKS_MIN_SRC = 40 KiB of
source, two blocks and more, and output within 64 x its input (csrc/forms.h inflate_blocks_fits) -- padded with stored
blocks of random bytes, the cheapest shape the path accepts.  All plain bytes together stay within 8 MiB.

catalogue() -> [Case]: name, group, stream, blocks (the symbol lists the stream was made from, None for an encoder's),
taken (the block path must run its tokens / must refuse it), props: the planted properties, each a tuple whose first entry
names a checker of test_token_rules.py.
"""
import collections
import functools
import os
import random
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "golden"))
import inflate_rules as R  # noqa: E402
import util  # noqa: E402

BLOCKS_MIN_SRC = 40 << 10  # csrc/forms.h
TILE = 4096                # csrc/inflate_span.h SPAN_TILE
ADLER_CHUNK = 5552
MAX_PLAIN = 8 << 20

Case = collections.namedtuple("Case", "name group stream blocks taken props")

CROSS_NEAR = (1, 2, 15, 16, 17, 63, 64, 65)
CROSS_FAR = (32767, 32768)
GRID_LEN = (3, 4, 8, 9, 15, 16, 17, 32, 33, 64, 65, 257, 258)
GRID_DIST = (15, 16, 17)
OVERLAP_DIST = tuple(range(1, 67)) + (127, 128, 129, 257)
CHAIN_SMALL = (255, 256, 257)
CHAIN_BIG = (65535, 65536, 65537)
ADLER_LENS = (0, 1, 5551, 5552, 5553, 11104, 2 * 5552 + 1)
TILE_PREFIX = (2399, 4038, 2022, 2527, 2021, 2025, 2024, 3038, 2029)
DEEP_DIST, DEEP_LEN, DEEP_OUT = 8192, 64, 1700 << 10


def lits(n, seed, alphabet=None):
    r = random.Random(seed)
    if alphabet is None:
        return list(r.randbytes(n))
    return [r.choice(alphabet) for _ in range(n)]


def pad(n_bytes, seed, piece=30000):
    """stored blocks of random bytes (bytes above 0x7F among them), n_bytes in all"""
    data = util.rand_bytes(n_bytes, seed)
    return [R.stored(data[i:i + piece]) for i in range(0, n_bytes, piece)]


def padded(blocks, seed, tail=None):
    """`blocks`, stored blocks up to BLOCKS_MIN_SRC and a little more of source, then `tail` (default: a final block of ONE literal)"""
    raw = R.assemble(blocks + [R.dynamic([0])])[0]
    need = max(BLOCKS_MIN_SRC + 4096 - len(raw), 1000)  # (and 40 KiB of output: a call of ONE stream opens the block path there)
    return blocks + pad(need, seed) + (tail if tail is not None else [R.dynamic([0x41])])


def _made(name, group, blocks, taken, props):
    stream, plain, _, _ = R.assemble(blocks)
    assert plain is not None, name
    return Case(name, group, stream, blocks, taken, tuple(props))


def _cross_near():
    blocks, props = [R.dynamic(lits(1000, 1))], []
    for d in CROSS_NEAR:  # the first symbol of a block: a match into the block before
        props.append(("block_starts_with_match", len(blocks), 20, d, 1))
        blocks.append(R.dynamic([("m", 20, d)] + lits(200, 100 + d)))
    for d in CROSS_NEAR:  # the same through an empty stored block: into the block before that
        blocks.append(R.stored(b""))
        props.append(("block_starts_with_match", len(blocks), 20, d, 2))
        blocks.append(R.dynamic([("m", 20, d)] + lits(200, 200 + d)))
    for d in CROSS_NEAR:  # and through a block of one byte (distance 1 copies that byte itself)
        blocks.append(R.dynamic([0x5A]))
        props.append(("block_starts_with_match", len(blocks), 20, d, 1 if d == 1 else 2))
        blocks.append(R.dynamic([("m", 20, d)] + lits(200, 300 + d)))
    # a source that begins in one block and ends in the next (and does not overlap its copy)
    props.append(("source_straddles_block_start", len(blocks)))
    blocks.append(R.dynamic(lits(5, 5) + [("m", 8, 10)] + lits(50, 6)))
    props.append(("final_block_is_one_literal",))
    return _made("cross_near", "cross", padded(blocks, 11), True, props)


def _cross_far():
    big = 33000
    blocks, props = [R.dynamic(lits(big, 2))], []
    for d in CROSS_FAR:
        props.append(("block_starts_with_match", len(blocks), 20, d, 1))
        # (a match of distance 32768 in the middle of a tile, between literals)
        blocks.append(R.dynamic([("m", 20, d)] + lits(2000, 400 + d) + [("m", 10, 32768)] + lits(big - 2000, 500 + d)))
    props.append(("has_match", 10, 32768))
    for d in CROSS_FAR:
        blocks.append(R.stored(b""))
        props.append(("block_starts_with_match", len(blocks), 20, d, 2))
        blocks.append(R.dynamic([("m", 20, d)] + lits(big, 600 + d)))
    for d in CROSS_FAR:
        blocks.append(R.dynamic([0x5A]))
        props.append(("block_starts_with_match", len(blocks), 20, d, 2))
        blocks.append(R.dynamic([("m", 20, d)] + lits(big, 700 + d)))
    return _made("cross_far", "cross", blocks + [R.dynamic([0x41])], True, props)


def _grid():
    syms, props = lits(100, 3), []
    for ln in GRID_LEN:
        for d in GRID_DIST:
            syms += lits(3, ln * 100 + d) + [("m", ln, d)]
            props.append(("has_match", ln, d))
    return _made("len_dist_grid", "grid", padded([R.dynamic(syms + lits(10, 4))], 12), True, props)


def _overlaps():
    a, b, pa, pb = lits(300, 5), lits(300, 6), [], []
    for d in OVERLAP_DIST:
        a += lits(4, 1000 + d) + [("m", 258, d)]           # between literals: a span tile holds them
        b += lits(2, 2000 + d) + [("m", 258, d)] * 3       # back to back: long matches in a row
        pa.append(("has_match", 258, d))
        pb.append(("matches_back_to_back", 258, d, 3))
    return [_made("overlap_between_literals", "overlap", padded([R.dynamic(a)], 13), True, pa),
            _made("overlap_back_to_back", "overlap", padded([R.dynamic(b)], 14), True, pb)]


def _tiles():
    blocks, props = [R.dynamic(lits(50, 7))], []
    # a match at tile position k whose source begins 3 bytes before the tile.  A tile is not 4096 bytes of literals: it holds at most
    # 64 granules of 256 bits and ends where the span's regions say, so where tiles start is read off the span decoder itself --
    # TILE_PREFIX[k] literals before the match put it at position k of a tile of the uncut span (found by running the host model to a
    # fixed point; test_token_rules.py::test_tile_positions_are_real asserts it against the model's tile starts).  The long tail
    # keeps the match inside a span: a span leaves the last stretch of a block to the plain decoder.
    for k in range(9):
        props.append(("match_at_tile_position", len(blocks), k, 6, k + 3, TILE_PREFIX[k]))
        # (and 10 literals on, a match whose source begins exactly AT the tile's first byte: the follow form's srcpos == 32768)
        props.append(("has_match", 5, k + 16))
        blocks.append(R.dynamic(lits(9000, 800 + k)[:TILE_PREFIX[k]] + [("m", 6, k + 3)] + lits(10, 850 + k) + [("m", 5, k + 16)]
                                + lits(5000, 900 + k)))
    r = random.Random(8)
    props.append(("tile_of_3_byte_matches", len(blocks)))
    blocks.append(R.dynamic(lits(600, 9) + [("m", 3, r.randrange(3, 500)) for _ in range(2 * TILE // 3)]))
    return _made("tile_edges", "tile", padded(blocks, 15), True, props)


def _chain(depths, seed):
    """per depth D: a phrase of 3 fresh literals, then D matches each copying the copy before it"""
    syms = []
    for k, D in enumerate(depths):
        syms += lits(40, seed * 10 + k) + [("m", 3, 3)] * D
    return syms


def _chains():
    out = [_made("chain_255_256_257", "chain", padded([R.dynamic(_chain(CHAIN_SMALL, 1))], 16), True,
                 [("chain_of_depth", D) for D in CHAIN_SMALL] + [("max_depth", max(CHAIN_SMALL))])]
    for D in CHAIN_BIG:
        out.append(_made("chain_%d" % D, "chain", padded([R.dynamic(_chain((D,), D))], D), True, [("chain_of_depth", D), ("max_depth", D)]))
    return out


def _deep():
    """most bytes deep, sources DEEP_DIST apart: byte i of the body has depth i // DEEP_DIST (the later rounds' second trip)"""
    n = (DEEP_OUT - DEEP_DIST) // DEEP_LEN
    syms = lits(DEEP_DIST, 21) + [("m", DEEP_LEN, DEEP_DIST)] * n
    return _made("deep", "deep", [R.dynamic(lits(64, 22)), R.dynamic(syms), R.dynamic([0x41])], True,
                 [("deeper_than", 3, 2048 * 256 + 1), ("max_depth", (64 + DEEP_DIST + n * DEEP_LEN - 64 - 1) // DEEP_DIST)])


def _kinds():
    text = lits(3000, 31, b"etaoin shrdlu,.\n")
    st = util.rand_bytes(5000, 32)
    blocks = [R.fixed(text[:500] + [("m", 12, 100)]),                                   # a first block that is fixed
              R.dynamic(lits(400, 33)), R.stored(st), R.dynamic([("m", 30, 2500)] + lits(200, 34) + [("m", 200, 4000)]),
              R.stored(b""), R.dynamic(lits(300, 35)), R.stored(b""), R.stored(b""),
              R.fixed(text[500:1500] + [("m", 40, 700)]), R.dynamic(lits(900, 36)), R.fixed([("m", 9, 9)] + text[1500:]),
              R.dynamic([]),                                                           # end-of-block alone
              R.dynamic(lits(100, 37))]
    props = [("block_kinds", (1, 2, 0, 2, 0, 2, 0, 0, 1, 2, 1, 2, 2)), ("match_into_stored", 3), ("empty_dynamic_block", 11),
             ("final_block_is_one_literal",)]
    a = _made("kinds_fixed_first", "kinds", padded(blocks, 17), True, props)
    blocks_b = [R.stored(st[:3000]), R.dynamic([("m", 100, 3000)] + lits(500, 38)), R.fixed(text[:800])]
    b = _made("kinds_stored_first", "kinds", padded(blocks_b, 18), True,
              [("block_kinds_prefix", (0, 2, 1)), ("match_into_stored", 1), ("final_block_is_one_literal",)])
    return [a, b]


def _intervals():
    n_long = 206000  # literals of 8 and 9 bits: about 200 KiB of input in one dynamic block, a checkpoint every 24576 bits at most
    long_syms = lits(n_long, 41)
    r = random.Random(42)
    for k in range(2000, n_long, 997):
        long_syms[k] = ("m", r.randrange(3, 259), r.randrange(1, 1900))
    a = _made("interval_long_block", "intervals", [R.dynamic(lits(300, 43)), R.dynamic(long_syms), R.dynamic([0x41])], True,
              [("block_input_bits_at_least", 1, 190 * 1024 * 8)])
    # blocks of 4096 k + 30 literals.  Where the dry run takes checkpoints is read off the span decoder's own tiles
    # (test_token_rules.py::test_a_last_checkpoint_lies_close_to_its_blocks_end): the first block's last one lies 736 bits before its
    # end; a span leaves a block's last stretch to the plain decoder, so no tile and no checkpoint starts closer
    tail = [R.dynamic(lits(300, 44))] + [R.dynamic(lits(TILE * k + 30, 45 + k)) for k in (1, 2, 3)]
    b = _made("interval_checkpoint_near_end", "intervals", padded(tail, 19), True,
              [("literal_block_of_length", j + 1, TILE * k + 30) for j, k in enumerate((1, 2, 3))])
    return [a, b]


@functools.lru_cache(maxsize=None)
def _text():
    return util.text(400000, 51)


def _encoders():
    import oracle

    t, out = _text(), []
    for lvl in (1, 6):
        c = zlib.compressobj(lvl, zlib.DEFLATED, -15)
        out.append(Case("zlib_%d" % lvl, "encoder", c.compress(t) + c.flush(), None, True, (("plain_is_text",),)))
    c = zlib.compressobj(9, zlib.DEFLATED, -15)
    s = c.compress(t[:150000]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(t[150000:]) + c.flush()
    out.append(Case("zlib_9_full_flush", "encoder", s, None, True, (("plain_is_text",), ("has_empty_stored_block",))))
    for name, lvl in (("default", oracle.LEVELS["default"]), ("fast", oracle.LEVELS["fast"])):
        st, s, _ = oracle.deflate(t, lvl)
        assert st == 0
        out.append(Case("oracle_" + name, "encoder", s, None, True, (("plain_is_text",),)))
    return out


def chain_cap(src_len, explore_stride=16384):
    """csrc/inflate_blocks.h blocks_job: the blocks a stream's chain may have"""
    return min(2 * min(src_len // 512 + 64, 65536) + 4 * (src_len // explore_stride + 1), 262144)


def _refused():
    one = _made("refuse_single_block", "refuse", [R.dynamic(lits(60 << 10, 61))], False, [("n_blocks", 1), ("src_at_least", BLOCKS_MIN_SRC)])
    short_blocks = [R.dynamic(lits(1000, 62))] + pad(37800, 63) + [R.dynamic([0x41])]
    short = _made("refuse_39k_source", "refuse", short_blocks, False, [("src_below", BLOCKS_MIN_SRC), ("src_at_least", 38 << 10)])
    # output beyond 64 x the input: runs, and stored bytes to reach BLOCKS_MIN_SRC
    # (13 bits a run of 258: 10300 of them are 16.7 KB of source and 2.66 MB of output; with 24200 stored bytes the source
    # passes BLOCKS_MIN_SRC by a few dozen bytes and the output is 65 x it -- the smallest such stream there is)
    n_run = 10300
    runs = [R.dynamic(lits(8, 64) + [("m", 258, 1)] * n_run)] + pad(24200, 65) + [R.dynamic([0x41])]
    x64 = _made("refuse_beyond_64x", "refuse", runs, False, [("out_beyond_64x",), ("src_at_least", BLOCKS_MIN_SRC)])
    # fixed blocks only, and more of them than the stream's chain can hold (chain_cap): the chain gives up
    text = lits(100 * 420, 66, b"etaoin shrdlu,.\n")
    fx = [R.fixed(text[i:i + 100]) for i in range(0, len(text), 100)]
    fixed_only = _made("refuse_fixed_only", "refuse", fx, False, [("fixed_only_beyond_chain_cap",), ("src_at_least", BLOCKS_MIN_SRC)])
    return [one, short, x64, fixed_only]


def _adler():
    out = []
    for k, seed in enumerate((71, 72, 73)):
        r = random.Random(seed)
        lens = list(ADLER_LENS) * 2
        r.shuffle(lens)
        blocks = [R.dynamic(lits(700, seed + 10))]
        for j, n in enumerate(lens):
            # bytes above 0x7F: random ones, and runs of 0xFF (large sums: the reference's signed remainder goes negative)
            data = bytes([0xFF]) * n if (j + k) % 3 == 0 else util.rand_bytes(n, seed * 100 + j)
            blocks.append(R.stored(data))
            if j % 4 == 3:
                blocks.append(R.dynamic([("m", 50, 600)] + lits(20, seed + j)))
        out.append(_made("adler_%d" % k, "adler", blocks + [R.dynamic([0x41])], True,
                         [("stored_block_lengths", ADLER_LENS), ("has_high_bytes",), ("src_at_least", BLOCKS_MIN_SRC)]))
    return out


def _one(fn):
    return lambda: [fn()]


# (the streams' names, their builder): by_name builds one group alone
GROUPS = [
    (("cross_near",), _one(_cross_near)), (("cross_far",), _one(_cross_far)), (("len_dist_grid",), _one(_grid)),
    (("overlap_between_literals", "overlap_back_to_back"), _overlaps), (("tile_edges",), _one(_tiles)),
    (("chain_255_256_257",) + tuple("chain_%d" % D for D in CHAIN_BIG), _chains), (("deep",), _one(_deep)),
    (("kinds_fixed_first", "kinds_stored_first"), _kinds), (("interval_long_block", "interval_checkpoint_near_end"), _intervals),
    (("zlib_1", "zlib_6", "zlib_9_full_flush", "oracle_default", "oracle_fast"), _encoders),
    (("refuse_single_block", "refuse_39k_source", "refuse_beyond_64x", "refuse_fixed_only"), _refused),
    (("adler_0", "adler_1", "adler_2"), _adler),
]
NAMES = tuple(n for names, _ in GROUPS for n in names)


@functools.lru_cache(maxsize=None)
def _group(k):
    cases = GROUPS[k][1]()
    assert tuple(c.name for c in cases) == GROUPS[k][0]
    return cases


@functools.lru_cache(maxsize=None)
def catalogue():
    return tuple(c for k in range(len(GROUPS)) for c in _group(k))


def by_name(name):
    k = next(k for k, (names, _) in enumerate(GROUPS) if name in names)
    return next(c for c in _group(k) if c.name == name)


# the six streams that also go alone, in the default row of the GPU test
ALONE = ("cross_near", "overlap_back_to_back", "chain_65536", "kinds_fixed_first", "interval_long_block", "oracle_default")
