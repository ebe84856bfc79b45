"""The tokens of inflate by blocks, without a GPU.

  - tests/token_ref.py, the serial reference, is held two ways: on every stream of tests/token_cases.py its bytes are
    oracle.inflate's, and where a stream was made from a symbol list its src[] is what the list says (a double entry).
  - every property the catalogue plants is asserted from that reference alone: this stream has a byte of depth exactly 256
    and one of 257, that one a match whose source straddles a block start, and so on.
  - the host model's token form (tests/host_sim/sim_inflate.cpp sim_inflate_token_words: tok[] as it stands before the model's
    own resolve) runs every stream with follow 0 and 1, both lane orders and spans cut every 9000 and 20000 bits, and every
    word is held to THE INVARIANT:
        tok[i] == i  iff  byte i is a literal or a stored byte;
        else tok[i] < i and tok[i] lies on byte i's chain of copies (an ancestor);
        follow 0 (sources written down plainly): tok[i] == src[i] exactly.
  - TOKEN_MUTANTS below: one-line changes of the span decoder's token parts, each built into a host model
    of its own; each is killed by the stream its entry names, or breaks no word of any stream (equivalent).
tests/test_gpu_inflate_tokens.py holds the device's words to the same reference.
"""
import json
import os
import zlib

import numpy as np
import pytest

import mutation
import token_cases as TC
import token_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(follow, desc, cut) for follow in (0, 1) for desc in (0, 1) for cut in (9000, 20000)]


@pytest.fixture(scope="module")
def refs():
    return {c.name: TR.decode(c.stream) for c in TC.catalogue()}


# ---- the reference is held ------------------------------------------------------------------------------------------
def test_reference_bytes_are_the_oracles(oracle, refs):
    total = 0
    for c in TC.catalogue():
        st, plain, _ = oracle.inflate(c.stream)
        assert st == 0 and plain == refs[c.name].plain, c.name
        assert zlib.decompressobj(-15).decompress(c.stream) == plain, c.name
        total += len(plain)
    assert total <= TC.MAX_PLAIN, total


def test_reference_sources_are_what_the_symbol_lists_say(refs):
    n = 0
    for c in TC.catalogue():
        if c.blocks is None:
            continue
        r = refs[c.name]
        want = TR.src_of_symbols(c.blocks)
        assert len(want) == len(r.src) and (want == r.src).all(), c.name
        assert [b.kind for b in r.blocks] == [{"stored": 0, "fixed": 1, "dynamic": 2}[b.kind] for b in c.blocks], c.name
        pos = np.cumsum([0] + [b.out_len for b in r.blocks])
        assert [b.out_pos for b in r.blocks] == pos[:-1].tolist() and pos[-1] == len(r.plain), c.name
        assert all(a.end_bit <= b.start_bit < a.end_bit + 8 for a, b in zip(r.blocks, r.blocks[1:])), c.name
        n += 1
    assert n >= 20


def test_reference_chains(refs):
    """root, depth and the ancestor test against a walk link by link, on a stream small enough for that"""
    r = refs["len_dist_grid"]
    n = len(r.src)
    for i in list(range(0, n, 97)) + list(range(100, 2000)):
        j, d, chain = i, 0, [i]
        while r.src[j] != j:
            j = int(r.src[j]); d += 1; chain.append(j)
        assert r.root[i] == j and r.depth[i] == d, i
        t = np.array(chain + [max(i - 1, 0)])
        want = [True] * len(chain) + [max(i - 1, 0) in chain]
        assert r.is_ancestor(t, np.full(len(t), i)).tolist() == want, i


def test_streams_fit_the_block_path(refs):
    for c in TC.catalogue():
        r = refs[c.name]
        if c.taken:
            assert len(c.stream) >= TC.BLOCKS_MIN_SRC and len(r.blocks) >= 2 and 8 <= len(r.plain) and len(r.plain) // 64 <= len(c.stream), c.name
            assert len(r.blocks) < TC.chain_cap(len(c.stream)), c.name
        assert c.props, c.name
    assert [c.name for c in TC.catalogue() if not c.taken] == ["refuse_single_block", "refuse_39k_source", "refuse_beyond_64x", "refuse_fixed_only"]
    # (alone, a stream's call opens the block path at BLOCKS_MIN_SRC of ROOM: csrc/forms.h inflate_blocks_gate)
    assert all(TC.by_name(n).taken and len(refs[n].plain) >= TC.BLOCKS_MIN_SRC for n in TC.ALONE) and len(TC.ALONE) == 6


# ---- the planted properties, from the reference alone ------------------------------------------------------------------
def _in_block(r, k, i):
    b = r.blocks[k]
    return b.out_pos <= i < b.out_pos + b.out_len


def _match_at(r, pos):
    j = int(np.searchsorted(r.m_pos, pos))
    return (int(r.m_len[j]), int(r.m_dist[j])) if j < len(r.m_pos) and r.m_pos[j] == pos else None


class Props:
    @staticmethod
    def block_starts_with_match(c, r, k, ln, d, back):
        p = r.blocks[k].out_pos
        assert _match_at(r, p) == (ln, d) and _in_block(r, k - back, p - d)
        assert all(r.blocks[j].out_len <= 1 for j in range(k - back + 1, k))  # (what lies between: an empty block, or one of one byte)

    @staticmethod
    def source_straddles_block_start(c, r, k):
        b = r.blocks[k]
        m = (r.m_pos >= b.out_pos) & (r.m_pos < b.out_pos + b.out_len) & (r.m_dist >= r.m_len)
        s = r.m_pos[m] - r.m_dist[m]
        assert ((s < b.out_pos) & (s + r.m_len[m] > b.out_pos)).any()

    @staticmethod
    def final_block_is_one_literal(c, r):
        assert r.blocks[-1].out_len == 1 and r.src[-1] == len(r.src) - 1

    @staticmethod
    def has_match(c, r, ln, d):
        assert ((r.m_len == ln) & (r.m_dist == d)).any()

    @staticmethod
    def matches_back_to_back(c, r, ln, d, cnt):
        hit = (r.m_len == ln) & (r.m_dist == d)
        follows = np.concatenate([[False], r.m_pos[1:] == r.m_pos[:-1] + r.m_len[:-1]])
        # (a run of cnt: entries j-cnt+1 .. j all hit, each but the first directly behind the one before)
        ok = [all(hit[j - s] for s in range(cnt)) and all(follows[j - s] for s in range(cnt - 1)) for j in range(cnt - 1, len(hit))]
        assert any(ok)

    @staticmethod
    def match_at_tile_position(c, r, k, t, ln, d, prefix):
        """(that a tile really starts t bytes before it: test_tile_positions_are_real, against the span decoder's own tiles)"""
        at = r.blocks[k].out_pos + prefix
        assert _match_at(r, at) == (ln, d) and at - d < at - t < at - d + ln
        assert r.is_literal()[r.blocks[k].out_pos:at].all()

    @staticmethod
    def tile_of_3_byte_matches(c, r, k):
        b = r.blocks[k]
        m = (r.m_pos >= b.out_pos) & (r.m_pos < b.out_pos + b.out_len)
        assert (r.m_len[m] == 3).all() and m.sum() * 3 >= 2 * TC.TILE - 600
        first = int(r.m_pos[m][0])
        assert not r.is_literal()[first:b.out_pos + b.out_len].any() and b.out_pos + b.out_len - first >= 2 * TC.TILE - 600

    @staticmethod
    def chain_of_depth(c, r, D):
        top = r.depth[r.m_pos] == D  # a match of depth D that no match of depth D + 1 follows: the chain's last copy
        nxt = np.concatenate([r.depth[r.m_pos[1:]] == D + 1, [False]])
        assert (top & ~nxt).any()
        j = int(np.nonzero(top & ~nxt)[0][0])
        assert r.m_len[j] == 3 and r.m_dist[j] == 3 and r.root[r.m_pos[j]] == r.m_pos[j] - 3 * D

    @staticmethod
    def max_depth(c, r, D):
        assert r.depth.max() == D

    @staticmethod
    def deeper_than(c, r, h, count):
        assert int((r.depth > h).sum()) >= count
        assert (r.m_dist >= 2 * TC.TILE).all()  # (sources far apart: no tile holds a match and its source)

    @staticmethod
    def block_kinds(c, r, kinds):
        assert tuple(b.kind for b in r.blocks[:len(kinds)]) == kinds

    block_kinds_prefix = block_kinds

    @staticmethod
    def match_into_stored(c, r, k):
        b = r.blocks[k]
        m = (r.m_pos >= b.out_pos) & (r.m_pos < b.out_pos + b.out_len)
        s = int((r.m_pos[m] - r.m_dist[m])[0])
        assert r.blocks[r.block_of(s)].kind == TR.STORED

    @staticmethod
    def empty_dynamic_block(c, r, k):
        assert r.blocks[k].kind == TR.DYNAMIC and r.blocks[k].out_len == 0 and r.blocks[k].end_bit > r.blocks[k].start_bit

    @staticmethod
    def block_input_bits_at_least(c, r, k, bits):
        assert r.blocks[k].kind == TR.DYNAMIC and r.blocks[k].end_bit - r.blocks[k].start_bit >= bits
        assert r.blocks[k - 1].end_bit - r.blocks[k - 1].start_bit < 8192  # (behind a short one)

    @staticmethod
    def literal_block_of_length(c, r, k, n):
        """(where its last checkpoint lies: test_a_last_checkpoint_lies_close_to_its_blocks_end, against the span decoder's own tiles)"""
        b = r.blocks[k]
        assert b.out_len == n and r.is_literal()[b.out_pos:b.out_pos + n].all()

    @staticmethod
    def plain_is_text(c, r):
        assert r.plain == TC._text() and len(r.plain) == 400000

    @staticmethod
    def has_empty_stored_block(c, r):
        assert any(b.kind == TR.STORED and b.out_len == 0 for b in r.blocks)

    @staticmethod
    def n_blocks(c, r, n):
        assert len(r.blocks) == n

    @staticmethod
    def src_at_least(c, r, n):
        assert len(c.stream) >= n

    @staticmethod
    def src_below(c, r, n):
        assert len(c.stream) < n

    @staticmethod
    def out_beyond_64x(c, r):
        assert len(r.plain) // 64 > len(c.stream)

    @staticmethod
    def fixed_only_beyond_chain_cap(c, r):
        assert all(b.kind == TR.FIXED for b in r.blocks) and len(r.blocks) > TC.chain_cap(len(c.stream))

    @staticmethod
    def stored_block_lengths(c, r, lens):
        have = {b.out_len for b in r.blocks if b.kind == TR.STORED}
        assert set(lens) <= have and 2 * TC.ADLER_CHUNK + 1 in lens and TC.ADLER_CHUNK in lens

    @staticmethod
    def has_high_bytes(c, r):
        assert max(r.plain) > 0x7F


def test_planted_properties_hold(refs):
    n = 0
    for c in TC.catalogue():
        for p in c.props:
            try:
                getattr(Props, p[0])(c, refs[c.name], *p[1:])
            except AssertionError as e:
                raise AssertionError("%s: %r does not hold%s" % (c.name, p, (": " + str(e)) if str(e) else "")) from e
            n += 1
    assert n > 250
    # the lists of the issue, whole
    planted = {c.name: c.props for c in TC.catalogue()}
    assert {p[3] for p in planted["cross_near"] if p[0] == "block_starts_with_match"} == set(TC.CROSS_NEAR)
    assert {p[3] for p in planted["cross_far"] if p[0] == "block_starts_with_match"} == set(TC.CROSS_FAR)
    assert {(p[1], p[2]) for p in planted["len_dist_grid"]} == {(ln, d) for ln in TC.GRID_LEN for d in TC.GRID_DIST}
    for name in ("overlap_between_literals", "overlap_back_to_back"):
        assert {p[2] for p in planted[name]} == set(range(1, 67)) | {127, 128, 129, 257}
    assert sorted(p[2] for p in planted["tile_edges"] if p[0] == "match_at_tile_position") == list(range(9))


def test_adler_quirk_is_live(oracle, refs):
    """on at least two streams of the Adler-32 group the reference's block-wise Adler-32 is not RFC 1950's"""
    differ = 0
    for c in TC.catalogue():
        if c.group != "adler":
            continue
        st, plain, ck = oracle.inflate(c.stream, None, 2)  # (CRC_ADLER32)
        assert st == 0
        differ += ck != zlib.adler32(plain)
    assert differ >= 2, differ


# ---- the host model ---------------------------------------------------------------------------------------------------
_CHILD = r"""
import ctypes as C, json, os, sys
root, so, tasks = sys.argv[1], sys.argv[2], json.loads(sys.argv[3])
sys.path.insert(0, os.path.join(root, "tests")); sys.path.insert(0, root)
import numpy as np
import token_cases as TC, token_ref as TR
from host_sim import _bind
sim = _bind(C.CDLL(so))
out = {}
for name, configs in tasks:
    c = TC.by_name(name)
    r = TR.decode(c.stream)
    n = len(r.plain)
    for follow, desc, cut in configs:
        dst = C.create_string_buffer(n + 64)
        tok = np.full(n + 1, 0xFFFFFFFF, dtype=np.uint32)
        ol = C.c_uint64()
        st = sim.sim_inflate_token_words(c.stream, len(c.stream), dst, n, follow, desc, cut, C.byref(ol), tok.ctypes.data)
        bad = TR.word_failures(r, tok, follow == 0) if st in (0, -1) and n else np.arange(min(n, 1))
        out["%s/f%d/o%d/c%d" % (name, follow, desc, cut)] = {
            "status": st, "bytes": bool(st != 0 or ol.value != n or dst.raw[:n] != r.plain), "words": int(len(bad)),
            "first": r.describe(int(bad[0])) + ", tok %d" % tok[int(bad[0])] if len(bad) else ""}
print(json.dumps(out))
"""


def _run_children(so, names, configs, workers=8):
    """the catalogue's streams `names` through the host model `so` under `configs`, in child processes side by side (the model
    keeps its wave's state in statics) -> {stream/config: verdict}"""
    tasks = [(len(TC.by_name(n).stream) * (12 if n == "refuse_fixed_only" else 1), n, cfg) for n in names for cfg in configs]
    lots, load = [[] for _ in range(workers)], [0] * workers
    for cost, n, cfg in sorted(tasks, reverse=True):
        k = load.index(min(load))
        lots[k].append((n, [cfg]))
        load[k] += cost + 20000
    lots = [lot for lot in lots if lot]

    def child(lot):
        rc, got, err = mutation.run_child(_CHILD, ROOT, so, json.dumps(lot))
        if rc != 0:  # (a mutant may crash its model: every stream of the lot counts as broken)
            return {"%s/crashed" % name: {"status": rc, "bytes": True, "words": -1, "first": err[-300:]} for name, _ in lot}
        return got

    out = {}
    for part in mutation.build_all(child, lots):
        out.update(part)
    return out


def test_host_model_words_meet_the_invariant():
    from host_sim import LIB, lib

    lib()
    got = _run_children(LIB, [c.name for c in TC.catalogue()], CONFIGS)
    assert len(got) == len(TC.catalogue()) * len(CONFIGS)
    bad = {k: v for k, v in got.items() if v["status"] != 0 or v["bytes"] or v["words"]}
    assert not bad, (len(bad), sorted(bad.items())[:3])


def _model_tiles(c, r, follow=0, desc=0, cut=0):
    """the tiles the span decoder forms of a stream (sim_inflate_token_tiles): rows of first bit, first output byte, length"""
    import ctypes as C

    from host_sim import lib

    sim, n = lib(), len(r.plain)
    dst, tok, ol = C.create_string_buffer(n + 64), np.zeros(n + 1, dtype=np.uint32), C.c_uint64()
    assert sim.sim_inflate_token_words(c.stream, len(c.stream), dst, n, follow, desc, cut, C.byref(ol), tok.ctypes.data) == 0
    t = np.zeros(3 * 8192, dtype=np.uint64)
    k = sim.sim_inflate_token_tiles(t.ctypes.data, 8192)
    assert 0 < k <= 8192
    return t[:3 * k].reshape(-1, 3).astype(np.int64), tok[:n]


def test_tile_positions_are_real(refs):
    """tile_edges: the matches planted at tile positions 0..8 sit there by the span decoder's OWN tiles (the uncut span, the form
    a token wave and the dry run walk), their sources begin before the tile and run into it, and the words of those tiles meet
    the invariant in both forms"""
    c, r = TC.by_name("tile_edges"), refs["tile_edges"]
    for follow in (0, 1):
        tiles, tok = _model_tiles(c, r, follow)
        starts = {int(p): int(ln) for _, p, ln in tiles}
        hit = []
        for p in c.props:
            if p[0] != "match_at_tile_position":
                continue
            _, k, t, ln, d, prefix = p
            at = r.blocks[k].out_pos + prefix
            assert at - t in starts and starts[at - t] > t + ln, (p, sorted(starts))
            assert at - d < at - t < at - d + ln  # the source begins before the tile's first byte and ends inside the tile
            assert _match_at(r, at + ln + 10) == (5, t + 16)  # and a source that begins exactly at the tile's first byte
            hit.append(t)
        assert hit == list(range(9))
        assert not len(TR.word_failures(r, tok, follow == 0)), follow


def _checkpoints(tiles, b):
    """the checkpoints the dry run takes of block b (inflate_span.h: at a tile's start, CK_GAP_BITS = 24576 bits behind the last)"""
    last, out = 0, []
    for bit, pos, _ in tiles:
        if b.start_bit <= bit < b.end_bit and bit - b.start_bit >= last + 24576:
            out.append((int(bit), int(pos)))
            last = int(bit) - b.start_bit
    return out


def test_a_last_checkpoint_lies_close_to_its_blocks_end(refs):
    """interval_checkpoint_near_end, against the span decoder's own tiles and the checkpoint rule.  A span leaves the last
    stretch of a block to the plain decoder, so no tile -- and no checkpoint -- starts within the last few hundred bits; the
    closest of the three blocks is asserted to be within NEAR_END_BITS"""
    c, r = TC.by_name("interval_checkpoint_near_end"), refs["interval_checkpoint_near_end"]
    tiles, _ = _model_tiles(c, r)
    gaps = []
    for p in c.props:
        b = r.blocks[p[1]]
        cks = _checkpoints(tiles, b)
        assert cks, p
        gaps.append(b.end_bit - cks[-1][0])
    print("bits from the last checkpoint to the block's end:", gaps)
    assert min(gaps) <= NEAR_END_BITS, gaps


NEAR_END_BITS = 1024


# ---- the mutants ------------------------------------------------------------------------------------------------------
# the streams the mutants run over: every made stream for the block path but the long ones (nothing in those is not in these)
MUTANT_STREAMS = ["cross_near", "len_dist_grid", "overlap_between_literals", "overlap_back_to_back", "tile_edges", "chain_255_256_257",
                  "kinds_fixed_first", "kinds_stored_first", "interval_checkpoint_near_end"]
# (name, file, text, replacement, killer): one-line mutants of the TOKEN parts of the span decoder (inflate_span.h: what a byte of a
# match is written down as a copy of), killed on the CPU only and never built for the GPU, in the manner of
# tests/test_inflate_room_rules.py ROOM_MUTANTS: each is built into a host model of its own and run in child processes by
# test_token_mutants_are_killed below, which holds every word of tok[] to tests/token_ref.py.  killer: the stream of
# tests/token_cases.py whose words it must break, or ("equivalent", why): it must break none.  The test prints per mutant whether
# the BYTES alone would have caught it.
TOKEN_MUTANTS = [
    ("follow_from_off_by_one", "inflate_span.h", "const uint32_t from = dp + 32768u - dist;", "const uint32_t from = dp + 32767u - dist;",
     "len_dist_grid"),
    ("follow_in_tile_test_strict", "inflate_span.h", "if (sp >= 32768u && (mbits[(sp - 32768u) >> 5] >> (sp & 31u)) & 1u)",
     "if (sp > 32768u && (mbits[(sp - 32768u) >> 5] >> (sp & 31u)) & 1u)",
     ("equivalent", "(tile_edges has sources that begin at a tile's first byte) sp == 32768 is tile position 0: not following it inside the tile leaves the byte a copy of tile byte 0, a byte of "
                    "the same chain one link further from the literal -- a longer way, never a wrong one")),
    ("follow_sweep_test_strict", "inflate_span.h", "v[u] = sp >= 32768u ? out_pos", "v[u] = sp > 32768u ? out_pos",
     ("equivalent", "sp == 32768 then reads tok[out_pos], the word of tile byte 0 itself: out_pos while nobody has written it, or what "
                    "tile byte 0 is a copy of -- the same chain either way")),
    ("follow_wrap_dropped", "inflate_span.h", "r = r + 1u == dist ? 0u : r + 1u;", "r = r + 1u;",
     ("equivalent", "without the wrap byte i >= dist of an overlapping match is written down as a copy of byte i - dist of the match "
                    "itself, which is src[i] to the letter: one link more per period, the same chain")),
    ("plain_source_not_advanced", "inflate_span.h", "tok[at + i] = from + i;", "tok[at + i] = from;", "len_dist_grid"),
    ("follow_step_reads_the_neighbour", "inflate_span.h", "srcpos[b] = srcpos[sp - 32768u];", "srcpos[b] = srcpos[sp - 32767u];",
     "len_dist_grid"),
    ("follow_store_inverted", "inflate_span.h", "if (v[u] != out_pos + b) tok[out_pos + b] = v[u];",
     "if (v[u] == out_pos + b) tok[out_pos + b] = v[u];", "len_dist_grid"),
]


def test_token_mutants_are_killed(tmp_path, capsys):
    assert all(TC.by_name(n).taken and TC.by_name(n).blocks is not None for n in MUTANT_STREAMS)
    sos = mutation.build_all(lambda m: mutation.host_model(m, tmp_path / m[0]), TOKEN_MUTANTS)
    rows = []
    for m, so in zip(TOKEN_MUTANTS, sos):
        killer = m[4]
        assert killer[0] == "equivalent" or killer in MUTANT_STREAMS, m[0]
        got = _run_children(so, MUTANT_STREAMS, CONFIGS)
        by_words = sorted({k.split("/")[0] for k, v in got.items() if v["words"]})
        by_bytes = sorted({k.split("/")[0] for k, v in got.items() if v["bytes"]})
        ok = mutation.verdict(killer, by_words + by_bytes if killer[0] == "equivalent" else by_words)
        rows.append((m[0], "equivalent" if killer[0] == "equivalent" else killer, len(by_words), len(by_bytes), ok))
    with capsys.disabled():
        print("\ntoken mutants in the host model (%d streams, %d runs each)" % (len(MUTANT_STREAMS), len(CONFIGS)))
        print("  %-34s %-26s %s" % ("mutant", "killer", "streams broken by words / by bytes alone"))
        for name, killer, nw, nb, ok in rows:
            print("  %-34s %-26s %2d / %2d  %s%s" % (name, killer, nw, nb, "bytes alone would have caught it" if nb else "bytes alone would NOT have caught it",
                                                  "" if ok else "  -- NOT AS EXPECTED"))
    assert all(r[4] for r in rows), rows
