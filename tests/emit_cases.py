"""Inputs for tests/test_gpu_emit_turns.py, and the CPU walker that says what they reach (no GPU import).

deflate_emit_wave (zipc_amd/csrc/deflate.hip) counts and packs a block's symbols by turns, and most turns in an interior
form: the histogram takes 512 symbols a turn, four consecutive ones a lane, where 1024 still lie ahead; the packer takes
PACK_TILES * 64 = 384 items a turn, and a turn of nothing but symbols two consecutive ones a lane, merged into one item of
up to 64 bits -- where some lane's pair is longer, the lanes of that tile place their two symbols one by one.  Which form a
turn takes depends on the block's symbol count (and on the length of its header), so the streams here are chosen by the
symbol counts of the ORACLE's blocks: walk() reads them from its streams, and the assertions of coverage() hold for the
oracle alone -- they guard the lists, not the kernel."""
import functools
import os
import random
import zipfile

import token_ref
import util

HIST_TURN = 512   # symbols of a histogram turn (interior: while two turns lie ahead)
PACK_TURN = 384   # items of a packer's turn (PACK_TILES * 64), an interior one 3 tiles of 128 symbols
PAIR_TILE = 128
EMIT_PART = 8192  # symbols of a pack wave's part (forms.h), where a block is written by parts
LEVELS = (1, 2, 3)
SWEEP_MAX_SYMS = 2 * 1024 + 4  # the counts the short streams cover: past the histogram's first interior turn


def walk(stream):
    """[(kind, [bits of every symbol, extra bits included; without the end-of-block symbol])] per block of a deflate stream"""
    data = bytes(stream)
    buf = cnt = pos = 0
    out = []

    def need(n):
        nonlocal buf, cnt, pos
        while cnt < n:
            buf |= (data[pos] if pos < len(data) else 0) << cnt
            pos += 1
            cnt += 8

    def take(n):
        nonlocal buf, cnt
        need(n)
        v = buf & ((1 << n) - 1)
        buf >>= n
        cnt -= n
        return v

    def sym(table, bits):
        nonlocal buf, cnt
        need(bits)
        e = table[buf & ((1 << bits) - 1)]
        assert e, "no such code"
        buf >>= e & 15
        cnt -= e & 15
        return e >> 4, e & 15

    final = False
    while not final:
        final, kind = bool(take(1)), take(2)
        assert kind != 3
        if kind == token_ref.STORED:
            take(cnt % 8)
            ln, nln = take(16), take(16)
            assert ln == (~nln & 0xFFFF) and cnt == 0
            pos += ln
            out.append((kind, []))
            continue
        if kind == token_ref.FIXED:
            (lt, lb), (dt, db) = token_ref._fixed_tables()
        else:
            hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
            cl = [0] * 19
            for k in range(hclen):
                cl[token_ref.CL_ORDER[k]] = take(3)
            ct, cb = token_ref._table(cl)
            lens = []
            while len(lens) < hlit + hdist:
                s, _ = sym(ct, cb)
                if s < 16:
                    lens.append(s)
                elif s == 16:
                    lens += [lens[-1]] * (3 + take(2))
                elif s == 17:
                    lens += [0] * (3 + take(3))
                else:
                    lens += [0] * (11 + take(7))
            assert len(lens) == hlit + hdist
            lt, lb = token_ref._table(lens[:hlit])
            dt, db = token_ref._table(lens[hlit:])
        bits = []
        while True:
            s, n = sym(lt, lb)
            if s == 256:
                break
            if s > 256:
                x = token_ref.LEXT[s - 257]
                take(x)
                d, dn = sym(dt, db)
                take(token_ref.DEXT[d])
                n += x + dn + token_ref.DEXT[d]
            bits.append(n)
        out.append((kind, bits))
    assert pos - cnt // 8 == len(data), "the stream ends where its last block does"
    return out


# ---- short streams: a wave per stream, symbol counts swept -------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _sources():
    from zipc_amd import synth

    docs = zipfile.ZipFile(os.path.join(util.GOLDEN, "zip-docs.zip"))
    pat = util.rand_bytes(64, 909)
    return {"nibbles": synth.stream_bytes_np(2, 5, 3400, 4).tobytes(), "text": docs.read("zip-docs/APPNOTE.TXT")[4000:4000 + 2048],
            "period64": (pat * 33)[:2048]}


@functools.lru_cache(maxsize=None)
def short_streams():
    """[(kind, length, bytes)], more than 2048 of them: prefixes of ONE source per kind, so that the symbol count climbs with
    the length a symbol or so at a time -- 4-bit symbols at every length up to 3400 (streams this short find few matches: counts up to
    some 3170), text and a period of 64 at every third and seventh length up to 2 KiB"""
    src = _sources()
    out = [("nibbles", ln, src["nibbles"][:ln]) for ln in range(0, 3401)]
    out += [("text", ln, src["text"][:ln]) for ln in range(0, 2049, 3)]
    out += [("period64", ln, src["period64"][:ln]) for ln in range(0, 2049, 7)]
    assert len(out) > 2048
    return tuple(out)


def turn_edges(limit):
    """the symbol counts on both sides (+- 2) of every multiple of a turn's size, histogram and packer, up to `limit`"""
    want = set()
    for turn in (HIST_TURN, PACK_TURN):
        for m in range(turn, limit + 1, turn):
            want |= set(range(m - 2, m + 3))
    return {w for w in want if w <= limit}


def coverage(oracle, named, level):
    """-> the set of symbol counts of the oracle's coded blocks over `named` at `level` (deflate_trace: the oracle's own count,
    which includes the end-of-block symbol; the kernel's turns count the symbols in front of it)"""
    counts = set()
    for _, _, s in named:
        st, _, _, blocks = oracle.deflate_trace(s, level=level)
        assert st == 0
        counts |= {int(b.n_syms) - 1 for b in blocks if b.kind != 0}
    return counts


def wanted_counts():
    """the symbol counts a list must reach: every residue of a tile of pairs -- spread over blocks of one to fifteen such
    tiles, not all in the smallest -- and both sides of every turn's multiple"""
    return {r + PAIR_TILE * (1 + r % 15) for r in range(PAIR_TILE)} | turn_edges(SWEEP_MAX_SYMS)


_BY_COUNT = {}


def streams_by_count(oracle):
    """[(kind, length, bytes)], a few hundred: for every level and every count of wanted_counts() ONE of the short streams of
    4-bit symbols whose block the oracle codes with that many symbols at that level -- the list for the calls of at most
    2048 streams, where every stream of short_streams() does not fit.  (One list for all levels: a stream chosen for one
    level has some other count at another, which does no harm.)"""
    if "list" not in _BY_COUNT:
        nib = [t for t in short_streams() if t[0] == "nibbles"]
        chosen = set()
        for level in LEVELS:
            first = {}
            for i, (_, _, s) in enumerate(nib):
                st, _, _, blocks = oracle.deflate_trace(s, level=level)
                assert st == 0
                if len(blocks) == 1 and blocks[0].kind != 0:
                    first.setdefault(int(blocks[0].n_syms) - 1, i)
            assert wanted_counts() <= set(first), sorted(wanted_counts() - set(first))
            chosen |= {first[c] for c in wanted_counts()}
        _BY_COUNT["list"] = tuple(nib[i] for i in sorted(chosen))
    return _BY_COUNT["list"]


def reaches_the_edges(oracle, named, level):
    """the two conditions on a list's symbol counts under the oracle: every residue of a tile of pairs, in blocks of at least
    one such tile, and both sides of every turn's multiple -> what is missing ([] : nothing)"""
    counts = coverage(oracle, named, level)
    return sorted(set(range(PAIR_TILE)) - {n % PAIR_TILE for n in counts if n >= PAIR_TILE}) + sorted(turn_edges(SWEEP_MAX_SYMS) - counts)


# ---- pairs of neighbouring symbols longer than 64 bits -------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def long_pairs_stream(seed=7, n=60000, n_pairs=20, near=3000):
    """Bytes of a geometric distribution over some 200 values (long literal codes for the rare ones), a few thousand copies
    of 3 to 6 bytes from less than 300 bytes before (so that the far distances' symbols are rare among the distances), and,
    two by two and back to back, copies of 140 to 260 bytes from more than 16384 bytes before: few enough that their length
    symbols are rare.  Such a match takes up to 37 bits (a long code and 5 extra bits for the length, a long code and 13
    extra bits for the distance), two neighbours 66 and more."""
    r = random.Random(seed)
    b = bytearray(min(int(r.expovariate(0.035)), 199) + 20 for _ in range(n))
    for _ in range(near):
        at = 400 + r.randrange(n - 500)
        ln, d = r.randrange(3, 7), r.randrange(1, 300)
        b[at:at + ln] = b[at - d:at - d + ln]
    lens = [140, 170, 200, 240]
    at = 33000
    for k in range(n_pairs):
        at += 900 + r.randrange(300)
        for j in range(2):
            ln = lens[(k + j) % 4] + r.randrange(20)
            frm = at - (16400 + r.randrange(15000))
            b[at:at + ln] = b[frm:frm + ln]
            at += ln
    return bytes(b[:n])


def long_pairs(blocks):
    """[(block, symbol index k)] of neighbours k, k + 1 of a dynamic block that are longer than 64 bits together and lie
    in the block's interior: a whole packer's turn away from its first and last symbols"""
    out = []
    for bi, (kind, bits) in enumerate(blocks):
        if kind != token_ref.DYNAMIC:
            continue
        for k in range(PACK_TURN, len(bits) - PACK_TURN - 1):
            if bits[k] + bits[k + 1] > 64:
                out.append((bi, k))
    return out


# ---- the benchmark's shape, and blocks at the parts' edges ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def bench_shape():
    """64 streams of 65536 bytes of 4-bit symbols (two blocks: the second a handful of symbols), and 64 of 65536 + 320"""
    from zipc_amd import synth

    return tuple([("c2_%d" % k, 65536, synth.stream_bytes_np(2, 300 + k, 65536, 4).tobytes()) for k in range(64)]
                 + [("c2p_%d" % k, 65536 + 320, synth.stream_bytes_np(2, 400 + k, 65536 + 320, 4).tobytes()) for k in range(64)])


@functools.lru_cache(maxsize=None)
def part_edge_streams():
    """[(kind, length, bytes)]: bytes that never repeat within the window -- every byte a literal, so a block of n bytes has n
    symbols -- with a skewed distribution (a dynamic block, not a stored one), n = 8192 +- 2 and 16384 +- 2: blocks that
    end two symbols before, at, and two behind the end of a pack wave's first and second part"""
    out = []
    for m in (EMIT_PART, 2 * EMIT_PART):
        for n in range(m - 2, m + 3):
            out.append(("literals", n, skewed_literals(n, 50 + n % 11)))
    return tuple(out)


def skewed_literals(n, seed):
    """n bytes, none of whose 3-byte groups occurs twice (no match of MIN_MATCH_LEN), mostly from a few values"""
    r = random.Random(seed)
    seen, out = set(), bytearray()
    while len(out) < n:
        c = min(int(r.expovariate(0.08)), 255)
        if len(out) >= 2:
            key = (out[-2], out[-1], c)
            if key in seen:
                continue
            seen.add(key)
        out.append(c)
    return bytes(out)
