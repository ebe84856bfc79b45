"""Streams and rooms that put the END of an inflate stream's destination inside every kind of write the decoders make
(include/zipc_hip.h at zipc_hip_inflate_batch: nothing is written in front of dst_off or behind dst_off + dst_cap,
whatever the status).  numpy, zlib and the oracle only: nothing here calls the code under test.
tests/test_inflate_room_rules.py (CPU: the planted properties, the host model, the mutants) and
tests/test_gpu_inflate_room.py (every inflate form on the GPU) run what this module lists.

A Stream is its deflate bytes, its plain bytes, and a serial reading of its symbols AS WRITTEN (segs: literal runs,
matches and stored blocks with the output position each starts at; symbol_table() spreads them to one entry per
symbol).  Streams that zlib or the oracle's deflate made are read by read_symbols(), a plain bit-by-bit reader.

Notation: N a stream's output length, R its room = min(limit, dst_cap).  rooms(stream): R = N and N + 1, and on the
failing side N - 1 and b - 1, b, b + 1, b + 15, b + 16, b + 17 for the output positions b at which the matches of
index 0, 1, 2, 63, 64, 65, 66, last - 1 and last start (a stored family: the stored blocks), clipped to [0, N - 1];
the span and by-blocks families add N // 2 and 4096 k +- 1.  Every (stream, R) is declared as

    limit   dst_cap   status when R < N
    none    R         16  ZIPC_HIP_ERR_DST_TOO_SMALL
    R       R         2   ZIPC_HIP_ERR_SIZE_EXCEEDED
    R       R + 40    2
    N + 5   R         16

dst_off = 0, 1, 5, 15 (mod 16) and crc_op = 0, 1, 2 rotate over the items.

What the catalogue's limits (under 8000 items, under 256 MiB of destination) cost: the full product of the streams,
rooms and declarations above is about 35 000 items, so
  - R = N - 1 and N of every stream get all four declarations; every other room (the b - 1 .. b + 17 groups, N // 2,
    4096 k +- 1, and N + 1) gets ONE, the four taking turns from room to room, so each group of six meets all four;
  - the lane family without a span is the full product of length, distance (those in reach) and g = 0 .. 9, but the
    rooms around the match's start come with g = 0 and g = 9 only (the match starts where it does for every g);
  - the lane family under a span (20 KiB of input in front) takes every (length, distance) pair once, g taking
    turns over the pairs;
  - the zlib- and oracle-made streams of the run family take the matches of index 0, 1, last - 1 and last;
  - the span family takes the last two matches of a stream.
What the span family has on top: two streams of skewed literals (2 .. 7 bits) that take 128 rooms in a row around N // 2
(SWEEP), each under one of the three declarations with dst_cap = R.  A span never commits a stream's last 50 to 130 bytes
(it wants input ahead), so with R = N no tile ends with the room; a tile ends with the room where R cuts the stream at
the end of what a tile is cut by -- in the host model four granules of input, 80 to 95 bytes of these streams, so 128
rooms in a row hold one (text: some 200 bytes; the letter streams: multiples of 16, where the flush has no tail).

Counts (COUNTS below; test_inflate_room_rules.py::test_the_catalogue holds them), streams / items per family:
    run_short 28 / 1344    run_long 41 / 1198    lane 300 / 2940    lane_span 36 / 471    stored 37 / 470
    span 62 / 1341    literal_last 6 / 54    by_blocks 2 / 125    --    512 streams, 7943 items,
    88 967 457 bytes of destination (DST_BYTES) when one arena holds every item's room and guards."""
import collections
import copy
import functools
import random
import sys
import zlib

import numpy as np

import util

sys.path.insert(0, util.GOLDEN)
import inflate_rules as R  # noqa: E402

# ---- the 4-bit-letter codes --------------------------------------------------------------------------------------
LETTERS = b"abcdefghijklmn"
# litlen lengths: 14 letters of 4 bits, then one symbol each of 4 .. 14 bits and two of 15 (a complete code)
LL = [0] * 285
for _c in LETTERS:
    LL[_c] = 4
for _sym, _n in ((258, 4), (259, 5), (261, 6), (262, 7), (263, 8), (257, 9), (ord("o"), 10), (ord("p"), 11), (ord("q"), 12),
                 (ord("r"), 13), (256, 14), (284, 15), (ord("s"), 15)):
    LL[_sym] = _n
assert sum(2.0 ** -n for n in LL if n) == 1.0
DL_LONG = [i + 1 for i in range(14)] + [0] * 14 + [15, 15]  # distance symbol 28 (13 extra bits): a 15-bit code
assert sum(2.0 ** -n for n in DL_LONG if n) == 1.0
# the same letters, and 6-bit codes for the end of block and the lengths 3, 4, 8, 9, 15-16, 31-34 and 258
LL_ROOM = [0] * 286
for _c in LETTERS:
    LL_ROOM[_c] = 4
for _sym in (256, 257, 258, 262, 263, 267, 272, 285):
    LL_ROOM[_sym] = 6
assert sum(2.0 ** -n for n in LL_ROOM if n) == 1.0


class Block:
    """one final dynamic block in `ll` (default LL) and the given distance lengths, written symbol by symbol; segs: the
    serial reading of what was written -- ['L', start, count, 0] literal runs and ('M', start, length, distance)"""

    def __init__(self, dl, ll=LL):
        self.w, self.out, self.segs = R.Writer(), R.Out(), []
        R.emit_block(self.w, self.out, R.dynamic([], ll=ll, dl=dl, eob=False), True)
        rev = lambda code, n: (int(format(code, "0%db" % n)[::-1], 2), n)
        self.lc = {s: rev(*c) for s, c in R.canonical(ll).items()}
        self.dc = {s: rev(*c) for s, c in R.canonical(dl).items()}

    def fork(self):
        """a copy that goes on from here (the codes are shared)"""
        b = copy.copy(self)
        b.w, b.out, b.segs = copy.deepcopy(self.w), R.Out(), [list(s) if s[0] == "L" else s for s in self.segs]
        b.out.b, b.out.bad = bytearray(self.out.b), self.out.bad
        return b

    def lits(self, data):
        f, lc = self.w.field, self.lc
        for b in data:
            f(*lc[b])
        if data:
            at = len(self.out.b)
            if self.segs and self.segs[-1][0] == "L" and self.segs[-1][1] + self.segs[-1][2] == at:
                self.segs[-1][2] += len(data)
            else:
                self.segs.append(["L", at, len(data), 0])
        self.out.b += data

    def match(self, length, dist):
        """-> the bit the match's first code starts at"""
        at = self.w.pos
        ls, le = R.len_sym(length)
        ds, de = R.dist_sym(dist)
        self.w.field(*self.lc[ls]); self.w.field(le, R.LEXT[ls - 257])
        self.w.field(*self.dc[ds]); self.w.field(de, R.DEXT[ds])
        self.segs.append(("M", len(self.out.b), length, dist))
        self.out.match(length, dist)
        return at

    def done(self):
        self.w.field(*self.lc[256])
        return self.w.bytes(), (None if self.out.bad else bytes(self.out.b))


# ---- a serial reading of a finished stream -------------------------------------------------------------------------

def _decoder(lengths):
    """lengths -> (table indexed by the next maxlen bits as they lie in the stream, maxlen)"""
    maxlen = max(lengths)
    tab = [None] * (1 << maxlen)
    for sym, (code, n) in R.canonical(lengths).items():
        first = int(format(code, "0%db" % n)[::-1], 2)
        for k in range(first, 1 << maxlen, 1 << n):
            tab[k] = (sym, n)
    return tab, maxlen


def read_symbols(raw):
    """RFC 1951, one symbol after the other -> (plain, segs).  For valid streams (zlib's, the oracle's): asserts, no
    error paths."""
    pos, out, segs = 0, bytearray(), []

    def peek(n):
        return (int.from_bytes(raw[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << n) - 1)

    def bits(n):
        nonlocal pos
        v = peek(n)
        pos += n
        return v

    def sym(dec):
        nonlocal pos
        s, n = dec[0][peek(dec[1])]
        pos += n
        return s

    fixed = None
    while True:
        final, btype = bits(1), bits(2)
        assert btype != 3
        if btype == 0:
            pos = (pos + 7) // 8 * 8
            n, inv = bits(16), bits(16)
            assert n == (~inv & 0xFFFF) and pos // 8 + n <= len(raw)
            segs.append(("S", len(out), n, 0))
            out += raw[pos // 8:pos // 8 + n]
            pos += 8 * n
        else:
            if btype == 1:
                fixed = fixed or (_decoder(R.FIXED_LL), _decoder(R.FIXED_DL))
                lit, dist = fixed
            else:
                hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[R.ORDER[i]] = bits(3)
                cdec, lens = _decoder(cl), []
                while len(lens) < hlit + hdist:
                    s = sym(cdec)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + bits(2))
                    else:
                        lens += [0] * (3 + bits(3) if s == 17 else 11 + bits(7))
                assert len(lens) == hlit + hdist
                lit = _decoder(lens[:hlit])
                dist = _decoder(lens[hlit:]) if any(lens[hlit:]) else None
            while True:
                s = sym(lit)
                if s < 256:
                    if segs and segs[-1][0] == "L" and segs[-1][1] + segs[-1][2] == len(out):
                        segs[-1][2] += 1
                    else:
                        segs.append(["L", len(out), 1, 0])
                    out.append(s)
                elif s == 256:
                    break
                else:
                    length = R.LBASE[s - 257] + bits(R.LEXT[s - 257])
                    ds = sym(dist)
                    d = R.DBASE[ds] + bits(R.DEXT[ds])
                    assert d <= len(out)
                    segs.append(("M", len(out), length, d))
                    for _ in range(length):
                        out.append(out[-d])
        if final:
            return bytes(out), segs


def _segs_of(blocks):
    """the serial reading of blocks handed to inflate_rules.assemble: symbol lists and stored data"""
    segs, pos = [], 0
    for blk in blocks:
        if blk.kind == "stored":
            segs.append(("S", pos, len(blk.syms), 0))
            pos += len(blk.syms)
            continue
        for s in blk.syms:
            if isinstance(s, int):
                if segs and segs[-1][0] == "L" and segs[-1][1] + segs[-1][2] == pos:
                    segs[-1][2] += 1
                else:
                    segs.append(["L", pos, 1, 0])
                pos += 1
            else:
                assert s[0] == "m"
                segs.append(("M", pos, s[1], s[2]))
                pos += s[1]
    return segs


# family, name, deflate bytes, plain bytes, segs, and what was planted (a dict: p, L, dist, g, k, d, made_by, ...)
Stream = collections.namedtuple("Stream", "family name raw plain segs meta")


def symbol_table(stream):
    """-> (starts, kinds): the output position every symbol starts at (uint32) and its kind (uint8: ord of L, M, S)"""
    starts, kinds = [], []
    for kind, at, n, _ in stream.segs:
        if kind == "L":
            starts.append(np.arange(at, at + n, dtype=np.uint32))
            kinds.append(np.full(n, ord("L"), np.uint8))
        else:
            starts.append(np.array([at], np.uint32))
            kinds.append(np.array([ord(kind)], np.uint8))
    if not starts:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint8)
    return np.concatenate(starts), np.concatenate(kinds)


def matches(stream):
    return [s for s in stream.segs if s[0] == "M"]


def anchors(stream):
    """the symbols whose starts the failing rooms are set around: the matches, or without any the stored blocks"""
    return matches(stream) or [s for s in stream.segs if s[0] == "S"]


def _assembled(family, name, blocks, **meta):
    raw, plain, _, _ = R.assemble(blocks)
    assert plain is not None
    return Stream(family, name, raw, plain, _segs_of(blocks), meta)


def _read(family, name, raw, plain, **meta):
    got, segs = read_symbols(raw)
    assert got == plain, name
    return Stream(family, name, raw, plain, segs, meta)


def _lits(r, n, below=144):
    return [r.randrange(below) for _ in range(n)]


def _period(r, p):
    """p literals, all different (p < 144): their periodic extension has no shorter period"""
    return r.sample(range(144), p)


# ---- the families ------------------------------------------------------------------------------------------------
RUN_SHORT_P = (1, 2, 3, 15, 16, 17, 63)
RUN_LONG_P = (64, 65, 79, 80, 81, 257, 258, 259, 1000, 4097)


@functools.lru_cache(maxsize=None)
def run_short():
    """match_run and wave_copy_match's first branch: a period p < 64 of literals, then 258-byte matches at distance p"""
    import oracle

    out, r = [], random.Random(61)
    for p in RUN_SHORT_P:
        syms = _period(r, p) + [("m", 258, p)] * ((20000 - p) // 258)
        for kind, blk in (("fixed", R.fixed), ("dynamic", R.dynamic)):
            out.append(_assembled("run_short", "p%d_%s" % (p, kind), [blk(syms)], p=p, made_by=kind))
        plain = out[-1].plain
        st, own, _ = oracle.deflate(plain, level=2)
        assert st == 0
        out.append(_read("run_short", "p%d_oracle" % p, own, plain, p=p, made_by="oracle"))
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        out.append(_read("run_short", "p%d_zlib" % p, c.compress(plain) + c.flush(), plain, p=p, made_by="zlib"))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def run_long():
    """wave_copy_match's second branch: periods of 64 and more; single short matches behind a match they read (so that
    they are not queued but handed to the wave: P < 16, and one or two 16-byte pieces)"""
    out, r = [], random.Random(62)
    for p in RUN_LONG_P:
        syms = _lits(r, p) + [("m", 258, p)] * (40000 // 258)
        out.append(_assembled("run_long", "p%d" % p, [R.fixed(syms)], p=p, single=False))
    for dist, lengths in ((64, tuple(range(3, 16)) + (16, 17, 31, 32, 33)), (5000, tuple(range(3, 16)))):
        for length in lengths:
            # ... m1 writes [q, q + 8); m2, `dist` behind its start, reads it (a hole while m1 is queued) and ends the output
            lead = _lits(r, dist + 40)
            syms = lead + [("m", 8, dist)] + _lits(r, dist - 8) + [("m", length, dist)]
            out.append(_assembled("run_long", "single_L%d_d%d" % (length, dist), [R.fixed(syms)], L=length, dist=dist, single=True))
    return tuple(out)


LANE_L = (3, 4, 8, 9, 16, 258)
LANE_DIST = (1, 7, 8, 9, 64, 32768)
LANE_G = tuple(range(10))


@functools.lru_cache(maxsize=None)
def lane():
    """one match and g literals to the end of the output, under 1 KiB of input: no span runs (inflate_lane.h
    lane_copy_match's `+ 8` gate in the host model; the wave's copy on the GPU)"""
    out, r = [], random.Random(63)
    for length in LANE_L:
        for dist in LANE_DIST:
            if dist > 70:
                continue  # (not reachable in under 1 KiB of input)
            for g in LANE_G:
                syms = _lits(r, 70) + [("m", length, dist)] + _lits(r, g)
                s = _assembled("lane", "L%d_d%d_g%d" % (length, dist, g), [R.fixed(syms)], L=length, dist=dist, g=g)
                assert len(s.raw) < 1024
                out.append(s)
    return tuple(out)


LANE_SPAN_PREFIX = 40960  # letters: 20 KiB of input


@functools.lru_cache(maxsize=None)
def lane_span():
    """the same behind 20 KiB of 4-bit letters (a span runs, and the distance 32768 is in reach); g takes turns"""
    out, r = [], random.Random(64)
    head = Block(R.FULL_DL, LL_ROOM)
    head.lits(bytes(r.choice(LETTERS) for _ in range(LANE_SPAN_PREFIX)))
    i = 0
    for length in LANE_L:
        for dist in LANE_DIST:
            g = LANE_G[i % len(LANE_G)]
            i += 1
            b = head.fork()
            b.match(length, dist)
            b.lits(bytes(r.choice(LETTERS) for _ in range(g)))
            raw, plain = b.done()
            assert plain is not None and len(raw) > 20 << 10
            out.append(Stream("lane_span", "L%d_d%d_g%d" % (length, dist, g), raw, plain, b.segs, dict(L=length, dist=dist, g=g)))
    return tuple(out)


STORED_LEN = (0, 1, 15, 16, 17, 1023, 1024, 1025, 65535)
STORED_BEHIND = (0, 1, 7, 4097)


@functools.lru_cache(maxsize=None)
def stored():
    out, r = [], random.Random(65)
    for n in STORED_LEN:
        for behind in STORED_BEHIND:
            blocks = ([R.fixed(_lits(r, behind))] if behind else []) + [R.stored(r.randbytes(n))]
            out.append(_assembled("stored", "len%d_behind%d" % (n, behind), blocks, n=n, behind=behind))
    out.append(_assembled("stored", "two_back_to_back", [R.stored(r.randbytes(1000)), R.stored(r.randbytes(17))], n=17, behind=1000))
    return tuple(out)


SPAN_K = (4, 5)
SPAN_D = (-33, -32, -31, -17, -16, -15, -1, 0, 1, 15, 16, 17, 31, 32, 33)
SPAN_FAR_L = (4, 8, 9, 33)


@functools.lru_cache(maxsize=None)
def span():
    """outputs of 4096 k + d bytes: tiles that end with the room, on both sides of the far pass's 32-byte gate and of
    the flush's bytewise tail.  The letter streams end in a far match (its source more than 4096 back) that starts
    within the last 40 bytes; the text streams are the oracle's deflate of util.text."""
    import oracle

    out, r = [], random.Random(66)
    head = Block(R.FULL_DL, LL_ROOM)
    head.lits(bytes(r.choice(LETTERS) for _ in range(16000)))
    i = 0
    for k in SPAN_K:
        for d in SPAN_D:
            n = 4096 * k + d
            length, tail = SPAN_FAR_L[i % 4], i % 7
            i += 1
            b = head.fork()
            b.lits(bytes(r.choice(LETTERS) for _ in range(n - tail - length - 16000)))
            b.match(length, 5000 + 37 * i)
            b.lits(bytes(r.choice(LETTERS) for _ in range(tail)))
            raw, plain = b.done()
            assert plain is not None and len(plain) == n
            out.append(Stream("span", "letters_k%d_d%d" % (k, d), raw, plain, b.segs, dict(k=k, d=d, L=length, tail=tail, made_by="letters")))
            text = util.text(n, 700 + i)
            st, own, _ = oracle.deflate(text, level=2)
            assert st == 0
            out.append(_read("span", "text_k%d_d%d" % (k, d), own, text, k=k, d=d, made_by="oracle"))
    # literals of 2 .. 7 bits (zlib's Z_HUFFMAN_ONLY over 16 skewed symbols): a granule inflates to 10 to 30 bytes, never
    # the same number twice in a row -- the streams of the room sweep (rooms())
    for k, d in ((4, 1), (5, 17)):
        q = np.array([2.0 ** -(1 + j // 2) for j in range(16)])
        plain = (np.random.RandomState(690 + k).choice(16, 4096 * k + d, p=q / q.sum()) * 11 + 5).astype(np.uint8).tobytes()
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
        out.append(_read("span", "skewed_k%d_d%d" % (k, d), c.compress(plain) + c.flush(), plain, k=k, d=d, made_by="zlib_huffman"))
    return tuple(out)


LITERAL_LAST_N = (1, 2, 63, 64, 65, 20000)


@functools.lru_cache(maxsize=None)
def literal_last():
    r = random.Random(67)
    return tuple(_assembled("literal_last", "n%d" % n, [R.fixed(_lits(r, n))], n=n) for n in LITERAL_LAST_N)


@functools.lru_cache(maxsize=None)
def by_blocks():
    """two streams of 256 KiB of output and more from 40 KiB of source and more: a one-stream call, and a batch call
    with max_dst_cap of 256 KiB, decode them by a wave per block"""
    import oracle

    text = util.text(300000, 68)
    st, own, _ = oracle.deflate(text, level=2)
    assert st == 0
    c, parts = zlib.compressobj(6, zlib.DEFLATED, -15), []
    for at in range(0, len(text), 50000):
        parts.append(c.compress(text[at:at + 50000]) + c.flush(zlib.Z_FULL_FLUSH))
    parts.append(c.flush())
    out = (_read("by_blocks", "oracle_level2", own, text, made_by="oracle"),
           _read("by_blocks", "zlib6_full_flush", b"".join(parts), text, made_by="zlib"))
    assert all(len(s.raw) >= 40 << 10 and len(s.plain) >= 256 << 10 for s in out)
    return out


FAMILIES = collections.OrderedDict((f.__name__, f) for f in (run_short, run_long, lane, lane_span, stored, span, literal_last, by_blocks))
# the families whose streams the host model can run (tests/host_sim/sim_inflate.cpp is one wave: no inflate by blocks)
SIM_FAMILIES = tuple(f for f in FAMILIES if f != "by_blocks")

# ---- rooms and items -------------------------------------------------------------------------------------------
ST_OK, ST_SIZE_EXCEEDED, ST_DST_TOO_SMALL = 0, 2, 16
# (limit, dst_cap) of a room R of a stream of N bytes, and the status when R < N
DECLS = (
    ("no limit, cap R", lambda n, r: (None, r), ST_DST_TOO_SMALL),
    ("limit R, cap R", lambda n, r: (r, r), ST_SIZE_EXCEEDED),
    ("limit R, cap R+40", lambda n, r: (r, r + 40), ST_SIZE_EXCEEDED),
    ("limit N+5, cap R", lambda n, r: (n + 5, r), ST_DST_TOO_SMALL),
)
B_INDEXES = (0, 1, 2, 63, 64, 65, 66, -2, -1)
B_OFFSETS = (-1, 0, 1, 15, 16, 17)
OFF_MODS = (0, 1, 5, 15)
CRC_OPS = (0, 1, 2)
GUARD = 64
POISON = 0xA5


def b_positions(stream):
    a = anchors(stream)
    idx = B_INDEXES
    if stream.family == "run_short" and stream.meta["made_by"] in ("oracle", "zlib"):
        idx = (0, 1, -2, -1)
    elif stream.family == "span":
        idx = (-2, -1)
    elif stream.family == "lane" and stream.meta["g"] not in (0, 9):
        idx = ()  # (the match starts where it does for every g: its rooms come with the first and the last g)
    return sorted({a[i][1] for i in idx if -len(a) <= i < len(a)})


SWEEP = 128  # consecutive rooms: more than four granules of the skewed streams inflate to (a granule: 64 bits of input)
SWEEP_STREAMS = ("skewed_k4_d1", "skewed_k5_d17")


def rooms(stream):
    """-> (the rooms that get every declaration: N - 1 and N; those that get one: the failing rooms around the symbol
    starts and tiles, and N + 1; the rooms of the sweep, which get one of the three declarations with dst_cap = R)"""
    n = len(stream.plain)
    near = {n - 1, n}
    fail = {b + o for b in b_positions(stream) for o in B_OFFSETS}
    if stream.family in ("span", "by_blocks"):
        fail |= {n // 2} | {4096 * k + e for k in SPAN_K for e in (-1, 1)}
    # A span's tile holds whole granules (the symbols that start in 64 bits of input), so it ends with the room only where
    # a granule does -- the decoder's business, not to be read off the symbols.  Of SWEEP rooms in a row one is such a room.
    sweep = set(range(n // 2 - SWEEP // 2, n // 2 + SWEEP // 2)) if stream.family == "span" and stream.name in SWEEP_STREAMS else set()
    return (sorted(x for x in near if x >= 0), sorted(x for x in fail if 0 <= x <= n - 1 and x not in near | sweep) + [n + 1],
            sorted(sweep))


# stream: index into the family's streams; R; decl: index into DECLS; limit (None: no limit), cap; want: the status;
# off_mod: dst_off mod 16; crc_op
Item = collections.namedtuple("Item", "family stream R decl limit cap want off_mod crc_op")


@functools.lru_cache(maxsize=None)
def items(family):
    out, turn = [], 0
    streams = FAMILIES[family]()

    def add(si, n, room, decl):
        limit, cap = DECLS[decl][1](n, room)
        i = len(out)
        out.append(Item(family, si, room, decl, limit, cap, ST_OK if room >= n else DECLS[decl][2], OFF_MODS[i % 4], CRC_OPS[i % 3]))

    for si, s in enumerate(streams):
        n = len(s.plain)
        near, fail, sweep = rooms(s)
        for room in near:
            for decl in range(4):
                add(si, n, room, decl)
        for room in fail:
            add(si, n, room, turn % 4)
            turn += 1
        for room in sweep:
            add(si, n, room, (0, 1, 3)[turn % 3])
            turn += 1
    return tuple(out)


def all_items():
    return [it for f in FAMILIES for it in items(f)]


def stream_of(item):
    return FAMILIES[item.family]()[item.stream]


def item_id(item):
    return "%s/%s/R=%d/%s" % (item.family, stream_of(item).name, item.R, DECLS[item.decl][0])


def layout(caps, off_mods):
    """Rooms in one poisoned arena, each with GUARD bytes in front of dst_off and GUARD behind dst_off + cap that
    belong to no other room -> (dst_off [n], arena bytes, [(front slice, back slice)])"""
    offs, guards, cursor = [], [], 0
    for cap, mod in zip(caps, off_mods):
        o = cursor + GUARD
        o += (mod - o) % 16
        offs.append(o)
        guards.append((slice(o - GUARD, o), slice(o + cap, o + cap + GUARD)))
        cursor = o + cap + GUARD
    return np.array(offs, np.uint64), cursor + 256, guards


def zlib_wrap(raw, adler):
    """a deflate stream in RFC 1950's six container bytes (the wrapper of tests/zlib_cases.py's good streams: CMF 0x78,
    FLG with its check bits, the Adler-32 big-endian)"""
    cmf, flg = 0x78, 0x80
    flg += (31 - (cmf * 256 + flg) % 31) % 31
    return bytes([cmf, flg]) + raw + adler.to_bytes(4, "big")


# what test_inflate_room_rules.py::test_the_catalogue asserts: streams and items per family
COUNTS = {"run_short": (28, 1344), "run_long": (41, 1198), "lane": (300, 2940), "lane_span": (36, 471), "stored": (37, 470),
          "span": (62, 1341), "literal_last": (6, 54), "by_blocks": (2, 125)}
DST_BYTES = 88967457
