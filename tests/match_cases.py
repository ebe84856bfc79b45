"""Named, deterministic inputs for the match finder, built to land on lz_match's seams (tests/test_match_rules.py holds
tests/host_sim/sim_match.cpp's reference to them on the CPU, tests/test_gpu_match_records.py the kernels' records to the
reference).  No GPU, no library: bytes and what each was planted for.

A case is a Stream: a name, its bytes and a list of properties.  A property is a tuple the CPU test evaluates on the
REFERENCE's records of that stream at one level (K, Kq):
  ("rec", p, fn, first, best)        fn(K, Kq) -> (best, first) expected at position p
  ("span", lo, hi, fn, first, best)  the same for every position lo <= p < hi: fn(p, K, Kq) -> (best, first)
                        (first, best: the levels at which that half is asserted.  The hash has 15 bits and the window 32 768
                        positions: in random bytes a position's chain holds about one hash-only candidate per window, so in
                        front of a far candidate one may come first -- `first` then says nothing at `Fast, Kq = 1 -- or, from
                        the far end of the window, four may fill K = 4.)
  ("two", lo, hi, levels)  at those levels some position in [lo, hi) has first != best (MATCH_SNAP, snap[], snap_used)
  ("no_two",)           no position has: snap_used stays 0
  ("share", lo, hi, a, b)  the share of the positions in [lo, hi) that have a match lies in [a, b]
Records are packed dist << 9 | len, 0 for none.

The long streams are prefixes of seven BASES of 82 192 bytes (tile 0 is 49 152 positions, the others 16 384: forms.h), cut
at the 36 lengths 49 152 + 16 384 k + d that put the stream's end on either side of a tile end, of the last staged
source byte (t1 + 264) and of the 16-byte tail; what a base plants near position p holds in every prefix that reaches
p + 258, and the three bases with copied regions around the tile ends give every prefix an end whose matches the
stream's end caps."""
import random

T0, TILE = 49152, 16384            # forms.h MATCHW_TILE0, MATCHW_TILE
TILE_STARTS = (T0, T0 + TILE, T0 + 2 * TILE)
BASE_LEN = T0 + 2 * TILE + 272
END_D = (-1, 0, 1, 3, 4, 5, 258, 263, 264, 265, 271, 272)
WINDOW = 32768
MAXLEN = 258
REGION = 300                       # a copied region is [t - REGION, t + REGION)

# 4-byte strings of equal hash4 and different first bytes, found by a search with the reference's hash4 (sim_match_hash4;
# tests/test_match_rules.py checks them): (the probe's, the fillers')
COLLIDING = [(b"\xc0\xdc\xc5\xd3", b"\xc1\xd2\xc0\xd0"), (b"\xc0\xdc\xc5\xd4", b"\xc1\xd2\xc0\xd1"), (b"\xc0\xdc\xc5\xd5", b"\xc1\xd2\xc0\xd2"),
             (b"\xc0\xdc\xc7\xd3", b"\xc1\xd2\xc2\xd0"), (b"\xc0\xdc\xc9\xd3", b"\xc1\xd2\xc4\xd0")]
LEVEL_K = {1: (4, 1), 2: (128, 32), 3: (4096, 1024)}
WORDS = [b"deflate", b"inflate", b"huffman", b"window", b"stream", b"block", b" ", b" the ", b"zip", b"archive", b"\n", b"checksum",
         b"0123456789"]


ALL, DEEP = (1, 2, 3), (2, 3)


def rec(dist, length):
    return (dist << 9) | length


def at_(p, fn, first=ALL, best=ALL):
    return ("rec", p, fn, first, best)


def span(lo, hi, fn, first=ALL, best=ALL):
    return ("span", lo, hi, fn, first, best)


class Stream:
    def __init__(self, name, data, props=(), base=None):
        self.name, self.data, self.props, self.base = name, bytes(data), list(props), base

    def __len__(self):
        return len(self.data)


def tile_of(p):
    """(tile index, offset in the tile) of position p as lz_match_window_kernel cuts a stream"""
    return (0, p) if p < T0 else (1 + (p - T0) // TILE, (p - T0) % TILE)


def _background(seed, n=BASE_LEN):
    return bytearray(random.Random(seed).randbytes(n))


def _text(n, seed):
    r = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        out += r.choice(WORDS)
    return bytes(out[:n])


# ---- chains of exactly n candidates whose longest is the n-th (the K rule) --------------------------------------------
def _k_group(g, n):
    """the n-th candidate from the probe is the one long match (10 bytes), the n - 1 nearer ones share 4 bytes and no more:
    -> (bytes, offset of the probe, fn(K, Kq) -> (best, first) at the probe)"""
    token, mark = bytes([0xF0 + g, 0xFD, 0xFE, 0xFF]), bytes([0xE0 + g]) * 6
    out = bytearray(token + mark + b"\x01\x02")
    for c in range(n - 1):
        out += token + bytes([(c >> 14) & 127, (c >> 7) & 127, c & 127])
    probe = len(out)
    out += token + mark + b"\x03\x04"
    near = rec(7, 4) if n > 1 else 0  # the nearest filler: every filler ties at 4 bytes

    def want(K, Kq):
        return (rec(probe, 10) if n <= K else near, rec(probe, 10) if n <= Kq else near)
    return bytes(out), probe, want


def _collide_group(pair, mark, n_fill):
    """the probe's chain holds n_fill candidates of equal hash that share no byte with it, then the one real match: found
    iff n_fill < K -- the hash-only candidates count"""
    c1, c2 = pair
    out = bytearray(c1 + bytes([mark]) * 6 + b"\x01\x02") + c2 * n_fill
    probe = len(out)
    out += c1 + bytes([mark]) * 6 + b"\x03\x04"

    def want(K, Kq):
        return (rec(probe, 10) if n_fill + 1 <= K else 0, rec(probe, 10) if n_fill + 1 <= Kq else 0)
    return bytes(out), probe, want


def _plant(data, props, at, group):
    blob, probe, want = group
    data[at:at + len(blob)] = blob
    props.append(at_(at + probe, want))
    return at + len(blob)


def _k_low(data, props, at):
    """the K-rule chains of `Fast and `Default (Kq, Kq + 1, K, K + 1 candidates) and their hash-only twins, from `at` on"""
    g = 0
    for level in (1, 2):
        K, Kq = LEVEL_K[level]
        for n in (Kq, Kq + 1, K, K + 1):
            at = _plant(data, props, at, _k_group(g, n)) + 16
            g += 1
    for i, n_fill in enumerate((3, 4, 127, 128)):  # K - 1 and K colliding candidates in front of the match
        at = _plant(data, props, at, _collide_group(COLLIDING[i], 0xD8 + i, n_fill)) + 16
    return at


# ---- the bases --------------------------------------------------------------------------------------------------------
def _copied_regions(data, props, dist):
    """[t - 300, t + 300) around every tile start is a copy from `dist` before: each position there has ONE candidate, at
    that distance, with 258 bytes (or none: dist beyond the window); the byte behind the region differs"""
    for t in TILE_STARTS:
        lo, hi = t - REGION, min(t + REGION, BASE_LEN)
        data[lo:hi] = data[lo - dist:hi - dist]
        if hi < BASE_LEN:
            data[hi] = data[hi - dist] ^ 0xFF
        want = rec(dist, MAXLEN) if dist <= WINDOW else 0
        far = dist == WINDOW
        props.append(span(lo, hi - MAXLEN + 1, lambda p, K, Kq, w=want: (w, w), first=DEEP if want else ALL, best=DEEP if far else ALL))
        if far:  # the seams themselves at every level: p = t0, t0 + 1 and, for the tile before, t1 - 1
            for p in (t - 1, t, t + 1):
                props.append(at_(p, lambda K, Kq, w=want: (w, w), first=DEEP))


def base_cross():
    """copies at distance 777 across every tile end (a match of 258 starts at t1 - 258, t1 - 257, t1 - 1 and its bytes run
    to t1 + 256); equal longest candidates; chains whose third candidate lies beyond the window"""
    d, props = _background(101), []
    _copied_regions(d, props, 777)
    u = bytes(range(0x90, 0x9A))  # two candidates with the same 10 bytes: the nearer one wins
    for k, tail in enumerate((b"\x01", b"\x02", b"\x03")):
        d[20000 + 100 * k:20000 + 100 * k + 11] = u + tail
    props.append(at_(20200, lambda K, Kq: (rec(100, 10), rec(100, 10))))
    _beyond_window(d, props, 70000)  # tile 2 stages from 32 768 on: the third candidate, at 37 100, is in its window's LDS
    return d, props


def _beyond_window(d, props, p):
    """links of 100, 100 and 32 700, each inside the window; the third candidate lies 32 900 back and is the longest of the
    three: the walk stops there.  At `Fast the second candidate is the better of the two that count: two answers."""
    w = bytes([0xA0 + (p // 1000) % 16]) + bytes(range(0x70, 0x83))
    d[p - 32900:p - 32900 + 20] = w
    d[p - 200:p - 200 + 20] = w[:6] + bytes(14)
    d[p - 100:p - 100 + 20] = w[:5] + b"\xff" * 15
    d[p:p + 20] = w
    props.append(at_(p, lambda K, Kq: (rec(200, 6), rec(200, 6) if Kq >= 2 else rec(100, 5))))


def base_edge(dist):
    """the same regions copied from exactly 32 768 before (found: the candidate of p = t0 is the first staged position w0,
    and so on for t0 + 1 and t1 - 1 of tiles 1 and 2) or from 32 769 (not found); nothing else: no second answer anywhere"""
    d, props = _background(102 if dist == WINDOW else 103), []
    _copied_regions(d, props, dist)
    if dist > WINDOW:
        props.append(("no_two",))
    return d, props


def base_k3a():
    """`Best's chains of Kq, Kq + 1 (in tile 2: two answers there at `Best) and K candidates, the last one across the first
    tile end; period 257 across the second, period 258 across the third"""
    d, props = _background(104), []
    _plant(d, props, 1000, _k_group(8, 1024))
    _plant(d, props, 67000, _k_group(9, 1025))
    _plant(d, props, 30000, _k_group(10, 4096))
    _periodic(d, props, 257, TILE_STARTS[1] - 600, TILE_STARTS[1] + 600, 41)
    _periodic(d, props, 258, TILE_STARTS[2] - 1000, BASE_LEN, 42)
    props.append(("two", TILE_STARTS[1], TILE_STARTS[2], (3,)))
    return d, props


def base_k3b():
    """`Best's chain of K + 1 candidates across two tile ends, 4096 hash-only candidates in front of a match, the chains of
    the lower levels, period 259 across the third tile end"""
    d, props = _background(105), []
    _k_low(d, props, 1000)
    _plant(d, props, 10000, _collide_group(COLLIDING[4], 0xDF, 4096))
    _plant(d, props, 38000, _k_group(11, 4097))
    _periodic(d, props, 259, TILE_STARTS[2] - 1000, BASE_LEN, 43)
    return d, props


def _periodic(data, props, period, lo, hi, seed):
    unit = bytes([seed]) * period if period == 1 else (random.Random(seed).randbytes(period) if period > 3 else bytes(range(0xB1, 0xB1 + period)))
    data[lo:hi] = (unit * ((hi - lo) // period + 1))[:hi - lo]
    if hi < BASE_LEN:
        data[hi] = data[hi - period] ^ 0xFF
    # from one period in, the nearest candidate is one period back and matches to the cap (the walk's l == maxlen exit)
    props.append(span(lo + period, hi - MAXLEN + 1, lambda p, K, Kq, w=rec(period, MAXLEN): (w, w), first=ALL if period <= 3 else DEEP))


def base_runs():
    """a run of one byte across the first tile end, period 2 across the second, period 3 across the third"""
    d, props = _background(106), []
    _periodic(d, props, 1, TILE_STARTS[0] - 600, TILE_STARTS[0] + 600, 0xAA)
    _periodic(d, props, 2, TILE_STARTS[1] - 600, TILE_STARTS[1] + 600, 0)
    _periodic(d, props, 3, TILE_STARTS[2] - 600, BASE_LEN, 0)
    props.append(("no_two",))
    return d, props


def base_pool():
    """text-like stretches of 20 000 bytes (many candidates everywhere) between stretches of random bytes (none), so that the
    per-tile form rule flips from tile to tile; the last 4096 positions of tile 0 lie in text: long chains where the pool
    hands out its small chunks (POOL_TAPER)"""
    d, props = _background(107), []
    for k, lo in enumerate(range(0, BASE_LEN, 40000)):
        hi = min(lo + 20000, BASE_LEN)
        d[lo:hi] = _text(hi - lo, 200 + k)
    _beyond_window(d, props, TILE_STARTS[1] + 50)  # ... the third candidate, at 32 686, lies below what tile 2 stages
    props.append(("share", T0 - 4096, T0, 0.9, 1.0))
    props.append(("share", 20000 + MAXLEN, 40000 - MAXLEN, 0.0, 0.01))
    props.append(("two", TILE_STARTS[0], TILE_STARTS[1], (1, 2)))  # a record with first != best in tile 1 (at `Best: base_k3a's, in tile 2)
    return d, props


BASES = ("cross", "edge32768", "edge32769", "k3a", "k3b", "pool", "runs")
CAPPED_END = {"cross": 777, "edge32768": WINDOW, "edge32769": 0}  # bases whose every prefix ends inside a copied region: the distance (0: none found)


def _bases():
    return {"cross": base_cross(), "edge32768": base_edge(WINDOW), "edge32769": base_edge(WINDOW + 1), "k3a": base_k3a(),
            "k3b": base_k3b(), "pool": base_pool(), "runs": base_runs()}


def _cut(props, n):
    """the properties of a base that hold in its prefix of n bytes: those whose positions' 258 bytes lie inside it"""
    out = []
    for pr in props:
        if pr[0] == "rec" and pr[1] + MAXLEN <= n:
            out.append(pr)
        elif pr[0] == "span" and min(pr[2], n - MAXLEN + 1) > pr[1]:
            out.append(("span", pr[1], min(pr[2], n - MAXLEN + 1)) + pr[3:])
        elif pr[0] in ("two", "share") and pr[2] + MAXLEN <= n:
            out.append(pr)
        elif pr[0] == "no_two":
            out.append(pr)
    return out


def long_streams():
    """the 36 tile-end lengths, longest first, dealt to the bases in turn: every base gets lengths of every k"""
    bases = _bases()
    lengths = sorted((T0 + TILE * k + dd for k in range(3) for dd in END_D), reverse=True)
    out = []
    for i, n in enumerate(lengths):
        b = BASES[i % len(BASES)]
        data, props = bases[b]
        props = _cut(props, n)
        if b in CAPPED_END:  # the last positions' one candidate matches up to the stream's end: every len - p in 4 .. 258
            dist = CAPPED_END[b]
            props.append(span(n - MAXLEN, n - 3, lambda p, K, Kq, n=n, dist=dist: (rec(dist, n - p),) * 2 if dist else (0, 0),
                              first=DEEP if dist else ALL, best=DEEP if dist == WINDOW else ALL))
        out.append(Stream("%s_%d" % (b, n), data[:n], props, base=b))
    return out


def small_streams():
    """streams of up to 8192 bytes (forms.h MATCHW_SMALL): lz_match_kernel's, 1024 positions a workgroup"""
    out = [Stream("empty", b""), Stream("len3", b"abc")]
    for n in (4, 5, 7, 8, 11):  # no 8-byte load fits the compare
        out.append(Stream("a%d" % n, b"a" * n, [span(1, n - 3, lambda p, K, Kq, n=n: (rec(1, n - p),) * 2), at_(0, lambda K, Kq: (0, 0))]))
    unit = random.Random(7).randbytes(300)
    for n in (1023, 1024, 1025, 1026, 1027, 1028):  # the last position on either side of the chunk's end
        out.append(Stream("per300_%d" % n, (unit * 4)[:n], [span(300, n - 3, lambda p, K, Kq, n=n: (rec(300, min(MAXLEN, n - p)),) * 2, first=DEEP)]))
    # a run of zeros to the stream's end: what would match on behind it if the end did not cap the compare
    out.append(Stream("zeros_tail", random.Random(8).randbytes(100) + bytes(600), [span(101, 697, lambda p, K, Kq: (rec(1, min(MAXLEN, 700 - p)),) * 2)]))
    for n in (8191, 8192):
        d, props = _background(300 + n, n), []
        end = _k_low(d, props, 100)
        d[end:] = _text(n - end, 9)
        props.append(("two", 100, end, (1, 2)))
        out.append(Stream("klow_%d" % n, d, props))
    return out


def window_8193():
    """one byte above MATCHW_SMALL: the same content by lz_match_window_kernel"""
    d, props = _background(301, 8193), []
    end = _k_low(d, props, 100)
    d[end:] = _text(8193 - end, 9)
    props.append(("two", 100, end, (1, 2)))
    return Stream("klow_8193", d, props)


def tiny_streams(count):
    """streams of 0, 3, 4, 15, 16 and 17 bytes: inside a call of long ones they have no (whole unit of) source to stage, and
    enough of them give a workgroup several groups one behind the other (forms.h gpw)"""
    out = []
    for i in range(count):
        n = (0, 3, 4, 15, 16, 17)[i % 6]
        out.append(Stream("tiny%d_%d" % (n, i), (bytes([0x41 + i % 7, 0x42, 0x43, 0x44]) * 5)[:n]))
    return out


TINY = 1070


def ragged_batch():
    """the window kernel's call: the 36 long streams, the 8193-byte one and TINY tiny ones, mixed -- a long stream after every
    29 tiny ones, so that workgroups that take several groups cross from stream to stream"""
    longs, tiny = long_streams() + [window_8193()], tiny_streams(TINY)
    out, k = [], 0
    for i, t in enumerate(tiny):
        if i % 29 == 3 and k < len(longs):
            out.append(longs[k])
            k += 1
        out.append(t)
    assert k == len(longs)
    return out


def batches():
    """name -> streams of one call"""
    return {"small": small_streams(), "alone8193": [window_8193()], "ragged": ragged_batch()}
