"""Named, deterministic inputs for the hash-chain links, built to land on lz_chain's seams (tests/test_chain_rules.py holds
tests/host_sim/sim_chain.cpp's reference and models to them on the CPU, tests/test_gpu_chain_links.py the four kernels'
links to the reference).  No GPU, no library: bytes and what each was planted for.

A case is a Stream: a name, its bytes, one line on what it is for, and a list of properties.  A property is a tuple the
CPU test evaluates on the REFERENCE's links of that stream (link = distance to the nearest earlier position of equal
hash if at most 32 768, else 0):
  ("link", p, d)            links[p] == d
  ("span", lo, hi, d)       links[p] == d for every lo <= p < hi
  ("only", word, positions) the hash of the 4-byte `word` occurs at exactly these positions of the stream -- the filler
                            never has it -- so the previous occurrence of each, window or no window, is the one before
                            it in the list: exactly one planted gap back
  ("share", lo, hi, a, b)   the share of the positions in [lo, hi) that have a link lies in [a, b]
  ("mean", lo, hi, a, b)    the mean link of [lo, hi) lies in [a, b]

The seams: lz_chain_kernel works in rounds of 1024 positions (CHAIN_ROUND), keeps positions mod 2^16 and sweeps its table
every 16 384 (SWEEP_PERIOD), takes a neighbour within NEAR = 8 for its predecessor once a round needs more than
PLAIN_TURNS turns; lz_chain_xchg_kernel hands a turn of 1024 positions (16 exchanges of 64 lanes) from wave to wave, four
waves; the forms by segments cut a stream every 32 768, 65 536 or 131 072 (peel) or 98 304 << k (exchange) positions and
warm an empty table up with the 32 768 positions before a segment."""
import random

import util

ROUND = 1024        # deflate.hip CHAIN_ROUND, and XCHG_TURN = 64 * XCHG_U
XCHG_WAVES = 4
SWEEP = 16384       # forms.h SWEEP_PERIOD
WINDOW = 32768
NEAR = 8
PEEL_SEGS = (32768, 65536, 131072)  # forms.h CHAIN_SEG_MIN .. CHAIN_SEG_MAX
XCHG_SEGS = (98304, 196608)         # forms.h xseg: 96 Ki << k
SPARE = 64          # bytes behind the arena of a call


class Stream:
    def __init__(self, name, data, what, props=()):
        self.name, self.data, self.what, self.props = name, bytes(data), what, list(props)

    def __len__(self):
        return len(self.data)


def _symbols(n, seed, bits):
    """n random symbols of `bits` bits"""
    return random.Random(seed).randbytes(n).translate(bytes(i & ((1 << bits) - 1) for i in range(256)))


# ---- the contents the short streams rotate over ----------------------------------------------------------------------
KINDS = ("zeros", "period2", "text", "random", "bits1", "bits2")


def _content(kind, n, seed):
    """-> (bytes, properties)"""
    if kind == "zeros":  # one hash, every position: the first has no link, every other one links one back
        return bytes(n), ([("link", 0, 0), ("span", 1, n - 3, 1)] if n >= 4 else [])
    if kind == "period2":
        props = [("link", p, 0) for p in range(min(2, max(n - 3, 0)))] + [("span", 2, n - 3, 2)]
        return (b"ab" * (n // 2 + 1))[:n], props if n >= 4 else []
    if kind == "text":
        return util.text(n, seed), []
    if kind == "random":
        return random.Random(seed).randbytes(n), []
    return _symbols(n, seed, 1 if kind == "bits1" else 2), []


TINY = (0, 1, 3, 4, 5, 7)
# len - 4 (the last position) on either side of: a wave, a round, two rounds, a sweep, the window
EDGE_LAST = (63, 64, 65, 1023, 1024, 1025, 2047, 2048, 16383, 16384, 16385, 32767, 32768, 32769)
MID = (40000, 55555, 65540, 70001)


def edges_batch():
    """about 60 short streams, to be packed end to end without a gap: a read past a stream's end sees its neighbour, a link
    stored past len - 4 lands in a slot the test requires untouched"""
    out, k = [], 0

    def add(n, why):
        nonlocal k
        kind = KINDS[k % len(KINDS)]
        data, props = _content(kind, n, 500 + k)
        out.append(Stream("%s_%d" % (kind, n), data, why, props))
        k += 1

    tiny = list(TINY)
    for j, last in enumerate(EDGE_LAST):
        for _ in range(3):
            add(last + 4, "the last position, %d, next to a multiple of %d" % (last, 64 if last < 100 else 1024 if last < 3000 else SWEEP))
        if j % 2 == 0 and tiny:  # a stream without positions (or with one, two, four) between longer ones
            n = tiny.pop(0)
            add(n, "%d bytes: %s" % (n, "no position" if n < 4 else "%d position(s)" % (n - 3)))
        k += 1  # (the next length starts on another content than this one did)
    for n in tiny:
        add(n, "%d bytes" % n)
    for n in MID:
        add(n, "more than a window, less than two; the last round holds %d positions" % ((n - 4) % ROUND + 1))
    assert len({s.name for s in out}) == len(out)
    return out


# ---- the long streams ------------------------------------------------------------------------------------------------
def _word(i):
    """planted 4-byte words: bytes no filler of few-bit symbols has"""
    return bytes([0x80 + i, 0x91, 0xA2, 0xB3])


# word -> its positions in the `window` stream.  own_lo: a segment's first position.
WINDOW_PLANTS = {
    # 32 768 apart, each later one the first position of a segment of every form, the earlier one exactly own_lo - 32768: the
    # first position a segment's warm-up inserts (exchange 96 Ki: 98 304 and 196 608; 192 Ki: 196 608; peel 32 Ki: all four,
    # 64 Ki: 131 072 and 196 608, 128 Ki: 131 072), and the first one a sweep at that position must keep
    0: [65536, 98304, 131072, 163840, 196608],
    # the earlier one at own_lo - 32769 (exchange 96 Ki and peel 32 Ki: own_lo = 294 912): one before the warm-up, no link
    1: [262143, 294912],
    # 32 767 back from the first position of the peel segment at 32 768, whose warm-up starts at 0
    2: [1, 32768],
    # the gaps around the window, then beyond it: 32767, 32768, 32769, 49152, 65535, 65536
    3: [5000, 37767, 70535, 103304, 152456, 217991, 283527],
    # 65541 (5 in 16 bits), 81920 (16384 in 16 bits), 131075 (3 in 16 bits): a table of positions mod 2^16 must not find these
    4: [20000, 85541, 167461, 298536],
}
WINDOW_GAPS = (32767, 32768, 32769, 49152, 65535, 65536, 65541, 81920, 131075)


def window_stream():
    n = 10 * WINDOW + 1 + 4  # the last position is 32768 k + 1
    d, props = bytearray(_symbols(n, 11, 3)), []  # 3-bit symbols: 4096 different words, none with a planted word's hash (seed 11)
    for w, ps in WINDOW_PLANTS.items():
        for p in ps:
            d[p:p + 4] = _word(w)
        props.append(("only", _word(w), tuple(ps)))
        props.append(("link", ps[0], 0))
        for a, b in zip(ps, ps[1:]):
            props.append(("link", b, b - a if b - a <= WINDOW else 0))
    return Stream("window", d, "one word at gaps around and beyond the window, on the segments' first positions and warm-up edges", props)


# (first, behind the last, byte) of the runs of the `runs` stream
RUNS = (
    (900, 1200, 0x11),        # across a round edge: 1024
    (4000, 8300, 0x22),       # across the turns of all four waves and their hand-overs: 4096 .. 8192
    (16000, 16800, 0x55),     # across a sweep: 16 384
    (98000, 98700, 0x33),     # across an exchange segment's edge: 98 304
    (130900, 131300, 0x44),   # across a peel segment's edge: 131 072
    (160768, 230768, 0x00),   # longer than two windows; starts on a round's first position with the hash of the empty word
)


def runs_stream():
    n = 3 * 98304 - 1 + 4  # the last position is 98304 k - 1: the segment behind it holds no position
    d, props = bytearray(random.Random(12).randbytes(n)), []
    for lo, hi, b in RUNS:
        d[lo:hi] = bytes([b]) * (hi - lo)
        d[lo - 1], d[hi] = b ^ 0xEE, b ^ 0xFF
        props.append(("span", lo + 1, hi - 3, 1))
    assert RUNS[-1][0] % ROUND == 0 and RUNS[-1][1] - RUNS[-1][0] > 2 * WINDOW
    props.append(("link", RUNS[-1][0], 0))  # no word of zeros before the long run
    return Stream("runs", d, "runs of one byte across round, turn, sweep and segment edges, one longer than two windows", props)


# period -> the round edge (a multiple of 1024) its stretch of 3000 positions lies across
PERIODS = {2: 20 * ROUND, 3: 40 * ROUND, 7: 60 * ROUND, 8: 98304, 9: SWEEP, 16: 131072, 17: 200 * ROUND}


def periods_stream():
    n = 7 * WINDOW + 4  # the last position is 32768 k: a segment of one position
    d, props = bytearray(random.Random(13).randbytes(n)), []
    for period, edge in PERIODS.items():
        lo, hi = edge - 1500, edge + 1500
        unit = bytes((0x30 + 7 * period + j) & 0xFF for j in range(period))
        d[lo:hi] = (unit * (3000 // period + 1))[:3000]
        d[hi] = d[hi - period] ^ 0xFF
        props.append(("span", lo + period, hi - 3, period))  # from the second repeat on
    return Stream("periods", d, "periods 2, 3, 7, 8, 9, 16 and 17 across round edges: either side of NEAR, the long peel", props)


ALPHABETS = ((97000, 127000, 1), (180000, 210000, 2))  # (first, behind the last, bits a symbol)


def alphabets_stream():
    n = 3 * 98304 + 4  # the last position is 98304 k: a segment of one position
    d, props = bytearray(random.Random(14).randbytes(n)), []
    for lo, hi, bits in ALPHABETS:
        d[lo:hi] = _symbols(hi - lo, 15 + bits, bits)
        words = 1 << (4 * bits)  # that many different words, about that far apart
        props.append(("share", lo + 20 * words, hi - 3, 0.999, 1.0))
        props.append(("mean", lo + 20 * words, hi - 3, 0.7 * words, 1.3 * words))
    return Stream("alphabets", d, "30 KB each of 1-bit and 2-bit symbols: chains thousands deep, many lanes an address", props)


def text_stream():
    n = 3 * 98304 + 1 + 4
    return Stream("text", util.text(n, 31), "text: the last position is 98304 k + 1", [("share", 1000, n - 3, 0.99, 1.0)])


def random_stream():
    n = 8 * WINDOW - 1 + 4
    # a hash of 15 bits and a window of 32 768: a position has an earlier one of its hash with probability 1 - 1/e
    return Stream("random", random.Random(16).randbytes(n), "random bytes: the last position is 32768 k - 1", [("share", WINDOW, n - 3, 0.60, 0.66)])


def long_batch():
    return [window_stream(), runs_stream(), periods_stream(), alphabets_stream(), text_stream(), random_stream()]


_BATCHES = {}


def batches():
    """name -> streams of one call (built once)"""
    if not _BATCHES:
        _BATCHES.update(edges=edges_batch(), long=long_batch())
    return _BATCHES


def arena(streams):
    """the call's source arena: the streams end to end, no gap, SPARE bytes behind"""
    return b"".join(s.data for s in streams) + bytes(SPARE)


# ---- where a position lies in each form (what a failure names) -----------------------------------------------------------
CHAIN_NAMES = ("exchange whole", "exchange segments", "peel whole", "peel segments")  # forms.h ChainKernel


def where(p, chain, seg_positions):
    """position p as the form (chain, seg_positions) takes it: round and offset, the exchange kernel's turn, wave and lane, the
    segment and the offset in it"""
    out = "round %d + %d" % (p // ROUND, p % ROUND)
    own_lo = p // seg_positions * seg_positions if seg_positions else 0
    if chain < 2:
        t_first = max(own_lo - WINDOW, 0) // ROUND
        out += ", turn %d wave %d exchange %d lane %d" % (p // ROUND, (p // ROUND - t_first) % XCHG_WAVES, p % ROUND // 64, p % 64)
    if seg_positions:
        out += ", segment %d + %d" % (p // seg_positions, p - own_lo)
    return out
