"""Inputs for the Adler-32 chunk chain and the CRC-32 finish, shared by tests/test_adler_chain_sim.py (CPU, against the
host model of zipc_amd/csrc/adler_chain.h) and tests/test_gpu_checksum_chain.py (the kernels).  numpy only.

The reference (zd.ml:175-198) walks a buffer in chunks of 5552 bytes, the first one of len mod 5552, and takes the SIGNED
32-bit remainder of s1 and s2 behind each.  With S1 = sum b_i and S2 = sum (n - i) b_i of a chunk and x = s2 before it,
s2 behind it is srem(wrap32(x + C)), C = n * s1 + S2.  The kernels predict the branch from C alone and replay the
chunks whose branch depends on x: C below 65521 ("low"), or within 65521 of 2^31 ("mid").  Random data has next to
none of them, so they are planned here: a Planner follows the reference's (s1, s2) through a buffer and chooses the sums
of a chunk so that it is of the kind wanted, chunk_with_sums() makes bytes with exactly those sums."""
import random

import numpy as np

N = 5552       # zd.ml:180,196
P = 65521      # zd.ml:172
HALF = 1 << 31


# ---- bytes with given sums -----------------------------------------------------------------------------------------

def _front(n, m):
    """S2 of m units packed into the first bytes of n (255 a byte)"""
    q, r = divmod(m, 255)
    return 255 * (q * n - q * (q - 1) // 2) + r * (n - q)


def _end(n, m):
    """S2 of m units packed into the last bytes of n"""
    q, r = divmod(m, 255)
    return 255 * q * (q + 1) // 2 + r * (q + 1)


def s2_range(n, S1):
    """the least and greatest S2 = sum (n - i) b_i of n bytes whose sum is S1.  Every integer between is reachable:
    moving one unit of a byte one position forward adds exactly 1."""
    assert 0 <= S1 <= 255 * n
    return _end(n, S1), _front(n, S1)


def chunk_sums(b):
    b = np.asarray(b, dtype=np.int64)
    return int(b.sum()), int((b * np.arange(len(b), 0, -1, dtype=np.int64)).sum())


def chunk_with_sums(n, S1, S2):
    """n bytes (uint8 array) with sum S1 and sum (n - i) b_i = S2: m units packed at the front, the others at the end --
    S2 grows with m -- and one unit of the end pack moved forward by what is still missing"""
    lo, hi = s2_range(n, S1)
    assert lo <= S2 <= hi, (n, S1, S2, lo, hi)
    a, z = 0, S1  # the largest m with S2(m) <= S2
    while a < z:
        m = (a + z + 1) // 2
        if _front(n, m) + _end(n, S1 - m) <= S2:
            a = m
        else:
            z = m - 1
    m = a
    b = np.zeros(n + 1, np.int64)  # (one spare byte in front of an empty pack's remainder: always 0)
    qf, rf = divmod(m, 255)
    b[:qf] = 255
    b[qf] += rf
    qe, re = divmod(S1 - m, 255)
    if qe:
        b[n - qe:n] = 255
    if re:
        b[n - qe - 1] += re
    D = S2 - _front(n, m) - _end(n, S1 - m)
    if D:
        pe = n - qe - 1 if re else n - qe  # the end pack's first unit; D < its distance to the front pack's next place
        b[pe] -= 1
        b[pe - D] += 1
    b = b[:n]
    assert 0 <= b.min() and b.max() <= 255
    return b.astype(np.uint8)


# ---- the reference's walk over chunk sums, in Python's integers ------------------------------------------------------

def _wrap32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v & HALF else v


def _srem(v, m):  # Int32.rem: the sign of the dividend
    return -((-v) % m) if v < 0 else v % m


def ref_step(s1, s2, n, S1, S2):
    """zd.ml:182-196 for one chunk, from its sums: the byte loop's wrapping adds come to one wrap at the end"""
    return _srem(_wrap32(s1 + S1), P), _srem(_wrap32(s2 + n * s1 + S2), P)


def kind_of(C):
    """how the kernels see a chunk by C alone: "low", "mid" (both ambiguous) or None"""
    if C < P:
        return "low"
    if HALF - P < C < HALF + P:
        return "mid"
    return None


def walk(sums, length, per=1):
    """The serial walk over the chunk sums [(S1, S2)] of a buffer of `length` bytes (chunk 0: its first length % 5552
    bytes).  -> (the Adler-32, counts): what the conditions on a plan are counted by, never by the code under test.
      low, mid         ambiguous chunks of each kind
      low_neg_stay     low chunks entered with s2 < 0 whose s2 + C is still negative
      low_neg_cross    low chunks entered with s2 < 0 that bring it to >= 0
      mid_against      mid chunks whose branch x decides against C: (x + C >= 2^31) != (C >= 2^31)
      pairs            pairs of adjacent ambiguous chunks
      open_run         ambiguous chunks at k = 0 mod per"""
    assert len(sums) == (length // N + 1 if length else 0)
    c = dict(low=0, mid=0, low_neg_stay=0, low_neg_cross=0, mid_against=0, pairs=0, open_run=0)
    s1, s2, prev_amb = 1, 0, False
    for k, (S1, S2) in enumerate(sums):
        n = length % N if k == 0 else N
        C = n * s1 + S2
        assert C < 1 << 32
        kind = kind_of(C)
        if kind:
            c[kind] += 1
            c["pairs"] += prev_amb
            c["open_run"] += k % per == 0
            if kind == "low" and s2 < 0:
                c["low_neg_stay" if s2 + C < 0 else "low_neg_cross"] += 1
            if kind == "mid" and (s2 + C >= HALF) != (C >= HALF):
                c["mid_against"] += 1
        prev_amb = kind is not None
        s1, s2 = ref_step(s1, s2, n, S1, S2)
    return ((s2 << 16) + s1) & 0xFFFFFFFF, c


# ---- the planner -----------------------------------------------------------------------------------------------------

class Planner:
    """Follows the reference's (s1, s2) and emits the sums of 5552-byte chunks of chosen kinds:
      neg    C >= 2^31 + 65521 (s2 <= 0 behind it, whatever it was), leaving s1 in 1..3 and s2 below -60000
      low    C < 65521 (needs s1 <= 11, so it follows a neg or a low); "low-" keeps a negative s2 negative, "low+" brings
             it to >= 0, "low" takes what comes
      mid    x + C within 3 of 2^31, from whichever sign x has; "mid!" so that x decides the branch against C
      free   the sums given (a chunk of the pool the plan is spliced into), or random ones"""

    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.s1, self.s2 = 1, 0
        self.sums, self.kinds = [], []

    def _emit(self, kind, S1, S2, n=N):
        lo, hi = s2_range(n, S1)
        assert lo <= S2 <= hi, (kind, S1, S2)
        self.sums.append((S1, S2))
        self.kinds.append(kind)
        self.s1, self.s2 = ref_step(self.s1, self.s2, n, S1, S2)

    def free(self, sums=None, n=N):
        if sums is None:
            S1 = self.rng.randrange(0, 255 * n + 1)
            sums = (S1, self.rng.randint(*s2_range(n, S1)))
        self._emit("free", sums[0], sums[1], n)

    def neg(self):
        rng = self.rng
        for _ in range(1000):
            S1 = (rng.randrange(1, 4) - self.s1) % P + P * rng.randrange(11, 19)
            lo, hi = s2_range(N, S1)
            # t = x + C must come out at v = srem(t - 2^32) in (-65521, -60000): t = 2^32 + v - m p
            v = -rng.randrange(60001, P)
            t_lo = max(HALF + P + abs(self.s2), self.s2 + N * self.s1 + lo)
            t_hi = min((1 << 32) - 1, self.s2 + N * self.s1 + hi)
            m_lo, m_hi = -((t_hi - (1 << 32) - v) // P), ((1 << 32) + v - t_lo) // P
            if m_lo > m_hi:
                continue
            t = (1 << 32) + v - rng.randint(m_lo, m_hi) * P
            S2 = t - self.s2 - N * self.s1
            if lo <= S2 <= hi and S2 + N * self.s1 >= HALF + P:
                self._emit("neg", S1, S2)
                assert 1 <= self.s1 <= 3 and self.s2 == v
                return
        raise AssertionError("no neg chunk from (%d, %d)" % (self.s1, self.s2))

    def low(self, how="low"):
        assert self.s1 <= 11, "a low chunk needs s1 <= 11"
        rng, x, base = self.rng, self.s2, N * self.s1
        S1 = rng.randrange(3, 12) if how == "low+" else (rng.randrange(0, 3) if self.s1 <= 8 else 0)
        if how == "low+" and x < 0 and s2_range(N, S1)[1] < -x - base:
            S1 = 11  # (11 units reach 61072: over any |x| - base)
        lo, hi = s2_range(N, S1)
        hi = min(hi, P - 1 - base)
        if how == "low-" and x < 0:
            hi = min(hi, -x - 1 - base)
        if how == "low+" and x < 0:
            lo = max(lo, -x - base)
        if lo > hi:  # (no room on that side: any low chunk)
            lo, hi = s2_range(N, S1)[0], min(s2_range(N, S1)[1], P - 1 - base)
        self._emit("low", S1, rng.randint(lo, hi))

    def mid(self, against=False):
        rng, x = self.rng, self.s2
        for _ in range(1000):
            d = rng.randrange(-3, 4)
            if against and x < 0:
                d = -rng.randrange(1, min(4, -x + 1))      # C = t - x >= 2^31 > t
            if against and x > 0:
                d = rng.randrange(0, min(3, x))            # C = t - x < 2^31 <= t
            S2 = HALF + d - x - N * self.s1
            S1 = 2 * S2 // N + rng.randrange(-40000, 40001)
            if 0 <= S1 <= 255 * N and s2_range(N, S1)[0] <= S2 <= s2_range(N, S1)[1]:
                self._emit("mid", S1, S2)
                return
        raise AssertionError("no mid chunk from (%d, %d)" % (self.s1, self.s2))

    def emit(self, kind, pool_sums=None):
        if kind == "neg":
            self.neg()
        elif kind.startswith("low"):
            self.low(kind)
        elif kind.startswith("mid"):
            self.mid(kind.endswith("!"))
        else:
            self.free(pool_sums)


BURSTS = (("neg", "low-", "low", "mid!"), ("mid", "mid!"), ("neg", "low+", "mid"), ("mid!",), ("neg", "low", "low-", "low+"),
          ("neg",), ("mid!", "mid!", "mid!"))


def random_sequence(rnd, n_chunks, r, dense):
    """(the sums of n_chunks chunks, chunk 0 of r bytes, and the buffer's length): random chunks with bursts of planned
    kinds, `dense` of 1 of the draws a burst"""
    pl = Planner(rnd.randrange(1 << 30))
    if n_chunks == 1 and r == 0:
        return [], 0  # (no bytes: no chunks)
    pl.free(n=r)
    while len(pl.sums) < n_chunks:
        if rnd.random() < dense:
            for kind in rnd.choice(BURSTS):
                pl.emit(kind)
        else:
            pl.free()
    return pl.sums[:n_chunks], r + N * (n_chunks - 1)


# the stated pattern: a low that opens a run of ambiguous chunks behind a hi chunk, lows entered negative that stay and
# that cross, a mid entered from a low, mids entered from whatever a free chunk left, two pairs of adjacent mids.  Seven
# kinds: coprime to the chunks of a run (per = 1, 3, 5 below), so every kind comes to open runs.
PERIOD = ("neg", "low-", "low", "mid!", "free", "mid!", "mid")


def pool_sums(pool):
    """(S1, S2) of every 5552-byte chunk of a uint8 array whose length is a multiple of 5552"""
    a = pool.reshape(-1, N)
    w = np.arange(N, 0, -1, dtype=np.int64)
    S1, S2 = np.empty(len(a), np.int64), np.empty(len(a), np.int64)
    for i in range(0, len(a), 256):
        blk = a[i:i + 256].astype(np.int64)
        S1[i:i + 256] = blk.sum(axis=1)
        S2[i:i + 256] = blk @ w
    return S1, S2


class Plan:
    """K chunks on the chunk grid: a random pool with PERIOD spliced in, `gap` pool chunks between two periods
    (gap 0: every chunk but the period's "free" is planned).  data: the K * 5552 bytes; sums: of the K + 1 chunks of the
    reference's grid over data (chunk 0 is empty); kinds: what each was planned as."""

    def __init__(self, name, K, gap, seed):
        self.name, self.K = name, K
        rng = np.random.default_rng(seed)
        self.data = rng.integers(0, 256, K * N, dtype=np.uint8)
        S1, S2 = pool_sums(self.data)
        pl = Planner(seed)
        pl.free((0, 0), n=0)  # chunk 0 of a length that is a multiple of 5552: empty (C = 0: a low chunk)
        cycle = PERIOD + ("free",) * gap
        for k in range(K):
            kind = cycle[k % len(cycle)]
            if kind == "low" and (k // len(cycle)) % 3 == 0:
                kind = "low+"
            pl.emit(kind, (int(S1[k]), int(S2[k])))
            if pl.kinds[-1] != "free":
                self.data[k * N:(k + 1) * N] = chunk_with_sums(N, *pl.sums[-1])
        self.sums, self.kinds = pl.sums, pl.kinds
        self.length = K * N


def grid_sums(data):
    """[(S1, S2)] of the reference's chunks of a uint8 array: its first len % 5552 bytes, then 5552 each"""
    data = np.asarray(data, dtype=np.uint8)
    if len(data) == 0:
        return []
    r = len(data) % N
    S1, S2 = pool_sums(data[r:])
    return [chunk_sums(data[:r])] + list(zip(S1.tolist(), S2.tolist()))


# the plans of the GPU tests: (name, chunks, pool chunks between two periods).  n_runs and per as api.hip takes them for
# K + 1 chunks: 601 -> 1024, 1; 3001 -> 1024, 3; 9001 -> 2048, 5; 17001 -> 4096, 5 (16-byte loads in the scan)
PLANS = (("p600", 600, 0), ("p3000", 3000, 0), ("p9000", 9000, 22), ("p17000", 17000, 22))
_plans = {}


def plan(name):
    if name not in _plans:
        for seed, (nm, K, gap) in enumerate(PLANS):
            if nm == name:
                _plans[name] = Plan(nm, K, gap, 1000 + seed)
    return _plans[name]


# what every plan a test uses must hold, counted by walk()
PLAN_MINIMA = dict(low_neg_stay=100, mid_against=100, pairs=20, open_run=20)

# ---- the named lengths -----------------------------------------------------------------------------------------------
# zeros: s1 stays 1 and every chunk has C = 5552 (chunk 0: 0 or its length): all ambiguous.  n_chunks = len // 5552 + 1.
ZERO_LENGTHS = tuple(N * k + d for k in (4095, 4096, 1024) for d in (-1, 0, 1))
# RFC mode: n_chunks 1023, 1024, 1025 (adler_rfc_finish_kernel's chunks per thread 1 -> 2)
RFC_LENGTHS = (N * 1022 + 7, N * 1023, N * 1024 + 5551)
# CRC-32 finish: 32 KiB segments; S segments and d bytes more or less
CRC_SEG = 32768
CRC_SEAMS = (16, 17, 256, 257, 2048, 2049, 4096, 4097)
CRC_DELTAS = (-32767, -1, 0, 1)
FUSED_SIDE_BYTES = 64 << 20  # the fused call finishes the CRC on a second queue from here on


def crc_shape(length):
    """(nseg, threads, rows, padp) of crc32_finish_kernel for a buffer, restated: one partial and up to 16 by one
    thread (rows 0), else 256 threads up to 4096 segments and 1024 beyond"""
    nseg = -(-length // CRC_SEG)
    nt = 1024 if max(nseg, 1) > 4096 else 256
    if nseg <= 16:
        return nseg, nt, 0, 0
    rows = -(-nseg // nt)
    return nseg, nt, rows, rows * nt - nseg


# ---- crafted sum sequences: the lines of adler_chain.h one by one ------------------------------------------------------

class Craft:
    """chunk sums chosen by where t = x + C is to land (sums only: they need not be those of bytes, but C < 2^32)"""

    def __init__(self):
        self.s1, self.s2, self.sums = 1, 0, [(0, 0)]  # chunk 0 of a multiple of 5552 bytes: empty

    def to(self, t, S1=0):
        S2 = t - self.s2 - N * self.s1
        assert 0 <= S2 and N * self.s1 + S2 < 1 << 32, (t, S2)
        self.sums.append((S1, S2))
        self.s1, self.s2 = ref_step(self.s1, self.s2, N, S1, S2)
        return self

    def leave(self, v):
        """a hi chunk (not ambiguous) that leaves s2 = v <= 0"""
        assert -P < v <= 0
        self.to((1 << 32) + v - 6 * P)
        assert self.s2 == v
        return self

    def case(self, **kw):
        return dict(sums=self.sums, length=N * (len(self.sums) - 1), **kw)


FF = (255 * N, 255 * N * (N + 1) // 2)


def mutation_cases():
    """name -> dict(sums, length, and the model's n_runs / replay_max): each sits on one line of adler_chain.h"""
    c = {}
    # C = 65519 entered with s2 = -65520: the one low chunk at the bound whose sum stays negative; it is the last chunk
    c["low_bound_stays_negative_last"] = Craft().leave(-65520).to(-1).case()
    # C = 2^31 - 65521 + 1 entered with s2 = 65520: x + C = 2^31, the first C at which x can lift a low chunk over
    c["mid_lower_bound"] = Craft().to(65520).to(HALF).to(10 ** 9).case()
    # C = 2^31 + 65521 - 1 entered with s2 = -65520: x + C = 2^31 - 1, the last C at which x can pull a hi chunk under
    c["mid_upper_bound"] = Craft().leave(-65520).to(HALF - 1).to(10 ** 9).case()
    # hi chunks that are not ambiguous: 2^32 mod 65521 = 225 in every step
    c["ff_chunks"] = dict(sums=[(0, 0)] + [FF] * 3, length=3 * N)
    # s2 = 0 left by a hi chunk (the reference holds 0, not -65521), then C = 2^31 + 5
    c["zero_behind_hi_then_mid"] = Craft().leave(0).to(HALF + 5).to(10 ** 9).case()
    # two adjacent ambiguous chunks: x pulls the first under 2^31 against its C, the second needs the exact positive s2
    a = Craft().leave(-65520).to(HALF + 100 - 65520)
    assert a.s2 > 0
    c["adjacent_exact"] = a.to(HALF).to(10 ** 9).case()
    # a chunk per run: a mid chunk that opens its run behind a hi chunk, itself below 2^31
    c["opens_run_behind_hi"] = Craft().leave(-100).to(HALF - 110).to(10 ** 9).case(n_runs=8)
    # a correction of +225 from one replayed chunk, a plain chunk, then a mid chunk that 225 less would pull under
    d = Craft().leave(-65520).to(HALF + 100 - 65520).to(10 ** 9 + 300)
    assert d.s2 >= 300
    c["delta_carried"] = d.to(HALF + 10).to(10 ** 9).case()
    # as many ambiguous chunks as the replay holds: zeros (9 chunks, every one low), REPLAY_MAX 9
    c["replay_at_its_limit"] = dict(sums=[(0, 0)] * 9, length=8 * N, replay_max=9)
    # 10 chunks in 4 runs: 3 a run
    c["ten_chunks_four_runs"] = dict(sums=[(16 * 255, 255 * 16 * 17 // 2)] + [FF] * 9, length=9 * N + 16, n_runs=4)
    return c
