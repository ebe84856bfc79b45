"""zipc_amd/csrc/host_pipeline.h plan_many -- where the streams of a many-stream call lie in the staging arenas, how many
sub-batches the call is cut into and where, what the largest of them needs -- compiled with g++ (tests/host_sim/sim_many.cpp)
and held against rows written out by hand from the rule's words.  A wrong cut still gives right bytes, so no parity test
sees any of this; tests/test_gpu_many_plan.py ties the library's calls to the same function.  No GPU."""
import ctypes as C
import os
import random

import pytest

import util  # noqa: F401  (sets sys.path through conftest)
import host_sim
import mutation
from host_sim import MANY_DEFLATE, MANY_INFLATE, MANY_RECODE

MIN_DST = 256 << 10  # forms.h BLOCKS_BATCH_MIN_DST
HAS_LIMIT, EXPECT_CRC32 = 1, 2


@pytest.fixture(scope="module")
def sim():
    return host_sim.lib()


def plan(L, op, src_len, dst_cap=None, **kw):
    return host_sim.many_plan(L, op, src_len, [0] * len(src_len) if dst_cap is None else dst_cap, **kw)


# ---- the rows: each a function of the library, so that the mutants below can be held to the same ones --------------------

def row_slots(L):
    """a slot is the length rounded up to 256 and 256 more; offsets are running sums, the arena's end their total"""
    assert [L.sim_many_slot(v) for v in (0, 1, 255, 256, 257)] == [256, 512, 512, 512, 768]
    assert L.sim_many_slot(65536) == 65792 and L.sim_many_slot((1 << 32) + 1) == (1 << 32) + 512
    p = plan(L, MANY_DEFLATE, [0, 1, 255, 256, 257], [257, 256, 255, 1, 0], chunks=1)
    assert p["src_off"] == [0, 256, 768, 1280, 1792] and p["src_arena_end"] == 2560
    assert p["dst_off"] == [0, 768, 1280, 1792, 2304] and p["dst_arena_end"] == 2560
    assert (p["max_src"], p["max_cap"], p["max_mid"]) == (257, 257, 0)
    assert p["cut"] == [0, 5] and p["n_max"] == 5 and p["total_max"] == 769


def row_count_settings(L):
    """ZIPC_HIP_HOST_CHUNKS as given, at most 64; below 1: by what is staged"""
    assert [L.sim_many_chunks(s, 0) for s in (-5, 0, 1, 2, 7, 64, 65, 1000)] == [4, 4, 1, 2, 7, 64, 64, 64]
    small = [1] * 64  # (64 streams, chunk_min 1: no count is shrunk)
    assert plan(L, MANY_DEFLATE, small, chunks=7, chunk_min=1)["K"] == 7
    assert plan(L, MANY_DEFLATE, small, chunks=1000, chunk_min=1)["K"] == 64
    assert plan(L, MANY_DEFLATE, small, chunks=0, chunk_min=1)["K"] == 4


def row_count_at_a_gib(L):
    """a setting of 0: 4 sub-batches, 6 from 2^30 staged bytes (sources' and destinations' arenas together) on"""
    assert [L.sim_many_chunks(0, v) for v in ((1 << 30) - 1, 1 << 30, (1 << 30) + 1, 1 << 31, 1 << 40)] == [4, 6, 6, 6, 6]
    # one stream whose slots are 2^29 and 2^29 - 256 bytes, then 2^29 and 2^29 (the byte clause keeps the count: 2^29 / 6 > 2^26)
    p = plan(L, MANY_DEFLATE, [(1 << 29) - 256], [(1 << 29) - 512])
    assert p["src_arena_end"] + p["dst_arena_end"] == (1 << 30) - 256 and p["K"] == 4 and p["cut"] == [0, 1, 1, 1, 1]
    p = plan(L, MANY_DEFLATE, [(1 << 29) - 256], [(1 << 29) - 256])
    assert p["src_arena_end"] + p["dst_arena_end"] == 1 << 30 and p["K"] == 6 and p["cut"] == [0, 1, 1, 1, 1, 1, 1]
    # ... and it is the sum that counts, not the sources alone
    assert plan(L, MANY_DEFLATE, [(1 << 29) - 256], [0])["K"] == 4


def row_shrink_by_streams(L):
    """the default chunk_min of 1024 with small streams (the byte clause holds for every K): K goes down while n / K < 1024"""
    for n, K in ((4096, 4), (4095, 3), (3072, 3), (3071, 2), (2048, 2), (2047, 1), (1, 1)):
        assert plan(L, MANY_DEFLATE, [100] * n)["K"] == K, n
    for n, K in ((47, 5), (48, 6), (40, 5), (39, 4), (8, 1), (16, 2)):
        assert plan(L, MANY_DEFLATE, [100] * n, chunks=6, chunk_min=8)["K"] == K, n


def row_shrink_bytes_at_the_limit(L):
    """a few long streams keep K through the byte clause: so / K >= chunk_min * 65536 = 2^26 at the default"""
    long_ = (1 << 26) - 256  # a slot of 2^26
    p = plan(L, MANY_DEFLATE, [long_] * 4)  # so = 2^28: so / 4 = 2^26, not below
    # (six shares of 2^28 / 6 = 44 739 242: boundaries 1, 3 and 5 shares are first reached by streams 1 and 2 and by none: the
    # stream at 3 * 2^26 lies below 223 696 210)
    assert p["src_arena_end"] == 1 << 28 and p["K"] == 4 and p["cut"] == [0, 1, 2, 4, 4]
    p = plan(L, MANY_DEFLATE, [long_] * 3 + [long_ - 256])  # so = 2^28 - 256: so / 4 < 2^26, so / 3 is not
    assert p["src_arena_end"] == (1 << 28) - 256 and p["K"] == 3
    # (four shares of (2^28 - 256) / 4 = 2^26 - 64: boundaries at 2^26 - 64 and 3 * 2^26 - 192)
    assert p["cut"] == [0, 1, 3, 4]
    # both clauses must hold for K to go down: many streams keep K however few their bytes
    assert plan(L, MANY_DEFLATE, [0] * 4096)["K"] == 4
    # chunk_min 8: 2^19 bytes a sub-batch.  Two streams of slots 2^20: so / 4 = 2^19 stays; 256 bytes less and it is 3
    assert plan(L, MANY_DEFLATE, [(1 << 20) - 256] * 2, chunks=4, chunk_min=8)["K"] == 4
    assert plan(L, MANY_DEFLATE, [(1 << 20) - 256, (1 << 20) - 512], chunks=4, chunk_min=8)["K"] == 3


TWELVE = [256] * 12  # slots of 512: so = 6144


def row_taper_K4(L):
    """K = 4: six shares of 1024; the boundaries at 1, 3 and 5 shares: the first and last sub-batch are half as large"""
    p = plan(L, MANY_DEFLATE, TWELVE, chunks=4, chunk_min=1)
    assert p["src_arena_end"] == 6144 and p["K"] == 4
    assert p["cut"] == [0, 2, 6, 10, 12] and p["n_max"] == 4 and p["total_max"] == 1024


def row_taper_K2_plain(L):
    """below K = 3 the shares are plain"""
    p = plan(L, MANY_DEFLATE, TWELVE, chunks=2, chunk_min=1)
    assert p["cut"] == [0, 6, 12] and p["n_max"] == 6 and p["total_max"] == 1536
    p = plan(L, MANY_DEFLATE, TWELVE, chunks=1, chunk_min=1)
    assert p["cut"] == [0, 12] and p["n_max"] == 12 and p["total_max"] == 3072


def row_taper_K3(L):
    """K = 3: four shares of 1536; boundaries at 1536 (stream 3) and 4608 (stream 9)"""
    p = plan(L, MANY_DEFLATE, TWELVE, chunks=3, chunk_min=1)
    assert p["cut"] == [0, 3, 9, 12] and p["n_max"] == 6 and p["total_max"] == 1536


def row_taper_ragged(L):
    """one stream larger than a whole share: slots 512, 512, 5376, 512, 512 at 0, 512, 1024, 6400, 6912; so = 7424, six
    shares of 1237.  Boundaries 1237, 3711, 6185: each is first reached by stream 3 (at 6400): two sub-batches are empty"""
    p = plan(L, MANY_DEFLATE, [256, 256, 5000, 256, 256], [10, 300, 0, 7000, 1], chunks=4, chunk_min=1)
    assert p["src_off"] == [0, 512, 1024, 6400, 6912] and p["src_arena_end"] == 7424
    assert p["dst_off"] == [0, 512, 1280, 1536, 8960] and p["dst_arena_end"] == 9472
    assert p["cut"] == [0, 3, 3, 3, 5] and p["n_max"] == 3 and p["total_max"] == 5512
    assert (p["max_src"], p["max_cap"]) == (5000, 7000)
    # the long one first: it is sub-batch 0 alone (boundary 1237 is first reached by stream 1 at 5376), then 3711 and 6185
    p = plan(L, MANY_DEFLATE, [5000, 256, 256, 256, 256], chunks=4, chunk_min=1)
    assert p["src_off"] == [0, 5376, 5888, 6400, 6912] and p["cut"] == [0, 1, 1, 3, 5] and p["n_max"] == 2 and p["total_max"] == 5000


MID_CAPS = [100, 0, 256, 257, 1, 1, 1, 1, 1000, 5, 5, 5]


def row_recode_mid_arena(L):
    """TWELVE at K = 3 (cut 0, 3, 9, 12): mid_off restarts at 0 in every sub-batch; the arena is the largest sub-batch's
    extent (4096 of the second), not the sum (6912); mid_total_max the most room a sub-batch declares (257 + 4 + 1000)"""
    p = plan(L, MANY_RECODE, TWELVE, [300] * 12, mid_cap=MID_CAPS, chunks=3, chunk_min=1)
    assert p["cut"] == [0, 3, 9, 12]
    assert [r["mid_off"] for r in p["rdescs"]] == [0, 512, 768, 0, 768, 1280, 1792, 2304, 2816, 0, 512, 1024]
    assert p["mid_arena"] == 4096 and p["mid_total_max"] == 1261 and p["max_mid"] == 1000
    assert p["n_max"] == 6 and p["total_max"] == 1536
    # one sub-batch: one run of offsets, the arena is all of it
    p = plan(L, MANY_RECODE, TWELVE, [300] * 12, mid_cap=MID_CAPS, chunks=1, chunk_min=1)
    assert [r["mid_off"] for r in p["rdescs"]][:5] == [0, 512, 768, 1280, 2048] and p["mid_arena"] == 6912 and p["mid_total_max"] == 1632
    # deflate and inflate have no middle arena
    p = plan(L, MANY_INFLATE, TWELVE, [300] * 12, chunks=3, chunk_min=1)
    assert (p["mid_arena"], p["mid_total_max"], p["max_mid"]) == (0, 0, 0)


def row_recode_descriptors(L):
    """a stream's recode descriptor: its slots, its room, the caller's limit and CRC-32 with their flags -- the CRC-32's only when given"""
    limits, crcs = list(range(1000, 1012)), [0xC0FFEE00 + i for i in range(12)]
    for limit, crc, flags in ((None, None, 0), (limits, None, HAS_LIMIT), (None, crcs, EXPECT_CRC32), (limits, crcs, HAS_LIMIT | EXPECT_CRC32)):
        p = plan(L, MANY_RECODE, TWELVE, [300 + i for i in range(12)], limit=limit, mid_cap=MID_CAPS, expect_crc32=crc, chunks=3, chunk_min=1)
        for i, r in enumerate(p["rdescs"]):
            want = dict(src_off=512 * i, src_len=256, mid_cap=MID_CAPS[i], dst_off=768 * i, dst_cap=300 + i, limit=limit[i] if limit else 0,
                        flags=flags, expect_crc32=crc[i] if crc else 0)
            assert {k: r[k] for k in want} == want, (i, r)
            # what inflate is handed: the stream into its room in the middle arena, the limit and its flag alone
            assert p["inflate_descs"][i] == (512 * i, 256, r["mid_off"], MID_CAPS[i], want["limit"], flags & HAS_LIMIT, 0)


def row_ahead(L):
    """the next sub-batch is sent ahead where a stream may inflate by blocks: inflate by max_cap, recode by max_mid, deflate never"""
    for cap, ahead in ((MIN_DST - 1, 0), (MIN_DST, 1), (MIN_DST + 1, 1)):
        assert plan(L, MANY_INFLATE, [10, 10], [5, cap])["ahead"] == ahead
        assert plan(L, MANY_RECODE, [10, 10], [5 << 20, 5 << 20], mid_cap=[cap, 5])["ahead"] == ahead
        assert plan(L, MANY_DEFLATE, [cap, 10], [cap, 5])["ahead"] == 0
    assert plan(L, MANY_RECODE, [MIN_DST, MIN_DST], [MIN_DST, MIN_DST], mid_cap=[MIN_DST - 1, 5])["ahead"] == 0
    assert plan(L, MANY_DEFLATE, [8 << 20], [8 << 20])["ahead"] == 0


ROWS = {f.__name__[4:]: f for f in (row_slots, row_count_settings, row_count_at_a_gib, row_shrink_by_streams, row_shrink_bytes_at_the_limit,
                                    row_taper_K4, row_taper_K2_plain, row_taper_K3, row_taper_ragged, row_recode_mid_arena,
                                    row_recode_descriptors, row_ahead)}


@pytest.mark.parametrize("name", sorted(ROWS))
def test_plan_rows(sim, name):
    ROWS[name](sim)


def test_inflate_descriptors_are_recode_open_of_the_streams(sim, tmp_path):
    """what plan_many hands inflate equals recode_rules.h recode_open of the stream's descriptor, as tests/recode_sim's
    program prints it (the table of tests/test_recode_rules.py stands behind that function)"""
    import test_recode_rules as RR

    class Stream:
        def __init__(self, r):
            self.r = r

        def line(self, i):
            r = self.r
            return "%d %d %d %d %d %d %d %d %d 0 0 0 0 0" % tuple(r[k] for k in host_sim.RECODE_DESC_FIELDS)

    assert max(MID_CAPS) == RR.MAX_MID  # (the call's max_mid_cap is what RR.run declares)
    p = plan(sim, MANY_RECODE, TWELVE, [300] * 12, limit=list(range(12)), mid_cap=MID_CAPS, expect_crc32=[7] * 12, chunks=3, chunk_min=1)
    got = RR.run(RR.build(tmp_path), [Stream(r) for r in p["rdescs"]], False)
    assert [g[2] for g in got] == p["inflate_descs"]
    assert all(g[1] == (0, 0, 0, 0) for g in got)  # (and every stream is opened: no room is beyond the largest)


def test_plan_invariants_of_random_shapes(sim):
    rnd = random.Random(20)
    for trial in range(300):
        n = rnd.randrange(1, 401)
        top = rnd.choice((300, 70000, 3 << 20))
        src_len = [rnd.randrange(0, top + 1) for _ in range(n)]
        dst_cap = [rnd.randrange(0, top + 1) for _ in range(n)]
        mid_cap = [rnd.randrange(0, top + 1) for _ in range(n)]
        op = rnd.choice((MANY_DEFLATE, MANY_INFLATE, MANY_RECODE))
        setting, chunk_min = rnd.randrange(0, 9), rnd.choice((1, 2, 8, 1024))
        p = plan(sim, op, src_len, dst_cap, mid_cap=mid_cap if op == MANY_RECODE else None, chunks=setting, chunk_min=chunk_min)
        K, cut = p["K"], p["cut"]
        assert 1 <= K <= (setting or 6) and len(cut) == K + 1 and cut[0] == 0 and cut[K] == n and cut == sorted(cut), (trial, cut)
        assert K == 1 or n // K >= chunk_min or p["src_arena_end"] // K >= chunk_min * 65536
        for off, lens, end in ((p["src_off"], src_len, p["src_arena_end"]), (p["dst_off"], dst_cap, p["dst_arena_end"])):
            assert off[0] == 0 and all(o % 256 == 0 for o in off) and end % 256 == 0
            nxt = off[1:] + [end]
            assert all(off[i] + lens[i] + 256 <= nxt[i] < off[i] + lens[i] + 768 for i in range(n)), trial
        sizes = [cut[g + 1] - cut[g] for g in range(K)]
        assert p["n_max"] == max(sizes) and p["total_max"] == max(sum(src_len[cut[g]:cut[g + 1]]) for g in range(K))
        assert (p["max_src"], p["max_cap"]) == (max(src_len), max(dst_cap))
        if op == MANY_RECODE:
            mid_off = [r["mid_off"] for r in p["rdescs"]]
            ext = []
            for g in range(K):
                lo, hi = cut[g], cut[g + 1]
                assert hi == lo or mid_off[lo] == 0
                assert all(mid_off[i] % 256 == 0 and mid_off[i] + mid_cap[i] + 256 <= mid_off[i + 1] for i in range(lo, hi - 1))
                ext.append(mid_off[hi - 1] + _slot(mid_cap[hi - 1]) if hi > lo else 0)
            assert p["mid_arena"] == max(ext) and p["max_mid"] == max(mid_cap)
            assert p["mid_total_max"] == max(sum(mid_cap[cut[g]:cut[g + 1]]) for g in range(K))


def _slot(v):
    return (v + 255) // 256 * 256 + 256


# ---- the mutants ---------------------------------------------------------------------------------------------------------

# (name, file, text, replacement, killer): one-line mutants of the many-stream forms' plan (host_pipeline.h plan_many), killed on
# the CPU only -- each built into a model of its own (tests/host_sim/sim_many.cpp) by test_plan_mutants_are_killed below.
# killer: the row of ROWS it must fail.  A wrong cut still gives right bytes: no parity test would notice any of these.
MANY_PLAN_MUTANTS = [
    ("taper_shares_not_doubled", "host_pipeline.h", "taper ? 2 * g - 1 : g;", "taper ? g : g;", "taper_K4"),
    ("taper_divides_by_K", "host_pipeline.h", "so / shares * before", "so / K * before", "taper_K4"),
    ("shrink_either_clause", "host_pipeline.h", "n / K < least && so / K < least * 65536", "n / K < least || so / K < least * 65536",
     "shrink_bytes_at_the_limit"),
    ("slot_without_its_gap", "host_pipeline.h", "return (len + 255) / 256 * 256 + 256;", "return (len + 255) / 256 * 256;", "slots"),
    ("mid_off_runs_on", "host_pipeline.h", "uint64_t mo = 0;", "uint64_t mo = p.mid_arena;", "recode_mid_arena"),
    ("six_from_two_gib", "host_pipeline.h", "staged_bytes >= ((uint64_t)1 << 30)", "staged_bytes >= ((uint64_t)1 << 31)", "count_at_a_gib"),
]


def _build_model(csrc_dir, so):
    """sim_many.cpp alone against a copy of zipc_amd/csrc"""
    return host_sim.bind_many(C.CDLL(mutation.single_model(os.path.join(host_sim.HERE, "sim_many.cpp"), "host_pipeline.h", csrc_dir, so)))


def test_plan_mutants_are_killed(tmp_path):
    """MANY_PLAN_MUTANTS: each one-line mutant of host_pipeline.h built into a model of its own; the
    row the table names must fail on it, and every row passes on the unmutated header built the same way."""
    from tools import kernel_mutants as KM

    names = [m[0] for m in MANY_PLAN_MUTANTS]
    assert len(names) == len(set(names)) >= 6 and all(m[4] in ROWS for m in MANY_PLAN_MUTANTS)
    base = _build_model(KM.CSRC, str(tmp_path / "plain.so"))
    for row in ROWS.values():
        row(base)

    def build(m):
        d = str(tmp_path / m[0])
        return _build_model(KM.mutated_tree(m, d), os.path.join(d, "mutant.so"))

    models = mutation.build_all(build, MANY_PLAN_MUTANTS)
    missed = []
    for m, model in zip(MANY_PLAN_MUTANTS, models):
        try:
            ROWS[m[4]](model)
            missed.append(m[0])
        except AssertionError:
            pass
    assert missed == []
