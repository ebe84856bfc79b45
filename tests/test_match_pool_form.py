"""zipc_amd/csrc/match_pool.h -- the rules by which a wave of lz_match_runs_pool (deflate_lane.h) hands the positions of its
chunk to the run slots that finish, and by which it runs its loop in the steady form (no `alive`, no `maxlen`, no park, no
exit test) or in the general one -- compiled with g++ (tests/match_pool_sim) and run: the predicate enumerated against the
line of arithmetic below, and whole tiles walked through a serial model of the pool, 16 waves of 64 lanes and 2 run slots
served in a seeded random order, a position's iterations those of deflate_lane.h's own step over sim_chain_serial's links:
  * every position of a tile is handed out exactly once, whatever the order, through the steady loop, its exit and the
    general loop behind it;
  * a wave is steady only while every one of its runs holds a real position whose maxlen is 258;
  * the steady form is taken where it may be (an always-false predicate would pass the two above).
A few one-line mutants of the header show that the model sees each rule.  No GPU; the kernel's records:
tests/test_gpu_match_steady.py."""
import ctypes as C
import os

import numpy as np
import pytest

import host_sim
import match_cases as mc
import match_steady_cases as sc
import mutation

HERE = os.path.dirname(os.path.abspath(__file__))
SIM = os.path.join(HERE, "match_pool_sim", "sim_match_pool.cpp")
STEPS = os.path.join(HERE, "match_pool_sim", "sim_match_steps.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "zipc_amd", "csrc")
HEADER = os.path.join(CSRC, "match_pool.h")
FLAGS = ["-Wall", "-Wno-unknown-pragmas"]
SEEDS = (1, 2)
# (name, the header's line, the mutant's, the checks of _judge that must fail -- any of them)
MUTANTS = [
    ("steady_bound_strict", "cend <= len - ((uint32_t)MAX_MATCH_LEN - 1u);", "cend < len - ((uint32_t)MAX_MATCH_LEN - 1u);", {"predicate"}),
    ("steady_bound_a_byte_late", "cend <= len - ((uint32_t)MAX_MATCH_LEN - 1u);", "cend <= len - ((uint32_t)MAX_MATCH_LEN - 2u);", {"predicate", "invariant"}),
    ("old_chunk_short_by_one", "if (!fresh) return taken <= cend - next;", "if (!fresh) return taken <= cend - next + 1u;", {"once", "range"}),
    ("fresh_chunk_need_not_be_whole", "return ce - c == POOL_CHUNK && match_chunk_steady(ce, len);", "return match_chunk_steady(ce, len);",
     {"once", "range", "invariant"}),
    ("fresh_chunks_lim", "h.lim = ce; }", "h.lim = cend; }", {"once"}),
    ("within_next_short_by_one", "return MatchHandout{next + rank, cend, next + taken, cend};",
     "return MatchHandout{next + rank, cend, next + taken - 1u, cend};", {"once"}),
]


def _bind(path):
    L = C.CDLL(path)
    L.sim_match_chunk_steady.restype = C.c_int
    L.sim_match_chunk_steady.argtypes = [C.c_uint32, C.c_uint32]
    L.sim_pool_chunk.restype = C.c_uint32
    L.sim_match_handout.restype = None
    L.sim_match_handout.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p]
    L.sim_match_pool_tile.restype = C.c_int
    L.sim_match_pool_tile.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("match_pool_sim")


@pytest.fixture(scope="module")
def sim(build_dir):
    return _bind(mutation.gxx(build_dir / "libmatch_pool_sim.so", [SIM], extra=FLAGS))


@pytest.fixture(scope="module")
def walks(build_dir):
    """[(length, {level: steps per position})] of every stream of the cases: the iterations the shared step takes"""
    L = C.CDLL(mutation.gxx(build_dir / "libmatch_steps_sim.so", [STEPS], extra=FLAGS))
    L.sim_match_steps.restype = C.c_uint32
    L.sim_match_steps.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    H = host_sim.lib()
    out = []
    for s in sc.streams():
        n = len(s)
        buf = np.zeros(n + host_sim.MATCH_SLACK, np.uint8)
        buf[:n] = np.frombuffer(s.data, np.uint8)
        links = np.zeros(n + 8, np.uint16)
        H.sim_chain_serial(buf.ctypes.data_as(C.c_char_p), n, links.ctypes.data)
        per = {}
        for level in (1, 2):
            K, Kq, _ = host_sim.MATCH_LEVELS[level]
            steps = np.zeros(n, np.uint32)
            assert L.sim_match_steps(buf.ctypes.data, n, links.ctypes.data, K, Kq, steps.ctypes.data) == 0, (s.name, level)
            assert (steps[:n - 3] >= 1).all() and int(steps[:n - 3].max()) <= max(K, 1)
            per[level] = steps
        out.append((s.name, n, per))
    return out


def _tile(L, n, t0, t1, steps, seed):
    handed, stats = np.zeros(n + 1, np.uint32), np.zeros(6, np.uint64)
    hung = L.sim_match_pool_tile(n, t0, t1, steps.ctypes.data, seed, handed.ctypes.data, stats.ctypes.data)
    return hung, handed, [int(x) for x in stats]


def _predicate_failures(L):
    """the predicate against cend - 1 + 258 <= len, around every chunk edge of the cases and near 4 GiB"""
    bad = []
    lens = sorted(set(sc.lengths()) | {0, 1, 256, 257, 258, 513, 0xFFFF0000, 0xFFFF0000 - 1})
    for n in lens:
        ends = {c for lo, hi in sc.steady_chunks(n)[-2:] for c in (hi,)} if n <= 65536 else set()
        ends |= {e for e in (0, 1, 256, n - 259, n - 258, n - 257, n - 256, n - 255, n - 3, n, 0xFFFFFF00, 0xFFFFFFFF) if 0 <= e <= 0xFFFFFFFF}
        for cend in ends:
            if bool(L.sim_match_chunk_steady(cend, n)) != (cend - 1 + sc.MAXLEN <= n):
                bad.append((cend, n))
    return bad


def _judge(L, walks, levels=(1, 2), seeds=SEEDS):
    """-> the names of the checks that fail with this build of the rules"""
    failed = set()
    if _predicate_failures(L):
        failed.add("predicate")
    for name, n, per in walks:
        for level in levels:
            for t0, t1 in sc.tiles(n) + _odd_tiles(n):
                for seed in seeds:
                    hung, handed, st = _tile(L, n, t0, t1, per[level], seed)
                    if hung:
                        failed.add("hang")
                    if not ((handed[t0:t1] == 1).all() and int(handed.sum()) == t1 - t0):
                        failed.add("once")
                    if st[3]:
                        failed.add("invariant")
                    if st[4]:
                        failed.add("range")
    return failed


def _odd_tiles(n):
    """tiles no kernel cuts: they end in a short chunk far from the stream's end, whose positions are steady ones -- what
    keeps a wave from staying steady over such a chunk is that it is not a whole one, and nothing else"""
    return [(0, sc.CHUNK * 20 + e) for e in (1, 5, 255)] if n == 65536 else []


def test_the_predicate_is_the_bound_and_cannot_wrap(sim):
    assert sim.sim_pool_chunk() == sc.CHUNK
    assert _predicate_failures(sim) == []
    # a stream at the longest length the kernels take: its last whole chunk but one is steady, a chunk end past 2^32 - 258 is not
    top = 0xFFFF0000
    assert sim.sim_match_chunk_steady(top - 512, top) == 1 and sim.sim_match_chunk_steady(top - 256, top) == 0
    assert sim.sim_match_chunk_steady(0xFFFFFFFF, top) == 0 and sim.sim_match_chunk_steady(0, 0) == 0 and sim.sim_match_chunk_steady(0, 256) == 0


def test_a_handout_is_the_old_chunk_then_the_fresh_one(sim):
    """match_handout by hand: 5 slots finish, 3 positions are left in [100, 103), the fresh chunk is [512, 768) -- or a short
    one of a single position, or none"""
    out = np.zeros(4 * 5, np.uint32)
    sim.sim_match_handout(5, 100, 103, 1, 512, 768, out.ctypes.data)
    assert out.reshape(5, 4).tolist() == [[100, 103, 514, 768], [101, 103, 514, 768], [102, 103, 514, 768], [512, 768, 514, 768], [513, 768, 514, 768]]
    sim.sim_match_handout(5, 100, 103, 1, 512, 513, out.ctypes.data)  # the last slot gets nothing: np == lim
    assert out.reshape(5, 4).tolist()[3:] == [[512, 513, 513, 513], [513, 513, 513, 513]]
    sim.sim_match_handout(5, 100, 103, 0, 0, 0, out.ctypes.data)  # the pool is empty: two slots get nothing
    assert out.reshape(5, 4).tolist() == [[100, 103, 103, 103], [101, 103, 103, 103], [102, 103, 103, 103], [103, 103, 103, 103], [103, 103, 103, 103]]
    sim.sim_match_handout(2, 100, 103, 0, 0, 0, out.ctypes.data)
    assert out.reshape(5, 4).tolist()[:2] == [[100, 103, 102, 103], [101, 103, 102, 103]]


def test_every_position_once_and_steady_only_on_steady_positions(sim, walks):
    assert _judge(sim, walks) == set()


def test_the_steady_form_is_taken_where_it_may_be(sim, walks):
    """by the waves' first chunks: chunk k of a tile goes to the k-th wave that starts, and that wave enters the steady form
    iff the chunk is a whole, steady one; on the benchmark's length most iterations of either tile are steady ones"""
    for name, n, per in walks:
        steady = set(sc.steady_chunks(n))
        for t0, t1 in sc.tiles(n):
            first = [(lo, lo + sc.CHUNK) for lo in range(t0, t1, sc.CHUNK)][:16]
            _, _, st = _tile(sim, n, t0, t1, per[2], 3)
            assert st[2] == sum(c in steady for c in first), (name, t0)
            assert st[5] == st[2]  # every wave that entered left through a handout: its last chunk is never a steady one
            assert (st[0] > 0) == (st[2] > 0)
        if n == 65536:
            share = []
            for t0, t1 in sc.tiles(n):
                _, _, st = _tile(sim, n, t0, t1, per[2], 3)
                share.append(st[0] / st[1])
            # (a wave of tile 0 walks a dozen chunks, of tile 1 four, and leaves with its last 128 positions or fewer in hand:
            # what it does in the general form is the end of one chunk and the tail of its longest walks)
            assert share[0] > 0.5 and share[1] > 0.5, share
        if n == 300:
            assert sc.steady_chunks(n) == []


def test_mutants_of_the_rules_are_seen(build_dir, walks):
    """each one-line change of match_pool.h fails the check named for it (over the cases' shortest and longest streams: the
    whole list takes no other path)"""
    some = [w for w in walks if w[1] in (513, 4609, 8705, sc.T0 + 256 + 257, 65536)]
    assert len(some) == 5

    def build(m):
        name, line, mutated, _ = m
        return mutation.header_model(SIM, "MATCH_POOL_H", HEADER, line, mutated, str(build_dir / name / "libmatch_pool_sim.so"),
                                     rewrite_includes=("zd_common.h",), extra=FLAGS)
    libs = mutation.build_all(build, MUTANTS)
    for (name, _, _, killers), so in zip(MUTANTS, libs):
        failed = _judge(_bind(so), some, levels=(2,))
        assert failed & killers, (name, failed)


def test_the_cases_reach_what_they_are_for():
    """the two planted streams of tests/match_steady_cases.py: their walks lie in steady chunks, and the reference's walks
    there end by l == 258 and, at `Fast and `Default, by K and K / 4 candidates"""
    L = host_sim.lib()
    by_name = {s.name: s for s in sc.streams()}
    run = by_name["run_of_one_byte"]
    steady = sc.steady_chunks(len(run))
    best, first = host_sim.match_reference(L, run.data, 2)
    for p in (2001, 3000, 4000 - mc.MAXLEN):
        assert any(lo <= p < hi for lo, hi in steady)
        assert int(best[p]) == mc.rec(1, mc.MAXLEN) and int(first[p]) == int(best[p])
    kg = by_name["k_groups"]
    steady = sc.steady_chunks(len(kg))
    seen = {1: 0, 2: 0}
    for level in (1, 2):
        K, Kq, _ = host_sim.MATCH_LEVELS[level]
        best, first = host_sim.match_reference(L, kg.data, level)
        for pr in kg.props:
            if pr[0] != "rec":
                continue
            p, want = pr[1], pr[2](K, Kq)
            assert any(lo <= p < hi for lo, hi in steady)
            assert (int(best[p]), int(first[p])) == want, (level, p)
            seen[level] += want[0] != want[1]  # K / 4 candidates gave another answer than K
    assert seen[1] and seen[2]
