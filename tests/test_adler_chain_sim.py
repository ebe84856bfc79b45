"""zipc_amd/csrc/adler_chain.h -- the arithmetic of the Adler-32 chunk chain (adler_runs_s1 / adler_scan_runs /
adler_runs_a / adler_replay, adler_rfc_finish) and the index grid of crc32_finish_kernel -- compiled with g++ into the
host model tests/host_sim/sim_adler.cpp and held against two references: the serial walk with adler_chunk_step (the
reference's order) and checksum_cases.walk (zd.ml:175-198 restated over chunk sums in Python's integers); both against
the oracle on bytes.  No GPU: the kernels are tests/test_gpu_checksum_chain.py's, on the same inputs."""
import os
import random
import sys
import zlib

import numpy as np
import pytest

import checksum_cases as CC
import host_sim
import mutation
import util

N, P = CC.N, CC.P
SIM_ADLER = os.path.join(host_sim.HERE, "sim_adler.cpp")


@pytest.fixture(scope="module")
def sim():
    return host_sim.lib()


def _cols(sums):
    return [s[0] for s in sums], [s[1] for s in sums]


def _chain(sim, sums, length, **kw):
    return host_sim.adler_chain(sim, *_cols(sums), length, **kw)


def _serial(sim, sums, length):
    return host_sim.adler_serial(sim, *_cols(sums), length)


# ---- the inputs ------------------------------------------------------------------------------------------------------

def test_chunk_with_sums_gives_exactly_those_sums():
    rnd = random.Random(11)
    for n in (1, 3, 15, 16, 255, 5551, N):
        points = []
        for S1 in (0, 1, 254, 255, 256, 255 * n - 1, 255 * n, 255 * (n // 2), 255 * (n // 2) + 7):
            if 0 <= S1 <= 255 * n:
                lo, hi = CC.s2_range(n, S1)
                points += [(S1, lo), (S1, hi), (S1, min(lo + 1, hi)), (S1, max(hi - 1, lo)), (S1, (lo + hi) // 2)]
        for _ in range(60):
            S1 = rnd.randrange(0, 255 * n + 1)
            points.append((S1, rnd.randint(*CC.s2_range(n, S1))))
        for S1, S2 in points:
            b = CC.chunk_with_sums(n, S1, S2)
            assert b.dtype == np.uint8 and len(b) == n and CC.chunk_sums(b) == (S1, S2), (n, S1, S2)
    # the ends of the range are the packs themselves, and nothing lies outside
    assert CC.s2_range(4, 300) == (255 + 45 * 2, 255 * 4 + 45 * 3)
    with pytest.raises(AssertionError):
        CC.chunk_with_sums(4, 300, 255 + 45 * 2 - 1)


def test_the_walk_over_sums_is_the_second_readings_adler_32(oracle):
    """checksum_cases.walk against the byte loop of the second reading (tests/golden/zd_second_reading.py) and the oracle, on
    bytes short enough for Python: the start of the first plan (every planned kind), at every first-chunk length"""
    sys.path.insert(0, util.GOLDEN)
    import zd_second_reading as Z2

    data = CC.plan("p600").data[:N * 15].tobytes()
    for extra in (b"", b"a", b"\xff" * 15, bytes(range(16)), b"\x80" * 5551):
        d = data + extra
        got, _ = CC.walk(CC.grid_sums(np.frombuffer(d, np.uint8)), len(d))
        assert got == Z2.adler_32_string(d) == oracle.adler32(d), len(extra)
    assert CC.walk([], 0)[0] == 1 == oracle.adler32(b"")


def test_every_plan_holds_its_conditions_and_both_references_agree_with_the_oracle(sim, oracle):
    """The plans the GPU tests run, as bytes: the sums recomputed from the bytes are the planned ones, the serial walk counts
    what the issue asks of a plan (never the code under test), and the walk, the serial model and the chain model all give
    the oracle's Adler-32 -- with three bytes appended too (the grid shifted: r = 3)."""
    for name, K, gap in CC.PLANS:
        pl = CC.plan(name)
        assert CC.grid_sums(pl.data) == pl.sums, name
        n_chunks, n_runs, per = host_sim.adler_shape(sim, pl.length)
        assert n_chunks == K + 1
        want, c = CC.walk(pl.sums, pl.length, per)
        print("%-7s chunks %5d  n_runs %4d per %d  %s" % (name, n_chunks, n_runs, per, " ".join("%s %d" % kv for kv in c.items())))
        for key, least in CC.PLAN_MINIMA.items():
            assert c[key] >= least, (name, key, c)
        assert c["low_neg_cross"] >= 20 and c["low"] + c["mid"] <= 4096, (name, c)  # (the replay, not the walk)
        assert want == oracle.adler32(pl.data), name
        assert _serial(sim, pl.sums, pl.length) == want, name
        got, info = _chain(sim, pl.sums, pl.length, seed=1)
        assert (got, info["path"], info["n_amb"]) == (want, host_sim.ADLER_REPLAY, c["low"] + c["mid"]), (name, info)
        more = np.concatenate([pl.data, np.frombuffer(b"xyz", np.uint8)])
        sums3 = CC.grid_sums(more)
        want3 = oracle.adler32(more)
        assert CC.walk(sums3, len(more))[0] == want3 and _chain(sim, sums3, len(more), seed=2)[0] == want3, name
    assert [host_sim.adler_shape(sim, CC.plan(n).length)[1:] for n, _, _ in CC.PLANS] == [(1024, 1), (1024, 3), (2048, 5), (4096, 5)]


# ---- the model against the two references -----------------------------------------------------------------------------

_sequence = CC.random_sequence


def _check(sim, sums, length, seeds=(0,), **kw):
    """the chain model on one sequence == serial model == walk; -> (info, counts)"""
    want, c = CC.walk(sums, length)
    assert _serial(sim, sums, length) == want
    for seed in seeds:
        got, info = _chain(sim, sums, length, seed=seed, **kw)
        n_amb = c["low"] + c["mid"]
        walks = n_amb > (kw.get("replay_max") or 4096) or n_amb > (kw.get("amb_cap") or 8192)
        assert (got, info["n_amb"], info["path"]) == (want, n_amb, host_sim.ADLER_WALK if walks else host_sim.ADLER_REPLAY), (length, kw, info)
    return info, c


def test_chain_model_equals_both_references_at_every_shape(sim):
    rnd = random.Random(2024)
    shapes = set()
    for n_chunks in (1, 2, 1023, 1024, 1025, 8192, 8193, 16385):
        for r in (0, 1, 15, 16, 5551):
            sums, length = _sequence(rnd, n_chunks, r, 0.04)
            info, c = _check(sim, sums, length)
            shapes.add((info["n_runs"], info["per"]))
            if n_chunks >= 1023:
                assert c["low"] and c["mid"] and c["pairs"], (n_chunks, r, c)
    assert shapes == {(1024, 1), (1024, 2), (1024, 8), (2048, 5), (4096, 5)}, shapes


def test_chain_model_with_few_runs_and_a_small_replay(sim):
    """Tens of chunks reach every branch once n_runs and REPLAY_MAX are small: dense sequences, runs of 1 .. all chunks
    (empty runs behind the last chunk when n_runs > n_chunks), the records shuffled three ways, the replay's limit set to
    the count of ambiguous chunks (replay) and to one less (walk), the list's capacity likewise."""
    rnd = random.Random(7)
    paths, seen = set(), dict(low_neg_stay=0, low_neg_cross=0, mid_against=0, pairs=0)
    for i in range(400):
        n_chunks = rnd.randrange(1, 70)
        sums, length = _sequence(rnd, n_chunks, rnd.choice((0, 0, 1, 15, 16, 5551)), rnd.choice((0.1, 0.5, 1.0)))
        n_runs = rnd.choice((1, 2, 3, 4, 7, 16, 64, 128))
        info, c = _check(sim, sums, length, seeds=(1, 2, 3), n_runs=n_runs)
        for k in seen:
            seen[k] += c[k]
        n_amb = info["n_amb"]
        if n_amb >= 2:
            for kw in (dict(replay_max=n_amb), dict(replay_max=n_amb - 1), dict(amb_cap=n_amb), dict(amb_cap=n_amb - 1),
                       dict(replay_max=n_amb + 1)):
                info2, _ = _check(sim, sums, length, n_runs=n_runs, **kw)
                paths.add((next(iter(kw)), kw[next(iter(kw))] - n_amb, info2["path"]))
    assert paths == {("replay_max", 0, 0), ("replay_max", -1, 1), ("replay_max", 1, 0), ("amb_cap", 0, 0), ("amb_cap", -1, 1)}
    assert min(seen.values()) >= 400, seen


def test_the_products_limits_on_zeros(sim):
    """all-zero buffers make every chunk ambiguous (s1 = 1, C = 5552): the lengths the GPU test runs, each on the side of
    REPLAY_MAX = 4096 the shared predicate puts it, with the chunks of a run api.hip takes"""
    seen = {}
    for length in CC.ZERO_LENGTHS:
        n_chunks, n_runs, per = host_sim.adler_shape(sim, length)
        sums = [(0, 0)] * n_chunks
        info, c = _check(sim, sums, length)
        assert c["low"] == n_chunks == info["n_amb"] and c["mid"] == 0
        assert _chain(sim, sums, length)[0] == zlib.adler32(bytes(length))  # (s2 never goes negative on zeros: RFC's value)
        seen[length] = (n_chunks, per, info["path"])
    assert seen == {N * 4095 - 1: (4095, 4, 0), N * 4095: (4096, 4, 0), N * 4095 + 1: (4096, 4, 0),
                    N * 4096 - 1: (4096, 4, 0), N * 4096: (4097, 5, 1), N * 4096 + 1: (4097, 5, 1),
                    N * 1024 - 1: (1024, 1, 0), N * 1024: (1025, 2, 0), N * 1024 + 1: (1025, 2, 0)}


def test_rfc_finish_model_equals_zlib(sim):
    rng = np.random.default_rng(5)
    datas = [CC.plan("p600").data, CC.plan("p3000").data, np.full(20000, 255, np.uint8)]
    datas += [rng.integers(0, 256, n, dtype=np.uint8) for n in CC.RFC_LENGTHS + (0, 1, 5551, 5552, 5553, 3 * N * 1000 + 17)]
    per = set()
    for d in datas:
        sums = CC.grid_sums(d)
        assert host_sim.adler_rfc(sim, *_cols(sums), len(d)) == zlib.adler32(d.tobytes()), len(d)
        per.add(-(-len(sums) // 1024))
    assert {0, 1, 2, 3} <= per
    assert [n // N + 1 for n in CC.RFC_LENGTHS] == [1023, 1024, 1025]


# ---- the mutation table ------------------------------------------------------------------------------------------------
# (name, file, text, replacement, killer): one-line mutants of the Adler-32 chunk chain's arithmetic, killed on the CPU only --
# each built into a host model of its own (tests/host_sim/sim_adler.cpp) and run in a child process by
# test_adler_chain_mutants_are_killed below.  killer: the case of tests/checksum_cases.py
# mutation_cases() whose result it must change, or ("equivalent", why): it must change none.
# (The ambiguity bounds the other way -- `<=` for `<` -- only replay a chunk more: equivalent by construction, not listed.)
ADLER_MUTANTS = [
    ("amb_low_bound_less_1", "adler_chain.h", "return C < ADLER_BASE ||", "return C < ADLER_BASE - 1 ||",
     ("equivalent", "|s2| <= 65520, so a chunk with C = 65520 never goes negative: the bound is one wider than it must be")),
    ("amb_low_bound_less_2", "adler_chain.h", "return C < ADLER_BASE ||", "return C < ADLER_BASE - 2 ||", "low_bound_stays_negative_last"),
    ("amb_mid_lower_bound_plus_1", "adler_chain.h", "(C > 0x80000000ull - ADLER_BASE &&", "(C > 0x80000000ull - ADLER_BASE + 1 &&",
     "mid_lower_bound"),
    ("amb_mid_upper_bound_less_1", "adler_chain.h", "C < 0x80000000ull + ADLER_BASE);", "C < 0x80000000ull + ADLER_BASE - 1);",
     ("equivalent", "s2 >= -65520, so C = 2^31 + 65520 stays at or above 2^31: the bound is one wider than it must be")),
    ("amb_mid_upper_bound_less_2", "adler_chain.h", "C < 0x80000000ull + ADLER_BASE);", "C < 0x80000000ull + ADLER_BASE - 2);",
     "mid_upper_bound"),
    ("a_term_without_225", "adler_chain.h", "hi_k ? ADLER_BASE - 225u : 0u", "hi_k ? 0u : 0u", "ff_chunks"),
    ("hi_k_strict", "adler_chain.h", "return C >= 0x80000000ull;", "return C > 0x80000000ull;",
     ("equivalent", "C = 2^31 is ambiguous: the chunk is replayed exactly, its a term is taken back out by the same function, "
                    "and the branch of an ambiguous chunk is read by nobody (the next chunk takes exact_next or does not care)")),
    ("zero_residue_negative", "adler_chain.h", "(rr == 0 ? 0 : (int32_t)rr - (int32_t)ADLER_BASE)", "((int32_t)rr - (int32_t)ADLER_BASE)",
     "zero_behind_hi_then_mid"),
    ("exact_at_ignored", "adler_chain.h", "k == st.exact_at ? st.exact_next : adler_signed_s2(rr, prev)", "adler_signed_s2(rr, prev)",
     "adjacent_exact"),
    ("prev_branch_no_walk_back", "adler_chain.h", "  while (run >= 0 && run_last_hi[run] == 0xFFFFFFFFu) run--;\n", "",
     ("equivalent", "run (k - 1) / per holds chunk k - 1, so it is never empty: the walk back never takes a step")),
    ("prev_branch_of_k", "adler_chain.h", "int64_t run = (int64_t)((k - 1) / per);", "int64_t run = (int64_t)(k / per);",
     "opens_run_behind_hi"),
    ("delta_not_carried", "adler_chain.h", "const uint32_t rr = addmod(res, st.delta);", "const uint32_t rr = addmod(res, 0u);",
     "delta_carried"),
    ("final_without_delta", "adler_chain.h", "(total_res + st.delta) % ADLER_BASE", "(total_res + 0u) % ADLER_BASE", "mid_upper_bound"),
    ("final_ignores_exact_at", "adler_chain.h", "if (st.exact_at == n_chunks) final_s2", "if (false && st.exact_at == n_chunks) final_s2",
     "low_bound_stays_negative_last"),
    ("fallback_at_the_limit", "adler_chain.h", "n_amb > amb_cap || n_amb > replay_max", "n_amb > amb_cap || n_amb >= replay_max",
     "replay_at_its_limit"),
    ("per_rounded_down", "adler_chain.h", "(n_chunks + n_runs - 1) / n_runs : 1", "n_chunks / n_runs : 1", "ten_chunks_four_runs"),
    ("rfc_chain_bytes_not_reduced", "adler_chain.h", "(nb[i] % ADLER_BASE) * c1", "nb[i] * c1",
     ("equivalent", "a run's bytes stay below 2^37 for any length the launches take and c1 < 2^16: the 64-bit product cannot wrap")),
]

_MUTANT_CHILD = r"""
import ctypes as C, json, os, random, sys
root = sys.argv[2]
sys.path.insert(0, os.path.join(root, "tests")); sys.path.insert(0, root)
import checksum_cases as CC, host_sim
sim = host_sim.bind_adler(C.CDLL(sys.argv[1]))
cols = lambda sums: ([s[0] for s in sums], [s[1] for s in sums])
cases = CC.mutation_cases()
first = sys.argv[3:]  # the case the table names: before any other (a mutant may end the child in one of those)
for name in first + [n for n in cases if n not in first]:
    c = cases[name]
    kw = {k: v for k, v in c.items() if k not in ("sums", "length")}
    v, info = host_sim.adler_chain(sim, *cols(c["sums"]), c["length"], seed=1, **kw)
    print(json.dumps([name, [v, info["path"]]]), flush=True)
    print(json.dumps([name + " (rfc)", host_sim.adler_rfc(sim, *cols(c["sums"]), c["length"])]), flush=True)
# a batch of dense random sequences on top: what an "equivalent" mutant must leave alone as well
rnd = random.Random(99)
out = []
for i in range(150):
    n_chunks = rnd.randrange(8, 60)
    sums, length = CC.random_sequence(rnd, n_chunks, rnd.choice((0, 16, 5551)), 1.0)
    out.append(host_sim.adler_chain(sim, *cols(sums), length, n_runs=rnd.choice((2, 4, 8)), seed=i)[0])
    out.append(host_sim.adler_rfc(sim, *cols(sums), length))
print(json.dumps(["random batch", out]), flush=True)
"""


def _run_child(so, first=()):
    rc, rows, err = mutation.run_child(_MUTANT_CHILD, so, mutation.ROOT, *first, timeout=300, every_line=True)
    return rc, dict(rows), err


def _build_model(m, tmp_path):
    """sim_adler.cpp alone against a copy of zipc_amd/csrc with the mutant `m` applied"""
    from tools import kernel_mutants as KM

    d = str(tmp_path / m[0])
    return mutation.single_model(SIM_ADLER, "adler_chain.h", KM.mutated_tree(m, d), os.path.join(d, "mutant.so"))


def judge(m, base, run):
    """a mutant's child against the unmutated header's `base` -> (the cases it changed, is that as its entry says)"""
    rc, got, _ = run
    changed = [k for k in base if got.get(k) != base[k]]
    return changed, mutation.verdict(m[4], [k for k in changed if k in got], crashed=rc != 0)  # (a case its child never reached kills nothing)


def test_adler_chain_mutants_are_killed(sim, tmp_path, capsys):
    """ADLER_MUTANTS: each one-line mutant of adler_chain.h built into a model of its own and run
    in a child process over checksum_cases.mutation_cases() (and a batch of random sequences).  A mutant must change the
    result of the case the table names (run first: rounding `per` down divides by zero in a later case, which ends that
    child, not this run); one listed as equivalent must change nothing at all.  The unmutated header gives
    the walk's value on every case, so a change is the mutant's."""
    from tools import kernel_mutants as KM

    cases = CC.mutation_cases()
    names = [m[0] for m in ADLER_MUTANTS]
    assert len(names) == len(set(names)) >= 14
    assert all(isinstance(m[4], tuple) and m[4][0] == "equivalent" or m[4] in cases for m in ADLER_MUTANTS)
    # the unmutated header, built the same way, in a child as well
    rc, base, err = _run_child(mutation.single_model(SIM_ADLER, "adler_chain.h", KM.CSRC, str(tmp_path / "plain.so")))
    assert rc == 0, err
    for name, c in cases.items():
        want, cnt = CC.walk(c["sums"], c["length"])
        assert base[name][0] == want and cnt["low"] + cnt["mid"] >= 1, name
        assert base[name][1] == host_sim.ADLER_REPLAY, name

    sos = mutation.build_all(lambda m: _build_model(m, tmp_path), ADLER_MUTANTS)
    runs = mutation.build_all(lambda a: _run_child(*a), zip(sos, [[] if isinstance(m[4], tuple) else [m[4]] for m in ADLER_MUTANTS]))
    rows, bad = [], []
    for m, run in zip(ADLER_MUTANTS, runs):
        changed, ok = judge(m, base, run)
        rows.append((m[0], "equivalent" if isinstance(m[4], tuple) else m[4], changed, run[0]))
        if not ok:
            bad.append(m[0])
    with capsys.disabled():
        print("\nzipc_amd/csrc/adler_chain.h mutants against %d crafted cases (tests/checksum_cases.py) and a random batch" % len(cases))
        print("  %-30s %-34s %6s  %s" % ("mutant", "named killer", "cases", "first change"))
        for name, killer, changed, rc in rows:
            verdict = ("ok" if not changed else "CHANGED") if killer == "equivalent" else ("ok" if killer in changed else "MISSED")
            print("  %-30s %-34s %6d  %s%s" % (name, "%s %s" % (killer, verdict), len(changed), changed[0] if changed else "-",
                                               "" if rc == 0 else "  (the child then ended with %d)" % rc))
        eq_names = [m[0] for m in ADLER_MUTANTS if isinstance(m[4], tuple)]
        n_eq = len(eq_names)
        print("  %d of %d killed by their named case, %d equivalent, %d wrong" % (len(rows) - n_eq - len([b for b in bad if b not in eq_names]), len(rows) - n_eq, n_eq, len(bad)))
        for m in ADLER_MUTANTS:
            if isinstance(m[4], tuple):
                print("  equivalent: %-30s %s" % (m[0], m[4][1]))
    assert bad == []


# ---- the CRC-32 finish's grid ------------------------------------------------------------------------------------------

def _nsegs():
    out = set(range(1, 41))
    for c in (256, 2048, 4096, 131072):
        out |= set(range(c - 2, c + 3))
    return sorted(out)


def test_crc_finish_reads_every_partial_once_in_order(sim):
    """For every count of partials around the finish's seams, with 256 and with 1024 threads and with what the launch
    takes: the places of the fold hold the virtual zeros, then partial 0, 1, 2 ... nseg - 1, each once; every word a thread
    fetches (clamped ones and the rows of a batch of eight behind the last row included) lies in [0, nseg)."""
    shapes = {}
    for nseg in _nsegs():
        for threads in (0, 256, 1024):
            used, loaded, info = host_sim.crc_finish_grid(sim, nseg, threads=threads)
            nt = info["threads"]
            assert nt == (threads or (1024 if nseg > 4096 else 256))
            if nseg <= 16:
                assert info["one_thread"] == 1 and used.tolist() == list(range(nseg)), nseg
            else:
                rows, padp = info["rows"], info["padp"]
                assert info["one_thread"] == 0 and rows == -(-nseg // nt) and padp == rows * nt - nseg and 0 <= padp < nt
                assert len(used) == rows * nt and len(loaded) == -(-rows // 8) * 8 * nt
                assert (used[:padp] == -1).all() and np.array_equal(used[padp:], np.arange(nseg)), (nseg, nt)
                if not threads:
                    assert (nseg, nt, rows, padp) == CC.crc_shape(nseg * CC.CRC_SEG)
            assert len(loaded) == 0 or int(loaded.max()) < nseg, (nseg, nt)
            if not threads:
                shapes[nseg] = (nt, info["rows"])
    assert [shapes[n] for n in (16, 17, 256, 257, 2048, 2049, 4096, 4097, 131072)] == [
        (256, 0), (256, 1), (256, 1), (256, 2), (256, 8), (256, 9), (256, 16), (1024, 5), (1024, 128)]
    # the lengths of the GPU test around a seam S: S * 32768 + d has S segments for d = -32767, -1, 0 and S + 1 for d = 1
    for S in CC.CRC_SEAMS:
        assert [CC.crc_shape(S * CC.CRC_SEG + d)[0] for d in CC.CRC_DELTAS] == [S, S, S, S + 1]
