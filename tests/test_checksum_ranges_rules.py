"""zipc_amd/csrc/checksum_ranges.h -- the rules of the ragged checksum pass (zipc_hip_checksum_batch), one header for
the kernels of checksum.hip and this test -- compiled with g++ into a host model (tests/checksum_ranges_sim/sim_ranges.cpp)
that runs the launches as loops and checks every index before it is used.  Held against the oracle and zlib on the
inputs of tests/checksum_batch_cases.py; a mutation table over the header; and the same model as a stand-alone program
under the address sanitizer (audit_main.cpp).  No GPU; the kernels are checked in tests/test_gpu_checksum_batch.py."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

import checksum_batch_cases as BC
import mutation
import util  # noqa: F401  (sets sys.path through conftest)

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_DIR = os.path.join(HERE, "checksum_ranges_sim")
HEADER = os.path.join(os.path.dirname(HERE), "zipc_amd", "csrc", "checksum_ranges.h")
RESULT = np.dtype([("status", "<u4"), ("crc32", "<u4"), ("adler32", "<u4"), ("reserved", "<u4")])
STATS = ("segs", "chunks", "segs_bound", "chunks_bound", "bad", "violations", "one_lane", "columns", "max_rows", "tiles",
         "loaded", "worked")


SIM = os.path.join(SIM_DIR, "sim_ranges.cpp")
FLAGS = dict(extra=["-Wall", "-Wno-unknown-pragmas"])


def _bind(so):
    L = C.CDLL(so)
    L.sim_ranges_run.restype = C.c_uint64
    L.sim_ranges_run.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_int, C.c_int,
                                 C.c_void_p, C.c_void_p]
    L.sim_range_verdict.restype = C.c_uint32
    L.sim_range_verdict.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64]
    for f in ("sim_ranges_plan_tile", "sim_ranges_horner_max", "sim_ranges_finish_lanes"):
        getattr(L, f).restype = C.c_uint32
    return L


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return _bind(mutation.gxx(tmp_path_factory.mktemp("ranges_sim") / "libranges_sim.so", [SIM], **FLAGS))


def run(L, arena, ranges, total, crc=True, adler=True, rfc=False):
    """-> (results as a RESULT array, stats as a dict)"""
    arena = np.ascontiguousarray(arena)
    r = BC.ranges_array(ranges)
    res = np.zeros(max(len(ranges), 1), RESULT)
    stats = np.zeros(len(STATS), np.uint64)
    L.sim_ranges_run(arena.ctypes.data, len(arena), r.ctypes.data, len(ranges), total, int(crc), int(adler), int(rfc),
                     res.ctypes.data, stats.ctypes.data)
    return res[:len(ranges)], dict(zip(STATS, (int(v) for v in stats)))


def test_constants_are_the_cases_files(sim):
    assert sim.sim_ranges_plan_tile() == BC.PLAN_TILE
    assert sim.sim_ranges_horner_max() == BC.HORNER_MAX
    assert sim.sim_ranges_finish_lanes() == BC.FINISH_LANES


@pytest.mark.parametrize("name", BC.NAMES)
def test_model_gives_the_oracles_checksums(sim, oracle, name):
    """every case: both checksums of every range are the oracle's (and zlib's CRC-32), the bad ranges say so and their
    neighbours are right, no index left its array, and exactly the ranges' bytes were loaded"""
    c = BC.case(name)
    ref = BC.reference(name, oracle)
    res, st = run(sim, c["arena"], c["ranges"], c["total"])
    assert st["violations"] == 0 and st["bad"] == 0
    assert st["segs"] <= st["segs_bound"] and st["chunks"] <= st["chunks_bound"]
    assert st["loaded"] == c["total"] and st["worked"] == st["segs"]
    for i, (crc, adler, _) in enumerate(ref):
        want = (BC.INVALID_ARG, 0, 0) if i in c["bad"] else (0, crc, adler)
        assert (int(res["status"][i]), int(res["crc32"][i]), int(res["adler32"][i])) == want, (name, i, c["ranges"][i])
    # RFC 1950's arithmetic: zlib's value
    res, st = run(sim, c["arena"], c["ranges"], c["total"], crc=False, rfc=True)
    assert st["violations"] == 0
    for i, (_, _, rfc) in enumerate(ref):
        assert (int(res["crc32"][i]), int(res["adler32"][i])) == (0, rfc), (name, i)


def test_every_threshold_of_the_finish_is_met(sim):
    """what the cases file names is what the model counts: lengths on both sides of one lane | columns and of one row |
    two rows, and the long range's nine rows"""
    c = BC.case("lengths_rand")
    shapes = [BC.finish_shape(n) for _, n in c["ranges"]]
    _, st = run(sim, c["arena"], c["ranges"], c["total"], adler=False)
    assert st["one_lane"] == sum(s[1] for s in shapes) and st["columns"] == sum(not s[1] for s in shapes) >= 3
    assert st["max_rows"] == max(s[2] for s in shapes) == 2
    lo, hi = BC.FINISH_THRESHOLDS["one lane | columns"]
    assert BC.finish_shape(lo)[:2] == (16, True) and BC.finish_shape(hi)[:2] == (17, False)
    lo, hi = BC.FINISH_THRESHOLDS["one row | two rows"]
    assert BC.finish_shape(lo) == (64, False, 1) and BC.finish_shape(hi) == (65, False, 2)
    assert {lo, hi} <= set(BC.LENGTHS)
    c = BC.case("ragged_middle")
    _, st = run(sim, c["arena"], c["ranges"], c["total"], adler=False)
    assert (st["columns"], st["max_rows"]) == (1, BC.finish_shape(BC.LONG)[2]) == (1, 9)
    assert st["tiles"] == 1
    for n, tiles in ((BC.PLAN_TILE, 1), (BC.PLAN_TILE + 1, 2), (2 * BC.PLAN_TILE, 2), (2 * BC.PLAN_TILE + 1, 3)):
        c = BC.case("n%d" % n)
        assert run(sim, c["arena"], c["ranges"], c["total"], adler=False)[1]["tiles"] == tiles


def test_bounds_hold_and_are_hit_by_ranges_of_one_byte(sim):
    arena = np.arange(5000, dtype=np.uint8)
    for n in (1, 7, 1023, 1025, 3000):
        ranges = [(i, 1) for i in range(n)]
        res, st = run(sim, arena, ranges, n)
        assert st["violations"] == 0 and (st["segs"], st["chunks"]) == (n, n) == (st["segs_bound"], st["chunks_bound"])
        assert all(int(res["crc32"][i]) == zlib.crc32(bytes([i & 255])) for i in range(n))
    # a declared total far above the truth only makes the grid larger
    res, st = run(sim, arena, [(0, 5000), (1, 1)], 10 ** 6)
    assert st["violations"] == 0 and st["segs"] == 2 and st["segs_bound"] == 10 ** 6 // 32768 + 2
    assert int(res["crc32"][0]) == zlib.crc32(arena.tobytes())


def test_verdicts(sim):
    A = 1000
    assert sim.sim_range_verdict(0, A, A) == 0 and sim.sim_range_verdict(A - 1, 1, A) == 0  # the end exactly at arena_len
    assert sim.sim_range_verdict(A, 0, A) == 0
    assert sim.sim_range_verdict(A - 1, 2, A) == BC.INVALID_ARG and sim.sim_range_verdict(A + 1, 0, A) == BC.INVALID_ARG  # one byte past it
    assert sim.sim_range_verdict(2 ** 64 - 1, 1, A) == BC.INVALID_ARG and sim.sim_range_verdict(5, 2 ** 64 - 5, 2 ** 64 - 1) == BC.INVALID_ARG  # off + len overflows
    assert sim.sim_range_verdict(5, 2 ** 64 - 6, 2 ** 64 - 1) == 0
    c = BC.case("shapes")
    ok = run(sim, c["arena"], c["ranges"], c["total"])
    assert ok[1]["bad"] == 0 and sorted(np.nonzero(ok[0]["status"])[0].tolist()) == list(c["bad"])
    # the declared total one too small: every result says INVALID_ARG, no checksum, no byte loaded
    res, st = run(sim, c["arena"], c["ranges"], c["total"] - 1)
    assert st["bad"] == 1 and st["loaded"] == 0 and st["violations"] == 0
    assert (res["status"] == BC.INVALID_ARG).all() and not res["crc32"].any() and not res["adler32"].any()


# ---- the mutation table: (name, the line as it stands, the line mutated) ---------------------------------------------
MUTANTS = (
    ("segments rounded down", "return (len - 1) / RANGES_SEG_BYTES + 1;", "return len / RANGES_SEG_BYTES;"),
    ("an empty range counted as one segment", "if (len == 0) return 0;", "if (len == 0) return 1;"),
    ("search: upper bound one short", "uint32_t lo = 0, hi = n_ranges;", "uint32_t lo = 0, hi = n_ranges - 1;"),
    ("search: base equal to w goes left", "if (seg_base[mid] <= w) lo = mid + 1;", "if (seg_base[mid] < w) lo = mid + 1;"),
    ("search: the first above w, not the last at or below", "return lo - 1;", "return lo;"),
    ("chunk base from the segment scan", "{ return before.chunks; }", "{ return before.segs; }"),
    ("arena check: >= for >", "if (end > arena_len) return ST_INVALID_ARG;", "if (end >= arena_len) return ST_INVALID_ARG;"),
    ("bad-call flag ignored by the segment pass", "return call.bad != 0 || w >= call.total_segs;", "return w >= call.total_segs;"),
    ("bad-call flag ignored by the results", "return call.bad != 0 ? (uint32_t)ST_INVALID_ARG : verdict;", "return verdict;"),
    ("overflow of off + len not looked at", "if (end < r.off) return ST_INVALID_ARG;", ""),
)


def _observe(L):
    """everything the model says about the small cases, a short declared total and ranges of one byte"""
    out = []
    for name in BC.SMALL:
        c = BC.case(name)
        for total in (c["total"], c["total"] - 1):
            res, st = run(L, c["arena"], c["ranges"], total)
            out.append((name, total, res.tobytes(), tuple(sorted(st.items()))))
    res, st = run(L, np.arange(64, dtype=np.uint8), [(i, 1) for i in range(9)], 9)
    out.append(("ones", 9, res.tobytes(), tuple(sorted(st.items()))))
    big = np.random.default_rng(1).integers(0, 256, 3 * BC.SEG, dtype=np.uint8)
    res, st = run(L, big, [(3, 2 * BC.SEG), (21, BC.SEG + 1), (0, 3 * BC.SEG)], 6 * BC.SEG + 1)
    out.append(("whole segments", 0, res.tobytes(), tuple(sorted(st.items()))))
    return out


def test_mutants_of_the_header_are_killed(sim, tmp_path):
    """each one-line mutant of checksum_ranges.h, built into a model of its own, changes what the model says of at least
    one case (a result, a count, or an index that leaves its array: the model counts such an index, it never follows it)"""
    base = _observe(sim)
    assert all(dict(row[3])["violations"] == 0 for row in base)
    alive = []
    for k, (name, line, mutated) in enumerate(MUTANTS):
        so = mutation.header_model(SIM, "RANGES_HEADER", HEADER, line, mutated, str(tmp_path / ("mutant%d" % k) / "libmutant.so"),
                                   rewrite_includes=("adler_chain.h", "zd_common.h"), **FLAGS)
        if _observe(_bind(so)) == base:
            alive.append(name)
    assert alive == []


def test_audit_program_under_the_address_sanitizer(tmp_path):
    """the model as a stand-alone program with its own main, built with -fsanitize=address,undefined and run as a process:
    the cases' seams and two thousand random ragged batches; it aborts on any index that leaves its array"""
    exe = str(tmp_path / "ranges_audit")
    mutation.gxx(exe, [os.path.join(SIM_DIR, "audit_main.cpp")], shared=False,
                 extra=["-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert b"no index left its array" in r.stdout
