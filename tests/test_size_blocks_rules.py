"""The HIP-free rules of sizing by blocks (zipc_amd/csrc/forms.h size_blocks_gate / size_blocks_pick, inflate_blocks.h
size_chain_at / size_blocks_verdict / size_blocks_groups), compiled with g++ (tests/size_blocks_sim/sim_size_blocks.cpp)
and pinned row by row.  The verdict's table covers every combination of its inputs; only two say "sized".  Every clause
of the rule has a mutant -- a text patch of a copy of inflate_blocks.h, in the manner of tests/golden/mutants.py -- that
must change at least one row.  No GPU; the kernels that apply the rules are checked in tests/test_gpu_inflate_size_blocks.py."""
import collections
import ctypes as C
import itertools
import os
import shutil

import pytest

import mutation

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "zipc_amd", "csrc")
SIM = os.path.join(HERE, "size_blocks_sim", "sim_size_blocks.cpp")
KIB, MIB = 1 << 10, 1 << 20
NONE, SAME, OTHER_POS = 0, 1, 2  # inflate_blocks.h SizeChainAt
U64P, U32P = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)


def _build(tmp, patch=None):
    """the sim as a shared library, over the repository's headers or -- patch = (old, new) -- over a copy of them whose
    inflate_blocks.h has that one change (it must match exactly once)"""
    src = SIM
    if patch is not None:
        tree = os.path.join(str(tmp), "zipc_amd", "csrc")
        os.makedirs(tree)
        for h in ("inflate_blocks.h", "forms.h", "tuning.h", "zd_common.h"):
            shutil.copy(os.path.join(CSRC, h), tree)
        p = os.path.join(tree, "inflate_blocks.h")
        text = mutation.patched(open(p).read(), patch[0], patch[1], "inflate_blocks.h")
        open(p, "w").write(text)
        os.makedirs(os.path.join(str(tmp), "tests", "size_blocks_sim"))
        src = os.path.join(str(tmp), "tests", "size_blocks_sim", "sim_size_blocks.cpp")
        shutil.copy(SIM, src)
    L = C.CDLL(mutation.gxx(os.path.join(str(tmp), "libsize_blocks_sim.so"), [src], opt="-O1", extra=["-Wall", "-Wno-unknown-pragmas"]))
    for f in ("sim_blocks_min_src", "sim_blocks_max_src", "sim_blocks_max_streams", "sim_size_scratch_budget"):
        getattr(L, f).restype = C.c_uint64
    L.sim_size_gate.restype = C.c_int
    L.sim_size_gate.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32]
    L.sim_size_pick.restype = C.c_uint64
    L.sim_size_pick.argtypes = [C.c_uint64, U64P, U64P, U64P, U32P, U32P]
    L.sim_size_groups.restype = C.c_uint64
    L.sim_size_groups.argtypes = [C.c_uint64, U64P, C.c_uint64, U64P, U64P]
    L.sim_size_chain_at.restype = C.c_int
    L.sim_size_chain_at.argtypes = [C.c_uint32, U64P, U32P, C.c_uint64, C.c_uint64]
    L.sim_size_verdict.restype = C.c_uint32
    L.sim_size_verdict.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_int, C.c_uint64, U64P]
    L.sim_size_head_scratch.restype = None
    L.sim_size_head_scratch.argtypes = [C.c_uint64, U64P]
    return L


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("size_blocks_sim"))


def pick(L, src_len, dst_off=None, dst_cap=None, flags=None):
    n = len(src_len)
    arr = lambda t, v: (t * n)(*v) if v is not None else None  # noqa: E731
    picked = (C.c_uint32 * max(n, 1))()
    k = L.sim_size_pick(n, arr(C.c_uint64, src_len), arr(C.c_uint64, dst_off), arr(C.c_uint64, dst_cap), arr(C.c_uint32, flags), picked)
    return [int(picked[i]) for i in range(k)]


def test_the_limits_are_the_decode_paths(sim):
    assert sim.sim_blocks_min_src() == 40 * KIB and sim.sim_blocks_max_src() == 0x1FFFFFFF
    from zipc_amd import _lib
    assert _lib.BLOCKS_MIN_SRC == sim.sim_blocks_min_src()


def test_gate_rows(sim):
    lo, hi = sim.sim_blocks_min_src(), sim.sim_blocks_max_src()
    rows = [(0, 0), (1, 0), (lo - 1, 0), (lo, 1), (lo + 1, 1), (MIB, 1), (hi - 1, 1), (hi, 1), (hi + 1, 0), (0xFFFF0000, 0), (0xFFFF0001, 0),
            (1 << 40, 0)]
    for src_len, want in rows:
        for dst_off, dst_cap in ((0, 0), (1 << 63, 1 << 40), (0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF), (7, 1)):
            for flags in (0, 1):  # (HAS_LIMIT is a stream's own business)
                assert sim.sim_size_gate(src_len, dst_off, dst_cap, flags) == want, (src_len, dst_off, dst_cap, flags)
    # a flag bit that is an argument error is the one wave's to report
    for flags in (2, 4, 1 | 2, 1 << 31, (1 << 31) | 1):
        assert sim.sim_size_gate(MIB, 0, 0, flags) == 0, flags


def test_pick_rows(sim):
    lo, hi = sim.sim_blocks_min_src(), sim.sim_blocks_max_src()
    # nothing under BLOCKS_MIN_SRC or over BLOCKS_MAX_SRC
    assert pick(sim, [lo - 1]) == [] and pick(sim, [hi + 1]) == [] and pick(sim, []) == []
    assert pick(sim, [lo - 1, 0, 1000, hi + 1, 0xFFFF0001]) == []
    # all of a few long streams
    assert pick(sim, [MIB]) == [0]
    assert pick(sim, [lo]) == [0]
    assert pick(sim, [64 * MIB]) == [0]
    assert pick(sim, [MIB, 2 * MIB, 300 * KIB]) == [0, 1, 2]
    assert pick(sim, [MIB] * 16) == list(range(16))
    assert pick(sim, [MIB] * 64) == list(range(64))
    # the few long ones among many short ones (in ascending order, wherever they stand)
    many = [3000 + 7 * i for i in range(400)]
    assert pick(sim, many) == []
    assert pick(sim, many[:100] + [MIB] + many[100:300] + [4 * MIB, 2 * MIB] + many[300:]) == [100, 301, 302]
    assert pick(sim, [MIB] + many + [lo - 1]) == [0]
    # (beside a stream too long for the path, whose one wave outlasts everything, nothing is gained: none)
    assert pick(sim, [MIB] + many + [hi + 1]) == []
    # none of thousands of equal ones: their one waves run side by side
    assert pick(sim, [MIB] * 4096) == []
    assert pick(sim, [256 * KIB] * 8192) == []
    # a stream with a flag bit that is an argument error stays with the one wave; HAS_LIMIT changes nothing
    assert pick(sim, [MIB, MIB, MIB], flags=[0, 2, 1]) == [0, 2]
    # dst_off / dst_cap of any value do not change the pick
    shapes = ([MIB], [MIB, 2 * MIB, 300 * KIB], many[:100] + [MIB] + many[100:], [MIB] * 4096, [lo - 1, lo, hi, hi + 1])
    for src_len in shapes:
        base = pick(sim, src_len)
        n = len(src_len)
        for off, cap in ((0, 0), (0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF), (1 << 63, 7), (0, 1), (12345, 0xFFFF0001)):
            assert pick(sim, src_len, dst_off=[off] * n, dst_cap=[cap] * n) == base, (src_len[:4], off, cap)
        assert pick(sim, src_len, dst_off=list(range(n)), dst_cap=[(i * 7919) % 100000 for i in range(n)]) == base


def test_pick_follows_its_model(sim):
    """the k longest streams go by blocks, k chosen by the model: adding short streams never removes a long one from the
    pick, and what is picked is always a set of the longest"""
    for n_long, n_short in itertools.product((1, 2, 5, 40), (0, 10, 1000)):
        src_len = [MIB + 1000 * i for i in range(n_long)] + [5000] * n_short
        got = pick(sim, src_len)
        assert got == sorted(got) and all(i < n_long for i in got)
        longest_left = max([src_len[i] for i in range(len(src_len)) if i not in got] or [0])
        assert all(src_len[i] >= longest_left for i in got)
        assert len(got) == n_long, (n_long, n_short, got)


def test_groups_hold_what_the_scratch_budget_allows(sim):
    budget = sim.sim_size_scratch_budget()

    def groups(src_len, stride=32768):
        n = len(src_len)
        ends, worst = (C.c_uint64 * n)(), C.c_uint64()
        g = sim.sim_size_groups(n, (C.c_uint64 * n)(*src_len), stride, ends, C.byref(worst))
        return [int(ends[i]) for i in range(g)], worst.value

    assert groups([MIB]) == ([1], groups([MIB])[1])
    ends, worst = groups([MIB] * 64)
    assert ends == [64] and worst <= budget
    ends, worst = groups([256 * MIB] * 9)  # a stream's lists are half its length and more: a few of these fill a group
    assert ends[-1] == 9 and len(ends) > 1 and ends == sorted(set(ends))
    sizes = [b - a for a, b in zip([0] + ends[:-1], ends)]
    assert all(s >= 1 for s in sizes) and worst <= budget
    ends, worst = groups([sim.sim_blocks_max_src()] * 3)  # (the longest stream there is: a group to itself if it must)
    assert ends[-1] == 3 and all(b - a >= 1 for a, b in zip([0] + ends[:-1], ends))


def test_head_scratch_layout(sim):
    for nj in (1, 2, 63, 64, 65, 1000):
        out = (C.c_uint64 * 4)()
        sim.sim_size_head_scratch(nj, out)
        heads, streams, span, total = (int(v) for v in out)
        assert heads == 0 and streams >= nj * 24 and span >= streams + 4 * nj and total == span + nj * 64 * 18 * 2
        assert streams % 256 == 0 and span % 256 == 0


# ---- the verdict

Row = collections.namedtuple("Row", "head_status head_final chain_ok chain_at")
HEAD_OUT, CHAIN_OUT = 40000, 1234567  # (the head's position at its end; the chain's sum)


def want_verdict(r):
    """the issue's rule, written down a second time: sized if and only if the head is OK and either it saw the final block
    (its own position is the size) or the chain is chain_ok and holds a block at exactly the head's bit and position"""
    if r.head_status != 0:
        return 0, 0
    if r.head_final:
        return 1, HEAD_OUT
    if r.chain_ok and r.chain_at == SAME:
        return 1, CHAIN_OUT
    return 0, 0


def verdict_rows():
    return [Row(*v) for v in itertools.product((0, 1, 2, 16, 18), (0, 1), (0, 1), (NONE, SAME, OTHER_POS))]


def run_verdict(L, r):
    ol = C.c_uint64(0xEEEE)
    sized = L.sim_size_verdict(r.head_status, r.head_final, HEAD_OUT, r.chain_ok, r.chain_at, CHAIN_OUT, C.byref(ol))
    return int(sized), int(ol.value)


# a chain of five blocks, and where a head may have ended: (bit, position) -> what the chain holds there
CHAIN_BITS, CHAIN_POS = [0, 1000, 5000, 5003, 90000], [0, 33000, 70000, 70000, 300000]
CHAIN_AT_ROWS = [((1000, 33000), SAME), ((1000, 32999), OTHER_POS), ((1000, 0), OTHER_POS), ((999, 33000), NONE), ((1001, 33000), NONE),
                 ((0, 0), SAME), ((0, 1), OTHER_POS), ((5000, 70000), SAME), ((5003, 70000), SAME), ((5003, 70001), OTHER_POS),
                 ((90000, 300000), SAME), ((90001, 300000), NONE), ((1 << 40, 300000), NONE), ((4999, 70000), NONE)]


def run_chain_at(L, at, n=None):
    n = len(CHAIN_BITS) if n is None else n
    return L.sim_size_chain_at(n, (C.c_uint64 * 5)(*CHAIN_BITS), (C.c_uint32 * 5)(*CHAIN_POS), at[0], at[1])


def test_verdict_table(sim):
    rows = verdict_rows()
    assert len(rows) == 60
    said = [r for r in rows if run_verdict(sim, r)[0]]
    for r in rows:
        assert run_verdict(sim, r) == want_verdict(r), r
    # only the two combinations may say "sized": the head OK and final (whatever the chain), or OK, chain_ok and a block at
    # the head's bit and position
    assert all(r.head_status == 0 and (r.head_final or (r.chain_ok and r.chain_at == SAME)) for r in said)
    assert len(said) == 6 + 1
    for at, want in CHAIN_AT_ROWS:
        assert run_chain_at(sim, at) == want, at
    assert run_chain_at(sim, (0, 0), n=0) == NONE and run_chain_at(sim, (1000, 33000), n=1) == NONE


# every clause of the rule, broken once: (name, what, (old, new) in inflate_blocks.h)
MUTANTS = [
    ("head_status_ignored", "a head that failed still lets the chain size the stream",
     ("  if (head_status != ST_OK) return v;\n", "")),
    ("head_final_dropped", "a head that saw the final block does not size the stream",
     ("  if (head_final != 0u) { v.sized = 1;", "  if (false) { v.sized = 1;")),
    ("head_always_final", "the head's position is taken for the size whether it saw the final block or not",
     ("  if (head_final != 0u) { v.sized = 1;", "  if (true) { v.sized = 1;")),
    ("chain_ok_ignored", "a chain that is not chain_ok sizes the stream",
     ("  if (chain_ok != 0u && chain_at == SIZE_CHAIN_SAME)", "  if (chain_at == SIZE_CHAIN_SAME)")),
    ("position_not_compared", "a chain block at the head's bit counts whatever its position",
     ("  if (chain_ok != 0u && chain_at == SIZE_CHAIN_SAME)", "  if (chain_ok != 0u && chain_at != SIZE_CHAIN_NONE)")),
    ("chain_block_not_needed", "chain_ok alone sizes the stream, no block at the head's end asked for",
     ("  if (chain_ok != 0u && chain_at == SIZE_CHAIN_SAME)", "  if (chain_ok != 0u)")),
    ("bit_not_compared", "the first chain block at or behind the head's bit counts as the one at it",
     ("  if (lo >= n_blocks || chain[lo].bit != bit) return SIZE_CHAIN_NONE;", "  if (lo >= n_blocks) return SIZE_CHAIN_NONE;")),
    ("chain_size_from_the_head", "the size of a stream sized by its chain is the head's position",
     ("{ v.sized = 1; v.out_len = chain_out; }", "{ v.sized = 1; v.out_len = head_out; }")),
]


@pytest.mark.parametrize("name", [m[0] for m in MUTANTS])
def test_every_clause_has_a_row(name, tmp_path):
    """the mutant changes at least one row of the two tables"""
    _, what, patch = next(m for m in MUTANTS if m[0] == name)
    L = _build(tmp_path, patch)
    changed = [r for r in verdict_rows() if run_verdict(L, r) != want_verdict(r)]
    changed += [at for at, want in CHAIN_AT_ROWS if run_chain_at(L, at) != want]
    assert changed, (name, what, "no row of the tables tells this mutant from the rule")
