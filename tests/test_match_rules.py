"""The match finder's rules on the CPU (no GPU): tests/host_sim/sim_match.cpp's serial reading of find_backref
(zipc_deflate.ml:1176-1201) against deflate_lane.h's lz_match_position at every position of every case of
tests/match_cases.py at the three levels, each case's planted property from the reference's own records, the launch
forms each call of tests/test_gpu_match_records.py gets, and a mutation table over the reference: every one-line mutant
must change a record of the cases, and the table says how many of the changed records the lazy parse would have read --
what the byte-parity tests could have seen."""
import concurrent.futures
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import host_sim  # noqa: E402
import match_cases as mc  # noqa: E402
import mutation  # noqa: E402

LEVELS = (1, 2, 3)
WORKERS = mutation.workers()


@pytest.fixture(scope="module")
def sim():
    return host_sim.lib()


def unique_streams():
    """every distinct stream of the three calls, by name"""
    out = {}
    for streams in mc.batches().values():
        for s in streams:
            out.setdefault(s.name, s)
    return out


def reference_records(L, streams, level):
    """name -> (best, first), the streams' references side by side (the library calls release the interpreter lock)"""
    with concurrent.futures.ThreadPoolExecutor(max_workers=WORKERS) as ex:
        return dict(zip([s.name for s in streams], ex.map(lambda s: host_sim.match_reference(L, s.data, level), streams)))


_REF = {}


@pytest.fixture(scope="module")
def refs(sim):
    def get(level):
        if level not in _REF:
            _REF[level] = reference_records(sim, list(unique_streams().values()), level)
        return _REF[level]
    return get


def test_the_cases_stay_small_and_the_colliding_strings_collide(sim):
    streams = unique_streams()
    assert sum(max(len(s) - 3, 0) for s in streams.values()) < 3_000_000
    lengths = {len(s) for s in streams.values()}
    for k in range(3):
        for d in mc.END_D:
            assert mc.T0 + mc.TILE * k + d in lengths
    assert {0, 3, 4, 5, 7, 8, 11, 15, 16, 17, 1023, 1024, 1025, 1026, 1027, 1028, 8191, 8192, 8193} <= lengths
    for a, b in mc.COLLIDING:
        assert sim.sim_match_hash4(a) == sim.sim_match_hash4(b) and a[0] != b[0]
    assert len({sim.sim_match_hash4(a) for a, _ in mc.COLLIDING}) == len(mc.COLLIDING)
    assert host_sim.MATCH_LEVELS == {lv: mc.LEVEL_K[lv] + (g,) for lv, g in zip(LEVELS, (4, 8, 32))}


@pytest.mark.parametrize("level", LEVELS)
def test_the_reference_equals_lz_match_position_everywhere(sim, refs, level):
    """sim_deflate proves that lz_match_position's records give the oracle's bytes; the plain reference is anchored by being
    equal to it at every position of every case"""
    streams = list(unique_streams().values())
    with concurrent.futures.ThreadPoolExecutor(max_workers=WORKERS) as ex:
        lane = list(ex.map(lambda s: host_sim.match_lane_position(sim, s.data, level), streams))
    for s, (lb, lf) in zip(streams, lane):
        rb, rf = refs(level)[s.name]
        bad = np.nonzero((rb != lb) | (rf != lf))[0]
        assert bad.size == 0, "%s level %d: %d positions differ, the first at %d: reference (%#x, %#x), lz_match_position (%#x, %#x)" % (
            s.name, level, bad.size, bad[0], rb[bad[0]], rf[bad[0]], lb[bad[0]], lf[bad[0]])


def check_property(s, pr, level, best, first):
    """None, or what is wrong"""
    K, Kq = mc.LEVEL_K[level]
    kind = pr[0]
    if kind in ("rec", "span"):
        if kind == "rec":
            ps, fn, lv_first, lv_best = [pr[1]], (lambda p, K, Kq, f=pr[2]: f(K, Kq)), pr[3], pr[4]
        else:
            ps, fn, lv_first, lv_best = range(pr[1], pr[2]), pr[3], pr[4], pr[5]
        for p in ps:
            wb, wf = fn(p, K, Kq)
            if level in lv_best and best[p] != wb:
                return "position %d: best (%d, %d), planted (%d, %d)" % (p, best[p] >> 9, best[p] & 511, wb >> 9, wb & 511)
            if level in lv_first and first[p] != wf:
                return "position %d: first (%d, %d), planted (%d, %d)" % (p, first[p] >> 9, first[p] & 511, wf >> 9, wf & 511)
    elif kind == "two":
        if level in pr[3] and not (best[pr[1]:pr[2]] != first[pr[1]:pr[2]]).any():
            return "no position of [%d, %d) has two answers" % (pr[1], pr[2])
    elif kind == "no_two":
        if (best != first).any():
            return "position %d has two answers" % np.nonzero(best != first)[0][0]
    elif kind == "share":
        share = float((best[pr[1]:pr[2]] != 0).mean())
        if not pr[3] <= share <= pr[4]:
            return "%.3f of [%d, %d) have a match, planted %.2f .. %.2f" % (share, pr[1], pr[2], pr[3], pr[4])
    else:
        return "unknown property %r" % (kind,)
    return None


@pytest.mark.parametrize("level", LEVELS)
def test_every_case_shows_what_it_was_planted_for(refs, level):
    wrong, n_props = [], 0
    for s in unique_streams().values():
        best, first = refs(level)[s.name]
        for pr in s.props:
            n_props += 1
            msg = check_property(s, pr, level, best, first)
            if msg:
                wrong.append("%s %s: %s" % (s.name, pr[0], msg))
    assert n_props > 150
    assert wrong == [], "\n".join(wrong[:20])


def test_the_seams_the_cases_are_for_are_reached(refs):
    """the planted positions, named: a 258-byte match at t1 - 258, t1 - 257 and t1 - 1 of every tile end, a candidate exactly
    32 768 back at p = t0, t0 + 1 and t1 - 1 of tiles 1 and 2 found and one 32 769 back not, every stream-end cap 4 .. 258,
    two answers in tile 1 (tile 2 at `Best), and a stream without any"""
    by = {s.name: s for s in unique_streams().values()}
    for level in LEVELS:
        best, _ = refs(level)["cross_82192"]
        for t1 in mc.TILE_STARTS:
            for p in (t1 - 258, t1 - 257, t1 - 1):
                assert best[p] == mc.rec(777, 258), (level, p)
        best, _ = refs(level)["edge32768_82191"]
        for p in (mc.T0, mc.T0 + 1, mc.T0 + mc.TILE - 1, mc.T0 + mc.TILE, mc.T0 + mc.TILE + 1, mc.T0 + 2 * mc.TILE - 1):
            assert best[p] == mc.rec(32768, 258), (level, p)
        best, first = refs(level)["edge32769_82185"]
        assert not best.any() and not first.any()
        caps = set()
        for name, s in by.items():
            if s.base == "cross":
                b = refs(level)[name][0]
                caps |= {int(b[p] & 511) for p in range(len(s) - 258, len(s) - 3) if b[p] >> 9 == 777}
        assert caps == set(range(4, 259))
        name, lo = ("pool_82178", mc.TILE_STARTS[0]) if level < 3 else ("k3a_82184", mc.TILE_STARTS[1])
        best, first = refs(level)[name]
        assert (best[lo:lo + mc.TILE] != first[lo:lo + mc.TILE]).any()


def test_which_kernel_each_call_gets(sim):
    """forms.h through sim_forms.cpp, with the arguments zipc_hip_debug_match_records computes the forms from (no exchange
    chain, one slice): the small call keeps lz_match_kernel, one byte more takes lz_match_window_kernel, and the ragged
    call's workgroups take two groups one behind the other at the levels that allow it"""
    B = mc.batches()

    def forms(streams, level, tpg):
        n, longest, total = len(streams), max(len(s) for s in streams), sum(len(s) for s in streams)
        return host_sim.deflate_forms(sim, n, longest, total, level=level, xchg_ok=0, match_tiles_per_group=tpg, slices_override=1)

    for level in LEVELS:
        for n in (8191, 8192):
            f, s = forms([x for x in B["small"] if len(x) <= n], level, 0)
            assert not s["match_window"] and f["cps"] == 8 and f["slices"] == 1
        f, s = forms(B["small"], level, 0)
        assert not s["match_window"]
        f, s = forms(B["alone8193"], level, 0)
        assert s["match_window"] and f["tps"] == 1 and s["gpw"] == 1
        for tpg, want_tpg, want_gps in ((0, 1, 4), (1, 1, 4), (2, 2, 2), (3, 3, 2)):
            f, s = forms(B["ragged"], level, tpg)
            assert s["match_window"] and f["tps"] == 4 and f["tpg"] == want_tpg and f["gps"] == want_gps and f["slices"] == 1
            assert s["gpw"] == (2 if level < 3 and want_gps == 4 else 1), (level, tpg, s["gpw"])
            assert s["chain"] == host_sim.CHAIN_PEEL


# ---- the mutation table ----------------------------------------------------------------------------------------------
# (name, the line of sim_match_reference as it stands, the mutant's, and for an equivalent mutant why no record can change)
MUTANTS = [
    ("K+1", "steps != K &&", "steps != K + 1 &&", None),
    ("K-1", "steps != K &&", "steps != K - 1 &&", None),
    ("Kq+1", "if (steps == Kq) {", "if (steps == Kq + 1) {", None),
    ("Kq-1", "if (steps == Kq) {", "if (steps == Kq - 1) {", None),
    ("tie >=", "if (l > best_len) {", "if (l >= best_len && l > 3) {", None),
    ("window >=", "p - i <= 32768)", "p - i < 32768)", None),
    ("cap 257", "uint32_t cap = 258; ", "uint32_t cap = 257; ", None),
    ("no stream-end cap", "if (cap > len - p) cap = len - p; ", "", None),
    ("snapshot before compare",
     "      if (l > best_len) { best_len = l; best_rec = ((p - i) << 9) | l; }  // strictly longer: the nearest wins a tie (zd.ml:1166-1174)\n"
     "      if (steps == Kq) { first_rec = best_rec; have_first = true; }\n",
     "      if (steps == Kq) { first_rec = best_rec; have_first = true; }\n"
     "      if (l > best_len) { best_len = l; best_rec = ((p - i) << 9) | l; }\n", None),
    ("hash-only not counted", "      steps++;  //", "      if (l >= 4) steps++;  //", None),
    ("no l == cap exit", "      if (l == cap) break;  // zd.ml:1194\n", "",
     "a candidate that reaches the cap is the best so far (strictly longer, or the walk would have ended at the earlier one), "
     "nothing behind it is longer than the cap, and a tie keeps the nearer one: best is the same, and first is best as it "
     "stands at the Kq-th candidate or at the chain's end, the same value either way"),
]
SPLIT = "// -----"  # the reference is the file's top half (sim_match.cpp)


def build_mutant(name, old, new, out_dir):
    src = open(os.path.join(HERE, "host_sim", "sim_match.cpp")).read()
    top = src[:src.index(SPLIT)]
    path = os.path.join(out_dir, "m_%d" % [m[0] for m in MUTANTS].index(name))
    with open(path + ".cpp", "w") as f:
        f.write(mutation.patched(top, old, new, "sim_match.cpp " + name))
    return host_sim.bind_match(C.CDLL(mutation.gxx(path + ".so", [path + ".cpp"], extra=["-Wall"])))


def mutant_streams():
    """the streams the mutants run on: each base once (its longest prefix) and the short cases"""
    seen, out = set(), []
    for s in mc.long_streams() + mc.small_streams() + [mc.window_8193()] + mc.tiny_streams(6):
        key = s.base or s.name
        if key not in seen:
            seen.add(key)
            out.append(s)
    return out


def test_every_mutant_of_the_reference_changes_a_record(sim, refs, tmp_path, capsys):
    streams = mutant_streams()
    libs = mutation.build_all(lambda m: build_mutant(m[0], m[1], m[2], str(tmp_path)), MUTANTS)
    reads = {lv: {s.name: host_sim.match_parse_reads(sim, len(s), lv, *refs(lv)[s.name]) for s in streams} for lv in LEVELS}
    rows, wrong = [], []
    for (name, _, _, why), ML in zip(MUTANTS, libs):
        per_level = []
        for lv in LEVELS:
            got = reference_records(ML, streams, lv)
            changed = read = 0
            first_case = None
            for s in streams:
                rb, rf = refs(lv)[s.name]
                mb, mf = got[s.name]
                db, df = rb != mb, rf != mf
                n = int((db | df).sum())
                if n and first_case is None:
                    first_case = "%s@%d" % (s.name, np.nonzero(db | df)[0][0])
                changed += n
                r = reads[lv][s.name]
                read += int(((r == 1) & db).sum() + ((r == 2) & df).sum())  # the record the parse reads there is a changed one
            per_level.append((changed, read, first_case))
        rows.append((name, why, per_level))
        total = sum(c for c, _, _ in per_level)
        if (why is None) != (total > 0):
            wrong.append(name)
    with capsys.disabled():
        print("\nsim_match.cpp mutants over %d streams: records changed / of those read by the lazy parse, per level" % len(streams))
        print("  %-26s %18s %18s %18s  %s" % ("mutant", "fast", "default", "best", "first change"))
        for name, why, per in rows:
            cells = ["%d / %d" % (c, r) for c, r, _ in per]
            first = next((f for _, _, f in per if f), "equivalent" if why else "SURVIVED")
            print("  %-26s %18s %18s %18s  %s" % (name, cells[0], cells[1], cells[2], first))
    assert wrong == []
    assert all(why is None or len(why) > 40 for _, _, _, why in MUTANTS)
