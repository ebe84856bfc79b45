"""The hash-chain links' rules on the CPU (no GPU): tests/host_sim/sim_chain.cpp's serial reading of insert_hash
(zipc_deflate.ml:1145-1152) on every case of tests/chain_cases.py -- each case's planted property from the reference's
own links, the reference against sim_chain_serial (whose links sim_deflate turns into the oracle's bytes), the models
of the four chain forms against the reference at every segment size tests/test_gpu_chain_links.py launches, the form a
call of each batch's shape gets -- and a mutation table over the reference and the two models: every one-line mutant
must change a link of a named case."""
import concurrent.futures
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import chain_cases as cc  # noqa: E402
import host_sim  # noqa: E402
import mutation  # noqa: E402

WORKERS = mutation.workers()
# (model, seg_positions) of every row of tests/test_gpu_chain_links.py
FORMS = [("xchg", 0)] + [("xchg", s) for s in cc.XCHG_SEGS] + [("peel", 0)] + [("peel", s) for s in cc.PEEL_SEGS]


@pytest.fixture(scope="module")
def sim():
    return host_sim.lib()


def unique_streams():
    out = {}
    for streams in cc.batches().values():
        for s in streams:
            assert s.name not in out
            out[s.name] = s
    return out


def links_of(L, streams, model, seg_positions=0):
    """name -> links, the streams side by side (the library calls release the interpreter lock)"""
    with concurrent.futures.ThreadPoolExecutor(max_workers=WORKERS) as ex:
        return dict(zip([s.name for s in streams], ex.map(lambda s: host_sim.chain_links(L, s.data, model, seg_positions), streams)))


_REF = {}


@pytest.fixture(scope="module")
def refs(sim):
    if not _REF:
        _REF.update(links_of(sim, list(unique_streams().values()), "reference"))
    return _REF


def hashes(data):
    """Lz77.hash4 (zd.ml:1145-1148) at every position 0 .. len - 4, by numpy"""
    b = np.frombuffer(data, np.uint8).astype(np.uint64)
    v = b[:-3] | (b[1:-2] << np.uint64(8)) | (b[2:-1] << np.uint64(16)) | (b[3:] << np.uint64(24))
    return ((v * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(17)


def test_the_batches_are_the_ones_the_seams_need(sim):
    B = cc.batches()
    edges, longs = B["edges"], B["long"]
    lengths = {len(s) for s in edges}
    assert set(cc.TINY) <= lengths and {d + 4 for d in cc.EDGE_LAST} <= lengths and 50 <= len(edges) <= 70
    assert sum(40000 <= len(s) <= 70 * 1024 for s in edges) >= 3
    for kind in cc.KINDS:  # every content at the round's edge and at the window's
        assert {len(s) - 4 for s in edges if s.name.startswith(kind)} & {1023, 1024, 1025}, kind
        assert {len(s) - 4 for s in edges if s.name.startswith(kind)} & {16383, 16384, 16385, 32767, 32768, 32769}, kind
    assert 6 <= len(longs) <= 8 and all(200000 <= len(s) <= 330 * 1024 for s in longs)
    last = {len(s) - 4 for s in longs}
    for unit in (98304, 32768):  # a last segment of no position, of one, of two
        for d in (-1, 0, 1):
            assert any((x - d) % unit == 0 for x in last), (unit, d)
    assert max(sum(len(s) for s in b) for b in B.values()) <= 2 << 20  # the largest call: about 2 MB
    # the planted gaps, and the earlier member of a pair on a warm-up's first position and one before it
    gaps = {b - a for ps in cc.WINDOW_PLANTS.values() for a, b in zip(ps, ps[1:])}
    assert set(cc.WINDOW_GAPS) <= gaps
    pairs = {(a, b) for ps in cc.WINDOW_PLANTS.values() for a, b in zip(ps, ps[1:])}
    for seg in cc.XCHG_SEGS + cc.PEEL_SEGS:
        assert any(b % seg == 0 and a == b - cc.WINDOW for a, b in pairs), seg
    for seg in (cc.XCHG_SEGS[0], cc.PEEL_SEGS[0]):
        assert any(b % seg == 0 and a == b - cc.WINDOW - 1 for a, b in pairs), seg
    for w in cc.WINDOW_PLANTS:
        assert sim.sim_chain_ref_hash4(cc._word(w)) == int(hashes(cc._word(w))[0])
    assert len({sim.sim_chain_ref_hash4(cc._word(w)) for w in cc.WINDOW_PLANTS}) == len(cc.WINDOW_PLANTS)


def check_property(s, pr, links):
    """None, or what is wrong"""
    kind = pr[0]
    if kind == "link":
        if links[pr[1]] != pr[2]:
            return "position %d: link %d, planted %d" % (pr[1], links[pr[1]], pr[2])
    elif kind == "span":
        lo, hi = pr[1], max(pr[2], pr[1])
        bad = np.nonzero(links[lo:hi] != pr[3])[0]
        if bad.size:
            return "position %d: link %d, planted %d over [%d, %d)" % (lo + bad[0], links[lo + bad[0]], pr[3], lo, hi)
    elif kind == "only":
        h = hashes(s.data)
        at = tuple(int(p) for p in np.nonzero(h == h[pr[2][0]])[0])
        if at != pr[2] or any(s.data[p:p + 4] != pr[1] for p in pr[2]):
            return "the hash of %s is at %r, planted at %r" % (pr[1].hex(), at[:12], pr[2])
    elif kind == "share":
        share = float((links[pr[1]:pr[2]] != 0).mean())
        if not pr[3] <= share <= pr[4]:
            return "%.4f of [%d, %d) have a link, planted %.3f .. %.3f" % (share, pr[1], pr[2], pr[3], pr[4])
    elif kind == "mean":
        mean = float(links[pr[1]:pr[2]].mean())
        if not pr[3] <= mean <= pr[4]:
            return "the mean link of [%d, %d) is %.1f, planted %.1f .. %.1f" % (pr[1], pr[2], mean, pr[3], pr[4])
    else:
        return "unknown property %r" % (kind,)
    return None


def test_every_case_shows_what_it_was_planted_for(refs):
    wrong, n_props = [], 0
    for s in unique_streams().values():
        assert s.what
        links = refs[s.name]
        n = max(len(s) - 3, 0)
        assert (links[:n] <= cc.WINDOW).all() and (links[n:] == host_sim.LINK_POISON).all(), s.name  # every position written, nothing behind
        for pr in s.props:
            n_props += 1
            msg = check_property(s, pr, links)
            if msg:
                wrong.append("%s %s: %s" % (s.name, pr[0], msg))
    assert n_props > 80
    assert wrong == [], "\n".join(wrong[:20])


def test_the_planted_gaps_read_as_the_window_says(refs):
    """named: 32767 and 32768 found, 32769 and everything beyond not -- 65541, 81920 and 131075 would read 5, 16384 and 3 in a
    table of 16-bit positions -- and the links on the segments' first positions"""
    links = refs["window"]
    ps = cc.WINDOW_PLANTS[3]
    assert [int(links[p]) for p in ps] == [0, 32767, 32768, 0, 0, 0, 0]
    assert [int(links[p]) for p in cc.WINDOW_PLANTS[4]] == [0, 0, 0, 0]
    assert [int(links[p]) for p in cc.WINDOW_PLANTS[0]] == [0, 32768, 32768, 32768, 32768]
    assert [int(links[p]) for p in cc.WINDOW_PLANTS[1]] == [0, 0] and [int(links[p]) for p in cc.WINDOW_PLANTS[2]] == [0, 32767]
    for period, edge in cc.PERIODS.items():
        assert int(refs["periods"][edge]) == period == int(refs["periods"][edge - 1])
    for lo, hi, _ in cc.RUNS:
        for edge in range((lo + cc.ROUND) // cc.ROUND * cc.ROUND, hi - 3, cc.ROUND):
            assert int(refs["runs"][edge]) == 1


def test_the_reference_equals_the_serial_chain_everywhere(sim, refs):
    """sim_deflate proves that sim_chain_serial's links (through lz_match_position) give the oracle's bytes; the plain
    reference, with its own hash, is anchored by being equal to it at every position of every case"""
    streams = list(unique_streams().values())
    serial = links_of(sim, streams, "serial")
    for s in streams:
        bad = np.nonzero(refs[s.name] != serial[s.name])[0]
        assert bad.size == 0, "%s: %d positions differ, the first at %d: reference %d, sim_chain_serial %d" % (
            s.name, bad.size, bad[0], refs[s.name][bad[0]], serial[s.name][bad[0]])


@pytest.mark.parametrize("model,seg", FORMS, ids=["%s-%d" % f for f in FORMS])
def test_the_models_equal_the_reference(sim, refs, model, seg):
    streams = list(unique_streams().values())
    got = links_of(sim, streams, model, seg)
    for s in streams:
        bad = np.nonzero(refs[s.name] != got[s.name])[0]
        assert bad.size == 0, "%s %s: %d slots differ, the first at %d (%s): reference %d, model %d" % (
            s.name, s.what, bad.size, bad[0], cc.where(int(bad[0]), 0 if model == "xchg" else 2, seg), refs[s.name][bad[0]], got[s.name][bad[0]])


def predicted_form(L, streams, xchg_ok):
    """(chain, seg_positions) a deflate call of this batch's shape gets: forms.h through sim_forms.cpp"""
    n, longest, total = len(streams), max(len(s) for s in streams), sum(len(s) for s in streams)
    f, s = host_sim.deflate_forms(L, n, longest, total, level=2, xchg_ok=xchg_ok, slices_override=1)
    chain = int(s["chain"])
    seg = int(f["xseg"]) if chain == host_sim.CHAIN_XCHG_SEGMENTS else int(f["chain_seg"]) if chain == host_sim.CHAIN_PEEL_SEGMENTS else 0
    return chain, seg


def test_which_form_each_batch_gets_and_which_segment_sizes_exist(sim):
    B = cc.batches()
    assert predicted_form(sim, B["edges"], 1) == (host_sim.CHAIN_XCHG, 0)
    assert predicted_form(sim, B["long"], 1) == (host_sim.CHAIN_XCHG_SEGMENTS, 98304)
    assert predicted_form(sim, B["edges"], 0) == (host_sim.CHAIN_PEEL_SEGMENTS, 32768)
    assert predicted_form(sim, B["long"], 0) == (host_sim.CHAIN_PEEL_SEGMENTS, 32768)
    for seg in (0, 1, 1024, 16384, 32767, 32768, 49152, 65536, 98304, 131072, 196608, 262144, 393216, 96 << 20):
        assert sim.sim_chain_seg_known(host_sim.CHAIN_PEEL_SEGMENTS, seg) == (seg in cc.PEEL_SEGS), seg
        assert sim.sim_chain_seg_known(host_sim.CHAIN_XCHG_SEGMENTS, seg) == (seg in (98304, 196608, 393216, 96 << 20)), seg
        assert not sim.sim_chain_seg_known(host_sim.CHAIN_XCHG, seg) and not sim.sim_chain_seg_known(host_sim.CHAIN_PEEL, seg)
    assert all(sim.sim_chain_seg_known(host_sim.CHAIN_XCHG_SEGMENTS, s) for s in cc.XCHG_SEGS)


# ---- the mutation table ----------------------------------------------------------------------------------------------
# (name, what it mutates, the line of sim_chain.cpp as it stands, the mutant's, and for an equivalent mutant why no link can change)
MUTANTS = [
    ("window <", "reference", "p - q <= 32768) link", "p - q < 32768) link", None),
    ("window <= 32769", "reference", "p - q <= 32768) link", "p - q <= 32769) link", None),
    ("last position len - 5", "reference", "  const uint32_t last = len - 4;  //", "  if (len < 5) return;\n  const uint32_t last = len - 5;  //", None),
    ("hash over three bytes", "reference", "  v |= (uint32_t)s[i + 3] << 24;\n", "", None),
    ("head kept where the link is 0", "reference", "    head[h] = p;  // insert_hash", "    if (link) head[h] = p;  // insert_hash", None),
    ("head kept where the last one left the window", "reference", "    head[h] = p;  // insert_hash",
     "    if (link || q == CHAIN_REF_NO_POS) head[h] = p;  // insert_hash", None),
    ("no sweep", "peel", "    if ((B % SWEEP_PERIOD) == 0) {", "    if (B == B_first) {", None),
    ("sweep keeps d < 32768", "peel", "keep = d >= 1 && d <= 32768; }", "keep = d >= 1 && d < 32768; }", None),
    ("NEAR - 1 in the successor test", "peel", "for (int k = 1; k <= NEAR; k++) has_succ", "for (int k = 1; k <= NEAR - 1; k++) has_succ",
     "a position with an equal hash exactly 8 to its right then goes on writing and peeling like any member of its group: it "
     "reads its bucket back every turn until the round ends, so it sees the later member land and leaves head to the group's last, "
     "and a reader that sees its stores as well still takes the nearest earlier member; links come from near_pred and pred_local, "
     "which the successor test does not touch -- the short-cut saves turns, never links"),
    ("NEAR - 1 in the predecessor test", "peel", "for (int k = NEAR; k >= 1; k--) if (hs", "for (int k = NEAR - 1; k >= 1; k--) if (hs", None),
    ("hs pads 0", "peel", "hs(T + 2 * NEAR, 0xFFFF);", "hs(T + 2 * NEAR, 0);", None),
    ("warm-up from own_lo - 16384", "peel", "lo > 32768 ? lo - 32768 : 0, lo, hi);", "lo > 16384 ? lo - 16384 : 0, lo, hi);", None),
    ("warm-up from own_lo - 32767", "xchg", "own_lo > 32768 ? own_lo - 32768 : 0;", "own_lo > 32767 ? own_lo - 32767 : 0;", None),
    ("link test <", "xchg", "(d <= 32768 ? d : 0u);", "(d < 32768 ? d : 0u);", None),
]
MUTANT_FORMS = {"reference": [("reference", 0)], "peel": [f for f in FORMS if f[0] == "peel"], "xchg": [f for f in FORMS if f[0] == "xchg"]}


def build_mutant(index, out_dir):
    name, _, old, new, _ = MUTANTS[index]
    src = open(os.path.join(HERE, "host_sim", "sim_chain.cpp")).read()
    path = os.path.join(out_dir, "m_%d" % index)
    with open(path + ".cpp", "w") as f:
        f.write(mutation.patched(src, old, new, "sim_chain.cpp " + name))
    so = mutation.gxx(path + ".so", [path + ".cpp"], include=[os.path.join(HERE, "host_sim")], extra=["-Wall"])
    return host_sim.bind_chain(C.CDLL(so))


def test_every_mutant_changes_a_link_of_a_named_case(refs, tmp_path, capsys):
    streams = list(unique_streams().values())
    libs = mutation.build_all(lambda i: build_mutant(i, str(tmp_path)), range(len(MUTANTS)))
    rows, wrong = [], []
    for (name, what, _, _, why), ML in zip(MUTANTS, libs):
        changed, cases, first = 0, 0, None
        for model, seg in MUTANT_FORMS[what]:
            got = links_of(ML, streams, model, seg)
            for s in streams:
                bad = np.nonzero(refs[s.name] != got[s.name])[0]
                if bad.size:
                    changed += int(bad.size)
                    cases += 1
                    if first is None:
                        p = int(bad[0])
                        first = "%s@%d%s: %d for %d" % (s.name, p, " by %d" % seg if seg else "", got[s.name][p], refs[s.name][p])
        rows.append((name, what, changed, cases, first or ("equivalent" if why else "SURVIVED")))
        if (why is None) != (changed > 0):
            wrong.append(name)
    with capsys.disabled():
        print("\nsim_chain.cpp mutants over %d streams: slots changed, over all the forms of the mutated code" % len(streams))
        print("  %-46s %-10s %10s %6s  %s" % ("mutant", "of", "slots", "cases", "first change"))
        for r in rows:
            print("  %-46s %-10s %10d %6d  %s" % r)
    assert wrong == []
    assert all(why is None or len(why) > 40 for _, _, _, _, why in MUTANTS)
