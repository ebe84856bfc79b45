"""The mutation table (tests/golden/mutants.py): every one-line mutant of either reading of the reference's encoder
must change a committed vector of tests/golden/deflate_vectors.json.  No GPU."""
import hashlib
import json
import os
import sys

import pytest

import mutation
import util

sys.path.insert(0, util.GOLDEN)
import mutants  # noqa: E402

KINDS = {0: "none", 1: "fixed", 2: "dynamic"}


def _vectors():
    return json.load(open(os.path.join(util.GOLDEN, "deflate_vectors.json")))


def _compact(kinds):
    out = []
    for k in kinds:
        if out and out[-1][0] == k:
            out[-1][1] += 1
        else:
            out.append([k, 1])
    return " ".join(k if n == 1 else "%s*%d" % (k, n) for k, n in out)


def _oracle_changes(O, doc):
    """the committed vectors the loaded oracle does not reproduce: [(name, level or "adler32_whole", field)]"""
    changed = []
    for name, v in doc["vectors"].items():
        data = util.vector_input(name)
        for level, want in v["levels"].items():
            lv = O.LEVELS[level]
            O.huffman_retries(reset=True)
            st, c, crc, blocks = O.deflate_trace(data, level=lv, crc_op=O.CRC_CRC32)
            retries = sum(O.huffman_retries())
            st2, c2, adler = O.deflate(data, level=lv, crc_op=O.CRC_ADLER32)
            got = {"clen": len(c), "sha256": hashlib.sha256(c).hexdigest(), "crc32": crc, "adler32_fused": adler,
                   "blocks": _compact([KINDS[b.kind] for b in blocks]), "huffman_retries": retries}
            diff = [k for k in want if got[k] != want[k]]
            if st != 0 or st2 != 0 or diff:
                changed.append((name, level, diff[0] if diff else "status"))
    for name, want in doc["adler32_whole"].items():
        if O.adler32(util.vector_input(name)) != want:
            changed.append((name, "adler32_whole", "adler32"))
    return changed


@pytest.fixture(scope="module")
def oracle_mutants(tmp_path_factory):
    """every oracle mutant built with gcc (as oracle/Makefile builds the oracle): name -> .so"""
    d = str(tmp_path_factory.mktemp("oracle_mutants"))
    sos = mutation.build_all(lambda m: mutants.build_oracle(m, d), mutants.MUTANTS)
    return {m.name: so for m, so in zip(mutants.MUTANTS, sos)}


def test_the_table_is_whole():
    names = [m.name for m in mutants.MUTANTS]
    assert len(names) == len(set(names)) >= 14
    doc = _vectors()
    for m in mutants.MUTANTS:
        name, level = m.killer
        assert level in doc["vectors"][name]["levels"], m.name
        assert m.c[0] != m.c[1] and m.py[0] != m.py[1], m.name


def test_every_oracle_mutant_changes_a_committed_vector(oracle, oracle_mutants, capsys):
    O = oracle
    doc = _vectors()
    assert _oracle_changes(O, doc) == []  # the real oracle reproduces every vector (so a change below is the mutant's)
    rows, survivors = [], []
    saved_lib, saved_env = O._lib, os.environ.get("ZD_ORACLE_LIB")
    try:
        for m in mutants.MUTANTS:
            os.environ["ZD_ORACLE_LIB"] = oracle_mutants[m.name]
            O._lib = None
            O.lib()
            changed = _oracle_changes(O, doc)
            killed_by_named = any((n, lv) == m.killer for n, lv, _ in changed)
            rows.append((m, changed, killed_by_named))
            if not changed or not killed_by_named:
                survivors.append(m.name)
    finally:
        O._lib = saved_lib
        if saved_env is None:
            os.environ.pop("ZD_ORACLE_LIB", None)
        else:
            os.environ["ZD_ORACLE_LIB"] = saved_env
    with capsys.disabled():
        print("\noracle/zd_oracle.c mutants against %d committed vectors" % sum(len(v["levels"]) for v in doc["vectors"].values()))
        print("  %-26s %-24s %8s  %-30s %s" % ("mutant", "reference", "vectors", "named killer", "first change"))
        for m, changed, named in rows:
            first = "%s %s (%s)" % changed[0] if changed else "-"
            print("  %-26s %-24s %8d  %-30s %s" % (m.name, m.ref, len(changed), "%s %s %s" % (m.killer + ("ok" if named else "MISSED",)), first))
        print("  %d of %d killed, %d surviving" % (len(rows) - len(survivors), len(rows), len(survivors)))
    assert survivors == []


def test_every_second_reading_mutant_changes_its_named_vector(capsys):
    """the same mutants in the second reading, each run on the one vector the table names (it is slow Python)"""
    doc = _vectors()
    plain = mutants.second_reading()
    rows, survivors = [], []
    for m in mutants.MUTANTS:
        name, level = m.killer
        data = util.vector_input(name)
        want = doc["vectors"][name]["levels"][level]
        # the unmutated copy reproduces the vector, so what changes below is the mutant's doing
        assert mutants.second_reading_record(plain, data, level) == want, (m.name, name, level)
        got = mutants.second_reading_record(mutants.second_reading(m), data, level)
        diff = [k for k in want if got[k] != want[k]]
        rows.append((m, diff))
        if not diff:
            survivors.append(m.name)
    with capsys.disabled():
        print("\nzd_second_reading.py mutants against their named vectors")
        for m, diff in rows:
            print("  %-26s %-30s %s" % (m.name, "%s %s" % m.killer, ("killed: " + ", ".join(diff)) if diff else "SURVIVED"))
        print("  %d of %d killed, %d surviving" % (len(rows) - len(survivors), len(rows), len(survivors)))
    assert survivors == []


def test_a_mutant_must_match_once():
    with pytest.raises(AssertionError, match="occurs 0 times"):
        mutants.patched("abc", "x", "y", "t")
    with pytest.raises(AssertionError, match="occurs 2 times"):
        mutants.patched("xx", "x", "y", "t")
    assert mutants.patched("abc", "b", "B", "t") == "aBc"


# ---- the harness itself (tests/mutation.py) ----------------------------------------------------------------------------

def test_patched_names_the_place_the_count_and_the_text():
    assert mutants.patched is mutation.patched  # one rule, one behaviour
    for text, n in (("abc", 0), ("a.x.b.x", 2)):
        with pytest.raises(AssertionError) as e:
            mutation.patched(text, "x", "y", "some_header.h a_mutant")
        assert "some_header.h a_mutant" in str(e.value) and "occurs %d times" % n in str(e.value) and "'x'" in str(e.value)
    assert mutation.patched("a.x.b", "x", "y", "t") == "a.y.b"


def test_verdict_corners():
    eq = ("equivalent", "why no input can tell")
    assert mutation.verdict("case_a", ["case_b", "case_a"]) and not mutation.verdict("case_a", ["case_b"])
    assert not mutation.verdict("case_a", [])  # a survivor
    assert mutation.verdict("case_a", ["case_a"], crashed=True)  # (the killer was seen to change before the child ended)
    assert mutation.verdict(eq, []) and not mutation.verdict(eq, ["case_b"])
    assert not mutation.verdict(eq, [], crashed=True)  # a child that ended early has not shown that nothing changes


def test_a_no_op_mutant_is_reported_as_a_survivor(tmp_path):
    """a line of adler_chain.h replaced by itself and a comment, through the build and the judge of
    tests/test_adler_chain_sim.py: the judge must say that the named killer did not change -- a table can not pass vacuously"""
    import checksum_cases as CC
    import host_sim
    import test_adler_chain_sim as T

    cases = CC.mutation_cases()
    small = sorted(cases, key=lambda n: len(cases[n]["sums"]))[:2]
    # what the unmutated header says of them: the walk's value by replay (asserted of it in test_adler_chain_mutants_are_killed)
    base = {n: [CC.walk(cases[n]["sums"], cases[n]["length"])[0], host_sim.ADLER_REPLAY] for n in small}
    line = "return C >= 0x80000000ull;"
    no_op = ("no_op", "adler_chain.h", line, line + "  /* the same line */", small[0])
    run = T._run_child(T._build_model(no_op, tmp_path), [small[0]])
    assert run[0] == 0 and all(n in run[1] for n in small), run[2]
    assert T.judge(no_op, base, run) == ([], False)  # survived
    assert T.judge(no_op[:4] + (("equivalent", "it is the same line"),), base, run) == ([], True)


# ---- inflate: tests/golden/inflate_rules.py against mutants.INFLATE_MUTANTS ------------------------------------------

def _inflate_changes(O, cases):
    """the rule cases the loaded oracle does not decode as built: [name]"""
    import zlib

    changed = []
    for name, c in cases.items():
        st, d, k = O.inflate(c.stream, decompressed_size=c.limit, crc_op=O.CRC_CRC32)
        if st != c.status or (st == 0 and (d != c.plain or k != zlib.crc32(c.plain))):
            changed.append(name)
    return changed


def test_every_inflate_oracle_mutant_is_killed_by_its_named_rule_case(oracle, tmp_path, capsys):
    """Every one-line mutant of the oracle's decoder (mutants.INFLATE_MUTANTS) changes the result of the rule case the
    table names; an equivalent one (killer None) changes none."""
    import inflate_rules

    O = oracle
    cases = inflate_rules.wrapped_cases()
    assert _inflate_changes(O, cases) == []
    names = [m.name for m in mutants.INFLATE_MUTANTS]
    assert len(names) == len(set(names)) >= 27
    assert all(m.killer is None or m.killer in cases for m in mutants.INFLATE_MUTANTS)
    sos = mutation.build_all(lambda m: mutants.build_oracle_patched(m.name, m.patches, str(tmp_path)), mutants.INFLATE_MUTANTS)
    rows, bad = [], []
    saved_lib, saved_env = O._lib, os.environ.get("ZD_ORACLE_LIB")
    try:
        for m, so in zip(mutants.INFLATE_MUTANTS, sos):
            os.environ["ZD_ORACLE_LIB"] = so
            O._lib = None
            O.lib()
            changed = _inflate_changes(O, cases)
            rows.append((m, changed))
            if (m.killer is None) != (not changed) or (m.killer is not None and m.killer not in changed):
                bad.append(m.name)
    finally:
        O._lib = saved_lib
        if saved_env is None:
            os.environ.pop("ZD_ORACLE_LIB", None)
        else:
            os.environ["ZD_ORACLE_LIB"] = saved_env
    with capsys.disabled():
        print("\noracle/zd_oracle.c decoder mutants against %d rule cases (tests/golden/inflate_rules.py)" % len(cases))
        print("  %-28s %-14s %6s  %-40s %s" % ("mutant", "reference", "cases", "named killer", "first change"))
        for m, changed in rows:
            verdict = "equivalent" if m.killer is None else ("ok" if m.killer in changed else "MISSED")
            print("  %-28s %-14s %6d  %-40s %s" % (m.name, m.ref, len(changed), "%s %s" % (m.killer, verdict),
                                                     changed[0] if changed else "-"))
        n_eq = sum(m.killer is None for m in mutants.INFLATE_MUTANTS)
        print("  %d of %d killed by their named case, %d equivalent, %d wrong" % (len(rows) - n_eq - len(bad), len(rows) - n_eq, n_eq, len(bad)))
    assert bad == []
