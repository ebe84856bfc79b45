"""The prefix forms on the CPU (include/zipc_hip.h at zipc_hip_inflate_prefix_batch): the first dst_cap bytes of a stream.
The host model is tests/prefix_sim/sim_prefix.cpp -- inflate_lane.h's plain step with `prefix` set and inflate_span.h on
an emulated wave, with real stores, the rule of inflate_prefix.h at the cut -- in four forms: the plain step at two
budgets of turns between refills of the input ring, the span decoder with the wave's lanes resumed in ascending and in
descending order.  What is expected comes from the catalogue (tests/inflate_room_cases.py), the planted cases
(tests/inflate_prefix_cases.py) and the oracle, never from the model.  This file holds

  - every item of the catalogue's SIM_FAMILIES and every planted case in all four forms, each room between guard bytes;
  - every CORRUPTED case of tests/golden/inflate_rules.py at four rooms, expected from the oracle;
  - a bit flipped behind the symbol that was cut: nothing changes;
  - zlib_container.h's zlib_close_prefix as a table;
  - PREFIX_MUTANTS, each built into a model of its own and run in a child process;
  - the model as a stand-alone program under the address sanitizer, every room a heap block of exactly dst_cap bytes.

wave_copy_match and the stored-block copy of inflate.hip have no host twin (the model copies a cut match serially):
tests/test_gpu_inflate_prefix.py is their coverage."""
import ctypes as C
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

import inflate_prefix_cases as PC
import inflate_room_cases as RC
import mutation
import util
from host_sim import HERE as HOST_SIM_DIR

sys.path.insert(0, util.GOLDEN)
import inflate_rules  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SIM_CPP = os.path.join(HERE, "prefix_sim", "sim_prefix.cpp")
FORMS = {"plain-512": (0, 512), "plain-7": (0, 7), "span-a": (1, 24), "span-d": (2, 24)}
GUARD, POISON = RC.GUARD, RC.POISON


def bind(so):
    L = C.CDLL(so)
    L.sim_prefix.restype = None
    L.sim_prefix.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_uint32, C.c_int, C.c_int,
                             C.POINTER(C.c_uint64)]
    L.sim_zlib_close_prefix.restype = None
    L.sim_zlib_close_prefix.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_ulonglong, C.POINTER(C.c_ulonglong)]
    return L


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return bind(mutation.gxx(tmp_path_factory.mktemp("prefix_sim") / "libprefix_sim.so", [SIM_CPP], include=[HOST_SIM_DIR],
                             extra=["-Wall", "-Wno-unknown-pragmas"]))


def run(sim, raw, cap, limit, form, off_mod=1, flags_extra=0):
    """the model over one stream, its room at off_mod (mod 16) of a poisoned buffer -> ((status, ended, out_len), the room's
    first out_len bytes, what is wrong with the guards or None)"""
    span, budget = FORMS[form]
    off = GUARD + (off_mod or 16)
    buf = (C.c_ubyte * (off + cap + GUARD))()
    C.memset(buf, POISON, len(buf))
    out = (C.c_uint64 * 3)(0xEE, 0xEE, 0xEE)
    sim.sim_prefix(raw, len(raw), C.byref(buf, off), cap, int(limit is not None), limit or 0, flags_extra, span, budget, out)
    got = np.frombuffer(buf, np.uint8)
    rec = (int(out[0]), int(out[1]), int(out[2]))
    guards = None
    if not (got[:off] == POISON).all():
        guards = "wrote in front of its room"
    elif not (got[off + cap:] == POISON).all():
        guards = "wrote %d bytes behind its room" % (int(np.flatnonzero(got[off + cap:] != POISON).max()) + 1)
    return rec, got[off:off + min(rec[2], cap)].tobytes(), guards


def item_want(it):
    """the catalogue's declaration of an item -> (status, ended, out_len)"""
    n = len(RC.stream_of(it).plain)
    return {0: (0, 1, n), 16: (0, 0, it.R), 2: (2, 0, 0)}[it.want]


def failures(sim, cases, forms):
    """cases: (id, raw, plain or None, cap, limit, want, off_mod) -> [(id, form, what)]"""
    bad = []
    for ident, raw, plain, cap, limit, want, off_mod in cases:
        for form in forms:
            rec, data, guards = run(sim, raw, cap, limit, form, off_mod)
            what = []
            if rec != want:
                what.append("%r, not %r" % (rec, want))
            elif plain is not None and data != plain[:want[2]]:
                what.append("bytes")
            if guards:
                what.append(guards)
            if what:
                bad.append((ident, form, "; ".join(what)))
    return bad


def catalogue_cases(family, every=1):
    return [(RC.item_id(it), RC.stream_of(it).raw, RC.stream_of(it).plain, it.cap, it.limit, item_want(it), it.off_mod)
            for it in RC.items(family)[::every]]


def planted_cases():
    return [(p.name, p.raw, p.plain, p.R, p.limit, p.want, 1 + 4 * (i % 4)) for i, p in enumerate(PC.planted())]


# ---- the catalogue ------------------------------------------------------------------------------------------------

def test_the_catalogue_is_what_it_claims(oracle):
    """the three kinds are all there, no item is left out; every item declared DST_TOO_SMALL is a stream the oracle refuses
    in a room of R bytes for its size -- the item is what it claims"""
    kinds = {0: 0, 16: 0, 2: 0}
    for f in RC.SIM_FAMILIES:
        for it in RC.items(f):
            kinds[it.want] += 1
    assert sum(kinds.values()) == sum(RC.COUNTS[f][1] for f in RC.SIM_FAMILIES) == 7818
    assert kinds == {0: 2550, 16: 2667, 2: 2601}, kinds
    seen = set()
    for f in RC.SIM_FAMILIES:
        for it in RC.items(f):
            if it.want == 16 and (f, it.stream, it.R) not in seen:
                seen.add((f, it.stream, it.R))
                st, _, _ = oracle.inflate(RC.stream_of(it).raw, decompressed_size=it.R)
                assert st == 2, (RC.item_id(it), st)


@pytest.mark.parametrize("family", RC.SIM_FAMILIES)
@pytest.mark.parametrize("form", sorted(FORMS))
def test_catalogue_items_come_out_by_the_rule(sim, form, family):
    """want 0: {0, 1, N} and the plain bytes; want 16: {0, 0, R} and the first R of them; want 2: {2, 0, 0}; both guards"""
    cases = catalogue_cases(family)
    assert len(cases) == RC.COUNTS[family][1]
    bad = failures(sim, cases, [form])
    assert not bad, (len(bad), bad[:5])


def test_planted_cases_come_out_by_the_rule(sim, oracle):
    cases = planted_cases()
    names = {c[0].split("/")[0] for c in cases}
    assert names == {"queued", "run", "start", "tiny", "stored", "fixed", "limit", "far"} and len(cases) == 93
    for p in PC.planted():  # what is planted is what the oracle says of the stream in that room
        st, data, _ = oracle.inflate(p.raw, decompressed_size=p.R if p.limit is None else min(p.R, p.limit))
        if p.plain is None:
            assert st == 1 and p.want == (1, 0, 0), p.name
        elif p.want[1] == 1:
            assert st == 0 and data == p.plain and p.want == (0, 1, len(p.plain)), p.name
        else:
            assert st == 2 and len(p.plain) > p.R, p.name
            if p.want[0] == 0:
                assert p.want == (0, 0, p.R), p.name
    bad = failures(sim, cases, sorted(FORMS))
    assert not bad, (len(bad), bad[:5])
    spans = (C.c_uint64 * 2).in_dll(sim, "sim_prefix_spans")
    assert spans[0] > 0  # (the long stream of `tiny` with 8 bytes of room is at the span decoder's gate, not below it)


# ---- errors ---------------------------------------------------------------------------------------------------------

def _bytes_before_the_error(oracle, stream):
    """the smallest room in which the oracle reaches the stream's error (in a smaller one a symbol overflows first)"""
    verdict = lambda room: oracle.inflate(stream, decompressed_size=room)[0]
    hi = 1
    while verdict(hi) != 1:
        hi *= 2
        assert hi <= 1 << 24
    lo = 0
    if verdict(0) == 1:
        return 0
    while hi - lo > 1:  # verdict(lo) == 2, verdict(hi) == 1
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if verdict(mid) == 1 else (mid, hi)
    return hi


@pytest.mark.parametrize("form", sorted(FORMS))
def test_corrupted_streams_at_four_rooms(sim, oracle, form):
    """every CORRUPTED case of tests/golden/inflate_rules.py (all 304 of wrapped_cases(): the table's own and those with
    valid blocks around them, 73 of them inside streams of 600 KB and more) with dst_cap 0, 1, half the bytes it produces before its
    error, and those bytes + 1: where the oracle says size exceeded in that room the stream is cut at dst_cap, where it
    says corrupted the record is {1, 0, 0}"""
    cases = {n: c for n, c in inflate_rules.wrapped_cases().items() if c.status == 1}
    assert len(cases) == 304
    n_cut = n_err = 0
    for name, c in sorted(cases.items()):
        p = _bytes_before_the_error(oracle, c.stream)
        for cap in sorted({0, 1, p // 2, p + 1}):
            st, _, _ = oracle.inflate(c.stream, decompressed_size=cap)
            assert st in (1, 2), (name, cap, st)
            want = (0, 0, cap) if st == 2 else (1, 0, 0)
            rec, data, guards = run(sim, c.stream, cap, None, form)
            assert rec == want and guards is None, (form, name, cap, rec, want, guards)
            if c.plain is not None and st == 2:
                assert data == c.plain[:cap], (form, name, cap)
            n_cut += st == 2
            n_err += st == 1
    assert n_cut > 300 and n_err > 300, (n_cut, n_err)


def test_a_flag_bit_and_a_length_out_of_range_are_the_streams_own(sim):
    p = PC.by_name("fixed/lazy/R=100")
    for form in FORMS:
        assert run(sim, p.raw, p.R, None, form, flags_extra=2)[0] == (18, 0, 0)
        assert run(sim, p.raw, p.R, None, form, flags_extra=1 << 31)[0] == (18, 0, 0)


FLIP_ITEMS = 10


def test_nothing_behind_the_cut_is_read_or_judged(sim):
    """ten streams of the catalogue (one fixed block each) in a room that cuts them, with the first bit behind the symbol
    that was cut flipped, and with every bit from there to the stream's end: the record and the bytes stay"""
    its = [it for it in RC.items("lane") if it.want == 16][::37][:FLIP_ITEMS]
    assert len(its) == FLIP_ITEMS
    kinds = set()
    for it in its:
        s = RC.stream_of(it)
        at, n, end = next(e for e in PC.fixed_symbol_ends(s) if e[0] + e[1] > it.R)  # the first symbol that does not fit
        kinds.add(n > 1)
        assert end < 8 * len(s.raw)
        one = bytearray(s.raw)
        one[end >> 3] ^= 1 << (end & 7)
        rest = bytearray(s.raw)
        rest[end >> 3] ^= (0xFF << (end & 7)) & 0xFF
        for k in range((end >> 3) + 1, len(rest)):
            rest[k] ^= 0xFF
        for form in FORMS:
            for raw in (s.raw, bytes(one), bytes(rest)):
                rec, data, guards = run(sim, raw, it.cap, it.limit, form, it.off_mod)
                assert rec == (0, 0, it.R) and data == s.plain[:it.R] and guards is None, (RC.item_id(it), form, rec, guards)
    assert kinds == {False, True}  # (literals and matches were cut)


# ---- the zlib close rule --------------------------------------------------------------------------------------------

def test_zlib_close_prefix_table(sim):
    """pre-status x {ended with the Adler-32 the stream says, ended with another, cut, an inner error}"""
    def close(pre, expect, adler, inner):
        out = (C.c_ulonglong * 3)()
        sim.sim_zlib_close_prefix(pre, expect, adler, inner[0], inner[1], inner[2], out)
        return tuple(int(x) for x in out)

    A, B = 0x11E60398, 0x00620062
    inners = {"ended_equal": ((0, 1, 500), A), "ended_differs": ((0, 1, 500), B), "cut": ((0, 0, 64), 0), "cut_other_adler": ((0, 0, 64), B),
              "corrupted": ((1, 0, 0), 0), "size_exceeded": ((2, 0, 0), 0), "invalid_arg": ((18, 0, 0), 0), "ended_empty": ((0, 1, 0), 1)}
    for pre in (0, 1, 3, 4, 5, 18):
        for name, (inner, adler) in inners.items():
            got = close(pre, A if name != "ended_empty" else 1, adler, inner)
            if pre != 0:
                want = (pre, 0, 0)  # the container's own verdict, whatever the body's
            elif name == "ended_differs":
                want = (6, 0, 0)    # ZIPC_HIP_ERR_CHECKSUM, no bytes, not ended
            else:
                want = inner        # an ended stream whose Adler-32 holds, a cut (nothing compared), the body's error
            assert got == want, (pre, name, got, want)


# ---- the mutants ----------------------------------------------------------------------------------------------------
# (name, file, text, replacement, killer): one-line mutants of inflate_prefix.h, of the lines inflate_lane.h got for the
# prefix forms, and one of the model's services.  killer: (form, the planted case or catalogue item that must fail), or
# ("equivalent", why): nothing may fail of the planted cases in all four forms and every eighth catalogue item in plain-512.
# SOME OF THESE WRITE OR READ OUT OF THEIR ROOM BY DESIGN (one byte; the 64-byte guards hold it inside the child's buffer):
# they are host-model mutants, built with g++ and run in child processes, never built into a GPU library.
_M = "queued/k1_long/R=708"
PREFIX_MUTANTS = [
    ("cut_one_byte_short", "inflate_prefix.h", "return cap_min - out_pos; }", "return cap_min - out_pos - 1u; }", ("plain-512", _M)),
    ("cut_one_byte_long", "inflate_prefix.h", "return cap_min - out_pos; }", "return cap_min - out_pos + 1u; }", ("plain-512", _M)),
    ("cut_although_the_limit_is_inside", "inflate_prefix.h", "return need <= (uint64_t)limit; }", "return true; }",
     ("plain-512", "limit/inside_match/R=100")),
    ("cut_limit_off_by_one", "inflate_prefix.h", "return need <= (uint64_t)limit; }", "return need <= (uint64_t)limit + 1u; }",
     ("plain-512", "limit/at_match_end_minus_1/R=100")),
    ("cut_refused_at_the_limit", "inflate_prefix.h", "return need <= (uint64_t)limit; }", "return need < (uint64_t)limit; }",
     ("plain-512", "limit/at_match_end/R=100")),
    ("cut_before_the_distance_check", "inflate_lane.h", "  if (dist > d.out_pos) { d.fail(ST_CORRUPTED); return SYM_STOP; }  // zd.ml:614",
     "  if (dist > d.out_pos && !(prefix && (uint64_t)d.out_pos + length > d.cap_min)) { d.fail(ST_CORRUPTED); return SYM_STOP; }",
     ("plain-512", "far/R=10")),
    ("ended_on_a_cut", "inflate_prefix.h", "r.status = ST_OK; r.ended = 0; r.out_len = cap_min;", "r.status = ST_OK; r.ended = 1; r.out_len = cap_min;",
     ("plain-512", "start/fixed_literal/R=0")),
    ("cut_out_len_is_out_pos", "inflate_prefix.h", "r.ended = 0; r.out_len = cap_min;", "r.ended = 0; r.out_len = out_pos;",
     ("equivalent", "behind the copy of the part that fits (lane_after_match, lane_after_copy) out_pos has reached cap_min, and a literal is cut "
                    "at out_pos == cap_min: the two are one number wherever a stream is cut")),
    ("not_ended_at_the_end", "inflate_prefix.h", "r.status = ST_OK; r.ended = 1;", "r.status = ST_OK; r.ended = 0;", ("plain-512", "limit/fits/R=400")),
    ("error_keeps_its_bytes", "inflate_prefix.h", "r.status = status; r.ended = 0; r.out_len = 0;", "r.status = status; r.ended = 0; r.out_len = out_pos;",
     ("plain-512", "far/R=40")),
    ("cut_match_from_one_byte_on", "inflate_prefix.h", "return out_pos - dist; }", "return out_pos - dist + 1u; }", ("plain-512", _M)),
    ("stored_cut_from_the_block_header", "inflate_lane.h", "d.req_src = prefix_stored_from(pos);", "d.req_src = prefix_stored_from(pos - 4u);",
     ("plain-512", "stored/behind7/R=8")),
    ("stored_cut_not_taken", "inflate_lane.h", "d.prefix_cut(prefix, (uint64_t)d.out_pos + length)) {  // the block's first req_len bytes",
     "d.prefix_cut(false, (uint64_t)d.out_pos + length)) {  // the block's first req_len bytes", ("plain-512", "stored/behind7/R=8")),
    ("fixed_literal_cut_not_taken", "inflate_lane.h",
     "\n    if (d.out_pos >= d.cap_min && d.prefix_cut(prefix, (uint64_t)d.out_pos + 1))", "\n    if (d.out_pos >= d.cap_min && d.prefix_cut(false, (uint64_t)d.out_pos + 1))",
     ("plain-512", "fixed/lazy/R=10")),
    ("literal_cut_not_taken", "inflate_lane.h",
     "\n      if (d.out_pos >= d.cap_min && d.prefix_cut(prefix, (uint64_t)d.out_pos + 1))", "\n      if (d.out_pos >= d.cap_min && d.prefix_cut(false, (uint64_t)d.out_pos + 1))",
     ("plain-512", "fixed/lazy/R=100")),
    ("cut_match_goes_on_decoding", "inflate_lane.h", "    d.phase = d.req_len ? PH_REQ_MATCH : PH_DONE;\n", "    d.phase = PH_REQ_MATCH;\n",
     ("equivalent", "a request for no bytes copies none, and the wave is done behind the service either way (status ST_PREFIX_CUT)")),
    ("queue_not_filled_before_the_cut", "sim_prefix.cpp", "for (uint32_t k = 0; k < d.q_count; k++) {",
     "for (uint32_t k = 0; d.status != ST_PREFIX_CUT && k < d.q_count; k++) {", ("plain-512", "queued/k1_literal/R=608")),
]

_CHILD = r"""
import json, os, sys
root, so, form, names = sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4].split("|")
sys.path.insert(0, os.path.join(root, "tests")); sys.path.insert(0, root)
import inflate_room_cases as RC
import test_inflate_prefix_rules as T
sim = T.bind(so)
cases = T.planted_cases()
if names == ["all"]:
    bad = T.failures(sim, cases, sorted(T.FORMS)) + T.failures(sim, [c for f in RC.SIM_FAMILIES for c in T.catalogue_cases(f, 8)], ["plain-512"])
else:
    cat = [c for f in {n.split("/")[0] for n in names} & set(RC.SIM_FAMILIES) for c in T.catalogue_cases(f)]
    bad = T.failures(sim, [c for c in cases + cat if c[0] in names], [form])
print(json.dumps(sorted({b[0] for b in bad})))
"""


def mutant_model(m, into):
    """the model over a copy of zipc_amd/csrc (and of itself) with one text changed -> its shared library"""
    name, fname, old, new = m[:4]
    csrc, sim_dir = os.path.join(str(into), "zipc_amd", "csrc"), os.path.join(str(into), "tests", "prefix_sim")
    shutil.copytree(os.path.join(ROOT, "zipc_amd", "csrc"), csrc, ignore=shutil.ignore_patterns("build", "*.hip"))
    os.makedirs(sim_dir)
    shutil.copy(SIM_CPP, sim_dir)
    path = os.path.join(sim_dir if fname == "sim_prefix.cpp" else csrc, fname)
    text = mutation.patched(open(path).read(), old, new, name)
    with open(path, "w") as f:
        f.write(text)
    return mutation.gxx(os.path.join(sim_dir, "libprefix_sim.so"), [os.path.join(sim_dir, "sim_prefix.cpp")], include=[HOST_SIM_DIR],
                        extra=["-Wno-unknown-pragmas"])


def test_prefix_mutants_are_killed(tmp_path, capsys):
    import concurrent.futures

    known = {c[0] for c in planted_cases()} | {RC.item_id(it) for f in RC.SIM_FAMILIES for it in RC.items(f)}
    sos = mutation.build_all(lambda m: mutant_model(m, tmp_path / m[0]), PREFIX_MUTANTS)

    def child(so, form, names):
        rc, failed, err = mutation.run_child(_CHILD, ROOT, so, form, "|".join(names))
        return rc, failed, err

    with concurrent.futures.ThreadPoolExecutor(max_workers=mutation.workers()) as ex:
        jobs = []
        for m, so in zip(PREFIX_MUTANTS, sos):
            killer = m[4]
            if killer[0] == "equivalent":
                jobs.append(ex.submit(child, so, "plain-512", ["all"]))
            else:
                assert killer[1] in known, (m[0], killer[1])
                jobs.append(ex.submit(child, so, killer[0], [killer[1]]))
        rows = []
        for m, job in zip(PREFIX_MUTANTS, jobs):
            rc, failed, err = job.result()
            killer = m[4]
            crashed = rc != 0 or failed is None
            ok = mutation.verdict(killer if killer[0] == "equivalent" else killer[1], failed or [], crashed)
            rows.append((m[0], "equivalent" if killer[0] == "equivalent" else killer[1], len(failed or []), crashed, ok, err[-300:] if crashed else ""))
    with capsys.disabled():
        print("\nprefix mutants in the host model")
        for name, killer, n, crashed, ok, _ in rows:
            print("  %-36s %4d cases fail%s  %s %s" % (name, n, " (child crashed)" if crashed else "", killer, "" if ok else "-- NOT AS EXPECTED"))
    assert all(r[4] and not r[3] for r in rows), [r for r in rows if not r[4] or r[3]]


def test_the_unmutated_model_fails_none_of_the_killers(sim):
    names = {m[4][1] for m in PREFIX_MUTANTS if m[4][0] != "equivalent"}
    cases = [c for c in planted_cases() if c[0] in names]
    assert len(cases) == len(names)
    assert not failures(sim, cases, sorted(FORMS))


# ---- the audit program ----------------------------------------------------------------------------------------------

def test_audit_program_under_the_address_sanitizer(tmp_path):
    """the model as a stand-alone program with its own main, built with -fsanitize=address,undefined and run as a process
    over the planted cases and one in eight of the catalogue's items: every room a heap block of exactly dst_cap bytes, so
    a store behind the cut trips the sanitizer; it aborts on any record or byte that differs from what is expected"""
    cases = planted_cases() + [c for f in RC.SIM_FAMILIES for c in catalogue_cases(f, 8)]
    blob = [struct.pack("<I", len(cases))]
    for _, raw, plain, cap, limit, want, _ in cases:
        with_bytes = plain is not None and want[0] == 0
        blob.append(struct.pack("<8I", len(raw), cap, int(limit is not None), limit or 0, want[0], want[1], want[2], int(with_bytes)))
        blob.append(raw)
        if with_bytes:
            blob.append(plain[:want[2]])
    path = tmp_path / "cases.bin"
    path.write_bytes(b"".join(blob))
    exe = str(tmp_path / "prefix_audit")
    mutation.gxx(exe, [os.path.join(HERE, "prefix_sim", "audit_main.cpp")], shared=False, include=[HOST_SIM_DIR],
                 extra=["-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert b"nothing outside a room" in r.stdout and ("%d cases" % len(cases)).encode() in r.stdout
