"""Inflate's room on the CPU: nothing is written in front of dst_off or behind dst_off + dst_cap, whatever the status
(include/zipc_hip.h at zipc_hip_inflate_batch).  The catalogue is tests/inflate_room_cases.py; this file holds

  - the planted properties of every stream, asserted from the serial reading of its symbols alone, and the oracle's
    verdict on every (stream, room);
  - the host model (tests/host_sim/sim_inflate.cpp: inflate_lane.h and inflate_span.h on an emulated wave) on every
    item of the families it can run, plain, with wide turns, and with spans in both lane orders, its destination at an
    unaligned offset inside a poisoned buffer: status, length, bytes, Adler-32 and both guards;
  - ROOM_MUTANTS below, each built into a host model of its own and run in child processes: every
    one must fail the item it names.

Limits of the CPU side: wave_copy_match, the stored-block copy of inflate.hip and the block path's stores have no host
twin.  Their coverage is tests/test_gpu_inflate_room.py."""
import ctypes as C
import os

import numpy as np
import pytest

import inflate_room_cases as RC
import mutation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# how the host model is run: environment of sim_inflate (read at every call)
MODES = {"plain": {}, "wide": {"SIM_INFLATE_WIDE": "1"}, "span_a": {"SIM_INFLATE_SPAN": "a"}, "span_d": {"SIM_INFLATE_SPAN": "d"}}


def test_the_catalogue():
    its = RC.all_items()
    counts = {f: (len(RC.FAMILIES[f]()), len(RC.items(f))) for f in RC.FAMILIES}
    assert counts == RC.COUNTS, counts
    assert len(its) < 8000
    offs, total, guards = RC.layout([it.cap for it in its], [it.off_mod for it in its])
    assert total < 256 << 20 and total == RC.DST_BYTES, total
    end = 0
    for it, o, (front, back) in zip(its, offs, guards):  # rooms and guards in order, nothing shared
        assert int(o) % 16 == it.off_mod and front.start >= end and front.stop == int(o) == back.start - it.cap
        assert front.stop - front.start == back.stop - back.start == RC.GUARD
        end = back.stop
    # the declarations, alignments and checksums all meet each other; every status is there on both sides of N
    assert {(it.decl, it.off_mod) for it in its} == {(d, m) for d in range(4) for m in RC.OFF_MODS}
    assert {(it.decl, it.crc_op) for it in its} == {(d, c) for d in range(4) for c in RC.CRC_OPS}
    for f in RC.FAMILIES:
        fam = RC.items(f)
        assert {(it.decl, it.want) for it in fam} == {(0, 0), (1, 0), (2, 0), (3, 0), (0, 16), (1, 2), (2, 2), (3, 16)}, f
        for it in fam:
            n = len(RC.stream_of(it).plain)
            limit, cap = RC.DECLS[it.decl][1](n, it.R)
            assert (it.limit, it.cap) == (limit, cap) and min(cap, cap if limit is None else limit) == it.R
            assert it.want == (0 if it.R >= n else (2 if limit is not None and limit <= cap else 16)), RC.item_id(it)
        for si, s in enumerate(RC.FAMILIES[f]()):  # N - 1 (where there is one) and N under every declaration
            n = len(s.plain)
            for room in {max(n - 1, 0), n}:
                assert {it.decl for it in fam if it.stream == si and it.R == room} == {0, 1, 2, 3}, (f, s.name, room)


def test_the_serial_reading_and_the_oracle_agree(oracle):
    """every stream: the plain bytes as written are the oracle's; the symbols' positions add up and every match is the
    copy it says; the oracle takes a room iff it holds the output"""
    for f in RC.FAMILIES:
        for s in RC.FAMILIES[f]():
            st, d, _ = oracle.inflate(s.raw)
            assert st == 0 and d == s.plain, (f, s.name)
            starts, kinds = RC.symbol_table(s)
            assert len(starts) == len(kinds) and (np.diff(starts.astype(np.int64)) >= 0).all()
            pos = 0
            for kind, at, n, dist in s.segs:
                assert at == pos and kind in "LMS", (f, s.name, at, pos)
                if kind == "M":
                    assert 3 <= n <= 258 and 1 <= dist <= at
                    src = s.plain[at - dist:at]
                    assert s.plain[at:at + n] == (src * (n // dist + 1))[:n], (f, s.name, at)
                pos += n
            assert pos == len(s.plain)
        for si, room in sorted({(it.stream, it.R) for it in RC.items(f)}):
            s = RC.FAMILIES[f]()[si]
            st, d, _ = oracle.inflate(s.raw, decompressed_size=room)
            assert (st == 0) == (room >= len(s.plain)) and st in (0, 2), (f, s.name, room, st)


def _rooms_of(family, si):
    return {it.R for it in RC.items(family) if it.stream == si}


def test_planted_properties():
    """what each family is there for, from the serial reading alone"""
    for si, s in enumerate(RC.run_short()):
        ms = RC.matches(s)
        run = ms if s.meta["made_by"] in ("fixed", "dynamic") else ms[:-1]  # (an encoder's last match is what is left)
        assert len(run) >= 64 or s.meta["made_by"] in ("oracle", "zlib")
        assert run and all(d < 64 and d < n and d == s.meta["p"] for _, _, n, d in run), s.name  # period < 64 and < length
    for s in RC.run_long():
        ms = RC.matches(s)
        if s.meta["single"]:
            (_, a1, n1, d1), (_, a2, n2, d2) = ms
            assert d2 >= 64 and a2 - d2 == a1 and n2 == s.meta["L"] and a2 + n2 == len(s.plain)  # reads the match before it
        else:
            assert len(ms) > 66 and all(d >= 64 and n == 258 and d == s.meta["p"] for _, _, n, d in ms), s.name
    for fam in (RC.lane, RC.lane_span):
        seen = set()
        for s in fam():
            (_, at, n, d), = RC.matches(s)
            assert (n, d) == (s.meta["L"], s.meta["dist"]) and len(s.plain) - (at + n) == s.meta["g"], s.name  # ends g bytes before N
            seen.add((n, d, s.meta["g"]))
        assert {g for _, _, g in seen} == set(RC.LANE_G) and {n for n, _, _ in seen} == set(RC.LANE_L)
        assert all(len(s.raw) < 1024 for s in RC.lane()) and all(len(s.raw) > 20 << 10 for s in RC.lane_span())
    assert {s.meta["dist"] for s in RC.lane()} == {1, 7, 8, 9, 64} and {s.meta["dist"] for s in RC.lane_span()} == set(RC.LANE_DIST)
    for s in RC.stored():
        kind, at, n, _ = s.segs[-1]
        assert kind == "S" and n == s.meta["n"] and at == s.meta["behind"] and at + n == len(s.plain), s.name
    assert {(s.meta["n"], s.meta["behind"]) for s in RC.stored()} >= {(n, b) for n in RC.STORED_LEN for b in RC.STORED_BEHIND}
    for si, s in enumerate(RC.span()):
        k, d, n = s.meta["k"], s.meta["d"], len(s.plain)
        assert n == 4096 * k + d
        if 0 < d < 32:  # the last tile has fewer than 32 bytes of room
            assert n in _rooms_of("span", si) and 0 < n - 4096 * k < 32
        assert {x for x in (n // 2, 4096 * k - 1, 4096 * k + 1) if x < n} <= _rooms_of("span", si)
        if s.meta["made_by"] == "letters":
            _, at, ln, dist = RC.matches(s)[-1]
            assert dist > 4096 and at >= n - 40 and at + ln + s.meta["tail"] == n and ln == s.meta["L"], s.name
    assert {s.meta["L"] for s in RC.span() if s.meta["made_by"] == "letters"} == set(RC.SPAN_FAR_L)
    for s in RC.literal_last():
        assert s.segs[-1][0] == "L" and len(s.plain) == s.meta["n"]
    # a room falls strictly inside every match the rooms are set around
    for f in RC.FAMILIES:
        for si, s in enumerate(RC.FAMILIES[f]()):
            rooms = _rooms_of(f, si)
            for b in RC.b_positions(s):
                kind, at, n, _ = next(x for x in s.segs if x[1] == b and x[0] in "MS")
                if kind == "M":
                    assert any(at < r < at + n for r in rooms), (f, s.name, at)


# ---- the host model ------------------------------------------------------------------------------------------------
_SUMS = {}


def _adler(oracle, s):
    if (s.family, s.name) not in _SUMS:
        _SUMS[(s.family, s.name)] = oracle.adler32(s.plain)
    return _SUMS[(s.family, s.name)]


def sim_failures(sim, oracle, its):
    """sim_inflate over the items, each into its room at an unaligned offset of a poisoned buffer -> [(item id, what)]"""
    bad = []
    for it in its:
        s = RC.stream_of(it)
        n = len(s.plain)
        off = RC.GUARD + (it.off_mod or 16)  # (16: what the allocator's alignment leaves of "0 mod 16")
        buf = (C.c_ubyte * (off + it.cap + RC.GUARD))()
        C.memset(buf, RC.POISON, len(buf))
        ol, ck = C.c_uint64(0xEEEEEEEE), C.c_uint32(0xEEEEEEEE)
        crc_op = 2 if it.crc_op == 2 else 0
        st = sim.sim_inflate(s.raw, len(s.raw), C.byref(buf, off), it.cap, int(it.limit is not None), it.limit or 0, crc_op,
                             C.byref(ol), C.byref(ck), 512)
        got = np.frombuffer(buf, np.uint8)
        what = []
        if st != it.want:
            what.append("status %d, not %d" % (st, it.want))
        if ol.value != (n if it.want == 0 else 0):
            what.append("out_len %d" % ol.value)
        if it.want == 0 and st == 0:
            if got[off:off + n].tobytes() != s.plain:
                what.append("bytes")
            if ck.value != (_adler(oracle, s) if crc_op == 2 else 0):
                what.append("checksum")
        if not (got[:off] == RC.POISON).all():
            what.append("wrote in front of its room")
        if not (got[off + it.cap:] == RC.POISON).all():
            what.append("wrote %d bytes behind its room" % (int(np.nonzero(got[off + it.cap:] != RC.POISON)[0].max()) + 1))
        if what:
            bad.append((RC.item_id(it), "; ".join(what)))
    return bad


@pytest.mark.parametrize("family", RC.SIM_FAMILIES)
@pytest.mark.parametrize("mode", sorted(MODES))
def test_host_model_keeps_to_its_room(oracle, monkeypatch, mode, family):
    from host_sim import lib as sim_lib

    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    bad = sim_failures(sim_lib(), oracle, RC.items(family))
    assert not bad, (mode, family, len(bad), bad[:5])


# ---- the mutants ---------------------------------------------------------------------------------------------------
# (name, file, text, replacement, killer): one-line mutants of inflate's ROOM -- where a stream's bytes may go and when it
# is refused for want of room -- killed on the CPU only, by test_room_mutants_are_killed below:
# each is built into a host model of its own and run in a child process over the items of tests/inflate_room_cases.py.
# killer: (the host model's mode, the item that must fail), or ("equivalent", why): no item may fail in any mode.
# THESE MUTANTS WRITE OUT OF THEIR ROOM BY DESIGN (up to 15 bytes; the test's 64-byte guards hold that inside its own
# buffer).  They are never built into a GPU library: the table lies here, where no tool that builds one can read it.
# Each runs in the ONE mode its entry names: the two literal mutants leave out_pos one past cap_min, and the wide turn's
# `cap_min - out_pos` would then wrap (its child would write all over its heap) -- "plain" decodes symbol by symbol.
ROOM_MUTANTS = [
    ("lane_copy_gate_without_its_8", "inflate_lane.h", "(uint64_t)pos + len + 8 <= hard_cap", "(uint64_t)pos + len <= hard_cap",
     ("plain", "lane/L9_d8_g0/R=79/limit R, cap R")),
    ("span_flush_quad_over_the_tail", "inflate_span.h", "if (i + 16u <= tile_len) {", "if (i < tile_len) {", ("span_a", "span/skewed_k5_d17/R=10220/no limit, cap R")),
    ("lane_literal_at_cap_min", "inflate_lane.h", "\n      if (d.out_pos >= d.cap_min) { d.overflow(",
     "\n      if (d.out_pos > d.cap_min) { d.overflow(", ("plain", "literal_last/n20000/R=19999/no limit, cap R")),
    ("lane_fixed_literal_at_cap_min", "inflate_lane.h", "\n    if (d.out_pos >= d.cap_min) { d.overflow(",
     "\n    if (d.out_pos > d.cap_min) { d.overflow(", ("plain", "literal_last/n1/R=0/no limit, cap R")),
    ("lane_match_to_cap_min_refused", "inflate_lane.h",
     "if ((uint64_t)d.out_pos + length > d.cap_min) { d.overflow((uint64_t)d.out_pos + length); return SYM_STOP; }",
     "if ((uint64_t)d.out_pos + length >= d.cap_min) { d.overflow((uint64_t)d.out_pos + length); return SYM_STOP; }",
     ("plain", "lane/L3_d1_g0/R=73/limit R, cap R")),
    ("lane_stored_to_cap_min_refused", "inflate_lane.h",
     "if ((uint64_t)d.out_pos + length > d.cap_min) { d.overflow((uint64_t)d.out_pos + length); return true; }",
     "if ((uint64_t)d.out_pos + length >= d.cap_min) { d.overflow((uint64_t)d.out_pos + length); return true; }",
     ("plain", "stored/len16_behind0/R=16/limit R, cap R")),
    ("cap_min_from_hard_cap_alone", "inflate_lane.h", "d.cap_min = d.limit < d.hard_cap ? d.limit : d.hard_cap;", "d.cap_min = d.hard_cap;",
     ("plain", "lane/L9_d8_g5/R=83/limit R, cap R+40")),
    ("span_far_pass_ungated", "inflate_span.h", "if (out_pos + 32u <= hard_cap && wv::any(has_far != 0u)) {", "if (wv::any(has_far != 0u)) {",
     ("equivalent", "the gate keeps 16-byte LOADS of far sources inside the room; the pass stores into the tile (LDS) only, and what it "
                    "does not fetch the rounds behind it copy: the host model, whose guards are readable, gives the same bytes")),
]

_CHILD = r"""
import ctypes as C, json, os, sys
root, so, families = sys.argv[1], sys.argv[2], sys.argv[3].split(",")
sys.path.insert(0, os.path.join(root, "tests")); sys.path.insert(0, root)
import oracle
import inflate_room_cases as RC
import test_inflate_room_rules as T
from host_sim import _bind
sim = _bind(C.CDLL(so))
print(json.dumps([i for f in families for i, _ in T.sim_failures(sim, oracle, RC.items(f))]))
"""


def test_room_mutants_are_killed(oracle, tmp_path, capsys):
    """ROOM_MUTANTS, each built into a host model of its own and run in child processes (they
    write out of their room by design: the guards hold it inside the child's own buffer), in the mode its entry names:
    the item it names must fail; one marked equivalent must fail none of the host model's items in any mode."""
    import concurrent.futures

    def child(so, mode, families):
        env = {k: v for k, v in os.environ.items() if not k.startswith("SIM_INFLATE")}
        env.update(MODES[mode])
        rc, failed, err = mutation.run_child(_CHILD, ROOT, so, ",".join(families), env=env)
        assert rc == 0, (mode, rc, err[-800:])
        return failed

    known = {RC.item_id(it) for it in RC.all_items()}
    sos = mutation.build_all(lambda m: mutation.host_model(m, tmp_path / m[0]), ROOM_MUTANTS)
    with concurrent.futures.ThreadPoolExecutor(max_workers=mutation.workers()) as ex:
        jobs = []
        for m, so in zip(ROOM_MUTANTS, sos):
            killer = m[4]
            if killer[0] == "equivalent":
                jobs += [(m[0], mode, ex.submit(child, so, mode, RC.SIM_FAMILIES)) for mode in sorted(MODES)]
            else:
                mode, item = killer
                assert item in known, (m[0], item)
                jobs.append((m[0], mode, ex.submit(child, so, mode, [item.split("/")[0]])))
        failed = {}
        for name, mode, job in jobs:
            failed.setdefault(name, []).extend(job.result())
    rows = []
    for m in ROOM_MUTANTS:
        killer, got = m[4], failed[m[0]]
        ok = mutation.verdict(killer if killer[0] == "equivalent" else killer[1], got)
        rows.append((m[0], "equivalent" if killer[0] == "equivalent" else killer[1], len(got), ok))
    with capsys.disabled():
        print("\ninflate room mutants in the host models")
        for name, killer, n, ok in rows:
            print("  %-34s %5d items fail  %s %s" % (name, n, killer, "" if ok else "-- NOT AS EXPECTED"))
    assert all(ok for _, _, _, ok in rows), rows
