"""What the prefix forms (include/zipc_hip.h at zipc_hip_inflate_prefix_batch) are held to, beside the catalogue of
tests/inflate_room_cases.py: streams written symbol by symbol with a room that ends inside, at or in front of one of
them, and what the rule says of each.  numpy, zlib and the oracle's tables only: nothing here calls the code under test.
tests/test_inflate_prefix_rules.py (the host model) and tests/test_gpu_inflate_prefix.py (the kernel) run what this lists.

A Planted case is a stream, a room R = dst_cap, a limit or None, and want = (status, ended, out_len); its bytes are
plain[:out_len] where plain is what the written symbols stand for (inflate_room_cases.Block's out.b, or the assembled
blocks' bytes; None for a stream that has an error in it).

  queued     k = 1, 63, 64, 65 matches that the decoder queues (length 8 <= 16 <= distance, no source in a hole), then
             directly the symbol that is cut: a literal, a match of 258 bytes 16 back (it reads the last two queued
             copies), a match of 258 bytes at distance 1 (it reads the last byte of the last one).  Rooms: at the symbol's
             first byte, one behind, 100 behind.
  run        70 identical (258, 1) matches: the room ends inside repetition 0, 1 and 63
  start      a cut at byte 0 and byte 1 of a stream, by a literal of a fixed and of a dynamic block, a match, a stored block
  tiny       dst_cap 0 .. 8 of a short stream and of one with 20 KiB of input (the span decoder's gate: hard_cap < 8)
  stored     a stored block cut at its first byte, at its last byte, and with no room at all
  fixed      a fixed block cut within its first 48 symbols (decoded without tables) and behind them, by a literal and a match
  limit      a limit inside the symbol that straddles the end of the room: SIZE_EXCEEDED, not a cut; a limit behind it: a cut
  far        a match that reaches in front of the output, with a room that ends at its first byte: CORRUPTED, not a cut
             (the distance is judged before the room is looked at, zd.ml:614)"""
import collections
import functools
import random
import sys

import inflate_room_cases as RC
import util

sys.path.insert(0, util.GOLDEN)
import inflate_rules as R  # noqa: E402

Planted = collections.namedtuple("Planted", "name raw plain R limit want")
OK, CORRUPTED, SIZE_EXCEEDED = 0, 1, 2


def want_of(n, room):
    """the rule for a stream of n bytes without an error in a room of `room` bytes and no limit below its end"""
    return (OK, 1, n) if room >= n else (OK, 0, room)


def _letters(r, n):
    return bytes(r.choice(RC.LETTERS) for _ in range(n))


def _add(out, name, raw, plain, room, limit=None, want=None):
    out.append(Planted("%s/R=%d" % (name, room), raw, plain, room, limit, want or want_of(len(plain), room)))


QUEUED_K = (1, 63, 64, 65)
QUEUED_LEAD = 600  # literals in front: the k-th queued match reads 560 back, in front of the first one's destination


@functools.lru_cache(maxsize=None)
def planted():
    out, r = [], random.Random(71)
    # ---- queued matches, then the cut
    for k in QUEUED_K:
        for kind in ("literal", "long", "dist1"):
            b = RC.Block(R.FULL_DL, RC.LL_ROOM)
            b.lits(_letters(r, QUEUED_LEAD))
            for _ in range(k):
                b.match(8, 560)
            at = len(b.out.b)
            assert at == QUEUED_LEAD + 8 * k
            if kind == "literal":
                b.lits(_letters(r, 30))
            else:
                b.match(258, 16 if kind == "long" else 1)
                b.lits(_letters(r, 5))
            raw, plain = b.done()
            for room in (at,) if kind == "literal" else (at, at + 1, at + 100):
                _add(out, "queued/k%d_%s" % (k, kind), raw, plain, room)
    # ---- a run of identical matches
    b = RC.Block(R.FULL_DL, RC.LL_ROOM)
    b.lits(_letters(r, 5))
    for _ in range(70):
        b.match(258, 1)
    raw, plain = b.done()
    for rep in (0, 1, 63):
        _add(out, "run/rep%d" % rep, raw, plain, 5 + 258 * rep + 100)
    # ---- the first bytes of a stream
    lit = RC._assembled("prefix", "fixed_literals", [R.fixed(RC._lits(r, 40))])
    b = RC.Block(R.FULL_DL, RC.LL_ROOM)
    b.lits(_letters(r, 40))
    dyn_raw, dyn_plain = b.done()
    m = RC._assembled("prefix", "match_at_1", [R.fixed(RC._lits(r, 1) + [("m", 20, 1)])])
    st = RC._assembled("prefix", "stored_first", [R.stored(r.randbytes(100))])
    for room in (0, 1):
        _add(out, "start/fixed_literal", lit.raw, lit.plain, room)
        _add(out, "start/dynamic_literal", dyn_raw, dyn_plain, room)
        _add(out, "start/match", m.raw, m.plain, room)
        _add(out, "start/stored", st.raw, st.plain, room)
    _add(out, "start/match", m.raw, m.plain, 2)
    # ---- rooms below the span decoder's gate
    long_one = RC.lane_span()[7]
    for room in range(9):
        _add(out, "tiny/short", lit.raw, lit.plain, room)
        _add(out, "tiny/lane_span_%s" % long_one.name, long_one.raw, long_one.plain, room)
    # ---- a stored block
    for behind in (0, 7):
        s = RC._assembled("prefix", "stored", ([R.fixed(RC._lits(r, behind))] if behind else []) + [R.stored(r.randbytes(1000)),
                                                                                                  R.fixed(RC._lits(r, 3))])
        for room in sorted({0, behind, behind + 1, behind + 999, behind + 1000}):
            _add(out, "stored/behind%d" % behind, s.raw, s.plain, room)
    # ---- a fixed block: its table-free start and behind it
    f1 = RC._assembled("prefix", "fixed_lazy", [R.fixed(RC._lits(r, 20) + [("m", 30, 10)] + RC._lits(r, 200))])
    for room in (10, 20, 25, 49, 51, 100, 249):
        _add(out, "fixed/lazy", f1.raw, f1.plain, room)
    f2 = RC._assembled("prefix", "fixed_behind", [R.fixed(RC._lits(r, 100) + [("m", 50, 60)] + RC._lits(r, 9))])
    for room in (100, 120, 149, 150, 158, 159):
        _add(out, "fixed/behind", f2.raw, f2.plain, room)
    # ---- a limit inside the straddling symbol, and behind it
    b = RC.Block(R.FULL_DL, RC.LL_ROOM)
    b.lits(_letters(r, 50))
    b.match(258, 20)  # [50, 308)
    b.lits(_letters(r, 4))
    raw, plain = b.done()
    _add(out, "limit/inside_match", raw, plain, 100, limit=200, want=(SIZE_EXCEEDED, 0, 0))
    _add(out, "limit/at_match_end_minus_1", raw, plain, 100, limit=307, want=(SIZE_EXCEEDED, 0, 0))
    _add(out, "limit/at_match_end", raw, plain, 100, limit=308, want=(OK, 0, 100))
    _add(out, "limit/behind_the_stream", raw, plain, 100, limit=400, want=(OK, 0, 100))
    _add(out, "limit/below_the_room", raw, plain, 100, limit=60, want=(SIZE_EXCEEDED, 0, 0))
    _add(out, "limit/fits", raw, plain, 400, limit=312, want=(OK, 1, 312))
    _add(out, "limit/inside_stored", st.raw, st.plain, 10, limit=99, want=(SIZE_EXCEEDED, 0, 0))
    _add(out, "limit/stored_end", st.raw, st.plain, 10, limit=100, want=(OK, 0, 10))
    _add(out, "limit/literal", lit.raw, lit.plain, 10, limit=10, want=(SIZE_EXCEEDED, 0, 0))
    _add(out, "limit/literal_behind", lit.raw, lit.plain, 10, limit=11, want=(OK, 0, 10))
    # ---- a match that reaches in front of the output
    far_raw, far_plain, _, _ = R.assemble([R.fixed(RC._lits(r, 10) + [("m", 8, 11)] + RC._lits(r, 3))])
    assert far_plain is None
    for room in (10, 12, 40):
        out.append(Planted("far/R=%d" % room, far_raw, None, room, None, (CORRUPTED, 0, 0)))
    assert len({p.name for p in out}) == len(out)
    return tuple(out)


def by_name(name):
    return next(p for p in planted() if p.name == name)


# ---- where a symbol of a single fixed block ends, in bits ----------------------------------------------------------

def fixed_symbol_ends(stream):
    """a Stream of ONE fixed block (the lane and literal_last families) -> [(first output byte, output bytes, the bit behind
    the symbol's last)] per symbol, from its serial reading and the fixed codes' lengths"""
    bit, out = 3, []
    for kind, at, n, dist in stream.segs:
        if kind == "L":
            for i in range(n):
                bit += R.FIXED_LL[stream.plain[at + i]]
                out.append((at + i, 1, bit))
        else:
            assert kind == "M"
            ls, _ = R.len_sym(n)
            ds, _ = R.dist_sym(dist)
            bit += R.FIXED_LL[ls] + R.LEXT[ls - 257] + 5 + R.DEXT[ds]
            out.append((at, n, bit))
    assert (bit + 7 + 7) // 8 == len(stream.raw), (stream.name, bit, len(stream.raw))  # (the end of block: 7 bits)
    return out
