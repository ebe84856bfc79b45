"""Deflate's destination-capacity rule (tests/deflate_fit.py) on the CPU: the properties of its case table, a mutation table
of the rule itself, and the host simulator held to it in both of its forms.  No GPU."""
import collections
import ctypes as C
import functools

import numpy as np

import deflate_fit as F
import util


# ---- the table's properties, by the oracle alone
def _rows():
    """(name, level, clen, blocks, needs) of every compressing (case, level)"""
    for name, data in F.inputs().items():
        for level in F.levels_of(name):
            out, blocks = F.trace(data, level)
            yield name, level, len(out), blocks, F.needs(blocks)


def test_trace_bit_positions_chain_and_end_at_clen(oracle):
    """bit_start / bit_end: a block starts where the one before ended, the first at 0, and the last one's end rounds up to
    the output's length -- at `None too"""
    for name in list(F.inputs()) + list(F.stored_inputs()):
        for level in (F.levels_of(name) if name in F.inputs() else (0,)):
            out, blocks = F.trace(F.data_of(name), level)
            assert blocks[0].bit_start == 0, (name, level)
            for a, b in zip(blocks, blocks[1:]):
                assert a.bit_end == b.bit_start, (name, level)
            assert (blocks[-1].bit_end + 7) // 8 == len(out), (name, level)
            for b in blocks:  # a fixed block's estimate is its size; a stored block's is its size, or 8 more (Q3)
                if level and b.kind == F.FIXED:
                    assert b.flen == b.bit_end - b.bit_start, (name, level)
                if level and b.kind == F.STORED:
                    assert b.nlen - (b.bit_end - b.bit_start) == (8 if b.bit_start % 8 == 5 else 0), (name, level)


def test_min_cap_is_within_the_bound(oracle):
    """zipc_hip_deflate_bound always fits: on the table, and on every input of util.deflate_cases() at every level"""
    seen = 0
    for name, data in list(F.inputs().items()) + list(util.deflate_cases().items()):
        for level in (F.levels_of(name) if name in F.inputs() else (1, 2, 3)):
            out, blocks = F.trace(data, level)
            assert len(out) <= F.min_cap(blocks) <= oracle.deflate_bound(len(data)), (name, level)
            assert F.expect(data, level, oracle.deflate_bound(len(data)))[:2] == (0, out), (name, level)
            seen += 1
    for name, data in F.stored_inputs().items():
        assert F.stored_need(len(data)) == len(F.trace(data, 0)[0]) <= oracle.deflate_bound(len(data)), name
    assert seen > 100


def test_the_first_blocks_dynamic_estimate_is_its_size(oracle):
    """the code-length counts hold one block's symbols at the first block: only later blocks run high (Q1)"""
    n = 0
    for name, level, clen, blocks, needs in _rows():
        if blocks[0].kind == F.DYNAMIC:
            assert blocks[0].dlen == blocks[0].bit_end - blocks[0].bit_start, (name, level)
            n += 1
        for b in blocks[1:]:
            if b.kind == F.DYNAMIC:
                assert b.dlen > b.bit_end - b.bit_start, (name, level)
    assert n >= 10


def test_the_table_holds_a_case_of_every_clause(oracle):
    rows = {(name, level): (clen, blocks, needs) for name, level, clen, blocks, needs in _rows()}
    # a capacity that holds the output and is refused
    assert any(max(needs) > clen for clen, blocks, needs in rows.values())
    clen, blocks, needs = rows["zeros70k", 2]
    assert (clen, max(needs)) == (97, 101)
    # a block in the middle decides, with need > clen
    clen, blocks, needs = rows["zeros196k", 2]
    assert (clen, needs) == (233, [77, 158, 238, 233])
    assert any(max(needs) > clen and needs.index(max(needs)) not in (0, len(needs) - 1) for clen, blocks, needs in rows.values())
    # a high estimate that does not bind: the stored block behind it does
    for level in (1, 2, 3):
        clen, blocks, needs = rows["far_match", level]
        assert [b.kind for b in blocks] == [F.STORED, F.DYNAMIC, F.STORED]
        assert blocks[1].dlen - (blocks[1].bit_end - blocks[1].bit_start) == 259 and max(needs) == needs[2] == clen
    # a stored block that starts at bit 5 of a byte: its estimate is 8 bits high (Q3), its real size decides
    clen, blocks, needs = rows["tie_nf_b2_loss8", 1]
    b = blocks[-1]
    assert (b.kind, b.bit_start % 8, b.nlen, b.bit_end - b.bit_start) == (F.STORED, 5, 307, 299) and max(needs) == clen
    # a last block that is fixed, behind dynamic ones
    clen, blocks, needs = rows["text200k", 2]
    assert [b.kind for b in blocks] == [F.DYNAMIC] * 3 + [F.FIXED]
    # every kind as the only block
    assert {rows[n, 2][1][0].kind for n in ("fox", "text5000", "rand3000")} == {F.FIXED, F.DYNAMIC, F.STORED}


def test_the_caps_of_the_table(oracle):
    """every (case, level) is run on both sides of every edge the rule has"""
    for name, level, clen, blocks, needs in _rows():
        caps = F.caps_of(F.inputs()[name], level)
        mc = max(needs)
        front = blocks[needs.index(mc)].bit_start // 8
        want = {0, 1, clen - 1, clen, mc - 1, mc, mc + 1, oracle.deflate_bound(len(F.inputs()[name])), front}
        assert set(caps) >= want and (front == 0 or front - 1 in caps), (name, level)
        assert [F.fits(F.inputs()[name], level, c) for c in (mc - 1, mc)] == [False, True]
    assert len(F.table()) == len(set(F.table())) > 250


# ---- a mutation table of the rule: each entry is `needs` (or the comparison, or `None's block count) in an "obvious"
# other reading, with the (case, level, cap) of the table at which its verdict differs from the rule's.  A mutant that no
# row of the table tells from the rule is a clause the table does not pin.  killer None: an equivalent mutant, which
# must change no verdict of the table.
RuleMutant = collections.namedtuple("RuleMutant", "name what parts killer")


def _real_sizes(blocks):
    return [(b.bit_start + b.bit_end - b.bit_start + 7) // 8 for b in blocks]


def _last_block_only(blocks):
    return [0] * (len(blocks) - 1) + F.needs(blocks)[-1:]


def _starts_from_estimates(blocks):
    out, at = [], 0
    for b in blocks:
        est = b.dlen if b.kind == F.DYNAMIC else b.bit_end - b.bit_start
        out.append((at + est + 7) // 8)
        at += est
    return out


def _floor(blocks):
    return [(b.bit_start + (b.dlen if b.kind == F.DYNAMIC else b.bit_end - b.bit_start)) // 8 for b in blocks]


def _stored_by_nlen(blocks):
    return [(b.bit_start + (b.dlen if b.kind == F.DYNAMIC else b.nlen if b.kind == F.STORED else b.bit_end - b.bit_start) + 7) // 8
            for b in blocks]


def _fixed_by_flen(blocks):
    return [(b.bit_start + (b.dlen if b.kind == F.DYNAMIC else b.flen if b.kind == F.FIXED else b.bit_end - b.bit_start) + 7) // 8
            for b in blocks]


def _flush_tested_too(blocks):
    n = F.needs(blocks)
    return n[:-1] + [max(n[-1], (blocks[-1].bit_end + 7) // 8)]


RULE_MUTANTS = [
    RuleMutant("dynamic_real_size", "a dynamic block tested with its real size, not with dlen", dict(needs=_real_sizes),
               ("zeros70k", 2, 100)),
    RuleMutant("last_block_only", "only the last block tested", dict(needs=_last_block_only), ("zeros196k", 2, 237)),
    RuleMutant("starts_from_estimates", "a block's start is the sum of the estimates in front of it, not of the real sizes",
               dict(needs=_starts_from_estimates), ("far_match", 1, 149953)),
    RuleMutant("floor", "bits rounded down to bytes", dict(needs=_floor), ("empty", 1, 1)),
    RuleMutant("ge", "a block is refused when its need is >= dst_cap", dict(unfit=lambda need, cap: need >= cap), ("fox", 1, 45)),
    RuleMutant("stored_by_nlen", "a stored block tested with the reference's estimate nlen (8 high at bit 5, Q3)",
               dict(needs=_stored_by_nlen), ("tie_nf_b2_loss8", 1, 35795)),
    RuleMutant("none_blocks_div_plus_1", "`None: len // 65534 + 1 blocks", dict(nblocks=lambda n: n // F.MAX_BLOCK_SRC_LEN + 1),
               ("none65534", 0, 65539)),
    RuleMutant("none_empty_is_free", "`None: no block, so no 5 bytes, for the empty input",
               dict(nblocks=lambda n: (n + F.MAX_BLOCK_SRC_LEN - 1) // F.MAX_BLOCK_SRC_LEN), ("none0", 0, 4)),
    # equivalent: a fixed block's estimate counts exactly the bits written (its code is known before the block is),
    # test_trace_bit_positions_chain_and_end_at_clen requires flen == bit_end - bit_start of every fixed block
    RuleMutant("fixed_by_flen", "a fixed block tested with flen", dict(needs=_fixed_by_flen), None),
    # equivalent: the last block's need is at least ceil(bit_end / 8), the byte the flush adds (dlen >= the real size)
    RuleMutant("flush_tested_too", "the final flush's byte tested by itself (deflate_emit_wave<0> does)", dict(needs=_flush_tested_too), None),
]


def _verdict(name, level, cap, needs=F.needs, unfit=F.unfit, nblocks=F.stored_nblocks):
    data = F.data_of(name)
    if level == 0:
        return not unfit(F.stored_need(len(data), nblocks), cap)
    return F.first_unfit(F.trace(data, level)[1], cap, needs, unfit) is None


def test_rule_mutants_are_killed_by_their_named_rows(oracle):
    table = F.table()
    lines = []
    for m in RULE_MUTANTS:
        differs = [row for row in table if _verdict(*row, **m.parts) != _verdict(*row)]
        if m.killer is None:
            assert not differs, "%s is listed as equivalent, and %r tells it from the rule" % (m.name, differs[0])
            lines.append("%-24s equivalent (changes none of %d rows)  %s" % (m.name, len(table), m.what))
            continue
        assert m.killer in table, "%s: its killer %r is not a row of the table" % (m.name, m.killer)
        assert _verdict(*m.killer) == F.fits(F.data_of(m.killer[0]), *m.killer[1:])
        assert m.killer in differs, "%s survives its killer %r (it changes %d rows)" % (m.name, m.killer, len(differs))
        lines.append("%-24s killed by %-34r rule %-7s mutant %-7s (%3d rows differ)  %s" % (
            m.name, m.killer, "fits" if _verdict(*m.killer) else "refuses",
            "fits" if _verdict(*m.killer, **m.parts) else "refuses", len(differs), m.what))
    print("\n".join(["deflate's capacity rule: %d mutants over %d rows" % (len(RULE_MUTANTS), len(table))] + lines))
    assert len({m.name for m in RULE_MUTANTS}) == len(RULE_MUTANTS) >= 9


# ---- the host simulator applies the rule, in both of its forms
def _sim_deflate_into(sim, data, level, cap, fill):
    dst = C.create_string_buffer(bytes([fill]) * (cap + 64), cap + 64)
    ol, ad, kinds, nk = C.c_uint64(99), C.c_uint32(99), (C.c_int * 64)(), C.c_int()
    st = sim.sim_deflate(data, len(data), level, dst, cap, C.byref(ol), C.byref(ad), kinds, 64, C.byref(nk))
    return st, ol.value, ad.value, dst.raw


@functools.lru_cache(maxsize=None)
def _adler(data, level):
    """the reference's Adler-32 of a deflate: one update per block (Q7)"""
    import oracle

    return oracle.deflate(data, level=level, crc_op=oracle.CRC_ADLER32)[2]


def _hold_sim_to_the_table(sim, oracle, by_blocks):
    n_refused = n_front = 0
    for name, level, cap in F.table():
        data = F.data_of(name)
        st0, out0, front = F.expect(data, level, cap)
        st, out_len, adler, dst = _sim_deflate_into(sim, data, level, cap, 0xA5)
        assert st == st0, (name, level, cap, st)
        assert dst[cap:] == b"\xa5" * 64, (name, level, cap)
        if st0 == 0:
            assert dst[:out_len] == out0 and adler == _adler(data, level), (name, level, cap)
            continue
        n_refused += 1
        assert (out_len, adler) == (0, 0), (name, level, cap)
        would_be = F.trace(data, level)[0]
        dst2 = _sim_deflate_into(sim, data, level, cap, 0x5A)[3]
        a, b = np.frombuffer(dst, np.uint8, cap), np.frombuffer(dst2, np.uint8, cap)
        written = np.flatnonzero((a != 0xA5) | (b != 0x5A))
        assert written.size == 0 or written[-1] < front, (name, level, cap)
        ref = np.frombuffer(would_be, np.uint8)
        assert (a[written] == ref[written]).all() and (b[written] == ref[written]).all(), (name, level, cap)
        if by_blocks or level == 0:
            assert written.size == 0, (name, level, cap)
        n_front += bool(written.size)
    assert n_refused > 100
    return n_front


def test_sim_deflate_one_wave_applies_the_rule(oracle):
    from host_sim import lib

    # deflate_emit_wave<0> leaves the blocks in front of the one that does not fit: the model does too
    assert _hold_sim_to_the_table(lib(), oracle, by_blocks=False) > 10


def test_sim_deflate_by_blocks_applies_the_rule(oracle, monkeypatch):
    from host_sim import lib

    monkeypatch.setenv("SIM_EMIT_BLOCKS", "1")
    monkeypatch.setenv("SIM_PARSE_SEGMENTS", "4096")
    assert _hold_sim_to_the_table(lib(), oracle, by_blocks=True) == 0
