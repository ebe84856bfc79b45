"""Every record of lz_match, at every position, against a serial find_backref (zipc_deflate.ml:1176-1201).

The byte-parity tests see the match finder through the lazy parse: positions a match skips are never read, the second
answer (snap[]) only behind a pending match of good_match or more, and a wrong record that does reach the bytes reports
"stream i differs".  Here zipc_hip_debug_match_records runs deflate_offsets, lz_chain and lz_match alone -- lz_match
through the pipeline's own launch, with the walk's form and the tiles per workgroup as arguments -- over poisoned
tables, and every slot is held to tests/host_sim/sim_match.cpp's reference (anchored on the CPU by
tests/test_match_rules.py, which also asserts what each case of tests/match_cases.py is planted for and which kernel
each of the three calls gets):
  * every position 0 .. len - 4 of every stream is written (no poison) and match & ~MATCH_SNAP is the best of the first K;
  * MATCH_SNAP is set iff the best of the first K / 4 is another record, and then snap holds that one (snap is not looked
    at anywhere else: poison there is correct);
  * the PARSE_PAD = 200 entries from len - 3 on are zero;
  * snap_used is 1 iff the stream has a position with two answers;
  * the slots of streams shorter than 4 bytes are untouched.
A failure names stream, case, position, tile and offset in the tile, level and form, and expected against got."""
import numpy as np
import pytest

import host_sim
import match_cases as mc

pytestmark = pytest.mark.gpu

PARSE_PAD = 200  # deflate_pipeline.h
POISON = 0x5A5A5A5A  # include/zipc_hip.h ZIPC_HIP_DEBUG_MATCH_POISON
POS_PAD = 256    # forms.h padded_positions
ROWS = [("small", lv, 0, 0) for lv in (1, 2, 3)]  # lz_match_kernel takes neither argument: a row per level
ROWS += [("alone8193", lv, form, 0) for lv in (1, 2, 3) for form in (0, 1, 2)]
ROWS += [("ragged", lv, form, tpg) for lv in (1, 2, 3) for form in (0, 1, 2) for tpg in (0, 1, 2, 3)]

_BATCH, _EXPECT = {}, {}


def _batch(name):
    """the call's streams, arena and descriptors on the device, and its slot map (built once)"""
    if name in _BATCH:
        return _BATCH[name]
    import torch

    from zipc_amd import batch

    dev = torch.device("cuda", 0)
    streams = mc.batches()[name]
    lens = np.array([len(s) for s in streams], np.int64)
    n = len(streams)
    off = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.uint64)
    descs = batch.make_descs(off, [int(x) for x in lens], np.zeros(n, np.uint64), [0] * n)
    src = torch.from_numpy(np.frombuffer(b"".join(s.data for s in streams) + b"\0" * 64, np.uint8).copy()).to(dev)
    slots = ((lens + 255) & ~255) + POS_PAD
    base = np.concatenate(([0], np.cumsum(slots)[:-1]))
    total = int(lens.sum())
    cap = total + (POS_PAD + 256) * n + 256  # forms.h scratch_caps
    # what is asserted of each slot: 1 a position, 2 a pad entry (zero), 3 a slot of a stream without positions (untouched)
    kind = np.zeros(cap, np.uint8)
    for b, ln, sl in zip(base, lens, slots):
        if ln >= 4:
            kind[b:b + ln - 3] = 1
            kind[b + ln - 3:b + ln - 3 + PARSE_PAD] = 2
        else:
            kind[b:b + sl] = 3
    _BATCH[name] = dict(streams=streams, lens=lens, n=n, src=src, d_descs=batch.to_device(descs, dev), base=base, total=total,
                        longest=int(lens.max()), cap=cap, kind=torch.from_numpy(kind).to(dev), dev=dev)
    return _BATCH[name]


def _expect(name, level):
    """the reference's records in slot coordinates, on the device (computed once per call and level)"""
    if (name, level) in _EXPECT:
        return _EXPECT[(name, level)]
    import concurrent.futures

    import torch

    B = _batch(name)
    L = host_sim.lib()
    best, first = np.zeros(B["cap"], np.int32), np.zeros(B["cap"], np.int32)
    used = np.zeros(B["n"], np.int32)
    with concurrent.futures.ThreadPoolExecutor(max_workers=16) as ex:
        recs = list(ex.map(lambda s: host_sim.match_reference(L, s.data, level), B["streams"]))
    for i, (b, (rb, rf)) in enumerate(zip(B["base"], recs)):
        best[b:b + len(rb)] = rb.view(np.int32)
        first[b:b + len(rf)] = rf.view(np.int32)
        used[i] = int((rb != rf).any())
    _EXPECT[(name, level)] = tuple(torch.from_numpy(a).to(B["dev"]) for a in (best, first, used))
    return _EXPECT[(name, level)]


def _pair(v):
    v = int(v) & 0xFFFFFFFF
    return "%#x" % v if v == POISON else "(%d, %d)%s" % ((v & 0x7FFFFFFF) >> 9, v & 511, " | SNAP" if v >> 31 else "")


@pytest.mark.parametrize("name,level,form,tpg", ROWS, ids=["%s-level%d-form%d-tpg%d" % r for r in ROWS])
def test_every_record_is_the_serial_find_backref(gpu_ctx, name, level, form, tpg):
    import torch

    from zipc_amd import batch

    assert batch.MATCH_POISON == POISON
    B = _batch(name)
    want_best, want_first, want_used = _expect(name, level)
    match, snap, used, pos_base = batch.debug_match_records(gpu_ctx, B["src"], B["d_descs"], B["n"], B["longest"], B["total"], level,
                                                            match_form=form, tiles_per_group=tpg)
    assert match.numel() == B["cap"]
    assert np.array_equal(pos_base.cpu().numpy(), B["base"])
    kind = B["kind"]
    flag, got = match < 0, match & 0x7FFFFFFF  # MATCH_SNAP is bit 31
    two = want_first != want_best
    bad = (kind == 1) & ((got != want_best) | (flag != two) | (flag & (snap != want_first)))
    bad |= (kind == 2) & (match != 0)
    bad |= (kind == 3) & ((match != POISON) | (snap != POISON))
    n_bad = int(bad.sum())
    if n_bad:
        lines = []
        for slot in torch.nonzero(bad).flatten()[:10].cpu().numpy():
            i = int(np.searchsorted(B["base"], slot, side="right") - 1)
            p = int(slot - B["base"][i])
            tile, offset = mc.tile_of(p) if name != "small" else (p // 1024, p % 1024)
            k = int(kind[slot])
            exp = ("best %s first %s" % (_pair(want_best[slot]), _pair(want_first[slot])) if k == 1 else "0 (pad)" if k == 2 else "poison (untouched)")
            lines.append("stream %d (%s, %d bytes) position %d, tile %d + %d, level %d form %d tiles_per_group %d: expected %s, got match %s snap %s"
                         % (i, B["streams"][i].name, B["lens"][i], p, tile, offset, level, form, tpg, exp, _pair(match[slot]), _pair(snap[slot])))
        assert False, "%d slots differ from the reference, the first:\n%s" % (n_bad, "\n".join(lines))
    wrong = torch.nonzero(used != want_used).flatten().cpu().numpy()
    assert wrong.size == 0, "snap_used: " + ", ".join("stream %d (%s) is %d, the reference has %stwo answers" % (
        i, B["streams"][i].name, int(used[i]), "" if int(want_used[i]) else "no position with ") for i in wrong[:10])
    if name == "ragged":  # both kinds of stream are in the call
        assert int(want_used.sum()) > 0 and int((want_used == 0).sum()) > 0
