"""The steady form of lz_match's first walk (deflate_lane.h lz_match_runs_pool; its rules: zipc_amd/csrc/match_pool.h,
tests/test_match_pool_form.py) against a serial find_backref at every position, as tests/test_gpu_match_records.py holds
the kernel's other paths: zipc_hip_debug_match_records with the first form forced, every level, 0 to 3 tiles per
workgroup, over ONE batch of 4-bit symbols (tests/match_steady_cases.py) whose lengths put the steady loop's entry, its
handouts and its exit on every side of a chunk edge, of a tile's supply of chunks and of the stream's end -- and two
streams whose walks end inside the steady loop by l == 258 and by K and K / 4 candidates.  Every slot is compared: a
position the steady loop's exit dropped stays poison, one handed out twice is written twice with the same record (the
CPU model counts those), the pad entries are zero.  A failure names stream, position, tile and offset."""
import numpy as np
import pytest

import host_sim
import match_cases as mc
import match_steady_cases as sc

pytestmark = pytest.mark.gpu

PARSE_PAD = 200  # deflate_pipeline.h
POISON = 0x5A5A5A5A  # include/zipc_hip.h ZIPC_HIP_DEBUG_MATCH_POISON
POS_PAD = 256    # forms.h padded_positions
ROWS = [(lv, tpg) for lv in (1, 2, 3) for tpg in (0, 1, 2, 3)]

_BATCH, _EXPECT = {}, {}


def _batch():
    """the call's streams, arena and descriptors on the device, and its slot map (built once)"""
    if _BATCH:
        return _BATCH
    import torch

    from zipc_amd import batch

    dev = torch.device("cuda", 0)
    streams = sc.streams()
    lens = np.array([len(s) for s in streams], np.int64)
    assert int(lens.sum()) < 3 << 20 and int(lens.max()) == 65536
    n = len(streams)
    off = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.uint64)
    descs = batch.make_descs(off, [int(x) for x in lens], np.zeros(n, np.uint64), [0] * n)
    src = torch.from_numpy(np.frombuffer(b"".join(s.data for s in streams) + b"\0" * 64, np.uint8).copy()).to(dev)
    slots = ((lens + 255) & ~255) + POS_PAD
    base = np.concatenate(([0], np.cumsum(slots)[:-1]))
    total = int(lens.sum())
    cap = total + (POS_PAD + 256) * n + 256  # forms.h scratch_caps
    kind = np.zeros(cap, np.uint8)  # 1 a position, 2 a pad entry (zero)
    for b, ln in zip(base, lens):
        kind[b:b + ln - 3] = 1
        kind[b + ln - 3:b + ln - 3 + PARSE_PAD] = 2
    _BATCH.update(streams=streams, lens=lens, n=n, src=src, d_descs=batch.to_device(descs, dev), base=base, total=total,
                  longest=int(lens.max()), cap=cap, kind=torch.from_numpy(kind).to(dev), dev=dev)
    return _BATCH


def _expect(level):
    """the reference's records in slot coordinates, on the device (computed once per level)"""
    if level in _EXPECT:
        return _EXPECT[level]
    import concurrent.futures

    import torch

    B = _batch()
    L = host_sim.lib()
    best, first = np.zeros(B["cap"], np.int32), np.zeros(B["cap"], np.int32)
    used = np.zeros(B["n"], np.int32)
    with concurrent.futures.ThreadPoolExecutor(max_workers=16) as ex:
        recs = list(ex.map(lambda s: host_sim.match_reference(L, s.data, level), B["streams"]))
    for i, (b, (rb, rf)) in enumerate(zip(B["base"], recs)):
        best[b:b + len(rb)] = rb.view(np.int32)
        first[b:b + len(rf)] = rf.view(np.int32)
        used[i] = int((rb != rf).any())
    _EXPECT[level] = tuple(torch.from_numpy(a).to(B["dev"]) for a in (best, first, used))
    return _EXPECT[level]


def _pair(v):
    v = int(v) & 0xFFFFFFFF
    return "%#x" % v if v == POISON else "(%d, %d)%s" % ((v & 0x7FFFFFFF) >> 9, v & 511, " | SNAP" if v >> 31 else "")


@pytest.mark.parametrize("level,tpg", ROWS, ids=["level%d-tpg%d" % r for r in ROWS])
def test_every_record_of_the_first_form_is_the_serial_find_backref(gpu_ctx, level, tpg):
    import torch

    from zipc_amd import batch

    assert batch.MATCH_POISON == POISON
    B = _batch()
    want_best, want_first, want_used = _expect(level)
    match, snap, used, pos_base = batch.debug_match_records(gpu_ctx, B["src"], B["d_descs"], B["n"], B["longest"], B["total"], level,
                                                            match_form=1, tiles_per_group=tpg)
    assert match.numel() == B["cap"]
    assert np.array_equal(pos_base.cpu().numpy(), B["base"])
    kind = B["kind"]
    flag, got = match < 0, match & 0x7FFFFFFF  # MATCH_SNAP is bit 31
    two = want_first != want_best
    bad = (kind == 1) & ((got != want_best) | (flag != two) | (flag & (snap != want_first)))
    bad |= (kind == 2) & (match != 0)
    n_bad = int(bad.sum())
    if n_bad:
        lines = []
        for slot in torch.nonzero(bad).flatten()[:10].cpu().numpy():
            i = int(np.searchsorted(B["base"], slot, side="right") - 1)
            p = int(slot - B["base"][i])
            tile, offset = mc.tile_of(p)
            exp = "best %s first %s" % (_pair(want_best[slot]), _pair(want_first[slot])) if int(kind[slot]) == 1 else "0 (pad)"
            lines.append("stream %d (%s, %d bytes) position %d, tile %d + %d (chunk %d + %d), level %d tiles_per_group %d: expected %s, got match %s snap %s"
                         % (i, B["streams"][i].name, B["lens"][i], p, tile, offset, offset // sc.CHUNK, offset % sc.CHUNK, level, tpg, exp,
                            _pair(match[slot]), _pair(snap[slot])))
        assert False, "%d slots differ from the reference, the first:\n%s" % (n_bad, "\n".join(lines))
    wrong = torch.nonzero(used != want_used).flatten().cpu().numpy()
    assert wrong.size == 0, "snap_used: " + ", ".join("stream %d (%s) is %d, the reference has %stwo answers" % (
        i, B["streams"][i].name, int(used[i]), "" if int(want_used[i]) else "no position with ") for i in wrong[:10])
