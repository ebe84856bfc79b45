"""Every link of lz_chain, at every position, in every one of its four forms, against a serial insert_hash
(zipc_deflate.ml:1145-1152).

The byte-parity tests see the links through lz_match and the lazy parse: a wrong link shows only where it changes the
best of the first K candidates at a position the parse reads, and then as "stream i differs"; test_gpu_limits.py holds
the exchange kernel to the peel kernel, which proves nothing where both share an error, and only over whole streams.
Here zipc_hip_debug_chain_links_form runs deflate_offsets and ONE chain form alone, through the pipeline's own launch
site, over links filled with 0xFFFF, and every slot is held to tests/host_sim/sim_chain.cpp's reference (anchored on the
CPU by tests/test_chain_rules.py, which also asserts what each case of tests/chain_cases.py is planted for):
  * every position 0 .. len - 4 of every stream of at least 4 bytes holds the reference's link;
  * every other slot still holds 0xFFFF: the pads, the slots of a stream's last three bytes, streams shorter than 4.
The rows: both batches by exchange over whole streams and by segments of 96 Ki and 192 Ki positions, by the peel kernel
over whole streams and by segments of 32 Ki, 64 Ki and 128 Ki, and in the form a deflate call of the batch's shape gets
(seg_positions = 0; the form is the one host_sim's build of forms.h predicts), with and without the exchange kernels.
Every position is compared, on the device.  A failure names stream, case, position, round, turn, wave, lane, segment, form
and segment size, the expected link with the position it points to, and the value got."""
import numpy as np
import pytest

import chain_cases as cc
import host_sim

pytestmark = pytest.mark.gpu

POISON = 0xFFFF  # include/zipc_hip.h ZIPC_HIP_DEBUG_LINK_POISON
POS_PAD = 256    # forms.h padded_positions
XCHG, XCHG_SEG, PEEL, PEEL_SEG = 0, 1, 2, 3  # forms.h ChainKernel
FORMS = [(XCHG, 0)] + [(XCHG_SEG, s) for s in cc.XCHG_SEGS] + [(PEEL, 0)] + [(PEEL_SEG, s) for s in cc.PEEL_SEGS]
ROWS = [(b, c, s) for b in ("edges", "long") for c, s in FORMS]
ROWS += [(b, own, 0) for b in ("edges", "long") for own in ("own", "own-peel")]  # the shape's own form, with / without the exchange kernels

_BATCH = {}


def _batch(name):
    """the call's streams, arena and descriptors on the device, and the reference's links in slot coordinates (built once)"""
    if name in _BATCH:
        return _BATCH[name]
    import concurrent.futures

    import torch

    from zipc_amd import batch

    dev = torch.device("cuda", 0)
    streams = cc.batches()[name]
    lens = np.array([len(s) for s in streams], np.int64)
    n = len(streams)
    off = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.uint64)  # end to end, no gap
    descs = batch.make_descs(off, [int(x) for x in lens], np.zeros(n, np.uint64), [0] * n)
    src = torch.from_numpy(np.frombuffer(cc.arena(streams), np.uint8).copy()).to(dev)
    slots = ((lens + 255) & ~255) + POS_PAD
    base = np.concatenate(([0], np.cumsum(slots)[:-1]))
    total = int(lens.sum())
    cap = total + (POS_PAD + 256) * n + 256  # forms.h scratch_caps
    L = host_sim.lib()
    want = np.full(cap, POISON, np.uint16)
    with concurrent.futures.ThreadPoolExecutor(max_workers=16) as ex:
        refs = list(ex.map(lambda s: host_sim.chain_links(L, s.data, "reference"), streams))
    for b, ln, r in zip(base, lens, refs):
        assert (r[max(ln - 3, 0):] == POISON).all() and (r[:max(ln - 3, 0)] <= cc.WINDOW).all()
        want[b:b + ln] = r  # (the last three bytes' slots: poison in the reference's array too)
    _BATCH[name] = dict(streams=streams, lens=lens, n=n, src=src, d_descs=batch.to_device(descs, dev), base=base, total=total,
                        longest=int(lens.max()), cap=cap, want=torch.from_numpy(want.view(np.int16)).to(dev), dev=dev)
    return _BATCH[name]


def _row_id(r):
    return "%s-%s-%d" % (r[0], r[1] if isinstance(r[1], str) else cc.CHAIN_NAMES[r[1]].replace(" ", "_"), r[2])


@pytest.mark.parametrize("name,chain,seg", ROWS, ids=[_row_id(r) for r in ROWS])
def test_every_link_is_the_serial_insert_hash(gpu_ctx, name, chain, seg):
    import torch

    from zipc_amd import batch

    assert batch.LINK_POISON == POISON == host_sim.LINK_POISON
    assert (batch.CHAIN_XCHG, batch.CHAIN_XCHG_SEGMENTS, batch.CHAIN_PEEL, batch.CHAIN_PEEL_SEGMENTS) == (XCHG, XCHG_SEG, PEEL, PEEL_SEG)
    B = _batch(name)
    seg_arg = seg
    if isinstance(chain, str):  # what forms.h gives a deflate call of this shape: the library is asked for that form with seg_positions = 0
        f, s = host_sim.deflate_forms(host_sim.lib(), B["n"], B["longest"], B["total"], level=2, xchg_ok=int(chain == "own"), slices_override=1)
        chain = int(s["chain"])
        seg = int(f["xseg"]) if chain == XCHG_SEG else int(f["chain_seg"]) if chain == PEEL_SEG else 0
        seg_arg = 0
    links, pos_base = batch.debug_chain_links_form(gpu_ctx, B["src"], B["d_descs"], B["n"], B["longest"], B["total"], chain, seg_arg)
    assert links.numel() == B["cap"]
    assert np.array_equal(pos_base.cpu().numpy(), B["base"])
    bad = links != B["want"]
    n_bad = int(bad.sum())
    if n_bad:
        form = cc.CHAIN_NAMES[chain] + (" of %d positions" % seg if seg else "")
        lines = []
        for slot in torch.nonzero(bad).flatten()[:10].cpu().numpy():
            i = int(np.searchsorted(B["base"], slot, side="right") - 1)
            p, ln = int(slot - B["base"][i]), int(B["lens"][i])
            s = B["streams"][i]
            got, exp = int(links[slot]) & 0xFFFF, int(B["want"][slot]) & 0xFFFF
            if ln >= 4 and p <= ln - 4:
                expected = "link %d (to position %d)" % (exp, p - exp) if exp else "link 0 (no earlier position of its hash within 32768)"
                lines.append("stream %d (%s, %d bytes: %s) position %d, %s, %s: expected %s, got %s" % (
                    i, s.name, ln, s.what, p, cc.where(p, chain, seg), form, expected, "0xFFFF (not written)" if got == POISON else got))
            else:
                kind = "a stream shorter than 4 bytes" if ln < 4 else "the last three bytes" if p < ln else "the pad behind the stream"
                lines.append("stream %d (%s, %d bytes) slot %d (%s), %s: expected 0xFFFF (untouched), got %d" % (i, s.name, ln, p, kind, form, got))
        assert False, "%d slots differ from the reference, the first:\n%s" % (n_bad, "\n".join(lines))
    assert int((links != -1).sum()) == int(np.maximum(B["lens"] - 3, 0).sum())  # exactly the positions are written


def test_a_segment_size_the_forms_cannot_produce_is_refused(gpu_ctx):
    from zipc_amd import ZipcHipError, batch

    B = _batch("edges")
    for chain, seg in ((XCHG_SEG, 65536), (XCHG_SEG, 98304 + 1024), (PEEL_SEG, 16384), (PEEL_SEG, 98304), (PEEL_SEG, 1)):
        with pytest.raises(ZipcHipError) as e:
            batch.debug_chain_links_form(gpu_ctx, B["src"], B["d_descs"], B["n"], B["longest"], B["total"], chain, seg)
        assert e.value.status == 18  # ZIPC_HIP_ERR_INVALID_ARG
    for chain in (XCHG, PEEL):  # the whole-stream forms ignore it
        links, _ = batch.debug_chain_links_form(gpu_ctx, B["src"], B["d_descs"], B["n"], B["longest"], B["total"], chain, 12345)
        assert bool((links == B["want"]).all())
