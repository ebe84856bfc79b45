"""zipc_hip_recode_batch (include/zipc_hip.h): deflate streams in a device arena inflated, CRC-checked and deflated again
on the device, between recode.hip's three kernels, nothing read back.  Every expectation is the oracle's
(tests/recode_cases.py: oracle.deflate(oracle.inflate(src), level), oracle.crc32); nothing is compared with another path of
the library except where the test says that the comparison of two paths is its point."""
import numpy as np
import pytest

import recode_cases as RC
import util

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _slot(cap):
    return (cap + 255) // 256 * 256 + 256


class Layout:
    """where the streams of a batch lie in the three arenas"""

    def __init__(self, cases):
        from zipc_amd import batch

        self.cases = cases
        self.src_off = np.cumsum([0] + [len(c.stream) for c in cases[:-1]]).astype(np.uint64)
        self.mid_slots = [_slot(c.mid_cap) for c in cases]
        self.mid_off = np.cumsum([0] + self.mid_slots[:-1]).astype(np.uint64)
        self.dst_caps = [RC.bound(c.mid_cap) if c.dst_cap is None else c.dst_cap for c in cases]
        self.dst_slots = [_slot(RC.bound(c.mid_cap)) for c in cases]
        self.dst_off = np.cumsum([0] + self.dst_slots[:-1]).astype(np.uint64)
        self.descs = batch.make_recode_descs(self.src_off, [len(c.stream) for c in cases], self.mid_off, [c.mid_cap for c in cases],
                                             self.dst_off, self.dst_caps)
        self.descs["limit"] = [c.limit or 0 for c in cases]
        self.descs["expect_crc32"] = [c.expect or 0 for c in cases]
        self.descs["flags"] = [(1 if c.limit is not None else 0) | (2 if c.expect is not None else 0) | c.flags for c in cases]
        self.max_mid = max(c.mid_cap for c in cases)
        self.total_mid = sum(c.mid_cap for c in cases)

    def arenas(self):
        import torch

        src = torch.from_numpy(np.frombuffer(b"".join(c.stream for c in self.cases) + b"\0" * 64, dtype=np.uint8).copy()).to(DEV)
        mid = torch.full((int(sum(self.mid_slots)) + 256,), 0xA5, dtype=torch.uint8, device=DEV)
        dst = torch.full((int(sum(self.dst_slots)) + 256,), 0xA5, dtype=torch.uint8, device=DEV)
        return src, mid, dst


def run_recode(ctx, lay, level, sync=True, total_mid=None):
    """one recode_batch: (results, the middle arena, the destination arena) as numpy arrays"""
    import torch

    from zipc_amd import batch

    n = len(lay.cases)
    src, mid, dst = lay.arenas()
    d_res = torch.full((n * 32,), 0xEE, dtype=torch.uint8, device=DEV)
    d_descs = batch.to_device(lay.descs, DEV)
    torch.cuda.synchronize()
    batch.recode_batch(ctx, src, mid, dst, d_descs, d_res, n, lay.max_mid, lay.total_mid if total_mid is None else total_mid, level, sync=sync)
    ctx.synchronize()
    return batch.recode_results_from_device(d_res), mid.cpu().numpy(), dst.cpu().numpy()


def check(lay, pairs, res, mid, dst, what):
    for i, (c, e) in enumerate(pairs):
        got = tuple(int(res[f][i]) for f in ("status", "stage", "checksum", "mid_len", "out_len", "reserved"))
        assert got == (e.status, e.stage, e.checksum, e.mid_len, len(e.out), 0), (what, c.name, got)
        o, m = int(lay.dst_off[i]), int(lay.mid_off[i])
        if e.status == 0:
            assert dst[o:o + len(e.out)].tobytes() == e.out, (what, c.name, "recoded bytes")
            assert mid[m:m + e.mid_len].tobytes() == e.data, (what, c.name, "decompressed bytes")
        else:
            # nothing, or at stage 3 nothing but whole bytes of the blocks in front of the one that did not fit
            slot = dst[o:o + lay.dst_slots[i]]
            k = int(np.flatnonzero(slot != 0xA5)[-1]) + 1 if (slot != 0xA5).any() else 0
            assert k <= e.may_write, (what, c.name, "the destination of a stream that stopped was written", k, e.may_write)
            assert slot[:k].tobytes() == e.would_be[:k], (what, c.name, "what lies in front of the block that did not fit is not the stream's")
        if e.stage == 0 and e.status != 0:
            assert (mid[m:m + lay.mid_slots[i]] == 0xA5).all(), (what, c.name, "the middle slot of a refused stream was written")
        assert (dst[o + lay.dst_caps[i]:o + lay.dst_slots[i]] == 0xA5).all(), (what, c.name, "bytes behind dst_cap")
        assert (mid[m + c.mid_cap:m + lay.mid_slots[i]] == 0xA5).all(), (what, c.name, "bytes behind mid_cap")


@pytest.fixture(scope="module")
def ragged():
    cases = RC.ragged_batch()
    assert 40 <= len(cases) <= 50
    assert sum(1 for c in cases if c.limit is not None and c.limit > len(RC._inflate(c.stream, c.limit)[1]) > 0) >= 5  # limits that are no equality
    return Layout(cases)


@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_ragged_batch_with_every_way_to_stop(gpu_ctx, ragged, level):
    pairs = [(c, RC.expectation(c, level)) for c in ragged.cases]
    RC.require_coverage(pairs)
    two = [e for c, e in pairs if c.name == "dst_cap_holds_the_first_block_only"]
    assert len(two) == 1 and (two[0].status, two[0].stage) == (16, 3) and (two[0].may_write > 0) == (level != 0)
    res, mid, dst = run_recode(gpu_ctx, ragged, level)
    check(ragged, pairs, res, mid, dst, "recode_batch level %d" % level)


def test_async_call_gives_the_same(gpu_ctx, ragged):
    """sync=False: the call only enqueues (no stream of this batch has room for 256 KiB); one synchronize, same results"""
    pairs = [(c, RC.expectation(c, 2)) for c in ragged.cases]
    res, mid, dst = run_recode(gpu_ctx, ragged, 2, sync=False)
    check(ragged, pairs, res, mid, dst, "recode_batch, not synchronised")


def host_link(descs, ires):
    """the link rule on the host, as include/zipc_hip.h words it: (deflate's descriptors, per stream the verdict so far)"""
    from zipc_amd import batch

    n = len(descs)
    d = batch.make_descs(descs["mid_off"], np.zeros(n, np.uint64), descs["dst_off"], np.zeros(n, np.uint64))
    verdict = []
    for i in range(n):
        flags, st = int(descs["flags"][i]), int(ires["status"][i])
        if flags & ~3:  # (no mid_cap of these batches is above the max_mid_cap they declare)
            verdict.append((18, 0, 0, 0))
        elif st != 0:
            verdict.append((st, 1, 0, 0))
        elif flags & 2 and int(ires["checksum"][i]) != int(descs["expect_crc32"][i]):
            verdict.append((6, 2, int(ires["checksum"][i]), int(ires["out_len"][i])))
        else:
            verdict.append((0, 0, int(ires["checksum"][i]), int(ires["out_len"][i])))
            d["src_len"][i], d["dst_cap"][i] = ires["out_len"][i], descs["dst_cap"][i]
    return d, verdict


def three_steps(ctx, lay, level, total_mid=None):
    """the library's own composition the header defines the call by: inflate_batch (CRC-32) into the middle arena, the
    results read back, the link on the host, deflate_batch (no checksum): (results as recode_batch words them, mid, dst)"""
    import torch

    from zipc_amd import batch

    n = len(lay.cases)
    src, mid, dst = lay.arenas()
    rd = lay.descs
    idescs = batch.make_descs(rd["src_off"], rd["src_len"], rd["mid_off"], rd["mid_cap"])
    idescs["limit"], idescs["flags"] = rd["limit"], rd["flags"] & 1
    refused = (rd["flags"] & ~np.uint32(3)) != 0
    idescs["src_len"][refused], idescs["dst_cap"][refused], idescs["flags"][refused] = 0, 0, 0
    d_ires = torch.zeros(n * 16, dtype=torch.uint8, device=DEV)
    batch.inflate_batch(ctx, src, mid, batch.to_device(idescs, DEV), d_ires, n, lay.max_mid, 1)
    blocks = ctx.last_inflate_blocks()
    ddescs, verdict = host_link(rd, batch.results_from_device(d_ires))
    d_dres = torch.zeros(n * 16, dtype=torch.uint8, device=DEV)
    batch.deflate_batch(ctx, mid, dst, batch.to_device(ddescs, DEV), d_dres, n, lay.max_mid, lay.total_mid if total_mid is None else total_mid,
                        level, 0)
    dres = batch.results_from_device(d_dres)
    out = np.zeros(n, dtype=batch.RECODE_RESULT_DTYPE)
    for i, (st, stage, crc, mid_len) in enumerate(verdict):
        if st == 0 and int(dres["status"][i]) != 0:
            out[i] = (int(dres["status"][i]), crc, 0, mid_len, 3, 0)
        else:
            out[i] = (st, crc, int(dres["out_len"][i]) if st == 0 else 0, mid_len, stage, 0)
    return out, mid.cpu().numpy(), dst.cpu().numpy(), blocks


@pytest.mark.parametrize("level", [1, 3])
def test_the_call_is_its_three_step_composition(gpu_ctx, ragged, level):
    """two PATHS compared, which is this test's point: results and both arenas, byte for byte"""
    res, mid, dst = run_recode(gpu_ctx, ragged, level)
    res3, mid3, dst3, _ = three_steps(gpu_ctx, ragged, level)
    assert res.tobytes() == res3.tobytes(), [(c.name, a, b) for c, a, b in zip(ragged.cases, res, res3) if a != b]
    assert (mid == mid3).all() and (dst == dst3).all()


def test_a_wrong_total_stops_the_streams_that_got_to_deflate_at_stage_3(gpu_ctx, ragged):
    """total_mid_cap a quarter of the sum: zipc_hip_deflate_batch's device-side check of its declared sizes refuses the
    batch; the streams that had stopped before keep their verdicts, nothing reaches the destination arena, and the
    honest call behind it is exact again"""
    pairs = [(c, RC.expectation(c, 2)) for c in ragged.cases]
    res, mid, dst = run_recode(gpu_ctx, ragged, 2, total_mid=ragged.total_mid // 4)
    for i, (c, e) in enumerate(pairs):
        got = tuple(int(res[f][i]) for f in ("status", "stage", "checksum", "mid_len", "out_len"))
        got_to_deflate = e.status == 0 or e.stage == 3
        want = (18, 3, e.checksum, e.mid_len, 0) if got_to_deflate else (e.status, e.stage, e.checksum, e.mid_len, 0)
        assert got == want, (c.name, got, want)
    assert (dst == 0xA5).all()
    res, mid, dst = run_recode(gpu_ctx, ragged, 2)
    check(ragged, pairs, res, mid, dst, "after a refused batch")


def test_long_member_goes_by_blocks(gpu_ctx):
    """one text-like member of 300 KiB among ten short ones: max_mid_cap is above 256 KiB, so the call takes
    zipc_hip_inflate_batch's block path (which reads the descriptors recode_open_kernel wrote back, and synchronises).
    Checked against the oracle; the block count is compared with the three-step PATH's, which reads the same shape"""
    import oracle

    long_data = util.text(300 * 1024, 5)
    cases = [c for c in RC.good_cases() if "6000" in c.name or "100_" in c.name][:10]
    cases.insert(4, RC.Case("text300k", RC._deflate(long_data, 2), len(long_data), len(long_data), oracle.crc32(long_data)))
    lay = Layout(cases)
    assert len(cases) == 11 and lay.max_mid >= 256 * 1024
    pairs = [(c, RC.expectation(c, 1)) for c in cases]
    assert all(e.status == 0 for _, e in pairs)
    res, mid, dst = run_recode(gpu_ctx, lay, 1)
    blocks = gpu_ctx.last_inflate_blocks()
    check(lay, pairs, res, mid, dst, "recode_batch with a long member")
    res3, mid3, dst3, blocks3 = three_steps(gpu_ctx, lay, 1)
    assert blocks == blocks3 and res.tobytes() == res3.tobytes() and (dst == dst3).all()


def test_scratch_grows_between_two_calls_of_one_context():
    """a context of its own: 8 streams, then 600 (the scratch of the three kernels is grown through the context)"""
    import zipc_amd

    ctx = zipc_amd.Context(0)
    try:
        base = RC.ragged_batch()
        for n in (8, 600):
            cases = [base[i % len(base)] for i in range(n)]
            lay = Layout(cases)
            pairs = [(c, RC.expectation(c, 2)) for c in cases]
            res, mid, dst = run_recode(ctx, lay, 2)
            check(lay, pairs, res, mid, dst, "%d streams" % n)
    finally:
        ctx.close()


def test_call_level_arguments(gpu_ctx):
    import torch

    from zipc_amd import _lib

    L = _lib.lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    p, h = buf.data_ptr(), gpu_ctx.handle
    assert L.zipc_hip_recode_batch(h, p, p, p, p, p, 0, 0, 0, 2) == 0
    for level in (-1, 4):
        assert L.zipc_hip_recode_batch(h, p, p, p, p, p, 1, 16, 16, level) == 18
    assert L.zipc_hip_recode_batch(h, p, p, p, p, p, 1, 0xFFFF0001, 0xFFFF0001, 2) == 18  # one stream with room beyond 4 GiB - 64 KiB
    assert L.zipc_hip_recode_batch(h, p, p, p, None, p, 1, 16, 16, 2) == 18
    assert L.zipc_hip_recode_batch(h, p, p, p, p, None, 1, 16, 16, 2) == 18
    assert L.zipc_hip_recode_batch(None, p, p, p, p, p, 1, 16, 16, 2) == 18


def test_the_three_kernels_run_once_a_call_and_deflate_takes_no_checksum(gpu_ctx, ragged):
    """recode_open / recode_link / recode_close under those names, once each; one CRC-32 pass per slice of inflate's and
    none for deflate: as many crc32_segments launches as a plain inflate_batch with CRC-32 of the same shape makes"""
    try:
        gpu_ctx.set_profiling(True)
        gpu_ctx.reset_kernel_times()
        run_recode(gpu_ctx, ragged, 2)
        t = gpu_ctx.kernel_times()
        assert t["recode_open"][0] == 1 and t["recode_link"][0] == 1 and t["recode_close"][0] == 1, t
        assert t["inflate_batch"][0] >= 1 and "zlib_open" not in t
        crc_launches = t["crc32_segments"][0]
        gpu_ctx.reset_kernel_times()
        three_steps(gpu_ctx, ragged, 2)
        t3 = gpu_ctx.kernel_times()
        assert not {"recode_open", "recode_link", "recode_close"} & set(t3)
        assert t3["crc32_segments"][0] == crc_launches, (t3["crc32_segments"], crc_launches)
    finally:
        gpu_ctx.set_profiling(False)
