"""zipc_hip_zlib_decompress_batch / zipc_hip_zlib_compress_batch (include/zipc_hip.h): whole zlib streams in device
arenas, the container opened and closed by zlib.hip's two kernels around the codec's.  Every expectation is the
oracle's (tests/zlib_cases.py) or, for RFC 1950's Adler-32, Python's zlib; nothing is compared with another path of the
library except where the test says that the comparison of two paths is its point."""
import zlib

import numpy as np
import pytest

import util
import zlib_cases as ZC

pytestmark = pytest.mark.gpu


def _slot(cap):
    return (cap + 255) // 256 * 256 + 256


def _arena(streams):
    import torch

    off = np.cumsum([0] + [len(s) for s in streams[:-1]]).astype(np.uint64)
    src = torch.from_numpy(np.frombuffer(b"".join(streams) + b"\0" * 64, dtype=np.uint8).copy()).to("cuda:0")
    return off, src


def run_decompress(ctx, cases, sync=True):
    """one zlib_decompress_batch over `cases` (zlib_cases.Case): (results, the destination arena, dst_off, slots)"""
    import torch

    from zipc_amd import batch

    n = len(cases)
    src_off, src = _arena([c.stream for c in cases])
    slots = [_slot(c.cap) for c in cases]
    dst_off = np.cumsum([0] + slots[:-1]).astype(np.uint64)
    descs = batch.make_descs(src_off, [len(c.stream) for c in cases], dst_off, [c.cap for c in cases])
    descs["limit"] = [c.limit or 0 for c in cases]
    descs["flags"] = [(1 if c.limit is not None else 0) | c.flags for c in cases]
    dst = torch.full((int(sum(slots)) + 256,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_res = torch.full((n * 16,), 0xEE, dtype=torch.uint8, device="cuda:0")
    batch.zlib_decompress_batch(ctx, src, dst, batch.to_device(descs, "cuda:0"), d_res, n, max(c.cap for c in cases), sync=sync)
    ctx.synchronize()
    return batch.results_from_device(d_res), dst.cpu().numpy(), dst_off, slots


def check_decompress(pairs, res, out, dst_off, slots, what):
    for i, (c, e) in enumerate(pairs):
        st, ln, ck = int(res["status"][i]), int(res["out_len"][i]), int(res["checksum"][i])
        o = int(dst_off[i])
        assert st == e.status, (what, c.name, st, e.status)
        if st == 0:
            assert ln == len(e.out) and out[o:o + ln].tobytes() == e.out and ck == e.checksum, (what, c.name)
        else:
            assert ln == 0, (what, c.name, ln)
        if st == 6:
            assert ck == e.checksum, (what, c.name, hex(ck), hex(e.checksum))  # the value found; expected: the stream's last 4 bytes
        if e.header:
            assert (out[o:o + slots[i]] == 0xA5).all(), (what, c.name, "a refused stream's destination was written")
        assert (out[o + c.cap:o + slots[i]] == 0xA5).all(), (what, c.name, "bytes behind dst_cap")


def test_ragged_decompress_with_every_error(gpu_ctx):
    pairs = ZC.decompress_expectations()  # (asserts on the oracle's side that statuses 0-6, 16 and 18 all occur)
    assert {e.status for _, e in pairs} >= ZC.REQUIRED_STATUSES
    res, out, dst_off, slots = run_decompress(gpu_ctx, [c for c, _ in pairs])
    check_decompress(pairs, res, out, dst_off, slots, "zlib_decompress_batch")
    assert sum(1 for _, e in pairs if e.header) >= 10


def test_both_adler_flavours(gpu_ctx, oracle):
    """streams Python's zlib made of bytes above 0x7F in bulk: with set_adler_rfc1950(1) they decode; with the default
    the result is exactly oracle.zlib_decompress's.  util.rand_bytes(20000, 2) is the input the feature's issue names as
    one the reference rejects -- it does not: the reference's signed remainders (zd.ml:95,196) happen to leave the RFC's
    value for these 20 000 bytes, and the oracle says OK.  The case stays, held to the oracle, and 30 000 bytes of the same
    generator -- which the oracle does reject with a checksum mismatch -- stand beside it, so both verdicts are there."""
    verdicts = set()
    for n in (20000, 30000):
        data = util.rand_bytes(n, 2)
        z = zlib.compress(data)
        case = ZC.Case("rfc_stream_%d" % n, z, len(data), len(data), 0)
        st0, d0, a0, expect0, found0 = oracle.zlib_decompress(z, decompressed_size=len(data))
        assert expect0 == zlib.adler32(data) and st0 in (0, 6)
        verdicts.add(st0)
        try:
            gpu_ctx.set_adler_rfc1950(True)
            res, out, dst_off, _ = run_decompress(gpu_ctx, [case])
            assert (int(res["status"][0]), int(res["out_len"][0]), int(res["checksum"][0])) == (0, len(data), zlib.adler32(data))
            assert out[:len(data)].tobytes() == zlib.decompress(z) == data
            gpu_ctx.set_adler_rfc1950(False)
            res, out, _, _ = run_decompress(gpu_ctx, [case])
            got = (int(res["status"][0]), int(res["out_len"][0]), int(res["checksum"][0]))
            if st0 == 6:  # (the reference rejects this valid stream: its Adler-32 is its own)
                assert found0 != expect0 and got == (6, 0, found0), (n, got)
            else:
                assert got == (0, len(data), a0) and out[:len(data)].tobytes() == d0 == data, (n, got)
        finally:
            gpu_ctx.set_adler_rfc1950(False)
    assert verdicts == {0, 6}, verdicts  # (on the oracle's side: the two flavours do part on one of the inputs)


def test_long_stream_goes_by_blocks_through_the_inner_descriptors(gpu_ctx):
    """one stream with room for 256 KiB and more: zipc_hip_inflate_batch reads the descriptors back and decodes by a wave
    per block -- here the descriptors it reads are the ones zlib_open_kernel wrote.  The two PATHS are compared: the
    block count is whatever a plain inflate_batch of the same body with the same descriptor shape reports."""
    import torch

    from zipc_amd import batch

    data = util.text(300000, 5)
    co = zlib.compressobj(6)
    z = b""
    for at in range(0, len(data), 32768):
        z += co.compress(data[at:at + 32768]) + co.flush(zlib.Z_FULL_FLUSH)
    z += co.flush()
    assert zlib.decompress(z) == data and len(data) >= 256 * 1024
    try:
        gpu_ctx.set_adler_rfc1950(True)
        res, out, _, _ = run_decompress(gpu_ctx, [ZC.Case("flushed", z, len(data), len(data), 0)])
        blocks = gpu_ctx.last_inflate_blocks()
        assert (int(res["status"][0]), int(res["out_len"][0]), int(res["checksum"][0])) == (0, len(data), zlib.adler32(data))
        assert out[:len(data)].tobytes() == data
    finally:
        gpu_ctx.set_adler_rfc1950(False)
    body = z[2:-2]
    descs = batch.make_descs([0], [len(body)], [0], [len(data)], limit=[len(data)])
    _, src = _arena([body])
    dst = torch.zeros(_slot(len(data)), dtype=torch.uint8, device="cuda:0")
    d_res = torch.zeros(16, dtype=torch.uint8, device="cuda:0")
    batch.inflate_batch(gpu_ctx, src, dst, batch.to_device(descs, "cuda:0"), d_res, 1, len(data), 3)
    r = batch.results_from_device(d_res)
    assert (int(r["status"][0]), int(r["checksum"][0])) == (0, zlib.adler32(data))
    assert gpu_ctx.last_inflate_blocks() == blocks


def run_compress(ctx, triples, level, total_delta=0, sync=True):
    """one zlib_compress_batch over zlib_cases.compress_expectations(level)-shaped triples"""
    import torch

    from zipc_amd import batch

    n = len(triples)
    datas = [c.data for c, _, _ in triples]
    src_off, src = _arena(datas)
    caps = [batch.zlib_bound(len(c.data)) if cap is None else cap for c, cap, _ in triples]
    slots = [_slot(batch.zlib_bound(len(c.data))) for c, _, _ in triples]
    dst_off = np.cumsum([0] + slots[:-1]).astype(np.uint64)
    descs = batch.make_descs(src_off, [len(d) for d in datas], dst_off, caps)
    dst = torch.full((int(sum(slots)) + 256,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_res = torch.full((n * 16,), 0xEE, dtype=torch.uint8, device="cuda:0")
    batch.zlib_compress_batch(ctx, src, dst, batch.to_device(descs, "cuda:0"), d_res, n, max(len(d) for d in datas),
                              sum(len(d) for d in datas) + total_delta, level, sync=sync)
    ctx.synchronize()
    return batch.results_from_device(d_res), dst.cpu().numpy(), dst_off, slots, caps


def check_compress(triples, res, out, dst_off, slots, caps, what):
    for i, (c, _, e) in enumerate(triples):
        st, ln, ck = int(res["status"][i]), int(res["out_len"][i]), int(res["checksum"][i])
        o = int(dst_off[i])
        assert st == e.status, (what, c.name, st, e.status)
        if st == 0:
            assert ln == len(e.out) and ck == e.checksum and out[o:o + ln].tobytes() == e.out, (what, c.name)
        else:
            assert ln == 0, (what, c.name)
        if e.header:
            assert (out[o:o + slots[i]] == 0xA5).all(), (what, c.name, "a stream without room for the container was written to")
        assert (out[o + caps[i]:o + slots[i]] == 0xA5).all(), (what, c.name, "bytes behind dst_cap")


@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_ragged_compress(gpu_ctx, level):
    triples = ZC.compress_expectations(level)
    assert {e.status for _, _, e in triples} == {0, 16} and sum(1 for _, _, e in triples if e.header) == 2
    res, out, dst_off, slots, caps = run_compress(gpu_ctx, triples, level)
    check_compress(triples, res, out, dst_off, slots, caps, "zlib_compress_batch level %d" % level)


def test_compress_with_a_wrong_total_is_refused_for_every_stream(gpu_ctx):
    """total_src_len a quarter of the sum (the scratch it sizes has a few hundred bytes of slack a stream, so a total that
    is short by less goes through, in the raw form too): zipc_hip_deflate_batch's device-side check fails the whole
    batch, and the container passes that on"""
    triples = [t for t in ZC.compress_expectations(2) if t[1] is None and len(t[0].data) <= 70000]
    total = sum(len(c.data) for c, _, _ in triples)
    res, out, dst_off, slots, caps = run_compress(gpu_ctx, triples, 2, total_delta=total // 4 - total)
    assert (res["status"] == 18).all() and (res["out_len"] == 0).all() and (res["checksum"] == 0).all(), res["status"]
    assert (out == 0xA5).all()
    res, out, dst_off, slots, caps = run_compress(gpu_ctx, triples, 2)  # (nothing sticks: the honest call is exact)
    check_compress(triples, res, out, dst_off, slots, caps, "after a refused batch")


def test_call_level_arguments(gpu_ctx):
    import torch

    from zipc_amd import _lib

    L = _lib.lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    p = buf.data_ptr()
    assert L.zipc_hip_zlib_decompress_batch(gpu_ctx.handle, p, p, p, p, 0, 0) == 0
    assert L.zipc_hip_zlib_compress_batch(gpu_ctx.handle, p, p, p, p, 0, 0, 0, 2) == 0
    for level in (-1, 4):
        assert L.zipc_hip_zlib_compress_batch(gpu_ctx.handle, p, p, p, p, 1, 0, 0, level) == 18
    # one stream with room beyond 4 GiB - 64 KiB: inflate's path for that has no Adler-32
    assert L.zipc_hip_zlib_decompress_batch(gpu_ctx.handle, p, p, p, p, 1, 0xFFFF0001) == 18
    assert L.zipc_hip_zlib_decompress_batch(gpu_ctx.handle, p, p, None, p, 1, 16) == 18


def test_device_round_trip_without_a_sync_between_the_calls(gpu_ctx, oracle):
    """compress and decompress enqueued back to back, one synchronize at the end.  The decompress descriptors are built
    BEFORE anything runs, from sizes known up front -- slots of zipc_hip_zlib_bound, src_len the oracle's size of each
    stream (the library's bytes are the oracle's, so the size is known without reading out_len back: no sync for it).
    Two streams get src_len = the bound instead, which is not exact: their trailer is read where it is not, and what the
    oracle says of such a stream (the zlib stream followed by the slot's fill) is what is expected of them."""
    import torch

    from zipc_amd import batch

    datas = [util.text(n, 60 + i) for i, n in enumerate((3000, 70000, 1, 20000))] + [util.rand_bytes(9000, 3), b"", util.text(5000, 9)]
    level, n = 2, len(datas)
    zs = [oracle.zlib_compress(d, level)[1] for d in datas]
    bounds = [batch.zlib_bound(len(d)) for d in datas]
    inexact = {2, 6}
    src_off, src = _arena(datas)
    cslots = [_slot(b) for b in bounds]
    coff = np.cumsum([0] + cslots[:-1]).astype(np.uint64)
    cdescs = batch.make_descs(src_off, [len(d) for d in datas], coff, bounds)
    comp = torch.full((int(sum(cslots)) + 256,), 0xA5, dtype=torch.uint8, device="cuda:0")
    dslots = [_slot(len(d)) for d in datas]
    doff = np.cumsum([0] + dslots[:-1]).astype(np.uint64)
    ddescs = batch.make_descs(coff, [bounds[i] if i in inexact else len(zs[i]) for i in range(n)], doff, [len(d) for d in datas],
                              limit=[len(d) for d in datas])
    back = torch.full((int(sum(dslots)) + 256,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_cdescs, d_ddescs = batch.to_device(cdescs, "cuda:0"), batch.to_device(ddescs, "cuda:0")
    d_cres = torch.zeros(n * 16, dtype=torch.uint8, device="cuda:0")
    d_dres = torch.zeros(n * 16, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    batch.zlib_compress_batch(gpu_ctx, src, comp, d_cdescs, d_cres, n, max(len(d) for d in datas), sum(len(d) for d in datas), level,
                              sync=False)
    batch.zlib_decompress_batch(gpu_ctx, comp, back, d_ddescs, d_dres, n, max(len(d) for d in datas), sync=False)
    gpu_ctx.synchronize()
    cres, dres, out = batch.results_from_device(d_cres), batch.results_from_device(d_dres), back.cpu().numpy()
    for i in range(n):
        assert (int(cres["status"][i]), int(cres["out_len"][i])) == (0, len(zs[i])), i
        stream = zs[i] + b"\xa5" * (bounds[i] - len(zs[i])) if i in inexact else zs[i]
        st0, d0, a0, _, found0 = oracle.zlib_decompress(stream, decompressed_size=len(datas[i]))
        assert int(dres["status"][i]) == st0, (i, int(dres["status"][i]), st0)
        if i not in inexact:
            assert st0 == 0
        if st0 == 0:
            o = int(doff[i])
            assert out[o:o + int(dres["out_len"][i])].tobytes() == d0 == datas[i] and int(dres["checksum"][i]) == a0, i
        elif st0 == 6:
            assert (int(dres["out_len"][i]), int(dres["checksum"][i])) == (0, found0), i


def test_only_the_new_calls_launch_the_container_kernels(gpu_ctx):
    """zlib_open / zlib_close are launched under those names by the two zlib batch forms, once each a call, and by
    nothing else: the raw batch forms run the kernels they ran before"""
    pairs = [p for p in ZC.decompress_expectations() if p[0].name.startswith("good_text3000")]
    try:
        gpu_ctx.set_profiling(True)
        gpu_ctx.reset_kernel_times()
        util.gpu_inflate_batch(gpu_ctx, [c.stream[2:-2] for c, _ in pairs], [c.cap for c, _ in pairs], [True] * len(pairs),
                               [c.limit for c, _ in pairs], 2)
        assert not {"zlib_open", "zlib_close"} & set(gpu_ctx.kernel_times())
        gpu_ctx.reset_kernel_times()
        run_decompress(gpu_ctx, [c for c, _ in pairs])
        t = gpu_ctx.kernel_times()
        assert t["zlib_open"][0] == 1 and t["zlib_close"][0] == 1 and t["inflate_batch"][0] >= 1, t
        gpu_ctx.reset_kernel_times()
        run_compress(gpu_ctx, ZC.compress_expectations(1)[:4], 1)
        t = gpu_ctx.kernel_times()
        assert t["zlib_open"][0] == 1 and t["zlib_close"][0] == 1, t
    finally:
        gpu_ctx.set_profiling(False)
