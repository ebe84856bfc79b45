"""Sizing on the MI355X: zipc_hip_inflate_size_batch / zipc_hip_zlib_size_batch / zipc_hip_inflate_size -- what a batch of
deflate or zlib streams inflates to, and whether it does, with nothing written.  Every expectation is the oracle's
(tests/size_cases.py); result slots are poisoned with 0xEE before every call, and the source arena is compared with what
was uploaded afterwards (there is no destination arena to compare)."""
import ctypes as C

import numpy as np
import pytest

import recode_cases
import size_cases
import util

pytestmark = pytest.mark.gpu

MAX_STREAM_LEN = 0xFFFF0000
Item = size_cases.Sized  # name, stream, limit, want = (status, out_len)


def _call(gpu_ctx, items, zlib=False, sync=True, dst=None, flags=None, src_len=None):
    """one sizing call over items [(name, stream, limit, ...)]: the results as a numpy record array.  dst: (dst_off, dst_cap)
    per stream (default: 0, 0 -- they are not to be looked at); flags / src_len: overrides per stream, or None"""
    import torch

    from zipc_amd import batch

    dev = torch.device("cuda", 0)
    n = len(items)
    lens = [len(it.stream) for it in items]
    src_off = np.cumsum([0] + lens[:-1]).astype(np.uint64)
    descs = batch.make_descs(src_off, lens, [d[0] for d in dst] if dst else np.zeros(n, np.uint64),
                             [d[1] for d in dst] if dst else np.zeros(n, np.uint64))
    for i, it in enumerate(items):
        if it.limit is not None:
            descs["limit"][i] = it.limit
            descs["flags"][i] = 1
        if flags is not None and flags[i] is not None:
            descs["flags"][i] = flags[i]
        if src_len is not None and src_len[i] is not None:
            descs["src_len"][i] = src_len[i]
    arena = np.frombuffer(b"".join(it.stream for it in items) + b"\0" * 64, dtype=np.uint8).copy()
    src = torch.from_numpy(arena).to(dev)
    d_descs = batch.to_device(descs, dev)
    d_res = torch.full((n * 16,), 0xEE, dtype=torch.uint8, device=dev)
    fn = batch.zlib_size_batch if zlib else batch.inflate_size_batch
    if sync:
        fn(gpu_ctx, src, d_descs, d_res, n)
    else:
        torch.cuda.synchronize()  # (the uploads are torch's; the call is enqueued on the context's stream)
        fn(gpu_ctx, src, d_descs, d_res, n, sync=False)
        gpu_ctx.synchronize()     # the one synchronize
    res = batch.results_from_device(d_res)
    assert np.array_equal(src.cpu().numpy(), arena), "the source arena changed"
    assert np.array_equal(batch.to_device(descs, "cpu").numpy(), d_descs.cpu().numpy()), "the descriptors changed"
    return res


def _check(res, items, what):
    for i, it in enumerate(items):
        got = (int(res["status"][i]), int(res["checksum"][i]), int(res["out_len"][i]))
        assert got == (it.want[0], 0, it.want[1]), (what, it.name, got, it.want)


def test_rule_table(gpu_ctx, oracle):
    """one call over the 413 short rule cases and one over the 73 inside long streams: status, checksum 0 and out_len of
    every stream as the oracle has it -- dist_eq_out / dist_out_plus1 and dist_32768_at_3276[78] prove the distance
    check at the true output position, the *limit_* families the limit"""
    names = {s.name for s in size_cases.rule_cases()}
    assert all(n in names for n in size_cases.REQUIRED_NAMES)
    assert sum("limit" in n for n in names) >= 40
    short, long_ = size_cases.short_rule_cases(), size_cases.long_rule_cases()
    assert (len(short), len(long_)) == (413, 73)
    _check(_call(gpu_ctx, short), short, "short")
    _check(_call(gpu_ctx, long_), long_, "long")


def test_results_without_a_synchronising_call(gpu_ctx, oracle):
    """sync=False: the call enqueues and returns; after ONE synchronize the results are those of test_rule_table's short call"""
    short = size_cases.short_rule_cases()
    _check(_call(gpu_ctx, short, sync=False), short, "short, sync=False")


def test_descriptor_rules(gpu_ctx, oracle):
    from zipc_amd import _lib

    data = util.text(5000, 3)
    s = oracle.deflate(data, level=2)[1]
    st_empty, d_empty, _ = oracle.inflate(b"")
    good = (0, len(data))
    items = [Item("flag_bit_1", s, None, (18, 0)), Item("flag_bit_2", s, len(data), (18, 0)), Item("flag_bit_31", s, None, (18, 0)),
             Item("src_len_over_the_limit", s, None, (18, 0)),
             Item("empty_source", b"", None, (st_empty, len(d_empty) if st_empty == 0 else 0)),
             Item("dst_fields_of_no_meaning", s, None, good), Item("dst_fields_of_no_meaning_limit", s, len(data), good),
             Item("plain", s, None, good), Item("limit_one_short", s, len(data) - 1, (2, 0))]
    flags = [2, 1 | 4, 1 << 31, None, None, None, None, None, None]
    src_len = [None, None, None, MAX_STREAM_LEN + 1, None, None, None, None, None]
    dst = [(0, 0)] * 5 + [(1 << 63, 1 << 40), (1 << 63, 1 << 40), (0, 0), (0, 0)]
    _check(_call(gpu_ctx, items, dst=dst, flags=flags, src_len=src_len), items, "descriptor rules")
    # the call's own arguments
    import torch

    from zipc_amd import batch

    L = _lib.lib()
    dev = torch.device("cuda", 0)
    d_res = torch.full((16,), 0xEE, dtype=torch.uint8, device=dev)
    d_descs = batch.to_device(batch.make_descs([0], [len(s)], [0], [0]), dev)
    src = torch.from_numpy(np.frombuffer(s + b"\0" * 64, dtype=np.uint8).copy()).to(dev)
    torch.cuda.synchronize()
    for fn in (L.zipc_hip_inflate_size_batch, L.zipc_hip_zlib_size_batch):
        assert fn(gpu_ctx.handle, src.data_ptr(), d_descs.data_ptr(), d_res.data_ptr(), 0) == 0      # n_streams 0: OK,
        assert fn(gpu_ctx.handle, None, None, None, 0) == 18                                         # ... null descs / results are not
        assert fn(None, src.data_ptr(), d_descs.data_ptr(), d_res.data_ptr(), 1) == 18
        assert fn(gpu_ctx.handle, src.data_ptr(), None, d_res.data_ptr(), 1) == 18
        assert fn(gpu_ctx.handle, src.data_ptr(), d_descs.data_ptr(), None, 1) == 18
        assert fn(gpu_ctx.handle, src.data_ptr(), d_descs.data_ptr(), d_res.data_ptr(), 0x80000000) == 18
    gpu_ctx.synchronize()
    assert (d_res.cpu().numpy() == 0xEE).all(), "a refused or empty call wrote a result"


def _use_streams(oracle):
    """the streams the feature exists for: the recode tests' good ones (levels 0-3, 0 to 70 000 bytes, zlib's fixed and
    stored blocks) and four long ones as the oracle's deflate makes them at `Default"""
    out = [(c.name, c.stream, oracle.inflate(c.stream)) for c in recode_cases.good_cases()]
    for name, data in (("zeros_1MiB", bytes(1 << 20)), ("period1000_1MiB", (util.rand_bytes(1000, 5) * 1049)[:1 << 20]),
                       ("text_1MiB", util.text(1 << 20, 6)), ("random_300KiB", util.rand_bytes(300 << 10, 7))):
        st, s, _ = oracle.deflate(data, level=2)
        assert st == 0
        out.append((name, s, (0, data, 0)))
    assert all(st == 0 for _, _, (st, _, _) in out)
    return [(name, s, d) for name, s, (_, d, _) in out]


def test_sized_exactly_then_inflated(gpu_ctx, oracle):
    """size a ragged batch in one call, lay the destinations out with dst_cap == out_len exactly and no limit, inflate in
    one call: every stream OK, its bytes the oracle's, nothing written behind any dst_cap"""
    import torch

    from zipc_amd import batch

    streams = _use_streams(oracle)
    zeros = next(x for x in streams if x[0] == "zeros_1MiB")
    assert len(zeros[2]) > 8 * 3 * len(zeros[1]), "the guess of three times the input would have held"
    items = [Item(name, s, None, (0, len(d))) for name, s, d in streams]
    res = _call(gpu_ctx, items)
    _check(res, items, "the use")
    dev = torch.device("cuda", 0)
    n = len(items)
    caps = [int(v) for v in res["out_len"]]
    assert 0 in caps and max(caps) == 1 << 20
    slots = [(k + 255) // 256 * 256 + 256 for k in caps]
    dst_off = np.cumsum([0] + slots[:-1]).astype(np.uint64)
    lens = [len(it.stream) for it in items]
    descs = batch.make_descs(np.cumsum([0] + lens[:-1]).astype(np.uint64), lens, dst_off, caps)
    src = torch.from_numpy(np.frombuffer(b"".join(it.stream for it in items) + b"\0" * 64, dtype=np.uint8).copy()).to(dev)
    dst = torch.full((int(sum(slots)) + 256,), 0xA5, dtype=torch.uint8, device=dev)
    d_res = torch.full((n * 16,), 0xEE, dtype=torch.uint8, device=dev)
    batch.inflate_batch(gpu_ctx, src, dst, batch.to_device(descs, dev), d_res, n, max(caps), 0)
    got = batch.results_from_device(d_res)
    out = dst.cpu().numpy()
    for i, (name, _, d) in enumerate(streams):
        o = int(dst_off[i])
        assert (int(got["status"][i]), int(got["out_len"][i])) == (0, len(d)), (name, got[i])
        assert out[o:o + caps[i]].tobytes() == d, (name, "bytes")
        assert (out[o + caps[i]:o + slots[i]] == 0xA5).all(), (name, "wrote past its dst_cap")


def test_zlib_size_batch(gpu_ctx, oracle):
    """zlib_cases.decompress_cases() in one call: the header's verdict, or the size of the body; a stream the oracle
    rejects for its Adler-32 (status 6) is sized OK"""
    pairs = size_cases.zlib_expectations()
    assert any(st0 == 6 and want[0] == 0 for _, want, st0 in pairs)
    items = [Item(c.name, c.stream, c.limit, want) for c, want, _ in pairs]
    flags = [(c.flags | (1 if c.limit is not None else 0)) if c.flags else None for c, _, _ in pairs]
    dst = [(0, c.cap) for c, _, _ in pairs]
    _check(_call(gpu_ctx, items, zlib=True, dst=dst, flags=flags), items, "zlib_size_batch")
    _check(_call(gpu_ctx, items, zlib=True, dst=dst, flags=flags, sync=False), items, "zlib_size_batch, sync=False")


def test_one_host_stream(gpu_ctx, oracle):
    """zipc_hip_inflate_size and its Python form on three streams, with and without a limit: OK with the length, the
    reference's two messages"""
    from zipc_amd import _lib, zipc_deflate as Z

    L = _lib.lib()
    by_name = {s.name: s for s in size_cases.rule_cases()}
    text = util.text(1 << 20, 6)
    long_ok = oracle.deflate(text, level=2)[1]
    picks = [Item("text_1MiB", long_ok, None, (0, len(text))), Item("text_1MiB_limit", long_ok, len(text), (0, len(text))),
             Item("text_1MiB_limit_short", long_ok, len(text) - 1, (2, 0)),
             by_name["dist_out_plus1/c"], by_name["limit_one_short/a"], by_name["limit_exact/a"], by_name["dist_32768_at_32768/e"]]
    assert {p.want[0] for p in picks} == {0, 1, 2}
    for it in picks:
        ol = C.c_size_t(0xEEEE)
        st = L.zipc_hip_inflate_size(gpu_ctx.handle, it.stream, len(it.stream), int(it.limit is not None), it.limit or 0, C.byref(ol))
        assert (st, ol.value) == it.want, (it.name, st, ol.value, it.want)
        r = Z.inflate_size(it.stream, decompressed_size=it.limit, ctx=gpu_ctx)
        if it.want[0] == 0:
            assert r.is_ok() and r.value == it.want[1], it.name
        else:
            assert not r.is_ok() and r.error == L.zipc_hip_strerror(it.want[0]).decode(), (it.name, r.error)
    assert L.zipc_hip_inflate_size(gpu_ctx.handle, long_ok, len(long_ok), 0, 0, None) == 18
    assert L.zipc_hip_inflate_size(None, long_ok, len(long_ok), 0, 0, C.byref(C.c_size_t())) == 18
