"""Sizing by blocks on the MI355X: zipc_hip_inflate_size_blocks_batch / zipc_hip_zlib_size_blocks_batch, and
zipc_hip_inflate_size, which goes through the former -- the long streams of a call sized by the block path's find, dry run
and chain and a head walk, the rest by their one waves.  Every expectation is the oracle's (tests/size_cases.py; for
tests/size_blocks_cases.py's streams oracle.inflate here, for lengths the plain bytes as built); result slots are poisoned
with 0xEE before every call, and the source arena and the descriptors are compared with what was uploaded afterwards."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import size_blocks_cases as cases
import size_cases
import zlib_cases

pytestmark = pytest.mark.gpu

Item = size_cases.Sized  # name, stream, limit, want = (status, out_len)
BLOCKS_ON = os.environ.get("ZIPC_HIP_INFLATE_BLOCKS") != "0"
ALL_ONES = 0xFFFFFFFFFFFFFFFF


def _call(gpu_ctx, items, form="blocks", dst=None, flags=None):
    """one sizing call over items: the results as a numpy record array.  form: "blocks" / "zlib_blocks" (the new forms),
    "one_wave" (zipc_hip_inflate_size_batch); dst: (dst_off, dst_cap) per stream (default 0, 0: they are not to be looked
    at); flags: overrides per stream, or None"""
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
    arena = np.frombuffer(b"".join(it.stream for it in items) + b"\0" * 64, dtype=np.uint8).copy()
    src = torch.from_numpy(arena).to(dev)
    d_descs = batch.to_device(descs, dev)
    d_res = torch.full((n * 16,), 0xEE, dtype=torch.uint8, device=dev)
    fn = {"blocks": batch.inflate_size_blocks_batch, "zlib_blocks": batch.zlib_size_blocks_batch, "one_wave": batch.inflate_size_batch}[form]
    fn(gpu_ctx, src, d_descs, d_res, n)
    res = batch.results_from_device(d_res)
    assert np.array_equal(src.cpu().numpy(), arena), "the source arena changed"
    assert np.array_equal(batch.to_device(descs, "cpu").numpy(), d_descs.cpu().numpy()), "the descriptors changed"
    return res


def _check(res, items, what):
    for i, it in enumerate(items):
        got = (int(res["status"][i]), int(res["checksum"][i]), int(res["out_len"][i]))
        assert got == (it.want[0], 0, it.want[1]), (what, it.name, got, it.want)


def _host(gpu_ctx, it):
    """zipc_hip_inflate_size of one item: (status, out_len)"""
    from zipc_amd import _lib

    ol = C.c_size_t(0xEEEE)
    st = _lib.lib().zipc_hip_inflate_size(gpu_ctx.handle, it.stream, len(it.stream), int(it.limit is not None), it.limit or 0, C.byref(ol))
    return st, ol.value


def _want(oracle, stream, limit=None):
    st, d, _ = oracle.inflate(stream, decompressed_size=limit)
    return st, len(d) if st == 0 else 0


# ---- 1. the rule cases inside long streams

def test_rule_cases_inside_long_streams_by_the_host_form(gpu_ctx, oracle):
    """the 73 /e cases through zipc_hip_inflate_size: status and out_len as size_cases has them; the accepted ones go by
    blocks, by chains of at least the four blocks the decode's have (tests/test_gpu_inflate_rules.py)"""
    long_ = size_cases.long_rule_cases()
    assert len(long_) == 73
    for it in long_:
        assert _host(gpu_ctx, it) == it.want, it.name
        if it.want[0] == 0 and BLOCKS_ON:
            assert gpu_ctx.last_size_blocks() >= 4, (it.name, gpu_ctx.last_size_blocks())


def test_rule_table_in_one_call(gpu_ctx, oracle):
    """all 73 together with the 413 short cases in ONE call of the new batch form"""
    items = size_cases.long_rule_cases() + size_cases.short_rule_cases()
    assert len(items) == 486
    _check(_call(gpu_ctx, items), items, "rule table, one call")
    print("rule table in one call: %d blocks sized streams" % gpu_ctx.last_size_blocks())  # (which streams go: the model's choice)


# ---- 2. the head

@functools.lru_cache(maxsize=None)
def _head_items():
    import oracle

    out = []
    for c in cases.head_cases():
        want = _want(oracle, c.stream)
        assert (want[0] == 0) == (c.plain is not None) and (c.plain is None or want[1] == len(c.plain)), (c.name, "the oracle left its case")
        out.append(Item(c.name, c.stream, None, want))
    return tuple(out)


HEAD_STATUS = {"dynamic_dist_out_plus1": 1, "dynamic_dist_eq_out": 0, "fixed_dist_out_plus1": 1, "fixed_dist_eq_out": 0,
               "stored_32767_then_dist_32768": 1, "stored_32768_then_dist_32768": 0, "literals_to_32760_then_dist_32768": 1,
               "head_sees_the_final_block": 0}


def test_the_head_makes_the_distance_check(gpu_ctx, oracle):
    """the one check the dry runs leave out, at every place it can fail: the new batch form (each stream in a call of its
    own, and all in one), the host form and the one-wave form say the same, and that is the oracle's word"""
    items = _head_items()
    assert {it.name: it.want[0] for it in items} == HEAD_STATUS  # (what the issue names for each)
    assert dict((it.name, it.want) for it in items)["head_sees_the_final_block"] == (0, 24000)
    for it in items:
        _check(_call(gpu_ctx, [it]), [it], "blocks, alone")
        n_alone = gpu_ctx.last_size_blocks()
        assert _host(gpu_ctx, it) == it.want, ("host", it.name)
        if it.want[0] == 0 and BLOCKS_ON:
            assert n_alone > 0 and gpu_ctx.last_size_blocks() > 0, (it.name, n_alone, gpu_ctx.last_size_blocks())
        if it.want[0] != 0:
            assert n_alone == 0 and gpu_ctx.last_size_blocks() == 0, (it.name, "an error is the one wave's to report")
    _check(_call(gpu_ctx, items), items, "blocks, one call")
    _check(_call(gpu_ctx, items, form="one_wave"), items, "one wave")
    assert gpu_ctx.last_size_blocks() == 0  # (the one-wave form: no stream by blocks)


# ---- 3. encoders

@functools.lru_cache(maxsize=None)
def _encoder_items():
    import oracle

    out = []
    for c in cases.encoder_streams():
        assert _want(oracle, c.stream) == (0, cases.N) and len(c.plain) == cases.N, (c.name, "the oracle left its case")
        out.append(Item(c.name, c.stream, None, (0, cases.N)))
    assert len(out) == 22
    return tuple(out)


def test_encoders(gpu_ctx, oracle):
    """every stream OK with length 400 000; sized again with a limit of the exact length: OK; with that limit minus one:
    status 2, out_len 0.  The oracle's and zlib's dynamic streams of text go by blocks."""
    for it in _encoder_items():
        assert _host(gpu_ctx, it) == (0, cases.N), it.name
        src, enc = it.name.split("/")
        if src == "text" and enc in cases.BY_BLOCKS and BLOCKS_ON:
            assert gpu_ctx.last_size_blocks() > 0, it.name
        assert _host(gpu_ctx, Item(it.name, it.stream, cases.N, None)) == (0, cases.N), (it.name, "limit exact")
        assert _host(gpu_ctx, Item(it.name, it.stream, cases.N - 1, None)) == (2, 0), (it.name, "limit one short")
        assert _want(oracle, it.stream, cases.N - 1) == (2, 0)
        assert gpu_ctx.last_size_blocks() == 0, (it.name, "an error is the one wave's to report")


# ---- 4. one call of everything

def _everything(oracle):
    """[(Item, flags override or None, (dst_off, dst_cap), plain or None)]"""
    rows = [(it, None, (0, 0), c.plain) for it, c in zip(_encoder_items(), cases.encoder_streams())]
    for c in cases.damaged_streams():
        rows.append((Item(c.name, c.stream, None, _want(oracle, c.stream)), None, (0, 0), None))
    assert [r[0].want[0] for r in rows[-2:]] == [1, 1]
    short = size_cases.short_rule_cases()[:300]
    rows += [(it, None, (0, 0), None) for it in short]
    rows.append((Item("empty_source", b"", None, _want(oracle, b"")), None, (0, 0), None))
    long_ok = _encoder_items()[0]
    rows.append((Item("stray_flag_bit", long_ok.stream, None, (18, 0)), 4, (0, 0), None))
    rows.append((Item("dst_fields_all_ones", long_ok.stream, None, long_ok.want), None, (ALL_ONES, ALL_ONES), None))
    # (in between the short ones, so that the long streams do not all stand first)
    return rows[:5] + rows[24:200] + rows[5:24] + rows[200:]


def test_one_call_of_everything(gpu_ctx, oracle):
    rows = _everything(oracle)
    items = [r[0] for r in rows]
    assert len(items) == 22 + 2 + 300 + 3
    res = _call(gpu_ctx, items, dst=[r[2] for r in rows], flags=[r[1] for r in rows])
    _check(res, items, "everything")
    if BLOCKS_ON:
        assert gpu_ctx.last_size_blocks() > 0


def test_one_call_of_everything_in_zlib_containers(gpu_ctx, oracle):
    """the same call through zipc_hip_zlib_size_blocks_batch, every stream in its container: the expectation is
    size_cases.expect_zlib_size's"""
    rows = _everything(oracle)
    zitems, flags = [], []
    for it, fl, _, plain in rows:
        z = cases.zlib_wrap(it.stream, plain)
        case = zlib_cases.Case(it.name, z, it.limit, 0, fl or 0)
        zitems.append(Item(it.name, z, it.limit, size_cases.expect_zlib_size(case)))
        flags.append(fl)
    by_name = {it.name: it for it in zitems}
    assert by_name["text/oracle-default"].want == (0, cases.N) and by_name["stray_flag_bit"].want == (18, 0)
    assert by_name["text_damaged_in_a_middle_block"].want[0] == 1 and by_name["dst_fields_all_ones"].want == (0, cases.N)
    res = _call(gpu_ctx, zitems, form="zlib_blocks", dst=[r[2] for r in rows], flags=flags)
    _check(res, zitems, "everything, zlib")
    if BLOCKS_ON:
        assert gpu_ctx.last_size_blocks() > 0


# ---- 5. counters

def test_counters_and_the_caller_without_a_size(gpu_ctx, oracle):
    """last_inflate_blocks is the same before and after a sizing call that went by blocks; Z.inflate(raw) with no size on
    a 400 000-byte stream of text returns the bytes (sized first, decoded once)"""
    from zipc_amd import zipc_deflate as Z

    text = next(c for c in cases.encoder_streams() if c.name == "text/oracle-default")
    got = Z.inflate(text.stream, decompressed_size=cases.N, ctx=gpu_ctx).get_ok()
    assert got == text.plain
    before = gpu_ctx.last_inflate_blocks()
    if BLOCKS_ON:
        assert before > 0
    it = Item(text.name, text.stream, None, (0, cases.N))
    assert _host(gpu_ctx, it) == it.want
    n_host = gpu_ctx.last_size_blocks()
    _check(_call(gpu_ctx, [it, it]), [it, it], "two long streams")
    if BLOCKS_ON:
        assert n_host > 0 and gpu_ctx.last_size_blocks() == 2 * n_host
    assert gpu_ctx.last_inflate_blocks() == before, "a sizing call touched zipc_hip_last_inflate_blocks"
    assert Z.inflate(text.stream, ctx=gpu_ctx).get_ok() == text.plain
    r = Z.inflate(cases.damaged_streams()[1].stream, ctx=gpu_ctx)
    assert not r.is_ok() and r.error == "Corrupted data stream"
