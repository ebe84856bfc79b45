"""The block path's front on the MI355X: the decode (inflate_blocks_group) and the sizing (inflate_size_blocks_group) of one
stream go through the same find-to-chain launches (inflate.hip BlocksRun::front), and only the sizing's own kernels stand
beside them.  The launch counts are zipc_hip_kernel_times' of one call each; the relations between them follow from the
code (a single stream is a single group), nothing here is recorded from a run.

The streams are the five encodings of text that must go by blocks (size_blocks_cases.BY_BLOCKS), 400 000 plain bytes each,
and symbols/oracle-default.  All five streams of text take the explore round: their chains come to a block no header search
lists (the empty stored block behind each of zlib's full flushes, a fixed block among the oracle's).  The oracle's stream
of 4-bit symbols, the smallest of size_blocks_cases.encoder_streams() that goes by blocks as a chain of dynamic blocks
alone, supplies the other arm: its first chain walk is through.  Which arm each took is printed (pytest -s)."""
import ctypes as C
import os

import pytest

import size_blocks_cases as cases

pytestmark = pytest.mark.gpu

FRONT = ("inflate_find_headers", "inflate_find_lengths", "inflate_blocks_dry", "inflate_sort_blocks", "inflate_chain", "inflate_explore")
DECODE_ONLY = ("inflate_tok_init", "inflate_blocks_token", "inflate_resolve", "inflate_gather")


def _launches(times):
    return {k: n for k, (n, ms) in times.items() if n}


def _one_call_each(gpu_ctx, c):
    """the launches of one decode with the exact size and of one sizing of stream c, each alone: (decode, sizing)"""
    from zipc_amd import _lib
    from zipc_amd import zipc_deflate as Z

    gpu_ctx.set_profiling(True)
    try:
        gpu_ctx.reset_kernel_times()
        assert Z.inflate(c.stream, decompressed_size=cases.N, ctx=gpu_ctx).get_ok() == c.plain, c.name
        decode = _launches(gpu_ctx.kernel_times())
        assert gpu_ctx.last_inflate_blocks() > 0, c.name
        gpu_ctx.reset_kernel_times()
        ol = C.c_size_t(0xEEEE)
        st = _lib.lib().zipc_hip_inflate_size(gpu_ctx.handle, c.stream, len(c.stream), 0, 0, C.byref(ol))
        assert (st, ol.value) == (0, cases.N), c.name
        sizing = _launches(gpu_ctx.kernel_times())
        assert gpu_ctx.last_size_blocks() > 0, c.name
    finally:
        gpu_ctx.set_profiling(False)
    return decode, sizing


@pytest.mark.skipif(os.environ.get("ZIPC_HIP_INFLATE_BLOCKS") == "0", reason="the block path is turned off")
def test_decode_and_sizing_share_the_front(gpu_ctx):
    names = ["text/" + enc for enc in cases.BY_BLOCKS] + ["symbols/oracle-default"]
    streams = [c for c in cases.encoder_streams() if c.name in names]
    assert len(streams) == 6 and all(len(c.plain) == cases.N for c in streams)
    explored = {}
    for c in streams:
        decode, sizing = _one_call_each(gpu_ctx, c)
        print("%s: decode %s | sizing %s" % (c.name, decode, sizing))
        for what, t in (("decode", decode), ("sizing", sizing)):
            n = {k: t.get(k, 0) for k in FRONT}
            assert n["inflate_find_headers"] == n["inflate_find_lengths"] == n["inflate_blocks_dry"] == 1, (c.name, what, n)
            assert n["inflate_explore"] in (0, 1), (c.name, what, n)
            assert n["inflate_sort_blocks"] == n["inflate_chain"] == 1 + n["inflate_explore"], (c.name, what, n)
        assert {k: decode.get(k, 0) for k in FRONT} == {k: sizing.get(k, 0) for k in FRONT}, (c.name, decode, sizing)
        assert sizing.get("inflate_size_head") == 1 and sizing.get("inflate_size_verdict") == 1, (c.name, sizing)
        stray = [k for k in sizing if k in DECODE_ONLY or k.startswith("inflate_adler_")]
        assert not stray, (c.name, "the sizing ran the decode's second half", stray)
        explored[c.name] = sizing.get("inflate_explore", 0)
    print("explore rounds:", explored)
    assert 1 in explored.values() and 0 in explored.values(), explored
