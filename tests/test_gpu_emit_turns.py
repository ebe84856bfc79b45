"""deflate_emit_wave (deflate.hip) takes a block's symbols by turns, most of them in an interior form: four symbols a lane by
one load in the histogram, two symbols a lane merged into one item in the packer (tests/emit_cases.py has the sizes and the
inputs).  Here the kernels: deflate_batch against the oracle, stream by stream, with blocks whose symbol counts lie at every
residue of a tile of pairs and on both sides of every turn's multiple, with neighbouring symbols of more than 64 bits, with
the benchmark's own two-block streams, and all of it again by the kernels that take a block, or a part of a block, a wave."""
import zlib

import numpy as np
import pytest

import emit_cases as E

_WANT = {}  # (bytes, level) -> the oracle's (status, stream, CRC-32): computed once, shared by the forms
FIVES = tuple(("five", 5, bytes([65 + j % 7, 66, 67, 68 + j % 3, 69])) for j in range(2100))


def _want(oracle, data, level):
    key = (data, level)
    if key not in _WANT:
        _WANT[key] = oracle.deflate(data, level=level, crc_op=oracle.CRC_CRC32)
    return _WANT[key]


def _deflate_and_compare(ctx, oracle, named, level):
    """one deflate_batch over `named` [(kind, length, bytes)] with kernel times on; every stream's status, length, CRC-32 and
    bytes against the oracle.  Returns the names of the kernels launched."""
    import torch

    from zipc_amd import batch

    dev = torch.device("cuda", 0)
    streams = [s for _, _, s in named]
    lens = [len(s) for s in streams]
    src_off = np.cumsum([0] + lens[:-1]).astype(np.uint64)
    caps = [batch.deflate_bound(n) for n in lens]
    slots = [(c + 255) // 256 * 256 for c in caps]
    dst_off = np.cumsum([0] + slots[:-1]).astype(np.uint64)
    descs = batch.make_descs(src_off, lens, dst_off, caps)
    src = torch.from_numpy(np.frombuffer(b"".join(streams) + b"\0" * 64, dtype=np.uint8).copy()).to(dev)
    dst = torch.zeros(int(sum(slots)) + 256, dtype=torch.uint8, device=dev)
    d_res = torch.zeros(len(streams) * 16, dtype=torch.uint8, device=dev)
    ctx.set_profiling(True)
    ctx.reset_kernel_times()
    try:
        batch.deflate_batch(ctx, src, dst, batch.to_device(descs, dev), d_res, len(streams), max(lens), int(sum(lens)), level, 1)
    finally:
        launched = {k for k, (n, ms) in ctx.kernel_times().items() if n}
        ctx.set_profiling(False)
    res = batch.results_from_device(d_res)
    out = dst.cpu().numpy()
    for i, (kind, ln, s) in enumerate(named):
        st0, c0, crc0 = _want(oracle, s, level)
        where = ("stream %d" % i, "length %d" % ln, kind, "level %d" % level)
        assert int(res["status"][i]) == st0 == 0, where
        assert int(res["out_len"][i]) == len(c0), where
        assert int(res["checksum"][i]) == crc0 == zlib.crc32(s), where
        o = int(dst_off[i])
        assert out[o:o + len(c0)].tobytes() == c0, where
    return launched


def _a_wave_per_stream(launched):
    assert "deflate_emit" in launched and "deflate_pack" not in launched and "deflate_plan" not in launched, sorted(launched)


def _assert_long_pairs(oracle, level):
    """the oracle's stream of the long-pairs input has neighbours of more than 64 bits at both parities of the symbol index"""
    st, c, _ = _want(oracle, E.long_pairs_stream(), level)
    found = E.long_pairs(E.walk(c))
    assert st == 0 and {k & 1 for _, k in found} == {0, 1} and len(found) >= 8, found


@pytest.mark.gpu
@pytest.mark.parametrize("level", E.LEVELS)
def test_blocks_at_every_turn_and_pair_edge_equal_oracle(gpu_ctx, oracle, level):
    """thousands of short streams, a wave per stream: blocks of every symbol count up to 2 Ki"""
    named = E.short_streams()
    assert E.reaches_the_edges(oracle, named, level) == []
    assert len(named) > 2048
    _a_wave_per_stream(_deflate_and_compare(gpu_ctx, oracle, list(named), level))


@pytest.mark.gpu
@pytest.mark.parametrize("level", E.LEVELS)
def test_pairs_over_64_bits_and_the_benchmarks_streams_equal_oracle(gpu_ctx, oracle, level):
    """a wave per stream (more than 2048 streams in the call): the stream whose neighbours exceed 64 bits, 64 streams of
    65536 bytes of 4-bit symbols -- two blocks, the second a handful of symbols -- and 64 of 65536 + 320"""
    _assert_long_pairs(oracle, level)
    named = [("long_pairs", 60000, E.long_pairs_stream())] + list(E.bench_shape()) + list(FIVES)
    _a_wave_per_stream(_deflate_and_compare(gpu_ctx, oracle, named, level))


@pytest.mark.gpu
@pytest.mark.parametrize("level", E.LEVELS)
@pytest.mark.parametrize("form", ["parts", "blocks"])
def test_the_same_by_a_wave_per_block_or_part_equal_oracle(gpu_ctx, oracle, level, form):
    """at most 2048 streams, one of them long: deflate_plan and deflate_pack, by parts of EMIT_PART symbols (deflate_bits)
    while the call has few blocks, else a wave per block -- with a stream for every symbol count the wave-per-stream test
    is held to (emit_cases.streams_by_count: chosen by the oracle's counts, the same two conditions asserted), and blocks
    of 8192 +- 2 and 16384 +- 2 symbols, whose last part is two symbols, or none, or two short of a whole one"""
    _assert_long_pairs(oracle, level)
    for _, n, s in E.part_edge_streams():
        st, _, _, blocks = oracle.deflate_trace(s, level=level)
        assert st == 0 and [(int(b.kind), int(b.n_syms) - 1) for b in blocks] == [(2, n)], n
    named = [("long_pairs", 60000, E.long_pairs_stream())] + list(E.bench_shape()) + list(E.part_edge_streams())
    by_count = list(E.streams_by_count(oracle))  # every residue and every turn's edge, as the oracle counts: asserted here
    assert E.reaches_the_edges(oracle, by_count, level) == []
    named += by_count
    if form == "blocks":  # more than 1024 streams of two block slots each: no parts
        named += list(E.short_streams()[3401::2]) + list(E.short_streams()[1:3401:5])
    assert len(named) * 2 <= 2048 if form == "parts" else 1024 < len(named) <= 2048, len(named)
    launched = _deflate_and_compare(gpu_ctx, oracle, named, level)
    assert "deflate_plan" in launched and "deflate_pack" in launched and "deflate_emit" not in launched, sorted(launched)
    assert ("deflate_bits" in launched) == (form == "parts"), sorted(launched)
