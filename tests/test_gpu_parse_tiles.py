"""lz_parse_wave (deflate.hip) runs a tile of 64 positions in one of two forms, chosen by parse_tile_interior
(zipc_amd/csrc/parse_tile.h; the predicate itself: tests/test_parse_tile_form.py).  Here the kernels: deflate_batch against the
oracle, stream by stream, at the lengths where the choice changes -- the tile multiples, the word edges + 3 and + 67 behind
them, the length at which the load three tiles ahead first fits -- and with a block cut at every offset of a literal, a
deferral and a match from source byte 65534, by a wave per stream and by a wave per segment."""
import functools
import os
import zipfile
import zlib

import numpy as np
import pytest

import util

LENGTHS = list(range(0, 5)) + [ln for lo in (60, 124, 188, 252, 316, 380) for ln in range(lo, lo + 13)]
KINDS = ("nibbles", "text", "run", "period2", "period3", "period64", "random")
CUT_STREAMS, CUT_LEN = 320, 65536 + 320


@functools.lru_cache(maxsize=None)
def _catalogue():
    """[(kind, length, bytes)]: every kind at every length"""
    from zipc_amd import synth

    docs = zipfile.ZipFile(os.path.join(util.GOLDEN, "zip-docs.zip"))
    text = docs.read("zip-docs/APPNOTE.TXT")
    out = []
    for i, ln in enumerate(LENGTHS):
        pat = util.rand_bytes(64, 100 + i)
        by_kind = {
            "nibbles": synth.stream_bytes_np(2, i, ln, 4).tobytes(),
            "text": text[1000 * i:1000 * i + ln],
            "run": bytes([i % 251 + 1]) * ln,  # steps of 258: whole tiles jumped over, and the loads behind a jump
            "period2": (pat[:2] * ln)[:ln], "period3": (pat[:3] * ln)[:ln], "period64": (pat * 8)[:ln],
            "random": util.rand_bytes(ln, 200 + i),  # no matches: every lane a literal
        }
        out += [(k, ln, by_kind[k]) for k in KINDS]
    assert all(len(s) == ln for _, ln, s in out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _cut_streams():
    """Stream k: 4-bit symbols with a copy of 40 earlier bytes planted at 65534 - 300 + k and the two bytes in front of it
    changed (so that the copy cannot start earlier, and the positions in front of it -- which match here and there, as
    4-bit symbols do -- are given up for it: a deferral's literals in front of the match).  Over the 320 streams the
    literals, the deferral and the match lie at every offset from source byte 65534, where the first block ends."""
    from zipc_amd import synth

    out = []
    for k in range(CUT_STREAMS):
        b = bytearray(synth.stream_bytes_np(2, 1000 + k, CUT_LEN, 4).tobytes())
        at = 65534 - 300 + k
        frm = at - (3000 + 7 * k)
        b[at:at + 40] = b[frm:frm + 40]
        for j in (1, 2):
            b[at - j] = (b[frm - j] + 1 + (k + j) % 15) % 16
        out.append(("cut%d" % k, CUT_LEN, bytes(b)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _cut_runs():
    return tuple(("cutrun%d" % k, CUT_LEN, bytes([k % 251 + 1]) * CUT_LEN) for k in range(CUT_STREAMS))


_WANT = {}  # (bytes, level) -> the oracle's (status, stream, CRC-32): computed once, shared by the forms


def _want(oracle, data, level):
    key = (data, level)
    if key not in _WANT:
        _WANT[key] = oracle.deflate(data, level=level, crc_op=oracle.CRC_CRC32)
    return _WANT[key]


def _deflate_and_compare(ctx, oracle, named, level, profile=False):
    """one deflate_batch over `named` [(kind, length, bytes)]; every stream's status, length, CRC-32 and bytes against the
    oracle.  Returns the names of the kernels launched (profile=True)."""
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
    launched = None
    if profile:
        ctx.set_profiling(True)
        ctx.reset_kernel_times()
    try:
        batch.deflate_batch(ctx, src, dst, batch.to_device(descs, dev), d_res, len(streams), max(lens), int(sum(lens)), level, 1)
    finally:
        if profile:
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


@pytest.mark.gpu
@pytest.mark.parametrize("level", [1, 2, 3])
def test_streams_around_the_tile_and_word_edges_equal_oracle(gpu_ctx, oracle, level):
    """thousands of short streams: a wave per stream (lz_parse_kernel), the edge form and -- from 259 bytes on -- the
    interior form for the first tiles"""
    named = list(_catalogue()) * 4  # (more than 2048 streams: never a wave per segment, whatever the lengths)
    assert len(named) > 2048
    launched = _deflate_and_compare(gpu_ctx, oracle, named, level, profile=True)
    assert "lz_parse" in launched and "lz_parse_spec" not in launched, sorted(launched)


@pytest.mark.gpu
@pytest.mark.parametrize("level", [1, 2, 3])
@pytest.mark.parametrize("form", ["segments", "streams"])
@pytest.mark.parametrize("data", ["planted", "runs"])
def test_a_block_cut_at_every_offset_equals_oracle(gpu_ctx, oracle, level, form, data):
    """the cut streams as a batch of 320 (a wave per segment: forms.h, n <= 2048) and followed by 1800 streams of 5 bytes
    (more than 2048 streams: a wave per stream, which cuts the blocks itself)"""
    named = list(_cut_streams() if data == "planted" else _cut_runs())
    if form == "streams":
        named = named + [("five", 5, bytes([65 + j % 7, 66, 67, 68 + j % 3, 69])) for j in range(1800)]
    launched = _deflate_and_compare(gpu_ctx, oracle, named, level, profile=True)
    if form == "segments":
        assert "lz_parse_spec" in launched and "lz_parse" not in launched, sorted(launched)
    else:
        assert "lz_parse" in launched and "lz_parse_spec" not in launched, sorted(launched)
