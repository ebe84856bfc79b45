"""Device-resident batch forms (zipc_hip_inflate_batch / _deflate_batch / _checksum_device / _checksum_batch).

torch is used only as the owner of device memory (uint8 arenas, descriptor and
result arrays); the work itself is enqueued by libzipc_hip.so on the context's
HIP stream.  Descriptors are numpy structured arrays with the layout of
zipc_hip_stream_desc / zipc_hip_stream_result (include/zipc_hip.h).
"""
from __future__ import annotations

import numpy as np

import ctypes as C

from ._lib import CRC_NOP, OK, STREAM_EXPECT_CRC32, STREAM_HAS_LIMIT, ChecksumResult, Context, lib

DESC_DTYPE = np.dtype([("src_off", "<u8"), ("src_len", "<u8"), ("dst_off", "<u8"),
                       ("dst_cap", "<u8"), ("limit", "<u8"), ("flags", "<u4"),
                       ("reserved", "<u4")])
RESULT_DTYPE = np.dtype([("status", "<u4"), ("checksum", "<u4"), ("out_len", "<u8")])
assert DESC_DTYPE.itemsize == 48 and RESULT_DTYPE.itemsize == 16
# zipc_hip_prefix_result: ended 1 -- the stream's final block ended within its room; 0 -- cut at dst_cap, or an error
PREFIX_RESULT_DTYPE = np.dtype([("status", "<u4"), ("ended", "<u4"), ("out_len", "<u8")])
assert PREFIX_RESULT_DTYPE.itemsize == 16
# zipc_hip_extent_result: RESULT_DTYPE's fields, then src_used -- the source bytes the stream took (0 unless OK)
EXTENT_RESULT_DTYPE = np.dtype([("status", "<u4"), ("checksum", "<u4"), ("out_len", "<u8"), ("src_used", "<u8"),
                                ("reserved", "<u8")])
assert EXTENT_RESULT_DTYPE.itemsize == 32
# zipc_hip_recode_desc / zipc_hip_recode_result
RECODE_DESC_DTYPE = np.dtype([("src_off", "<u8"), ("src_len", "<u8"), ("mid_off", "<u8"), ("mid_cap", "<u8"),
                              ("dst_off", "<u8"), ("dst_cap", "<u8"), ("limit", "<u8"), ("flags", "<u4"),
                              ("expect_crc32", "<u4")])
RECODE_RESULT_DTYPE = np.dtype([("status", "<u4"), ("checksum", "<u4"), ("out_len", "<u8"), ("mid_len", "<u8"),
                                ("stage", "<u4"), ("reserved", "<u4")])
assert RECODE_DESC_DTYPE.itemsize == 64 and RECODE_RESULT_DTYPE.itemsize == 32
# zipc_hip_packed_result
PACKED_RESULT_DTYPE = np.dtype([("status", "<u4"), ("checksum", "<u4"), ("out_len", "<u8"), ("dst_off", "<u8"), ("reserved", "<u8")])
assert PACKED_RESULT_DTYPE.itemsize == 32
# zipc_hip_range / zipc_hip_checksum_result
RANGE_DTYPE = np.dtype([("off", "<u8"), ("len", "<u8")])
CHECKSUM_RESULT_DTYPE = np.dtype([("status", "<u4"), ("crc32", "<u4"), ("adler32", "<u4"), ("reserved", "<u4")])
assert RANGE_DTYPE.itemsize == 16 and CHECKSUM_RESULT_DTYPE.itemsize == 16


def make_descs(src_off, src_len, dst_off, dst_cap, limit=None) -> np.ndarray:
    n = len(src_off)
    d = np.zeros(n, dtype=DESC_DTYPE)
    d["src_off"], d["src_len"], d["dst_off"], d["dst_cap"] = src_off, src_len, dst_off, dst_cap
    if limit is not None:
        d["limit"] = limit
        d["flags"] = STREAM_HAS_LIMIT
    return d


def make_recode_descs(src_off, src_len, mid_off, mid_cap, dst_off, dst_cap, limit=None, expect_crc32=None) -> np.ndarray:
    """descriptors of zipc_hip_recode_batch; limit / expect_crc32: None, or one value per stream (the flag bits follow)"""
    d = np.zeros(len(src_off), dtype=RECODE_DESC_DTYPE)
    d["src_off"], d["src_len"], d["mid_off"], d["mid_cap"] = src_off, src_len, mid_off, mid_cap
    d["dst_off"], d["dst_cap"] = dst_off, dst_cap
    if limit is not None:
        d["limit"] = limit
        d["flags"] |= STREAM_HAS_LIMIT
    if expect_crc32 is not None:
        d["expect_crc32"] = expect_crc32
        d["flags"] |= STREAM_EXPECT_CRC32
    return d


def to_device(arr: np.ndarray, device):
    import torch

    return torch.from_numpy(arr.view(np.uint8).reshape(-1).copy()).to(device)


def results_from_device(t) -> np.ndarray:
    return t.cpu().numpy().view(RESULT_DTYPE).copy()


def _sync_torch(t):
    import torch

    torch.cuda.current_stream(t.device).synchronize()


def inflate_batch(ctx: Context, src, dst, descs_dev, results_dev, n_streams: int, max_dst_cap: int,
                  crc_op: int = CRC_NOP, sync: bool = True):
    """src/dst: uint8 cuda tensors (arenas); descs_dev/results_dev: uint8 cuda tensors."""
    if sync:
        _sync_torch(src)
    st = lib().zipc_hip_inflate_batch(ctx.handle, src.data_ptr(), dst.data_ptr(), descs_dev.data_ptr(),
                                      results_dev.data_ptr(), n_streams, max_dst_cap, crc_op)
    ctx.check(st)
    if sync:
        ctx.synchronize()


def deflate_batch(ctx: Context, src, dst, descs_dev, results_dev, n_streams: int, max_src_len: int,
                  total_src_len: int, level: int, crc_op: int = CRC_NOP, sync: bool = True):
    if sync:
        _sync_torch(src)
    st = lib().zipc_hip_deflate_batch(ctx.handle, src.data_ptr(), dst.data_ptr(), descs_dev.data_ptr(),
                                      results_dev.data_ptr(), n_streams, max_src_len, total_src_len,
                                      level, crc_op)
    ctx.check(st)
    if sync:
        ctx.synchronize()


def zlib_decompress_batch(ctx: Context, src, dst, descs_dev, results_dev, n_streams: int, max_dst_cap: int, sync: bool = True):
    """zipc_hip_zlib_decompress_batch: stream i of `src` is a whole zlib stream; header checks, inflate and the Adler-32
    comparison all on the device (the context's Adler-32 flavour: Context.set_adler_rfc1950)."""
    if sync:
        _sync_torch(src)
    st = lib().zipc_hip_zlib_decompress_batch(ctx.handle, src.data_ptr(), dst.data_ptr(), descs_dev.data_ptr(),
                                              results_dev.data_ptr(), n_streams, max_dst_cap)
    ctx.check(st)
    if sync:
        ctx.synchronize()


def zlib_compress_batch(ctx: Context, src, dst, descs_dev, results_dev, n_streams: int, max_src_len: int,
                        total_src_len: int, level: int, sync: bool = True):
    """zipc_hip_zlib_compress_batch: every stream's destination slot receives a whole zlib stream (out_len counts its six
    container bytes, checksum is the Adler-32); slots of zlib_bound(src_len) always fit."""
    if sync:
        _sync_torch(src)
    st = lib().zipc_hip_zlib_compress_batch(ctx.handle, src.data_ptr(), dst.data_ptr(), descs_dev.data_ptr(),
                                            results_dev.data_ptr(), n_streams, max_src_len, total_src_len, level)
    ctx.check(st)
    if sync:
        ctx.synchronize()


def inflate_size_batch(ctx: Context, src, descs_dev, results_dev, n_streams: int, sync: bool = True):
    """zipc_hip_inflate_size_batch: what every raw deflate stream of `src` inflates to -- status and out_len as
    inflate_batch reports them into a destination of the largest size, checksum 0 -- with nothing written: there is no
    destination arena, and dst_off / dst_cap of the descriptors are not looked at."""
    if sync:
        _sync_torch(src)
    st = lib().zipc_hip_inflate_size_batch(ctx.handle, src.data_ptr(), descs_dev.data_ptr(), results_dev.data_ptr(), n_streams)
    ctx.check(st)
    if sync:
        ctx.synchronize()


def zlib_size_batch(ctx: Context, src, descs_dev, results_dev, n_streams: int, sync: bool = True):
    """zipc_hip_zlib_size_batch: the same for whole zlib streams -- the header's verdict, or the size of the body.  The
    Adler-32 is not compared: a stream sized OK can still fail its checksum when it is decompressed."""
    if sync:
        _sync_torch(src)
    st = lib().zipc_hip_zlib_size_batch(ctx.handle, src.data_ptr(), descs_dev.data_ptr(), results_dev.data_ptr(), n_streams)
    ctx.check(st)
    if sync:
        ctx.synchronize()


def prefix_results_from_device(t) -> np.ndarray:
    return t.cpu().numpy().view(PREFIX_RESULT_DTYPE).copy()


def inflate_prefix_batch(ctx: Context, src, dst, descs_dev, results_dev, n_streams: int, sync: bool = True):
    """zipc_hip_inflate_prefix_batch: the first dst_cap bytes of every raw deflate stream of `src` -- a stream that
    inflate_batch reports OK is (OK, ended 1, its length), one it reports DST_TOO_SMALL is (OK, ended 0, dst_cap) with the
    first dst_cap bytes of its output in its room, every other status is the stream's own.  results_dev: a uint8 cuda
    tensor of PREFIX_RESULT_DTYPE records.  Always a wave per stream; nothing is read back."""
    if sync:
        _sync_torch(src)
    st = lib().zipc_hip_inflate_prefix_batch(ctx.handle, src.data_ptr(), dst.data_ptr(), descs_dev.data_ptr(),
                                             results_dev.data_ptr(), n_streams)
    ctx.check(st)
    if sync:
        ctx.synchronize()


def zlib_decompress_prefix_batch(ctx: Context, src, dst, descs_dev, results_dev, n_streams: int, sync: bool = True):
    """zipc_hip_zlib_decompress_prefix_batch: the same for whole zlib streams -- the header's verdict first; a stream that
    ended within its room has its Adler-32 compared (CHECKSUM on a mismatch), one that was cut has not."""
    if sync:
        _sync_torch(src)
    st = lib().zipc_hip_zlib_decompress_prefix_batch(ctx.handle, src.data_ptr(), dst.data_ptr(), descs_dev.data_ptr(),
                                                     results_dev.data_ptr(), n_streams)
    ctx.check(st)
    if sync:
        ctx.synchronize()


# zipc_hip_history: hist_len bytes of history lie in front of dst_off; the first block header starts at bit start_bit of the byte at src_off
HISTORY_DTYPE = np.dtype([("hist_len", "<u4"), ("start_bit", "<u4")])
assert HISTORY_DTYPE.itemsize == 8


def make_history(hist_len, start_bit=None) -> np.ndarray:
    h = np.zeros(len(hist_len), dtype=HISTORY_DTYPE)
    h["hist_len"] = hist_len
    if start_bit is not None:
        h["start_bit"] = start_bit
    return h


def _ptr(t):
    return t.data_ptr() if t is not None else None


def inflate_history_batch(ctx: Context, src, dst, descs_dev, hist_dev, results_dev, n_streams: int, max_dst_cap: int,
                          crc_op: int = CRC_NOP, sync: bool = True):
    """zipc_hip_inflate_history_batch: inflate_batch from a start point -- stream i begins at bit start_bit of its first byte and
    may copy from the hist_len bytes the caller has put in front of its room.  hist_dev: a uint8 cuda tensor of HISTORY_DTYPE
    records, or None (no stream has history).  Always a wave per stream."""
    if sync:
        _sync_torch(src)
    st = lib().zipc_hip_inflate_history_batch(ctx.handle, src.data_ptr(), dst.data_ptr(), descs_dev.data_ptr(), _ptr(hist_dev),
                                              results_dev.data_ptr(), n_streams, max_dst_cap, crc_op)
    ctx.check(st)
    if sync:
        ctx.synchronize()


def inflate_prefix_history_batch(ctx: Context, src, dst, descs_dev, hist_dev, results_dev, n_streams: int, sync: bool = True):
    """zipc_hip_inflate_prefix_history_batch: the first dst_cap bytes from the start point (PREFIX_RESULT_DTYPE records): the
    read of a chunk of a long stream from an access point"""
    if sync:
        _sync_torch(src)
    st = lib().zipc_hip_inflate_prefix_history_batch(ctx.handle, src.data_ptr(), dst.data_ptr(), descs_dev.data_ptr(), _ptr(hist_dev),
                                                     results_dev.data_ptr(), n_streams)
    ctx.check(st)
    if sync:
        ctx.synchronize()


def inflate_size_history_batch(ctx: Context, src, descs_dev, hist_dev, results_dev, n_streams: int, sync: bool = True):
    """zipc_hip_inflate_size_history_batch: what inflate_history_batch reports into the largest room, nothing written"""
    if sync:
        _sync_torch(src)
    st = lib().zipc_hip_inflate_size_history_batch(ctx.handle, src.data_ptr(), descs_dev.data_ptr(), _ptr(hist_dev),
                                                   results_dev.data_ptr(), n_streams)
    ctx.check(st)
    if sync:
        ctx.synchronize()


def zlib_decompress_dict_batch(ctx: Context, src, dst, descs_dev, results_dev, n_streams: int, max_dst_cap: int, dict_dev, dict_len: int,
                               sync: bool = True):
    """zipc_hip_zlib_decompress_dict_batch: whole zlib streams against one preset dictionary (a uint8 cuda tensor, or None with
    dict_len 0); the call writes the dictionary to [dst_off - dict_len, dst_off) of every stream that was made with it"""
    if sync:
        _sync_torch(src)
    st = lib().zipc_hip_zlib_decompress_dict_batch(ctx.handle, src.data_ptr(), dst.data_ptr(), descs_dev.data_ptr(),
                                                   results_dev.data_ptr(), n_streams, max_dst_cap, _ptr(dict_dev), dict_len)
    ctx.check(st)
    if sync:
        ctx.synchronize()


def zlib_size_dict_batch(ctx: Context, src, descs_dev, results_dev, n_streams: int, dict_dev, dict_len: int, sync: bool = True):
    """zipc_hip_zlib_size_dict_batch: the same streams sized, nothing written"""
    if sync:
        _sync_torch(src)
    st = lib().zipc_hip_zlib_size_dict_batch(ctx.handle, src.data_ptr(), descs_dev.data_ptr(), results_dev.data_ptr(), n_streams,
                                             _ptr(dict_dev), dict_len)
    ctx.check(st)
    if sync:
        ctx.synchronize()


def inflate_history(ctx: Context, raw: bytes, hist: bytes = b"", start_bit: int = 0, dst_cap: int = 0, limit=None, crc_op: int = CRC_NOP):
    """zipc_hip_inflate_history, one stream from host memory -> (status, bytes, checksum)"""
    out = (C.c_ubyte * max(dst_cap, 1))()
    n, ck = C.c_size_t(), C.c_uint32()
    st = lib().zipc_hip_inflate_history(ctx.handle, raw, len(raw), start_bit, hist, len(hist), int(limit is not None), limit or 0,
                                        out, dst_cap, crc_op, C.byref(n), C.byref(ck))
    return st, bytes(out[:n.value]), int(ck.value)


def zlib_decompress_dict(ctx: Context, raw: bytes, zdict: bytes, dst_cap: int):
    """zipc_hip_zlib_decompress_dict, one zlib stream from host memory against `zdict` -> (status, bytes)"""
    out = (C.c_ubyte * max(dst_cap, 1))()
    n = C.c_size_t()
    st = lib().zipc_hip_zlib_decompress_dict(ctx.handle, raw, len(raw), zdict, len(zdict), out, dst_cap, C.byref(n))
    return st, bytes(out[:n.value])


def inflate_size_blocks_batch(ctx: Context, src, descs_dev, results_dev, n_streams: int):
    """zipc_hip_inflate_size_blocks_batch: inflate_size_batch's results, the long streams of the call sized by a wave per
    block (Context.last_size_blocks tells how many blocks went that way).  The call synchronises the context's stream."""
    _sync_torch(src)
    st = lib().zipc_hip_inflate_size_blocks_batch(ctx.handle, src.data_ptr(), descs_dev.data_ptr(), results_dev.data_ptr(), n_streams)
    ctx.check(st)
    ctx.synchronize()


def zlib_size_blocks_batch(ctx: Context, src, descs_dev, results_dev, n_streams: int):
    """zipc_hip_zlib_size_blocks_batch: the same for whole zlib streams (zlib_size_batch's results)."""
    _sync_torch(src)
    st = lib().zipc_hip_zlib_size_blocks_batch(ctx.handle, src.data_ptr(), descs_dev.data_ptr(), results_dev.data_ptr(), n_streams)
    ctx.check(st)
    ctx.synchronize()


def extent_results_from_device(t) -> np.ndarray:
    return t.cpu().numpy().view(EXTENT_RESULT_DTYPE).copy()


def inflate_extent_batch(ctx: Context, src, dst, descs_dev, results_dev, n_streams: int, max_dst_cap: int, crc_op: int,
                         sync: bool = True):
    """zipc_hip_inflate_extent_batch: inflate_batch's status, checksum, out_len and bytes for raw deflate streams whose
    src_len is only an upper bound, and src_used -- the source bytes each OK stream took (0 otherwise).  results_dev: a
    uint8 cuda tensor of EXTENT_RESULT_DTYPE records.  Always a wave per stream, whatever max_dst_cap; nothing is read back."""
    if sync:
        _sync_torch(src)
    st = lib().zipc_hip_inflate_extent_batch(ctx.handle, src.data_ptr(), dst.data_ptr(), descs_dev.data_ptr(),
                                             results_dev.data_ptr(), n_streams, max_dst_cap, crc_op)
    ctx.check(st)
    if sync:
        ctx.synchronize()


def zlib_decompress_extent_batch(ctx: Context, src, dst, descs_dev, results_dev, n_streams: int, max_dst_cap: int,
                                 sync: bool = True):
    """zipc_hip_zlib_decompress_extent_batch: the same for whole zlib streams -- the trailer is found behind the body's
    extent, not at src_len - 4 (CORRUPTED where it does not lie inside src_len); src_used counts header and trailer."""
    if sync:
        _sync_torch(src)
    st = lib().zipc_hip_zlib_decompress_extent_batch(ctx.handle, src.data_ptr(), dst.data_ptr(), descs_dev.data_ptr(),
                                                     results_dev.data_ptr(), n_streams, max_dst_cap)
    ctx.check(st)
    if sync:
        ctx.synchronize()


def inflate_size_extent_batch(ctx: Context, src, descs_dev, results_dev, n_streams: int, sync: bool = True):
    """zipc_hip_inflate_size_extent_batch: inflate_size_batch's results with src_used; no destination, nothing written."""
    if sync:
        _sync_torch(src)
    st = lib().zipc_hip_inflate_size_extent_batch(ctx.handle, src.data_ptr(), descs_dev.data_ptr(), results_dev.data_ptr(), n_streams)
    ctx.check(st)
    if sync:
        ctx.synchronize()


def zlib_size_extent_batch(ctx: Context, src, descs_dev, results_dev, n_streams: int, sync: bool = True):
    """zipc_hip_zlib_size_extent_batch: zlib_size_batch's results with src_used; no checksum is compared, the trailer must
    still lie inside src_len."""
    if sync:
        _sync_torch(src)
    st = lib().zipc_hip_zlib_size_extent_batch(ctx.handle, src.data_ptr(), descs_dev.data_ptr(), results_dev.data_ptr(), n_streams)
    ctx.check(st)
    if sync:
        ctx.synchronize()


def inflate_size_extent_blocks_batch(ctx: Context, src, descs_dev, results_dev, n_streams: int):
    """zipc_hip_inflate_size_extent_blocks_batch: inflate_size_blocks_batch's results with src_used (Context.last_size_blocks
    as there).  The call synchronises the context's stream."""
    _sync_torch(src)
    st = lib().zipc_hip_inflate_size_extent_blocks_batch(ctx.handle, src.data_ptr(), descs_dev.data_ptr(), results_dev.data_ptr(), n_streams)
    ctx.check(st)
    ctx.synchronize()


def zlib_size_extent_blocks_batch(ctx: Context, src, descs_dev, results_dev, n_streams: int):
    """zipc_hip_zlib_size_extent_blocks_batch: the same for whole zlib streams (zlib_size_extent_batch's results)."""
    _sync_torch(src)
    st = lib().zipc_hip_zlib_size_extent_blocks_batch(ctx.handle, src.data_ptr(), descs_dev.data_ptr(), results_dev.data_ptr(), n_streams)
    ctx.check(st)
    ctx.synchronize()


# zipc_hip_gzip_result: EXTENT_RESULT_DTYPE's layout, the last word split into the member's header length and FLG
GZIP_RESULT_DTYPE = np.dtype([("status", "<u4"), ("checksum", "<u4"), ("out_len", "<u8"), ("src_used", "<u8"),
                              ("hdr_len", "<u4"), ("flg", "<u4")])
assert GZIP_RESULT_DTYPE.itemsize == 32
GZIP_PLAIN, GZIP_BGZF = 0, 1


def gzip_results_from_device(t) -> np.ndarray:
    return t.cpu().numpy().view(GZIP_RESULT_DTYPE).copy()


def gzip_decompress_batch(ctx: Context, src, dst, descs_dev, results_dev, n_streams: int, max_dst_cap: int, sync: bool = True):
    """zipc_hip_gzip_decompress_batch: stream i of `src` holds a gzip member (RFC 1952) from src_off on, src_len an upper
    bound of its length; header checks, inflate, the CRC-32 and ISIZE comparisons all on the device.  results_dev: a uint8
    cuda tensor of GZIP_RESULT_DTYPE records; src_used counts header, body and trailer.  Always a wave per member."""
    if sync:
        _sync_torch(src)
    st = lib().zipc_hip_gzip_decompress_batch(ctx.handle, src.data_ptr(), dst.data_ptr(), descs_dev.data_ptr(),
                                              results_dev.data_ptr(), n_streams, max_dst_cap)
    ctx.check(st)
    if sync:
        ctx.synchronize()


def gzip_size_batch(ctx: Context, src, descs_dev, results_dev, n_streams: int, sync: bool = True):
    """zipc_hip_gzip_size_batch: what every member inflates to and where it ends; no destination, no CRC-32 compared,
    ISIZE compared."""
    if sync:
        _sync_torch(src)
    st = lib().zipc_hip_gzip_size_batch(ctx.handle, src.data_ptr(), descs_dev.data_ptr(), results_dev.data_ptr(), n_streams)
    ctx.check(st)
    if sync:
        ctx.synchronize()


def gzip_size_blocks_batch(ctx: Context, src, descs_dev, results_dev, n_streams: int):
    """zipc_hip_gzip_size_blocks_batch: gzip_size_batch's results with the long members sized by a wave per block
    (Context.last_size_blocks).  The call synchronises the context's stream."""
    _sync_torch(src)
    st = lib().zipc_hip_gzip_size_blocks_batch(ctx.handle, src.data_ptr(), descs_dev.data_ptr(), results_dev.data_ptr(), n_streams)
    ctx.check(st)
    ctx.synchronize()


def gzip_compress_batch(ctx: Context, src, dst, descs_dev, results_dev, n_streams: int, max_src_len: int, total_src_len: int,
                        level: int, flavour: int = GZIP_PLAIN, sync: bool = True):
    """zipc_hip_gzip_compress_batch: every stream's destination slot receives one gzip member (out_len counts its 18
    container bytes, BGZF 26; checksum is the CRC-32 of the source); slots of gzip_bound(src_len) always fit the plain
    flavour, a BGZF member never exceeds 65 536 bytes."""
    if sync:
        _sync_torch(src)
    st = lib().zipc_hip_gzip_compress_batch(ctx.handle, src.data_ptr(), dst.data_ptr(), descs_dev.data_ptr(),
                                            results_dev.data_ptr(), n_streams, max_src_len, total_src_len, level, flavour)
    ctx.check(st)
    if sync:
        ctx.synchronize()


def gzip_bound(n: int, flavour: int = GZIP_PLAIN) -> int:
    return lib().zipc_hip_gzip_bound(n, flavour)


def packed_results_from_device(t) -> np.ndarray:
    return t.cpu().numpy().view(PACKED_RESULT_DTYPE).copy()


def _packed_args(dst, dst_arena_len, need_dev):
    return (dst.data_ptr() if dst is not None else None, dst.numel() if dst_arena_len is None else dst_arena_len,
            need_dev.data_ptr() if need_dev is not None else None)


def inflate_packed_batch(ctx: Context, src, dst, descs_dev, results_dev, n_streams: int, max_out_len: int, align: int = 1,
                         crc_op: int = CRC_NOP, need_dev=None, dst_arena_len=None, sync: bool = True):
    """zipc_hip_inflate_packed_batch: every raw deflate stream of `src` is sized, given room in `dst` by the layout rule of
    include/zipc_hip.h (in index order, lengths padded to `align`) and inflated there, in one call; results_dev: a uint8
    cuda tensor of PACKED_RESULT_DTYPE records (status, checksum, out_len and the dst_off the stream was given);
    need_dev: None, or a cuda tensor of 8 bytes that receives the arena length with which every stream fits;
    dst_arena_len: the arena's length where it is not the whole of `dst`.  dst_off / dst_cap of the descriptors are not
    looked at.  Below max_out_len = 256 KiB the call only enqueues."""
    if sync:
        _sync_torch(src)
    d, dlen, need = _packed_args(dst, dst_arena_len, need_dev)
    st = lib().zipc_hip_inflate_packed_batch(ctx.handle, src.data_ptr(), d, dlen, descs_dev.data_ptr(), results_dev.data_ptr(),
                                             n_streams, max_out_len, align, crc_op, need)
    ctx.check(st)
    if sync:
        ctx.synchronize()


def zlib_decompress_packed_batch(ctx: Context, src, dst, descs_dev, results_dev, n_streams: int, max_out_len: int, align: int = 1,
                                 need_dev=None, dst_arena_len=None, sync: bool = True):
    """zipc_hip_zlib_decompress_packed_batch: the same for whole zlib streams (the context's Adler-32 flavour): a header
    failure takes no room, a checksum mismatch reports the value found, no bytes and the dst_off it was given."""
    if sync:
        _sync_torch(src)
    d, dlen, need = _packed_args(dst, dst_arena_len, need_dev)
    st = lib().zipc_hip_zlib_decompress_packed_batch(ctx.handle, src.data_ptr(), d, dlen, descs_dev.data_ptr(),
                                                     results_dev.data_ptr(), n_streams, max_out_len, align, need)
    ctx.check(st)
    if sync:
        ctx.synchronize()


def deflate_packed_batch(ctx: Context, src, dst, descs_dev, results_dev, n_streams: int, max_src_len: int, total_src_len: int,
                         level: int, crc_op: int = CRC_NOP, align: int = 1, need_dev=None, dst_arena_len=None, sync: bool = True):
    """zipc_hip_deflate_packed_batch: every stream of `src` is deflated at `level` into a staging slot of the context's
    scratch, given room in `dst` by the layout rule of include/zipc_hip.h (in index order, lengths padded to `align`) and
    copied there, in one call; results_dev: a uint8 cuda tensor of PACKED_RESULT_DTYPE records (status, checksum, out_len
    and the dst_off the stream was given); need_dev: None, or a cuda tensor of 8 bytes that receives the arena length with
    which every stream fits; dst_arena_len: the arena's length where it is not the whole of `dst`.  dst_off / dst_cap of
    the descriptors are not looked at.  An arena of deflate_packed_bound(n_streams, total_src_len, align) always fits."""
    if sync:
        _sync_torch(src)
    d, dlen, need = _packed_args(dst, dst_arena_len, need_dev)
    st = lib().zipc_hip_deflate_packed_batch(ctx.handle, src.data_ptr(), d, dlen, descs_dev.data_ptr(), results_dev.data_ptr(),
                                             n_streams, max_src_len, total_src_len, level, crc_op, align, need)
    ctx.check(st)
    if sync:
        ctx.synchronize()


def zlib_compress_packed_batch(ctx: Context, src, dst, descs_dev, results_dev, n_streams: int, max_src_len: int, total_src_len: int,
                               level: int, align: int = 1, need_dev=None, dst_arena_len=None, sync: bool = True):
    """zipc_hip_zlib_compress_packed_batch: the same with every stream a whole zlib stream in `dst` (the context's Adler-32
    flavour): out_len counts the six container bytes, checksum is the Adler-32."""
    if sync:
        _sync_torch(src)
    d, dlen, need = _packed_args(dst, dst_arena_len, need_dev)
    st = lib().zipc_hip_zlib_compress_packed_batch(ctx.handle, src.data_ptr(), d, dlen, descs_dev.data_ptr(), results_dev.data_ptr(),
                                                   n_streams, max_src_len, total_src_len, level, align, need)
    ctx.check(st)
    if sync:
        ctx.synchronize()


def deflate_packed_bound(n_streams: int, total_src_len: int, align: int = 1, zlib: bool = False) -> int:
    """zipc_hip_deflate_packed_bound / zipc_hip_zlib_compress_packed_bound: an arena length with which every stream fits"""
    f = lib().zipc_hip_zlib_compress_packed_bound if zlib else lib().zipc_hip_deflate_packed_bound
    return f(n_streams, total_src_len, align)


def recode_results_from_device(t) -> np.ndarray:
    return t.cpu().numpy().view(RECODE_RESULT_DTYPE).copy()


def recode_batch(ctx: Context, src, mid, dst, descs_dev, results_dev, n_streams: int, max_mid_cap: int, total_mid_cap: int,
                 level: int, sync: bool = True):
    """zipc_hip_recode_batch: stream i of `src` (a raw deflate stream) is inflated into its room in `mid`, its CRC-32
    taken and compared where the descriptor expects one, and deflated at `level` into its slot of `dst`, all on the
    device; descs_dev / results_dev: uint8 cuda tensors of RECODE_DESC_DTYPE / RECODE_RESULT_DTYPE records."""
    if sync:
        _sync_torch(src)
    st = lib().zipc_hip_recode_batch(ctx.handle, src.data_ptr(), mid.data_ptr(), dst.data_ptr(), descs_dev.data_ptr(),
                                     results_dev.data_ptr(), n_streams, max_mid_cap, total_mid_cap, level)
    ctx.check(st)
    if sync:
        ctx.synchronize()


def debug_chain_links(ctx: Context, src, descs_dev, n_streams: int, max_src_len: int, total_src_len: int, which: int):
    """Tests only (include/zipc_hip.h zipc_hip_debug_chain_links): the hash-chain links of a device-resident batch as the
    library's chain kernel `which` makes them (0: ordered LDS exchange, 1: the kernel that orders equal hashes itself):
    (links, pos_base) as an int16 and an int64 cuda tensor."""
    import torch

    _sync_torch(src)
    cap = int(lib().zipc_hip_debug_chain_positions(n_streams, total_src_len))
    links = torch.empty(cap, dtype=torch.int16, device=src.device)
    base = torch.empty(n_streams, dtype=torch.int64, device=src.device)
    torch.cuda.current_stream(src.device).synchronize()
    ctx.check(lib().zipc_hip_debug_chain_links(ctx.handle, src.data_ptr(), descs_dev.data_ptr(), n_streams, max_src_len,
                                               total_src_len, which, links.data_ptr(), cap, base.data_ptr()))
    ctx.synchronize()
    return links, base


LINK_POISON = 0xFFFF  # include/zipc_hip.h ZIPC_HIP_DEBUG_LINK_POISON
CHAIN_XCHG, CHAIN_XCHG_SEGMENTS, CHAIN_PEEL, CHAIN_PEEL_SEGMENTS = 0, 1, 2, 3  # csrc/forms.h ChainKernel


def debug_chain_links_form(ctx: Context, src, descs_dev, n_streams: int, max_src_len: int, total_src_len: int, chain: int,
                           seg_positions: int = 0):
    """Tests only (include/zipc_hip.h zipc_hip_debug_chain_links_form): the hash-chain links of a device-resident batch as
    the chain form `chain` makes them (CHAIN_*; seg_positions: 0 for the shape's own segment size, else the size of a form
    by segments), launched by the pipeline's own launch site: (links, pos_base) as an int16 and an int64 cuda tensor; slots
    nobody wrote hold LINK_POISON."""
    import torch

    _sync_torch(src)
    cap = int(lib().zipc_hip_debug_chain_positions(n_streams, total_src_len))
    links = torch.empty(cap, dtype=torch.int16, device=src.device)
    base = torch.empty(n_streams, dtype=torch.int64, device=src.device)
    torch.cuda.current_stream(src.device).synchronize()
    ctx.check(lib().zipc_hip_debug_chain_links_form(ctx.handle, src.data_ptr(), descs_dev.data_ptr(), n_streams, max_src_len,
                                                    total_src_len, chain, seg_positions, links.data_ptr(), cap, base.data_ptr()))
    ctx.synchronize()
    return links, base


MATCH_POISON = 0x5A5A5A5A  # include/zipc_hip.h ZIPC_HIP_DEBUG_MATCH_POISON


def debug_match_records(ctx: Context, src, descs_dev, n_streams: int, max_src_len: int, total_src_len: int, level: int,
                        match_form: int = 0, tiles_per_group: int = 0):
    """Tests only (include/zipc_hip.h zipc_hip_debug_match_records): lz_match's tables of a device-resident batch after
    deflate_offsets, lz_chain and lz_match alone, lz_match launched as a deflate call of this shape launches it under
    that match_form / tiles_per_group: (match, snap, snap_used, pos_base) as int32, int32, int32 and int64 cuda tensors;
    slots nobody wrote hold MATCH_POISON."""
    import torch

    _sync_torch(src)
    cap = int(lib().zipc_hip_debug_chain_positions(n_streams, total_src_len))
    match = torch.empty(cap, dtype=torch.int32, device=src.device)
    snap = torch.empty(cap, dtype=torch.int32, device=src.device)
    used = torch.empty(n_streams, dtype=torch.int32, device=src.device)
    base = torch.empty(n_streams, dtype=torch.int64, device=src.device)
    torch.cuda.current_stream(src.device).synchronize()
    ctx.check(lib().zipc_hip_debug_match_records(ctx.handle, src.data_ptr(), descs_dev.data_ptr(), n_streams, max_src_len,
                                                 total_src_len, level, match_form, tiles_per_group, match.data_ptr(),
                                                 snap.data_ptr(), cap, used.data_ptr(), base.data_ptr()))
    ctx.synchronize()
    return match, snap, used, base


# zipc_hip_debug_token_record (include/zipc_hip.h)
TOKEN_RECORD_DTYPE = np.dtype([("taken", "<u4"), ("form", "<i4"), ("n_blocks", "<u4"), ("n_intervals", "<u4"), ("token_bad", "<u4"),
                               ("rounds", "<u4"), ("more", "<u4", (12,)), ("blocks_done", "<u4"), ("reserved", "<u4")])
assert TOKEN_RECORD_DTYPE.itemsize == 80


def debug_inflate_tokens(ctx: Context, src, dst, descs_dev, results_dev, n_streams: int, max_dst_cap: int, tok_raw, tok_done,
                         form: int = -1, hops0: int = 0, hops1: int = 0) -> np.ndarray:
    """Tests only (include/zipc_hip.h zipc_hip_debug_inflate_tokens): inflate_batch without a checksum, every stream that
    fits the block path handed to it, the token run in `form` (0 by intervals, 1 following, -1 the call's own rule) and
    the resolve rounds with hops0 / hops1 links (0: the tuning's).  tok_raw / tok_done: int32 cuda tensors of dst.numel()
    words, written only at [dst_off, dst_off + out_len) of the streams that went into the token run: tok[] behind the
    token run and behind the last resolve round.  Returns the records, one per stream (TOKEN_RECORD_DTYPE)."""
    assert tok_raw.numel() >= dst.numel() and tok_done.numel() >= dst.numel() and tok_raw.element_size() == 4 and tok_done.element_size() == 4
    _sync_torch(src)
    rec = np.zeros(n_streams, dtype=TOKEN_RECORD_DTYPE)
    ctx.check(lib().zipc_hip_debug_inflate_tokens(ctx.handle, src.data_ptr(), dst.data_ptr(), descs_dev.data_ptr(), results_dev.data_ptr(),
                                                  n_streams, max_dst_cap, form, hops0, hops1, tok_raw.data_ptr(), tok_done.data_ptr(),
                                                  rec.ctypes.data))
    ctx.synchronize()
    return rec


def checksum_device(ctx: Context, buf, want_crc32=True, want_adler32=True):
    """(crc32, adler32) of a uint8 cuda tensor, computed on the device."""
    import torch

    _sync_torch(buf)
    out = torch.zeros(2, dtype=torch.int32, device=buf.device)
    torch.cuda.current_stream(buf.device).synchronize()
    st = lib().zipc_hip_checksum_device(ctx.handle, buf.data_ptr(), buf.numel(), int(want_crc32),
                                        int(want_adler32), out.data_ptr())
    ctx.check(st)
    ctx.synchronize()
    v = out.cpu().numpy().view(np.uint32)
    return int(v[0]), int(v[1])


def make_ranges(off, length) -> np.ndarray:
    """zipc_hip_range records: range i is arena[off[i], off[i] + length[i])"""
    r = np.zeros(len(off), dtype=RANGE_DTYPE)
    r["off"], r["len"] = off, length
    return r


def checksum_results_from_device(t) -> np.ndarray:
    return t.cpu().numpy().view(CHECKSUM_RESULT_DTYPE).copy()


def checksum_batch(ctx: Context, arena, ranges_dev, results_dev, n_ranges: int, total_len: int, want_crc32=True,
                   want_adler32=True, arena_len=None, sync: bool = True):
    """zipc_hip_checksum_batch: CRC-32 and / or Adler-32 of n_ranges ranges of `arena` (a uint8 cuda tensor), ragged, in
    one call; ranges_dev / results_dev: uint8 cuda tensors of RANGE_DTYPE / CHECKSUM_RESULT_DTYPE records; total_len: the
    sum of the ranges' lengths, or more.  A range outside the arena reports INVALID_ARG in its own result."""
    if sync:
        _sync_torch(arena)
    st = lib().zipc_hip_checksum_batch(ctx.handle, arena.data_ptr(), arena.numel() if arena_len is None else arena_len,
                                       ranges_dev.data_ptr(), results_dev.data_ptr(), n_ranges, total_len,
                                       int(want_crc32), int(want_adler32))
    ctx.check(st)
    if sync:
        ctx.synchronize()


def checksum_many(ctx: Context, streams, want_crc32=True, want_adler32=True, check: bool = True) -> np.ndarray:
    """zipc_hip_checksum_many: the checksums of host-resident streams (bytes-like objects; None stands for a null
    pointer) as CHECKSUM_RESULT_DTYPE records, through the pipeline of the other many-stream forms.  check=False: the
    call's status is returned beside the results instead of raised."""
    n = len(streams)
    keep = [None if s is None else (s if isinstance(s, bytes) else bytes(s)) for s in streams]
    src = (C.c_void_p * max(n, 1))(*[None if b is None else C.cast(C.c_char_p(b), C.c_void_p) for b in keep])
    lens = (C.c_size_t * max(n, 1))(*[0 if b is None else len(b) for b in keep])
    return checksum_many_raw(ctx, n, src, lens, want_crc32, want_adler32, check)


def checksum_many_raw(ctx: Context, n, src, lens, want_crc32=True, want_adler32=True, check: bool = True):
    """checksum_many over ctypes arrays of pointers and lengths as they are"""
    res = (ChecksumResult * max(n, 1))()
    C.memset(res, 0xEE, C.sizeof(res))
    st = lib().zipc_hip_checksum_many(ctx.handle, n, src, lens, int(want_crc32), int(want_adler32), res)
    out = np.frombuffer(bytes(res), dtype=CHECKSUM_RESULT_DTYPE)[:n].copy()
    if check:
        ctx.check(st)
        return out
    return st, out


def reserve(ctx: Context, n_streams: int, max_src_len: int, total_src_len: int):
    ctx.check(lib().zipc_hip_reserve(ctx.handle, n_streams, max_src_len, total_src_len))


def deflate_bound(n: int) -> int:
    return lib().zipc_hip_deflate_bound(n)


def zlib_bound(n: int) -> int:
    return lib().zipc_hip_zlib_bound(n)


def uniform_layout(n_streams: int, src_len: int, dst_cap: int, limit=None) -> np.ndarray:
    """n equal streams laid back to back in both arenas (dst slots 256-byte aligned)."""
    slot = (dst_cap + 255) // 256 * 256
    i = np.arange(n_streams, dtype=np.uint64)
    return make_descs(i * np.uint64(src_len), np.full(n_streams, src_len, np.uint64),
                      i * np.uint64(slot), np.full(n_streams, dst_cap, np.uint64),
                      None if limit is None else np.full(n_streams, limit, np.uint64))


def compact_descs(results: np.ndarray, descs: np.ndarray, dst_cap_of_out, limit_exact=True) -> np.ndarray:
    """Descriptors for the inverse operation: the outputs of one batch (at their
    dst offsets, with their out_len) become the inputs of the next."""
    n = len(results)
    slot = (int(dst_cap_of_out) + 255) // 256 * 256
    i = np.arange(n, dtype=np.uint64)
    d = make_descs(descs["dst_off"], results["out_len"], i * np.uint64(slot),
                   np.full(n, dst_cap_of_out, np.uint64),
                   descs["src_len"] if limit_exact else None)
    return d


__all__ = ["DESC_DTYPE", "RESULT_DTYPE", "RECODE_DESC_DTYPE", "RECODE_RESULT_DTYPE", "make_descs", "make_recode_descs", "to_device",
           "results_from_device", "recode_results_from_device", "recode_batch",
           "inflate_batch", "deflate_batch", "inflate_size_batch", "zlib_size_batch", "inflate_size_blocks_batch", "zlib_size_blocks_batch", "zlib_decompress_batch", "zlib_compress_batch", "checksum_device", "reserve",
           "PACKED_RESULT_DTYPE", "inflate_packed_batch", "zlib_decompress_packed_batch", "packed_results_from_device",
           "deflate_packed_batch", "zlib_compress_packed_batch", "deflate_packed_bound",
           "RANGE_DTYPE", "CHECKSUM_RESULT_DTYPE", "make_ranges", "checksum_results_from_device", "checksum_batch", "checksum_many",
           "PREFIX_RESULT_DTYPE", "inflate_prefix_batch", "zlib_decompress_prefix_batch", "prefix_results_from_device",
           "EXTENT_RESULT_DTYPE", "extent_results_from_device", "inflate_extent_batch", "zlib_decompress_extent_batch",
           "inflate_size_extent_batch", "zlib_size_extent_batch", "inflate_size_extent_blocks_batch", "zlib_size_extent_blocks_batch",
           "GZIP_RESULT_DTYPE", "GZIP_PLAIN", "GZIP_BGZF", "gzip_results_from_device", "gzip_decompress_batch", "gzip_size_batch",
           "gzip_size_blocks_batch", "gzip_compress_batch", "gzip_bound",
           "deflate_bound", "zlib_bound",
           "uniform_layout", "compact_descs", "OK"]
