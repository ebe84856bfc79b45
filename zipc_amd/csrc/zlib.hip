// zlib.hip -- the zlib container of a batch of device-resident streams (zipc_hip_zlib_decompress_batch / _compress_batch).
//
// Two kernels around the codec's, a lane per stream each, six bytes of a stream touched between them:
//   zlib_open_kernel   reads a stream's descriptor (and, to decompress, its two header and four trailer bytes), applies
//                      the container's checks and writes the descriptor the codec is to run with -- the body of the
//                      stream, or the room behind the header -- into the context's scratch, with the check's verdict;
//   zlib_close_kernel  puts that verdict and the codec's result together: the Adler-32 compared with the stream's own,
//                      or the header and the trailer stored around what deflate wrote.
//   zlib_close_size_kernel  the same behind inflate's size kernel (zipc_hip_zlib_size_batch): the verdict, or the body's size.
//   zlib_close_prefix_kernel  the same behind inflate's prefix kernel (zipc_hip_zlib_decompress_prefix_batch): an ended stream's
//                      Adler-32 compared, a cut one's not.
//   zlib_close_extent_kernel, zlib_close_size_extent_kernel  the same behind inflate's extent kernels (zipc_hip_zlib_decompress_extent_batch,
//                      zipc_hip_zlib_size_extent_batch): the trailer found behind the body's extent, not at src_len - 4.
//   zlib_open_dict_kernel, zlib_seed_dict_kernel, zlib_close_dict_kernel  the dictionary forms (zipc_hip_zlib_decompress_dict_batch,
//                      zipc_hip_zlib_size_dict_batch): the open that reads a DICTID and leaves a history record per stream, the
//                      copy of the dictionary in front of the rooms that decode with it, the close that reports a DICTID.
// The rules themselves are zlib_container.h's (the host forms and the tests compile the same functions).  Nothing is
// read back: the calls enqueue and return like the raw batch forms.  The launches at the end of this file are the one
// way to the kernels (ctx.h).
#include "ctx.h"
#include "deflate_packed.h"
#include "inflate_history.h"
#include "wave_ops.h"
#include "zlib_container.h"

namespace zd {

// A stream the codec is not to touch: nothing to read, no room to write.  (inflate reports a corrupted stream for it,
// deflate a destination too small, neither stores a byte; zlib_close_kernel puts the container's verdict in its place.)
__device__ __forceinline__ StreamDesc zlib_no_stream(const StreamDesc &sd) {
  StreamDesc in = sd;
  in.src_len = 0;
  in.dst_cap = 0;
  in.flags = 0;
  return in;
}

__global__ __launch_bounds__(256) void zlib_open_kernel(const uint8_t *__restrict__ src_arena, const StreamDesc *__restrict__ descs,
                                                        uint32_t n_streams, int compress, StreamDesc *__restrict__ inner,
                                                        ZlibPre *__restrict__ pre) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_streams) return;
  const StreamDesc sd = descs[i];
  ZlibPre p;
  p.status = ST_OK;
  p.expect = 0;
  StreamDesc in = sd;
  if ((sd.flags & ~STREAM_HAS_LIMIT) != 0) {
    p.status = ST_INVALID_ARG;
  } else if (compress) {
    if (sd.dst_cap < ZLIB_OVERHEAD) {
      p.status = ST_DST_TOO_SMALL;
    } else {
      in.dst_off = zlib_payload_off(sd.dst_off);
      in.dst_cap = zlib_payload_cap(sd.dst_cap);
    }
  } else {
    uint32_t cmf = 0, flg = 0;
    if (sd.src_len >= ZLIB_MIN_LEN) {  // (the reference looks at the length first, and so nothing is read of a shorter one)
      const uint8_t *s = src_arena + sd.src_off;
      cmf = s[0];
      flg = s[1];
      p.expect = zlib_expect(s + sd.src_len - 4);
    }
    p.status = zlib_open_status(sd.src_len, cmf, flg);
    if (p.status == ST_OK) {
      in.src_off = zlib_body_off(sd.src_off);
      in.src_len = zlib_body_len(sd.src_len);
    }
  }
  if (p.status != ST_OK) { in = zlib_no_stream(sd); p.expect = 0; }
  inner[i] = in;
  pre[i] = p;
}

__global__ __launch_bounds__(256) void zlib_close_kernel(uint8_t *__restrict__ dst_arena, const StreamDesc *__restrict__ descs,
                                                         const ZlibPre *__restrict__ pre, StreamResult *__restrict__ results,
                                                         uint32_t n_streams, int compress, int level) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_streams) return;
  const ZlibPre p = pre[i];
  const StreamResult inner = results[i];
  if (!compress) {
    results[i] = zlib_close_decompress(p.status, p.expect, inner);
    return;
  }
  bool wrap;
  const StreamResult r = zlib_close_compress(p.status, inner, &wrap);
  if (wrap) {  // (inner.out_len <= dst_cap - 6: deflate said its bytes fit)
    uint8_t *o = dst_arena + descs[i].dst_off;
    o[0] = (uint8_t)zlib_cmf();
    o[1] = (uint8_t)zlib_flg(level);
    zlib_put_trailer(o + 2 + inner.out_len, inner.checksum);
  }
  results[i] = r;
}

// zipc_hip_zlib_size_batch's close: the container check's verdict over the size kernel's (zlib_close_size)
__global__ __launch_bounds__(256) void zlib_close_size_kernel(const ZlibPre *__restrict__ pre, StreamResult *__restrict__ results,
                                                              uint32_t n_streams) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_streams) return;
  results[i] = zlib_close_size(pre[i].status, results[i]);
}

// zipc_hip_zlib_decompress_prefix_batch's close: the container check's verdict over the prefix kernel's (zlib_close_prefix)
__global__ __launch_bounds__(256) void zlib_close_prefix_kernel(const ZlibPre *__restrict__ pre, const uint32_t *__restrict__ adlers,
                                                                PrefixResult *__restrict__ results, uint32_t n_streams) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_streams) return;
  results[i] = zlib_close_prefix(pre[i].status, pre[i].expect, adlers[i], results[i]);
}

// The extent forms' closes, a lane per stream: src_len is only a bound, so zlib_open_kernel's `expect` (read at src_len - 4)
// is not used; the trailer is read from the source arena at 2 + u, u the body's extent, if it lies inside the declared
// bytes (zlib_container.h zlib_close_extent).  The sizing form compares nothing and holds the same bound.
__global__ __launch_bounds__(256) void zlib_close_extent_kernel(const uint8_t *__restrict__ src_arena, const StreamDesc *__restrict__ descs,
                                                                const ZlibPre *__restrict__ pre, ExtentResult *__restrict__ results,
                                                                uint32_t n_streams) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_streams) return;
  results[i] = zlib_close_extent(pre[i].status, descs[i].src_len, src_arena + descs[i].src_off, results[i], true);
}
__global__ __launch_bounds__(256) void zlib_close_size_extent_kernel(const uint8_t *__restrict__ src_arena, const StreamDesc *__restrict__ descs,
                                                                     const ZlibPre *__restrict__ pre, ExtentResult *__restrict__ results,
                                                                     uint32_t n_streams) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_streams) return;
  results[i] = zlib_close_extent(pre[i].status, descs[i].src_len, src_arena + descs[i].src_off, results[i], false);
}

// The dictionary forms' open, a lane per stream (zlib_container.h zlib_open_dict): zlib_open_kernel's decompress half with
// the FDICT branch -- the descriptor the history kernel runs with (the body; the room is the caller's), the stream's
// history record, the verdict.  dict_adler: a device word, not read when dict_len is 0.
__global__ __launch_bounds__(256) void zlib_open_dict_kernel(const uint8_t *__restrict__ src_arena, const StreamDesc *__restrict__ descs,
                                                             uint32_t n_streams, uint64_t dict_len, const uint32_t *__restrict__ dict_adler,
                                                             StreamDesc *__restrict__ inner, HistoryRec *__restrict__ hist,
                                                             ZlibPre *__restrict__ pre) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_streams) return;
  const StreamDesc sd = descs[i];
  ZlibPre p;
  p.status = ST_OK;
  p.expect = 0;
  StreamDesc in = sd;
  HistoryRec h;
  h.hist_len = 0; h.start_bit = 0;
  if ((sd.flags & ~STREAM_HAS_LIMIT) != 0) {
    p.status = ST_INVALID_ARG;
  } else {
    uint32_t cmf = 0, flg = 0, dictid = 0;
    const uint8_t *s = src_arena + sd.src_off;
    if (sd.src_len >= ZLIB_MIN_LEN) {  // (the length first: nothing is read of a shorter stream)
      cmf = s[0];
      flg = s[1];
      dictid = zlib_dictid(s + 2);
    }
    const ZlibDictOpen o = zlib_open_dict(sd.src_len, cmf, flg, dictid, dict_len, dict_len ? dict_adler[0] : 0u);
    p.status = o.status;
    if (o.status == ST_OK) {
      p.expect = zlib_expect(s + sd.src_len - 4);
      in.src_off = sd.src_off + o.body_off;
      in.src_len = o.body_len;
      h.hist_len = o.hist_len;
    } else {
      p.expect = o.dictid;
    }
  }
  if (p.status != ST_OK) in = zlib_no_stream(sd);
  inner[i] = in;
  hist[i] = h;
  pre[i] = p;
}

// The seed, a workgroup per stream: the dictionary to [dst_off - hist_len, dst_off) of every stream zlib_dict_seeds names,
// at any byte alignment of either side -- deflate_packed.h's copy rule (dpacked_span: single bytes up to the destination's
// first 16-byte boundary, whole aligned units loaded unaligned, single bytes behind them).  The one kernel of these forms
// that writes in front of dst_off; nothing is written in front of the gap.
static_assert(HISTORY_MAX_LEN <= DPACKED_SEG_BYTES, "a dictionary is one segment of the copy rule");
__global__ __launch_bounds__(DPACKED_COPY_THREADS) void zlib_seed_dict_kernel(uint8_t *__restrict__ dst_arena, const StreamDesc *__restrict__ descs,
                                                                              const HistoryRec *__restrict__ hist, const ZlibPre *__restrict__ pre,
                                                                              uint32_t n_streams, const uint8_t *__restrict__ dict) {
  const uint32_t i = blockIdx.x;
  if (i >= n_streams) return;
  const uint32_t len = hist[i].hist_len;
  const uint64_t dst_off = descs[i].dst_off;
  if (!zlib_dict_seeds(pre[i].status, len, dst_off)) return;
  uint8_t *d = dst_arena + (dst_off - len);
  const DpackedSpan sp = dpacked_span(len, 0, (uint64_t)(uintptr_t)d);
  const uint8_t *s = dict;
  const uint32_t t = threadIdx.x;
  const uint32_t rounds = dpacked_rounds(sp.units);
  for (uint32_t r = 0; r < rounds; r++) {
    u32x4 v[DPACKED_IN_FLIGHT];
#pragma unroll
    for (uint32_t j = 0; j < DPACKED_IN_FLIGHT; j++) {
      const uint32_t u = dpacked_unit_of(r, j, t);
      if (u < sp.units) v[j] = load16_unaligned(s + dpacked_unit_at(sp, u));
    }
#pragma unroll
    for (uint32_t j = 0; j < DPACKED_IN_FLIGHT; j++) {
      const uint32_t u = dpacked_unit_of(r, j, t);
      if (u < sp.units) *reinterpret_cast<u32x4 *>(d + dpacked_unit_at(sp, u)) = v[j];
    }
  }
  if (t < sp.head) d[t] = s[t];
  if (t < sp.tail) d[dpacked_tail_at(sp) + t] = s[dpacked_tail_at(sp) + t];
}

// The dictionary forms' closes (zlib_close_dict): size 0 -- the Adler-32 of the output alone against the trailer; 1 -- nothing compared
__global__ __launch_bounds__(256) void zlib_close_dict_kernel(const ZlibPre *__restrict__ pre, StreamResult *__restrict__ results,
                                                              uint32_t n_streams, int size) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_streams) return;
  results[i] = zlib_close_dict(pre[i].status, pre[i].expect, results[i], size != 0);
}

int zlib_crc_op(const zipc_hip_ctx *ctx) { return ctx->adler_rfc1950 ? ZIPC_HIP_CRC_ADLER32_RFC1950 : ZIPC_HIP_CRC_ADLER32; }

// zlib_open_kernel over the caller's descriptors: the codec's descriptors and the checks' verdicts, in the context's scratch
int launch_zlib_open(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs, size_t n, int compress) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, ctx->ensure(ctx->zlib_descs, n * sizeof(StreamDesc)));
  HIP_TRY(ctx, ctx->ensure(ctx->zlib_pre, n * sizeof(ZlibPre)));
  ZD_LAUNCH(ctx, "zlib_open", zlib_open_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (const uint8_t *)d_src_arena,
            (const StreamDesc *)d_descs, (uint32_t)n, compress, (StreamDesc *)ctx->zlib_descs.p, (ZlibPre *)ctx->zlib_pre.p);
  HIP_TRY(ctx, hipGetLastError());
  return ZIPC_HIP_OK;
}
int launch_zlib_close(zipc_hip_ctx *ctx, void *d_dst_arena, const zipc_hip_stream_desc *d_descs, zipc_hip_stream_result *d_results,
                      size_t n, int compress, int level) {
  ZD_LAUNCH(ctx, "zlib_close", zlib_close_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (uint8_t *)d_dst_arena,
            (const StreamDesc *)d_descs, (const ZlibPre *)ctx->zlib_pre.p, (StreamResult *)d_results, (uint32_t)n, compress, level);
  HIP_TRY(ctx, hipGetLastError());
  return ZIPC_HIP_OK;
}
int launch_zlib_close_size(zipc_hip_ctx *ctx, zipc_hip_stream_result *d_results, size_t n) {
  ZD_LAUNCH(ctx, "zlib_close_size", zlib_close_size_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
            (const ZlibPre *)ctx->zlib_pre.p, (StreamResult *)d_results, (uint32_t)n);
  HIP_TRY(ctx, hipGetLastError());
  return ZIPC_HIP_OK;
}

int launch_zlib_close_prefix(zipc_hip_ctx *ctx, zipc_hip_prefix_result *d_results, size_t n) {
  ZD_LAUNCH(ctx, "zlib_close_prefix", zlib_close_prefix_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
            (const ZlibPre *)ctx->zlib_pre.p, (const uint32_t *)ctx->prefix_adlers.p, (PrefixResult *)d_results, (uint32_t)n);
  HIP_TRY(ctx, hipGetLastError());
  return ZIPC_HIP_OK;
}

int launch_zlib_open_dict(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs, size_t n, size_t dict_len,
                          const uint32_t *d_dict_adler) {
  HIP_TRY(ctx, ctx->ensure(ctx->zlib_descs, n * sizeof(StreamDesc)));
  HIP_TRY(ctx, ctx->ensure(ctx->zlib_pre, n * sizeof(ZlibPre)));
  HIP_TRY(ctx, ctx->ensure(ctx->zlib_hist, n * sizeof(HistoryRec)));
  ZD_LAUNCH(ctx, "zlib_open_dict", zlib_open_dict_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (const uint8_t *)d_src_arena,
            (const StreamDesc *)d_descs, (uint32_t)n, (uint64_t)dict_len, d_dict_adler, (StreamDesc *)ctx->zlib_descs.p,
            (HistoryRec *)ctx->zlib_hist.p, (ZlibPre *)ctx->zlib_pre.p);
  HIP_TRY(ctx, hipGetLastError());
  return ZIPC_HIP_OK;
}
int launch_zlib_seed_dict(zipc_hip_ctx *ctx, void *d_dst_arena, const zipc_hip_stream_desc *d_descs, size_t n, const void *d_dict, size_t dict_len) {
  if (dict_len == 0) return ZIPC_HIP_OK;  // (no stream was opened with FDICT)
  ZD_LAUNCH(ctx, "zlib_seed_dict", zlib_seed_dict_kernel, dim3((unsigned)n), dim3(DPACKED_COPY_THREADS), 0, (uint8_t *)d_dst_arena,
            (const StreamDesc *)d_descs, (const HistoryRec *)ctx->zlib_hist.p, (const ZlibPre *)ctx->zlib_pre.p, (uint32_t)n,
            (const uint8_t *)d_dict);
  HIP_TRY(ctx, hipGetLastError());
  return ZIPC_HIP_OK;
}
int launch_zlib_close_dict(zipc_hip_ctx *ctx, zipc_hip_stream_result *d_results, size_t n, int size) {
  ZD_LAUNCH(ctx, "zlib_close_dict", zlib_close_dict_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
            (const ZlibPre *)ctx->zlib_pre.p, (StreamResult *)d_results, (uint32_t)n, size);
  HIP_TRY(ctx, hipGetLastError());
  return ZIPC_HIP_OK;
}

int launch_zlib_close_extent(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs,
                             zipc_hip_extent_result *d_results, size_t n, int compare) {
  if (compare)
    ZD_LAUNCH(ctx, "zlib_close_extent", zlib_close_extent_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (const uint8_t *)d_src_arena,
              (const StreamDesc *)d_descs, (const ZlibPre *)ctx->zlib_pre.p, (ExtentResult *)d_results, (uint32_t)n);
  else
    ZD_LAUNCH(ctx, "zlib_close_size_extent", zlib_close_size_extent_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
              (const uint8_t *)d_src_arena, (const StreamDesc *)d_descs, (const ZlibPre *)ctx->zlib_pre.p, (ExtentResult *)d_results, (uint32_t)n);
  HIP_TRY(ctx, hipGetLastError());
  return ZIPC_HIP_OK;
}

}  // namespace zd
