// packed.hip -- a batch of device-resident deflate or zlib streams of unknown size inflated into ONE destination arena that
// is laid out on the device (zipc_hip_inflate_packed_batch / zipc_hip_zlib_decompress_packed_batch): sizing, layout, decode
// and close with nothing read back between them.
//
// Two kernels around the codec's; neither touches a stream's bytes:
//   packed_layout_kernel  one workgroup, tiles of PACKED_TILE streams: reads what the sizing pass said of every stream, scans
//                         the rooms (64-bit, exclusive: a wave scan per wave, the waves' totals through LDS, a base carried
//                         from tile to tile), and writes every stream's verdict, the descriptor inflate is to run with --
//                         the stream into exactly its room, or "no stream" -- and the call's `need`;
//   packed_close_kernel   a lane per stream: puts the verdict and inflate's result together into the caller's result.
// Inner descriptors, the sizing pass's results (inflate's own go over them) and verdicts live in the context's scratch
// (launch_inflate_packed below, the one way to the kernels: ctx.h).  The rules themselves are packed_layout.h's (the
// launcher and the tests compile the same functions); the zlib form's open and its two closes are zlib.hip's and
// zlib_container.h's.
#include "ctx.h"
#include "packed_layout.h"
#include "wave_ops.h"

namespace zd {

static_assert(PACKED_TILE == 1024 && PACKED_WAVE == 64, "sixteen waves of 64");
constexpr uint32_t PACKED_WAVES = PACKED_TILE / PACKED_WAVE;

// pre: null, or the zlib container checks' verdicts (the sizes are then the bodies': zlib_close_size puts the verdict over them);
// need_out: null, or where the call's `need` goes
__global__ __launch_bounds__(PACKED_TILE) void packed_layout_kernel(const StreamDesc *__restrict__ descs, const StreamResult *__restrict__ sized,
                                                                    const ZlibPre *__restrict__ pre, uint32_t n_streams, uint64_t max_out_len,
                                                                    uint64_t align, uint64_t dst_arena_len, PackedVerdict *__restrict__ verdicts,
                                                                    StreamDesc *__restrict__ inner, uint64_t *__restrict__ need_out) {
  __shared__ uint64_t wave_total[PACKED_WAVES], wave_end[PACKED_WAVES];
  const uint32_t t = threadIdx.x, lane = t & (PACKED_WAVE - 1), w = t / PACKED_WAVE;
  uint64_t base = 0, need = 0;
  for (uint64_t t0 = 0; t0 < n_streams; t0 += PACKED_TILE) {  // (uniform: every thread takes every tile)
    const uint64_t i = t0 + t;
    const bool live = i < n_streams;
    StreamResult s;
    s.status = ST_CORRUPTED; s.checksum = 0; s.out_len = 0;  // (past the end: no room)
    if (live) {
      s = sized[i];
      if (pre) s = zlib_close_size(pre[i].status, s);
    }
    const uint64_t room = packed_room(s, max_out_len, align);
    const uint64_t incl = packed_scan_join(wave_scan_incl(packed_scan_lo(room)), wave_scan_incl(packed_scan_hi(room)));
    if (lane == PACKED_WAVE - 1) wave_total[w] = incl;
    __syncthreads();
    uint64_t before = 0, tile_total = 0;
    for (uint32_t k = 0; k < PACKED_WAVES; k++) {
      const uint64_t v = wave_total[k];
      if (k < w) before = packed_add(before, v);
      tile_total = packed_add(tile_total, v);
    }
    const uint64_t off = packed_add(packed_add(base, before), incl - room);
    const PackedVerdict v = packed_verdict(s, off, max_out_len, dst_arena_len);
    if (live) {
      verdicts[i] = v;
      inner[i] = packed_inner_desc(descs[i], v, s.out_len);
    }
    // the last end among the wave's roomed streams (0: none), for `need`
    unsigned long long end = packed_end(v.roomed != 0, off, s.out_len);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) end = packed_need_join(end, __shfl_xor(end, o, 64));
    if (lane == 0) wave_end[w] = end;
    __syncthreads();
    for (uint32_t k = 0; k < PACKED_WAVES; k++) need = packed_need_join(need, wave_end[k]);
    base = packed_tile_base(base, tile_total);
    __syncthreads();  // (the next tile overwrites the two arrays)
  }
  if (t == 0 && need_out) need_out[0] = need;
}

// pre: null, or the zlib container checks' verdicts (zlib_close_decompress: the Adler-32 compared with the stream's own)
__global__ __launch_bounds__(256) void packed_close_kernel(uint32_t n_streams, const PackedVerdict *__restrict__ verdicts,
                                                           const StreamResult *__restrict__ decoded, const ZlibPre *__restrict__ pre,
                                                           PackedResult *__restrict__ results) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_streams) return;
  StreamResult d = decoded[i];
  if (pre) d = zlib_close_decompress(pre[i].status, pre[i].expect, d);
  results[i] = packed_close(verdicts[i], d);
}

// The context's scratch of a packed call of n streams: the descriptors inflate runs with, the sizing pass's results and
// then inflate's, the verdicts.
int packed_reserve(zipc_hip_ctx *ctx, size_t n) {
  HIP_TRY(ctx, ctx->ensure(ctx->packed_descs, n * sizeof(StreamDesc)));
  HIP_TRY(ctx, ctx->ensure(ctx->packed_res, n * sizeof(StreamResult)));
  HIP_TRY(ctx, ctx->ensure(ctx->packed_verdicts, n * sizeof(PackedVerdict)));
  return ZIPC_HIP_OK;
}

// (zlib: open ->) size -> layout -> inflate -> close, all on the context's stream.  Below packed_size_form's threshold
// nothing here waits for the device; from there on the sizing by blocks and inflate's block path synchronise as they do
// when they are called alone.
int launch_inflate_packed(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena, size_t dst_arena_len,
                          const zipc_hip_stream_desc *d_descs, zipc_hip_packed_result *d_results, size_t n, size_t max_out_len,
                          size_t align, int crc_op, uint64_t *d_need, bool zlib) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int st = packed_reserve(ctx, n);
  if (st) return st;
  const ZlibPre *pre = nullptr;
  const zipc_hip_stream_desc *read_descs = d_descs;  // the streams as inflate is to read them
  if (zlib) {
    st = launch_zlib_open(ctx, d_src_arena, d_descs, n, 0);
    if (st) return st;
    pre = (const ZlibPre *)ctx->zlib_pre.p;
    read_descs = (const zipc_hip_stream_desc *)ctx->zlib_descs.p;
  }
  StreamDesc *inner = (StreamDesc *)ctx->packed_descs.p;
  zipc_hip_stream_result *inner_res = (zipc_hip_stream_result *)ctx->packed_res.p;
  PackedVerdict *verdicts = (PackedVerdict *)ctx->packed_verdicts.p;
  if (packed_size_form(max_out_len) == PACKED_SIZE_ONE_WAVE) st = launch_inflate_size(ctx, d_src_arena, read_descs, inner_res, n);
  else st = launch_inflate_size_blocks(ctx, d_src_arena, read_descs, inner_res, n, nullptr);
  if (st) return st;
  ZD_LAUNCH(ctx, "packed_layout", packed_layout_kernel, dim3(1), dim3(PACKED_TILE), 0, (const StreamDesc *)read_descs,
            (const StreamResult *)inner_res, pre, (uint32_t)n, (uint64_t)max_out_len, (uint64_t)align, (uint64_t)dst_arena_len, verdicts, inner,
            d_need);
  HIP_TRY(ctx, hipGetLastError());
  st = launch_inflate(ctx, d_src_arena, d_dst_arena, (const zipc_hip_stream_desc *)inner, inner_res, n, max_out_len, crc_op, nullptr, true);
  if (st) return st;
  ZD_LAUNCH(ctx, "packed_close", packed_close_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (uint32_t)n,
            (const PackedVerdict *)verdicts, (const StreamResult *)inner_res, pre, (PackedResult *)d_results);
  HIP_TRY(ctx, hipGetLastError());
  return ZIPC_HIP_OK;
}

}  // namespace zd
