// deflate_packed.hip -- a batch of device-resident streams deflated into ONE destination arena that is laid out on the device
// (zipc_hip_deflate_packed_batch / zipc_hip_zlib_compress_packed_batch): stage, deflate, layout, copy and close with nothing
// read back between them.
//
// Four kernels around the codec's; only the copy touches a stream's bytes:
//   dpacked_stage_kernel   one workgroup, tiles of DPACKED_TILE streams: first the declared-size check over every descriptor,
//                          then the scan of the staging slots (64-bit, exclusive: packed.hip's scan) and the descriptors
//                          deflate is to run with -- the stream into exactly its slot, or "no stream";
//   dpacked_layout_kernel  one workgroup, the same tiles: reads what deflate said of every stream in its slot, scans the
//                          rooms, writes every stream's verdict, scans the segment counts of the streams that fit, and
//                          leaves the call's `need` and the number of segments;
//   dpacked_copy_kernel    a workgroup per 32 KiB segment that exists, on a grid sized from the declared numbers: bisects
//                          the segment bases for its (stream, segment) and moves that segment from the slot to the arena;
//   dpacked_close_kernel   a lane per stream: the caller's result.
// Inner descriptors, deflate's results, the stage's statuses, the segment bases, the verdicts and the staging arena live in
// the context's scratch (launch_deflate_packed below, the one way to the kernels: ctx.h).  The rules are deflate_packed.h's.
#include "ctx.h"
#include "deflate_packed.h"
#include "wave_ops.h"

namespace zd {

static_assert(DPACKED_TILE == 1024 && DPACKED_WAVE == 64, "sixteen waves of 64");
constexpr uint32_t DPACKED_WAVES = DPACKED_TILE / DPACKED_WAVE;

__global__ __launch_bounds__(DPACKED_TILE) void dpacked_stage_kernel(const StreamDesc *__restrict__ descs, uint32_t n_streams, uint64_t max_src_len,
                                                                     uint64_t total_src_len, int zlib, DpackedCall *__restrict__ call,
                                                                     uint32_t *__restrict__ stage_status, StreamDesc *__restrict__ inner) {
  __shared__ uint64_t wave_total[DPACKED_WAVES];
  __shared__ uint32_t wave_over[DPACKED_WAVES];
  const uint32_t t = threadIdx.x, lane = t & (DPACKED_WAVE - 1), w = t / DPACKED_WAVE;
  // ---- the declared sizes, before any slot is used
  unsigned long long mine = 0;
  uint32_t over = 0;
  for (uint64_t i = t; i < n_streams; i += DPACKED_TILE) {
    const uint64_t l = descs[i].src_len;
    mine = packed_add(mine, dpacked_declared_len(l));
    over |= dpacked_over_max(l, max_src_len) ? 1u : 0u;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mine = packed_add(mine, __shfl_xor(mine, o, 64));
    over |= __shfl_xor(over, o, 64);
  }
  if (lane == 0) { wave_total[w] = mine; wave_over[w] = over; }
  __syncthreads();
  uint64_t sum_len = 0;
  uint32_t any_over = 0;
  for (uint32_t k = 0; k < DPACKED_WAVES; k++) { sum_len = packed_add(sum_len, wave_total[k]); any_over |= wave_over[k]; }
  const uint32_t bad = dpacked_declared_bad(any_over != 0, sum_len, total_src_len);
  __syncthreads();  // (the scan overwrites wave_total)
  // ---- the slots and the descriptors deflate runs with
  uint64_t base = 0;
  for (uint64_t t0 = 0; t0 < n_streams; t0 += DPACKED_TILE) {  // (uniform: every thread takes every tile)
    const uint64_t i = t0 + t;
    const bool live = i < n_streams;
    StreamDesc sd{};
    if (live) sd = descs[i];
    const uint64_t room = live ? dpacked_slot_room(sd.src_len, zlib != 0) : 0;
    const uint64_t incl = packed_scan_join(wave_scan_incl(packed_scan_lo(room)), wave_scan_incl(packed_scan_hi(room)));
    if (lane == DPACKED_WAVE - 1) wave_total[w] = incl;
    __syncthreads();
    uint64_t before = 0, tile_total = 0;
    for (uint32_t k = 0; k < DPACKED_WAVES; k++) {
      const uint64_t v = wave_total[k];
      if (k < w) before = packed_add(before, v);
      tile_total = packed_add(tile_total, v);
    }
    if (live) {
      const uint64_t off = packed_add(packed_add(base, before), incl - room);
      const uint32_t st = dpacked_stage_status(bad, sd.src_len);
      stage_status[i] = st;
      inner[i] = dpacked_inner_desc(sd, st, off, zlib != 0);
    }
    base = packed_tile_base(base, tile_total);
    __syncthreads();  // (the next tile overwrites the array)
  }
  if (t == 0) {
    DpackedCall c;
    c.need = 0; c.total_segs = 0; c.bad = bad; c.reserved[0] = c.reserved[1] = 0;
    call[0] = c;
  }
}

// need_out: null, or where the call's `need` goes
__global__ __launch_bounds__(DPACKED_TILE) void dpacked_layout_kernel(const uint32_t *__restrict__ stage_status, const StreamResult *__restrict__ staged,
                                                                      uint32_t n_streams, uint64_t align, uint64_t dst_arena_len,
                                                                      PackedVerdict *__restrict__ verdicts, uint32_t *__restrict__ seg_base,
                                                                      DpackedCall *__restrict__ call, uint64_t *__restrict__ need_out) {
  __shared__ uint64_t wave_total[DPACKED_WAVES], wave_end[DPACKED_WAVES];
  __shared__ uint32_t wave_segs[DPACKED_WAVES];
  const uint32_t t = threadIdx.x, lane = t & (DPACKED_WAVE - 1), w = t / DPACKED_WAVE;
  uint64_t base = 0, need = 0;
  uint32_t segs_carried = 0;
  for (uint64_t t0 = 0; t0 < n_streams; t0 += DPACKED_TILE) {  // (uniform: every thread takes every tile)
    const uint64_t i = t0 + t;
    const bool live = i < n_streams;
    uint32_t st = ST_INVALID_ARG;  // (past the end: no room)
    StreamResult s;
    s.status = ST_INVALID_ARG; s.checksum = 0; s.out_len = 0;
    if (live) { st = stage_status[i]; s = staged[i]; }
    const uint64_t room = dpacked_room(st, s, align);
    const uint64_t incl = packed_scan_join(wave_scan_incl(packed_scan_lo(room)), wave_scan_incl(packed_scan_hi(room)));
    if (lane == DPACKED_WAVE - 1) wave_total[w] = incl;
    __syncthreads();
    uint64_t before = 0, tile_total = 0;
    for (uint32_t k = 0; k < DPACKED_WAVES; k++) {
      const uint64_t v = wave_total[k];
      if (k < w) before = packed_add(before, v);
      tile_total = packed_add(tile_total, v);
    }
    const uint64_t off = packed_add(packed_add(base, before), incl - room);
    const PackedVerdict v = dpacked_verdict(st, s, off, dst_arena_len);
    if (live) verdicts[i] = v;
    // the segments of the streams that fit: a 32-bit exclusive scan (the total is at most the copy's grid)
    const uint32_t segs = (uint32_t)dpacked_copy_segs(v, s.out_len);
    const uint32_t segs_incl = wave_scan_incl(segs);
    if (lane == DPACKED_WAVE - 1) wave_segs[w] = segs_incl;
    // the last end among the wave's roomed streams (0: none), for `need`
    unsigned long long end = dpacked_end(v, s.out_len);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) end = packed_need_join(end, __shfl_xor(end, o, 64));
    if (lane == 0) wave_end[w] = end;
    __syncthreads();
    uint32_t segs_before = 0, segs_total = 0;
    for (uint32_t k = 0; k < DPACKED_WAVES; k++) {
      const uint32_t x = wave_segs[k];
      if (k < w) segs_before += x;
      segs_total += x;
      need = packed_need_join(need, wave_end[k]);
    }
    if (live) seg_base[i] = segs_carried + segs_before + (segs_incl - segs);
    segs_carried += segs_total;
    base = packed_tile_base(base, tile_total);
    __syncthreads();  // (the next tile overwrites the three arrays)
  }
  if (t == 0) {
    call[0].need = need;
    call[0].total_segs = segs_carried;
    if (need_out) need_out[0] = need;
  }
}

// The compaction.  Workgroup w of the grid bound takes segment w of the segments that exist: the slot side is on unit
// boundaries, the arena side at any byte, so the body's loads are unaligned (one global_load_dwordx4 each: wave_ops.h) and
// its stores aligned, with DPACKED_IN_FLIGHT loads of a thread ahead of its stores; head and tail go by single bytes.
__global__ __launch_bounds__(DPACKED_COPY_THREADS) void dpacked_copy_kernel(const uint8_t *__restrict__ staging, uint8_t *__restrict__ dst_arena,
                                                                            const StreamDesc *__restrict__ inner,
                                                                            const StreamResult *__restrict__ staged,
                                                                            const PackedVerdict *__restrict__ verdicts,
                                                                            const uint32_t *__restrict__ seg_base, uint32_t n_streams,
                                                                            const DpackedCall *__restrict__ call) {
  const DpackedCall c = call[0];
  if (dpacked_wg_idle(c, blockIdx.x)) return;
  const DpackedWork k = dpacked_work(seg_base, n_streams, blockIdx.x);
  const uint64_t len = staged[k.stream].out_len;
  const PackedVerdict verdict = verdicts[k.stream];
  if (k.seg >= dpacked_copy_segs(verdict, len)) return;  // (never: the bases are the scan of these counts)
  uint8_t *d = dst_arena + verdict.dst_off;
  const DpackedSpan sp = dpacked_span(len, k.seg, (uint64_t)(uintptr_t)d);
  const uint8_t *s = staging + inner[k.stream].dst_off + sp.lo;
  d += sp.lo;
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

__global__ __launch_bounds__(256) void dpacked_close_kernel(uint32_t n_streams, const PackedVerdict *__restrict__ verdicts,
                                                            const uint32_t *__restrict__ stage_status, const StreamResult *__restrict__ staged,
                                                            int crc_op, PackedResult *__restrict__ results) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_streams) return;
  results[i] = dpacked_close(verdicts[i], stage_status[i], staged[i], crc_op);
}

// The plan's scratch: the call-wide word in 256 bytes, then the stage's statuses and the segment bases, each array on a
// 256-byte boundary.
static size_t dpacked_plan_words_at(size_t n) { return 256 + (n * sizeof(uint32_t) + 255) / 256 * 256; }

// The context's scratch of a packed encode call, from n and the declared total alone: the staging arena (the slots, and a
// unit to spare behind the last), the descriptors deflate runs with, its results, the plan, the verdicts.
int dpacked_reserve(zipc_hip_ctx *ctx, size_t n, size_t total_src_len, bool zlib) {
  HIP_TRY(ctx, ctx->ensure(ctx->dpacked_staging, (size_t)dpacked_staging_bound(n, total_src_len, zlib) + DPACKED_UNIT));
  HIP_TRY(ctx, ctx->ensure(ctx->dpacked_descs, n * sizeof(StreamDesc)));
  HIP_TRY(ctx, ctx->ensure(ctx->dpacked_res, n * sizeof(StreamResult)));
  HIP_TRY(ctx, ctx->ensure(ctx->dpacked_plan, dpacked_plan_words_at(n) + n * sizeof(uint32_t)));
  HIP_TRY(ctx, ctx->ensure(ctx->dpacked_verdicts, n * sizeof(PackedVerdict)));
  return ZIPC_HIP_OK;
}

// stage -> (zlib: open ->) deflate (-> zlib close) -> layout -> copy -> close, all on the context's stream.  The codec's
// part is the batch form's own entry over the inner descriptors: it grows deflate's scratch and synchronises where it does
// when it is called alone, and nowhere else.
int launch_deflate_packed(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena, size_t dst_arena_len,
                          const zipc_hip_stream_desc *d_descs, zipc_hip_packed_result *d_results, size_t n, size_t max_src_len,
                          size_t total_src_len, int level, int crc_op, size_t align, uint64_t *d_need, bool zlib) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int st = dpacked_reserve(ctx, n, total_src_len, zlib);
  if (st) return st;
  uint8_t *staging = (uint8_t *)ctx->dpacked_staging.p;
  StreamDesc *inner = (StreamDesc *)ctx->dpacked_descs.p;
  StreamResult *staged = (StreamResult *)ctx->dpacked_res.p;
  DpackedCall *call = (DpackedCall *)ctx->dpacked_plan.p;
  uint32_t *stage_status = (uint32_t *)((uint8_t *)ctx->dpacked_plan.p + 256);
  uint32_t *seg_base = (uint32_t *)((uint8_t *)ctx->dpacked_plan.p + dpacked_plan_words_at(n));
  PackedVerdict *verdicts = (PackedVerdict *)ctx->dpacked_verdicts.p;
  ZD_LAUNCH(ctx, "dpacked_stage", dpacked_stage_kernel, dim3(1), dim3(DPACKED_TILE), 0, (const StreamDesc *)d_descs, (uint32_t)n,
            (uint64_t)max_src_len, (uint64_t)total_src_len, zlib ? 1 : 0, call, stage_status, inner);
  HIP_TRY(ctx, hipGetLastError());
  if (zlib)
    st = zipc_hip_zlib_compress_batch(ctx, d_src_arena, staging, (const zipc_hip_stream_desc *)inner, (zipc_hip_stream_result *)staged, n,
                                      max_src_len, total_src_len, level);
  else
    st = zipc_hip_deflate_batch(ctx, d_src_arena, staging, (const zipc_hip_stream_desc *)inner, (zipc_hip_stream_result *)staged, n, max_src_len,
                                total_src_len, level, crc_op);
  if (st) return st;
  ZD_LAUNCH(ctx, "dpacked_layout", dpacked_layout_kernel, dim3(1), dim3(DPACKED_TILE), 0, (const uint32_t *)stage_status,
            (const StreamResult *)staged, (uint32_t)n, (uint64_t)align, (uint64_t)dst_arena_len, verdicts, seg_base, call, d_need);
  HIP_TRY(ctx, hipGetLastError());
  const uint64_t grid = dpacked_copy_grid(n, total_src_len, zlib);  // (at most 0x7FFFFFFF: dpacked_call_status)
  ZD_LAUNCH(ctx, "dpacked_copy", dpacked_copy_kernel, dim3((unsigned)grid), dim3(DPACKED_COPY_THREADS), 0, (const uint8_t *)staging,
            (uint8_t *)d_dst_arena, (const StreamDesc *)inner, (const StreamResult *)staged, (const PackedVerdict *)verdicts,
            (const uint32_t *)seg_base, (uint32_t)n, (const DpackedCall *)call);
  HIP_TRY(ctx, hipGetLastError());
  ZD_LAUNCH(ctx, "dpacked_close", dpacked_close_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (uint32_t)n,
            (const PackedVerdict *)verdicts, (const uint32_t *)stage_status, (const StreamResult *)staged, crc_op, (PackedResult *)d_results);
  HIP_TRY(ctx, hipGetLastError());
  return ZIPC_HIP_OK;
}

}  // namespace zd
