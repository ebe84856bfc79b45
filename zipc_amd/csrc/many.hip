// many.hip -- the many-stream host forms of include/zipc_hip.h (zipc_hip_deflate_many, _inflate_many, _inflate_many_check,
// _recode_many, _zlib_compress_many, _zlib_decompress_many): the device half of their pipeline and the entry points.
//
// The rule of a call -- where every stream lies in the staging arenas, how the call is cut into sub-batches, what the
// largest of them needs -- is host_pipeline.h's plan_many, free of HIP; the host threads that gather, feed, take back
// and scatter are that header's many_pipeline.  What is here: the two kernels of the way back, the reservations sized by
// the plan, the five callbacks that put a sub-batch's copies, kernels and events on three HIP queues, and the checks
// and guards around the C entry points.  The kernels' step itself is the batch forms' (api.hip, recode.hip).
#include <stdio.h>
#include <string.h>

#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "ctx.h"
#include "host_pipeline.h"
#include "inflate_blocks.h"
#include "tuning.h"
#include "zlib_container.h"

using namespace zd;
using namespace zd_host;

static_assert(sizeof(StreamResult) == sizeof(zipc_hip_stream_result), "result layout");
// (the checksum form's results travel through the pipeline in the plain results' place: status on status, crc32 on
// checksum, adler32 and reserved on out_len)
static_assert(sizeof(zipc_hip_checksum_result) == sizeof(zipc_hip_stream_result) && sizeof(zipc_hip_range) == sizeof(Range), "checksum layouts");

// ---- the way back: a sub-batch's outputs end to end, written by a kernel -------------------------------------------
// What a sub-batch made goes into the pinned host buffer by a KERNEL's stores, one output behind the other on 16-byte
// boundaries, not by the copy engine:
//  * how many bytes that is is known on the device when the kernels are through -- deflate's destination slots are as
//    large as the caller's capacities (the bound: more than the source), what is in them is half of that or less; an
//    engine copy's size would have to come from the host, which would have to wait for the results first;
//  * on this pool an engine copy out beside an engine copy in runs at a third of the bus whenever no kernel happens to
//    be running (tools/probes/host_copy.hip, profiles/r05_host_copy.txt: 256 MiB each way 13.4 / 14.1 ms, 4.8 / 5.5 with
//    a kernel spinning beside them; a kernel's stores beside an engine copy in: 5.3 / 6.3): the calls took 8 or 15 ms,
//    30 or 55, from one process to the next.
// The price: stores that wait for the bus hold up the memory path they share with everybody else (the same probe: a
// kernel that copies device memory takes 2.9 ms instead of 1.5 beside 8 such workgroups, 5.9 beside 64), so the kernel
// is as few workgroups as fill the bus.  The host makes the same sums from the results (host_pipeline.h packed_size).
extern "C" {

// off[i] = base + the packed sizes of streams [0, i), i = 0 .. n (one workgroup)
__global__ __launch_bounds__(1024) void pack_offsets_kernel(const StreamDesc *descs, const StreamResult *res, uint32_t n,
                                                            uint64_t base, uint64_t *off) {
  __shared__ uint64_t part[1024];
  const uint32_t per = (n + 1023) / 1024, lo = threadIdx.x * per, hi = lo + per < n ? lo + per : n;
  uint64_t sum = 0;
  for (uint32_t i = lo; i < hi; i++) sum += packed_size(res[i].status, res[i].out_len, descs[i].dst_cap);
  part[threadIdx.x] = sum;
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d *= 2) {
    const uint64_t v = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  uint64_t at = base + part[threadIdx.x] - sum;
  for (uint32_t i = lo; i < hi; i++) {
    off[i] = at;
    at += packed_size(res[i].status, res[i].out_len, descs[i].dst_cap);
  }
  if (threadIdx.x == 1023) off[n] = base + part[1023];
}

// Workgroup w of G moves the w-th part of the packed bytes (parts of whole 4 KiB): the stream its part begins in is
// found by bisection of off[], the next ones follow; every thread moves 16 bytes at a time, four loads in flight (slots
// begin on 256-byte boundaries).
constexpr unsigned PACK_COPY_WGS = 6;
__global__ __launch_bounds__(256) void pack_copy_kernel(const uint8_t *dst_arena, uint8_t *pack_arena, const StreamDesc *descs,
                                                        const uint64_t *off, uint32_t n, uint64_t base) {
  const uint64_t total_end = off[n];
  const uint64_t per = ((total_end - base + gridDim.x - 1) / gridDim.x + 4095) / 4096 * 4096;
  uint64_t pos = base + blockIdx.x * per;
  if (pos >= total_end) return;
  const uint64_t end = total_end - pos < per ? total_end : pos + per;
  uint32_t a = 0, b = n;  // the last stream that begins at or before pos
  while (b - a > 1) {
    const uint32_t m = a + (b - a) / 2;
    if (off[m] <= pos) a = m; else b = m;
  }
  for (uint32_t s = a; s < n && pos < end; s++) {
    const uint64_t s_beg = off[s], s_end = off[s + 1] < end ? off[s + 1] : end;
    if (s_end <= pos) continue;  // (a stream with nothing to hand over)
    const uint4 *from = (const uint4 *)(dst_arena + descs[s].dst_off + (pos - s_beg));
    uint4 *to = (uint4 *)(pack_arena + pos);
    const uint64_t n16 = (s_end - pos) / 16;
    uint64_t i = threadIdx.x;
    for (; i + 768 < n16; i += 1024) {
      const uint4 v0 = from[i], v1 = from[i + 256], v2 = from[i + 512], v3 = from[i + 768];
      to[i] = v0; to[i + 256] = v1; to[i + 512] = v2; to[i + 768] = v3;
    }
    for (; i < n16; i += 256) to[i] = from[i];
    pos = s_end;
  }
}

}  // extern "C"

// ---- the host's threads --------------------------------------------------------------------------------------------

// host-side loop over streams [lo, hi) of a batch on a few threads (memcpy bound).
// ZIPC_HIP_HOST_THREADS overrides the count (default: 8 or the core count, if lower).
static size_t host_threads() {
  static const size_t nt = [] {
    long v = zd::tuning().host_threads;
    if (v < 1) {
      const unsigned hw = std::thread::hardware_concurrency();
      v = hw >= 8 ? 8 : (hw ? hw : 1);
    }
    return (size_t)(v > 64 ? 64 : v);
  }();
  return nt;
}
// The threads behind the host memcpys of the many-stream forms, the copies that go around the cache and the pipeline of a
// call's sub-batches live in host_pipeline.h (no HIP in it: tests/host_sim compiles the same code under the thread and
// address sanitizers with host threads standing in for the device).  The pools are shared by the process's contexts,
// made on first use, and their threads are joined when the last context is destroyed.
static Pools &host_pools() {
  static Pools *const p = new Pools;  // (the object outlives every context; its threads do not)
  return *p;
}
void zd::many_pools_acquire() { host_pools().acquire(); }
void zd::many_pools_release() { host_pools().release(); }

// ---- the device's part of the pipeline (host_pipeline.h Device) -----------------------------------------------------

// events of one call, destroyed on every exit path
struct EventSet {
  std::vector<hipEvent_t> ev;
  ~EventSet() { for (auto e : ev) (void)hipEventDestroy(e); }
  hipError_t make(size_t k, bool timed = false) {
    for (size_t i = 0; i < k; i++) {
      hipEvent_t e;
      hipError_t r = hipEventCreateWithFlags(&e, timed ? hipEventDefault : hipEventDisableTiming);
      if (r != hipSuccess) return r;
      ev.push_back(e);
    }
    return hipSuccess;
  }
};

// a HIP call of a ManyDevice callback: a failure is written down in `error` and ends the callback
#define PIPE_TRY(expr)                                                                   \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess) {                                                              \
      error = std::string(#expr) + ": " + hipGetErrorString(_e);                         \
      return ZIPC_HIP_ERR_HIP;                                                           \
    }                                                                                    \
  } while (0)

// Copies, kernels and events on three queues.  From begin() on, work is in flight that reads the plan's descriptors and
// the pinned buffers and records into the event sets: many_pipeline returns only when its second thread is through, and
// after a failure all three queues are waited for (many_drain) before anything is freed or the next call reuses the buffers.
struct ManyDevice {
  zipc_hip_ctx *const ctx;
  const ManyOp op;
  const ManyPlan &plan;
  const int level, crc_op;
  const bool packed, want_bytes, timing;
  bool first_batch = true;
  EventSet ev_in, ev_k, ev_out;  // a sub-batch's sources are in, its kernels through, its outputs back
  EventSet ev_t;                 // timing: the call's begin on the device, a sub-batch's first copy in, its kernels' begin
  std::string error;

  ManyDevice(zipc_hip_ctx *ctx_, ManyOp op_, const ManyPlan &plan_, int level_, int crc_op_, bool packed_, bool want_bytes_, bool timing_)
      : ctx(ctx_), op(op_), plan(plan_), level(level_), crc_op(crc_op_), packed(packed_), want_bytes(want_bytes_), timing(timing_) {}

  // the call's events; then earlier work of this context (the previous call's kernels read io_src / io_desc; a call that
  // failed half way may have left copies on the two copy streams) first
  int ready() {
    const size_t K = plan.K();
    HIP_TRY(ctx, ev_in.make(K, timing));
    HIP_TRY(ctx, ev_k.make(K, timing));
    HIP_TRY(ctx, ev_out.make(K, timing));
    if (timing) HIP_TRY(ctx, ev_t.make(1 + 2 * K, true));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->copy_in));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->copy_out));
    return ZIPC_HIP_OK;
  }
  int begin() {
    const size_t n = plan.descs.size();
    if (timing) PIPE_TRY(hipEventRecord(ev_t.ev[0], ctx->copy_in));
    PIPE_TRY(hipMemcpyAsync(ctx->io_desc.p, plan.descs.data(), n * sizeof(StreamDesc), hipMemcpyHostToDevice, ctx->copy_in));
    if (op == MANY_RECODE)
      PIPE_TRY(hipMemcpyAsync(ctx->io_rdesc.p, plan.rdescs.data(), n * sizeof(RecodeDesc), hipMemcpyHostToDevice, ctx->copy_in));
    if (op == MANY_CHECKSUM)
      PIPE_TRY(hipMemcpyAsync(ctx->io_ranges.p, plan.ranges.data(), n * sizeof(Range), hipMemcpyHostToDevice, ctx->copy_in));
    return ZIPC_HIP_OK;
  }
  int send(size_t g, bool first, uint64_t from, uint64_t to) {
    if (timing && first) PIPE_TRY(hipEventRecord(ev_t.ev[1 + 2 * g], ctx->copy_in));
    PIPE_TRY(hipMemcpyAsync((uint8_t *)ctx->io_src.p + from, (const uint8_t *)ctx->pin_src.p + from, to - from,
                            hipMemcpyHostToDevice, ctx->copy_in));
    return ZIPC_HIP_OK;
  }
  int sent(size_t g) {
    PIPE_TRY(hipEventRecord(ev_in.ev[g], ctx->copy_in));
    return ZIPC_HIP_OK;
  }
  int launch(size_t g, size_t lo, size_t hi) {
    PIPE_TRY(hipStreamWaitEvent(ctx->stream, ev_in.ev[g], 0));
    if (timing) PIPE_TRY(hipEventRecord(ev_t.ev[2 + 2 * g], ctx->stream));
    zipc_hip_stream_desc *dd = (zipc_hip_stream_desc *)ctx->io_desc.p + lo;
    zipc_hip_stream_result *dr = (zipc_hip_stream_result *)ctx->io_res.p + lo;
    int st;
    if (op == MANY_RECODE) {  // (the plain results the way back works with are recode_close_kernel's second output)
      size_t total_mid = 0;
      for (size_t i = lo; i < hi; i++) total_mid += plan.rdescs[i].mid_cap;
      st = launch_recode(ctx, ctx->io_src.p, ctx->io_mid.p, ctx->io_dst.p, (const RecodeDesc *)ctx->io_rdesc.p + lo,
                         (RecodeResult *)ctx->io_rres.p + lo, (StreamResult *)dr, hi - lo, plan.max_mid, total_mid, level,
                         plan.inflate_descs.data() + lo, first_batch);
      if (st == ZIPC_HIP_OK)
        PIPE_TRY(hipMemcpyAsync((RecodeResult *)ctx->pin_rres.p + lo, (const RecodeResult *)ctx->io_rres.p + lo,
                                (hi - lo) * sizeof(RecodeResult), hipMemcpyDeviceToHost, ctx->stream));
    } else if (op == MANY_CHECKSUM) {  // (level: the selectors, bit 0 the CRC-32's, bit 1 the Adler-32's; dr holds zipc_hip_checksum_results)
      size_t total_g = 0;
      for (size_t i = lo; i < hi; i++) total_g += plan.descs[i].src_len;
      st = zipc_hip_checksum_batch(ctx, ctx->io_src.p, plan.src_arena_end, (const zipc_hip_range *)ctx->io_ranges.p + lo,
                                   (zipc_hip_checksum_result *)dr, hi - lo, total_g, level & 1, level & 2);
    } else if (op == MANY_INFLATE) {  // (with the descriptors it has on the host: no read-back, nothing waited for unless a stream goes by blocks)
      st = launch_inflate(ctx, ctx->io_src.p, ctx->io_dst.p, dd, dr, hi - lo, plan.max_cap, crc_op, plan.descs.data() + lo, first_batch);
    } else {
      size_t total_g = 0;
      for (size_t i = lo; i < hi; i++) total_g += plan.descs[i].src_len;
      st = zipc_hip_deflate_batch(ctx, ctx->io_src.p, ctx->io_dst.p, dd, dr, hi - lo, plan.max_src, total_g, level, crc_op);
    }
    first_batch = false;
    if (st) { error = ctx->last_error; return st; }
    PIPE_TRY(hipMemcpyAsync((StreamResult *)ctx->pin_res.p + lo, dr, (hi - lo) * sizeof(StreamResult),
                            hipMemcpyDeviceToHost, ctx->stream));
    const uint64_t c = plan.dst_end(lo), e = plan.dst_end(hi);
    uint64_t *off = packed ? (uint64_t *)ctx->io_pack_off.p + lo + g : nullptr;
    if (packed)
      ZD_LAUNCH(ctx, "pack_offsets", pack_offsets_kernel, dim3(1), dim3(1024), 0, (const StreamDesc *)dd,
                (const StreamResult *)dr, (uint32_t)(hi - lo), c, off);
    PIPE_TRY(hipGetLastError());
    PIPE_TRY(hipEventRecord(ev_k.ev[g], ctx->stream));
    if (!want_bytes) {  // results only: they are on their way behind the kernels, nothing else comes back
      PIPE_TRY(hipEventRecord(ev_out.ev[g], ctx->stream));
      return ZIPC_HIP_OK;
    }
    PIPE_TRY(hipStreamWaitEvent(ctx->copy_out, ev_k.ev[g], 0));
    if (packed) {  // its stores ARE the copy back, of as many bytes as the device knows it made, beside the next sub-batch's kernels
      hipLaunchKernelGGL(pack_copy_kernel, dim3(PACK_COPY_WGS), dim3(256), 0, ctx->copy_out,
                         (const uint8_t *)ctx->io_dst.p, (uint8_t *)ctx->pin_dst.p, (const StreamDesc *)dd,
                         (const uint64_t *)off, (uint32_t)(hi - lo), c);
      PIPE_TRY(hipGetLastError());
    } else {
      PIPE_TRY(hipMemcpyAsync((uint8_t *)ctx->pin_dst.p + c, (const uint8_t *)ctx->io_dst.p + c, e - c,
                              hipMemcpyDeviceToHost, ctx->copy_out));
    }
    PIPE_TRY(hipEventRecord(ev_out.ev[g], ctx->copy_out));
    return ZIPC_HIP_OK;
  }
  int wait_back(size_t g) {  // (the taker's thread)
    PIPE_TRY(hipSetDevice(ctx->device));
    PIPE_TRY(hipEventSynchronize(ev_out.ev[g]));  // (behind ev_k[g]: the results have landed too)
    return ZIPC_HIP_OK;
  }
};
#undef PIPE_TRY

// ---- one call, step by step ------------------------------------------------------------------------------------------

constexpr uint32_t RESULT_UNSET = 0xFFFFFFFFu;  // a status no call gives: an entry nothing has written yet

// every entry of results[] carries `status` and nothing else; returns status
template <class Result>
static int fill_results(Result *results, size_t n, int status) {
  if (results)
    for (size_t i = 0; i < n; i++) {
      results[i] = Result{};
      results[i].status = (uint32_t)status;
    }
  return status;
}

// the arrays of a call and what each stream's entries point at (want_bytes false: results only, dst may be null)
static bool many_pointers_ok(const zipc_hip_ctx *ctx, size_t n, const void *const *src, const size_t *src_len, void *const *dst,
                             const size_t *dst_cap, const void *results, bool want_bytes) {
  if (!ctx) return false;
  if (n == 0) return true;
  if (!src || !src_len || (!dst && want_bytes) || !dst_cap || !results) return false;
  for (size_t i = 0; i < n; i++)
    if ((!src[i] && src_len[i]) || (want_bytes && !dst[i] && dst_cap[i])) return false;
  return true;
}

// Everything is allocated before the first sub-batch is under way (growing a buffer synchronises the stream): the
// staging arenas and their pinned mirrors, the descriptor and result tables, and what the largest sub-batch's kernels
// need of the context's scratch.
static int many_reserve(zipc_hip_ctx *ctx, ManyOp op, const ManyPlan &plan, int level, int crc_op, bool packed, bool want_bytes) {
  const size_t n = plan.descs.size();
  HIP_TRY(ctx, ctx->ensure(ctx->io_src, plan.src_arena_end + 64));
  HIP_TRY(ctx, ctx->ensure(ctx->io_dst, plan.dst_arena_end + 64));
  HIP_TRY(ctx, ctx->ensure(ctx->io_desc, n * sizeof(StreamDesc)));
  HIP_TRY(ctx, ctx->ensure(ctx->io_res, n * sizeof(StreamResult)));
  if (packed) HIP_TRY(ctx, ctx->ensure(ctx->io_pack_off, (n + plan.K() + 1) * sizeof(uint64_t)));
  HIP_TRY(ctx, ctx->ensure_pinned(ctx->pin_src, plan.src_arena_end + 64));
  if (want_bytes) HIP_TRY(ctx, ctx->ensure_pinned(ctx->pin_dst, plan.dst_arena_end + 64));
  HIP_TRY(ctx, ctx->ensure_pinned(ctx->pin_res, n * sizeof(StreamResult)));
  if (op == MANY_RECODE) {
    HIP_TRY(ctx, ctx->ensure(ctx->io_mid, plan.mid_arena + 64));
    HIP_TRY(ctx, ctx->ensure(ctx->io_rdesc, n * sizeof(RecodeDesc)));
    HIP_TRY(ctx, ctx->ensure(ctx->io_rres, n * sizeof(RecodeResult)));
    HIP_TRY(ctx, ctx->ensure_pinned(ctx->pin_rres, n * sizeof(RecodeResult)));
    memset(ctx->pin_rres.p, 0xFF, n * sizeof(RecodeResult));  // (RESULT_UNSET: what has not come back says so)
    int st = recode_reserve(ctx, plan.n_max);
    if (st) return st;
    st = zipc_hip_reserve(ctx, plan.n_max, plan.max_mid, plan.mid_total_max);
    if (st) return st;
  }
  if (op == MANY_CHECKSUM) {  // (level: launch()'s selectors)
    HIP_TRY(ctx, ctx->ensure(ctx->io_ranges, n * sizeof(Range)));
    const int st = checksum_ranges_reserve(ctx, plan.n_max, plan.total_max, level & 2);
    if (st) return st;
  } else if (op == MANY_DEFLATE) {
    const int st = zipc_hip_reserve(ctx, plan.n_max, plan.max_src, plan.total_max);
    if (st) return st;
  } else {
    HIP_TRY(ctx, ctx->ensure(ctx->inflate_scratch, plan.n_max * INFLATE_SCRATCH_PER_STREAM));
  }
  if (crc_op == ZIPC_HIP_CRC_CRC32) {
    const size_t longest = op == MANY_RECODE ? plan.max_mid : op == MANY_INFLATE ? plan.max_cap : plan.max_src;
    HIP_TRY(ctx, ctx->ensure(ctx->crc_partials, plan.n_max * crc32_segs(longest) * sizeof(uint32_t)));
  }
  if (!ctx->copy_in) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->copy_in, hipStreamNonBlocking));
  if (!ctx->copy_out) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->copy_out, hipStreamNonBlocking));
  return ZIPC_HIP_OK;
}

// a batch call refused its arguments or a HIP call failed: the call fails as a whole (sub-batches scattered before that
// stay where they are, with their results; every other entry of results[] carries the call's status and no bytes)
static int many_drain(zipc_hip_ctx *ctx, int status, const std::string &why) {
  (void)hipStreamSynchronize(ctx->copy_in);
  (void)hipStreamSynchronize(ctx->stream);
  (void)hipStreamSynchronize(ctx->copy_out);
  ctx->last_error = why;
  return status;
}

// ZIPC_HIP_HOST_TIMING: where each sub-batch was when -- host clock from the call's begin, device clock from the first copy's begin
static void many_report(const ManyDevice &dev, const ManyTimes &times, double ms_setup, double ms_whole) {
  const ManyPlan &plan = dev.plan;
  const size_t K = plan.K();
  fprintf(stderr, "zipc_hip %s_many n=%zu src_arena=%llu dst_arena=%llu ms: setup %.2f feed %.2f (of it gather %.2f) "
                  "scatter %.2f whole %.2f (threads %zu sub-batches %zu)\n",
          dev.op == MANY_CHECKSUM ? "checksum" : dev.op == MANY_RECODE ? "recode" : dev.op == MANY_INFLATE ? "inflate" : "deflate", plan.descs.size(),
          (unsigned long long)plan.src_arena_end, (unsigned long long)plan.dst_arena_end, ms_setup, times.ms_feed,
          times.ms_gather, times.ms_scatter, ms_whole, host_threads(), K);
  for (size_t g = 0; g < K; g++) {
    if (plan.cut[g] == plan.cut[g + 1]) continue;
    float h0 = 0, h1 = 0, k0 = 0, k1 = 0, o1 = 0;
    (void)hipEventElapsedTime(&h0, dev.ev_t.ev[0], dev.ev_t.ev[1 + 2 * g]);
    (void)hipEventElapsedTime(&h1, dev.ev_t.ev[0], dev.ev_in.ev[g]);
    (void)hipEventElapsedTime(&k0, dev.ev_t.ev[0], dev.ev_t.ev[2 + 2 * g]);
    (void)hipEventElapsedTime(&k1, dev.ev_t.ev[0], dev.ev_k.ev[g]);
    (void)hipEventElapsedTime(&o1, dev.ev_t.ev[0], dev.ev_out.ev[g]);
    fprintf(stderr, "  sub-batch %zu (%zu streams): host gathered at %.2f, scatter %.2f - %.2f | device copy in %.2f - %.2f, "
                    "kernels %.2f - %.2f, back by %.2f\n",
            g, plan.cut[g + 1] - plan.cut[g], times.gathered[g], times.scatter_begin[g], times.scatter_end[g], h0, h1, k0, k1, o1);
  }
}

// n host-resident streams through the batch kernels: the arenas are the context's staging buffers, the streams lie in
// them as plan_many says, and sub-batch g goes through
//   gather (host threads, into pinned memory) -> copy in (the engine, queue copy_in, in runs of 16 MiB as they are
//   gathered) -> kernels (the context's queue) -> the way back (the kernel above, queue copy_out) -> scatter (host threads)
// on its own, so the bus and the kernels of one sub-batch run under the host memcpys of the others; PCIe is full
// duplex and the kernels do not touch it.  This thread gathers and feeds the device; a second one (many_pipeline's
// taker) waits for what comes back and scatters it with threads of its own, so the first sub-batch's results are in the
// caller's buffers while the last one's sources are still being gathered.  Thousands of small pageable copies -- the
// first version of this function -- cost far more than the kernels.
// mid_cap, expect_crc32: MANY_RECODE's (expect_crc32 may be null).
static int many_streams(zipc_hip_ctx *ctx, ManyOp op, size_t n, const void *const *src, const size_t *src_len,
                        const size_t *limit, int level, int crc_op, void *const *dst, const size_t *dst_cap,
                        zipc_hip_stream_result *results, bool want_bytes = true, const size_t *mid_cap = nullptr,
                        const uint32_t *expect_crc32 = nullptr) {
  if (!many_pointers_ok(ctx, n, src, src_len, dst, dst_cap, results, want_bytes)) return ZIPC_HIP_ERR_INVALID_ARG;
  if (op == MANY_RECODE && n && !mid_cap) return ZIPC_HIP_ERR_INVALID_ARG;
  if (crc_op < 0 || crc_op > 3 || level < 0 || level > 3 || n > 0x7FFFFFFFull) return ZIPC_HIP_ERR_INVALID_ARG;
  if (n == 0) return ZIPC_HIP_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const Tuning &tun = zd::tuning();
  const auto t_begin = std::chrono::steady_clock::now();
  auto since_begin = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(); };
  const ManyPlan plan = plan_many(op, n, src_len, dst_cap, limit, mid_cap, expect_crc32, tun.host_chunks, tun.host_chunk_min);
  if (op == MANY_DEFLATE && plan.max_src > MAX_STREAM_LEN) return ZIPC_HIP_ERR_INVALID_ARG;  // (inflate reports it per stream)
  if (op == MANY_RECODE && plan.max_mid > MAX_STREAM_LEN) return ZIPC_HIP_ERR_INVALID_ARG;   // (zipc_hip_recode_batch's rule)
  const bool packed = tun.host_pack && want_bytes;  // (false: whole destination slots by the copy engine)
  int st = many_reserve(ctx, op, plan, level, crc_op, packed, want_bytes);
  if (st) return st;
  ManyDevice dev(ctx, op, plan, level, crc_op, packed, want_bytes, tun.host_timing);
  st = dev.ready();
  if (st) return st;
  const double ms_setup = since_begin();

  ManyJob<StreamDesc> job;
  job.n = n; job.src = src; job.src_len = src_len; job.dst = dst; job.dst_cap = dst_cap; job.results = results;
  job.take(plan); job.packed = packed; job.want_bytes = want_bytes;
  job.h2d_bytes = (uint64_t)16 << 20;  // (sources sent in runs of about 16 MiB as they are gathered)
  job.pin_src = (uint8_t *)ctx->pin_src.p; job.pin_dst = want_bytes ? (const uint8_t *)ctx->pin_dst.p : nullptr;
  job.pin_res = (const zipc_hip_stream_result *)ctx->pin_res.p;
  job.threads = host_threads();
  ManyTimes times;
  std::string why;
  st = many_pipeline(job, dev, host_pools(), why, dev.timing ? &times : nullptr);
  if (st) return many_drain(ctx, st, why);
  HIP_TRY(ctx, hipStreamSynchronize(ctx->copy_in));
  if (dev.timing) many_report(dev, times, ms_setup, since_begin());
  return ZIPC_HIP_OK;
}

// An entry point's body behind the C boundary.  Host vectors sized by n: whatever they throw -- bad_alloc when memory runs
// out, length_error, system_error from a mutex or a thread -- stays on this side: the call fails as out of memory, says
// so in zipc_hip_last_error, and every entry of results[] is defined.  Only the setup before the pipeline can throw:
// many_pipeline itself does not.
template <class Result, class Body>
static int many_guarded(zipc_hip_ctx *ctx, size_t n, Result *results, Body body) {
  try { return body(); }
  catch (...) {
    try { if (ctx) ctx->last_error = "zipc_hip: out of memory (or no thread) on the host while setting up a many-stream call"; } catch (...) {}
    return fill_results(results, n, ZIPC_HIP_ERR_NOMEM);
  }
}

// zipc_hip_recode_many: many_streams with the recode sequence as its kernels' step.  The pipeline works with plain
// results (status, checksum, out_len); the zipc_hip_recode_results come back beside them into pinned memory of their own
// (ctx->pin_rres), on the context's queue in front of the event the pipeline waits for before it takes a sub-batch.
//  * The call succeeded: every sub-batch was taken, and results[] is what came back.
//  * The call failed: the pipeline has overwritten the plain results of the sub-batches it did not take with the call's
//    status and no bytes, and does not say which those were.  A stream keeps what came back for it only where that says
//    the same as its plain result: an OK stream's plain result is OK only if its sub-batch was taken (its bytes are in
//    the caller's buffer), and a stream that stopped has no bytes either way, so its own verdict is as true as the
//    call's.  Every other entry carries the plain status at stage 0.
static int recode_many(zipc_hip_ctx *ctx, size_t n, const void *const *src, const size_t *src_len, const size_t *limit,
                       const uint32_t *expect_crc32, const size_t *mid_cap, int level, void *const *dst, const size_t *dst_cap,
                       zipc_hip_recode_result *results) {
  if (!many_pointers_ok(ctx, n, src, src_len, dst, dst_cap, results, true) || (n && !mid_cap) || level < 0 || level > 3)
    return fill_results(results, n, ZIPC_HIP_ERR_INVALID_ARG);
  if (n == 0) return ZIPC_HIP_OK;
  std::vector<zipc_hip_stream_result> plain(n, zipc_hip_stream_result{RESULT_UNSET, 0, 0});
  const int st = many_streams(ctx, MANY_RECODE, n, src, src_len, limit, level, ZIPC_HIP_CRC_CRC32, dst, dst_cap, plain.data(), true, mid_cap,
                              expect_crc32);
  const zipc_hip_recode_result *back = ctx->pin_rres.cap >= n * sizeof(RecodeResult) ? (const zipc_hip_recode_result *)ctx->pin_rres.p : nullptr;
  if (st == ZIPC_HIP_OK && back) {
    memcpy(results, back, n * sizeof *results);
    return st;
  }
  for (size_t i = 0; i < n; i++) {
    const zipc_hip_stream_result &p = plain[i];
    if (p.status == RESULT_UNSET) results[i] = zipc_hip_recode_result{(uint32_t)(st ? st : ZIPC_HIP_ERR_HIP), 0, 0, 0, 0, 0};  // (the pipeline never ran)
    else if (back && back[i].status == p.status && back[i].out_len == p.out_len) results[i] = back[i];
    else results[i] = zipc_hip_recode_result{p.status, 0, 0, 0, 0, 0};
  }
  return st;
}

// zipc_hip_checksum_many: many_streams with the ragged checksum pass as its kernels' step and nothing but results on
// the way back.  The pipeline carries plain results: a checksum result lies in one's place (status, crc32 as checksum,
// adler32 as out_len's low half), so the capacities it is told are 2^32 - 1 -- it takes an out_len above dst_cap for an
// overrun -- and plan_many gives the checksum form no destination arena whatever they say.  The selectors travel as
// `level` (bit 0: CRC-32, bit 1: Adler-32).  results[] is defined on every return.
static int checksum_many(zipc_hip_ctx *ctx, size_t n, const void *const *src, const size_t *src_len, int want_crc32, int want_adler32,
                         zipc_hip_checksum_result *results) {
  bool ok = ctx && (want_crc32 || want_adler32) && (n == 0 || (src && src_len && results));
  for (size_t i = 0; ok && i < n; i++) ok = src[i] || !src_len[i];
  if (!ok) return fill_results(results, n, ZIPC_HIP_ERR_INVALID_ARG);
  if (n == 0) return ZIPC_HIP_OK;
  const std::vector<size_t> caps(n, (size_t)0xFFFFFFFFu);
  std::vector<zipc_hip_stream_result> plain(n, zipc_hip_stream_result{RESULT_UNSET, 0, 0});
  const int st = many_streams(ctx, MANY_CHECKSUM, n, src, src_len, nullptr, (want_crc32 ? 1 : 0) | (want_adler32 ? 2 : 0), ZIPC_HIP_CRC_NOP,
                              nullptr, caps.data(), plain.data(), false);
  for (size_t i = 0; i < n; i++) {
    const zipc_hip_stream_result &p = plain[i];
    if (p.status == RESULT_UNSET) results[i] = zipc_hip_checksum_result{(uint32_t)(st ? st : ZIPC_HIP_ERR_HIP), 0, 0, 0};  // (the pipeline never ran)
    else results[i] = zipc_hip_checksum_result{p.status, p.checksum, (uint32_t)p.out_len, 0};
  }
  return st;
}

// The zlib container around many_streams (zlib_container.h has the rules): the same two steps as zlib.hip's kernels, on
// the host -- the streams' bodies (or the room behind their headers) go through it as raw streams, a stream that fails
// the container's check as one of no bytes and no room.  results[] is defined on every return: an entry the pipeline
// never wrote carries the call's status.
static int zlib_many(zipc_hip_ctx *ctx, bool decompress, size_t n, const void *const *src, const size_t *src_len, const size_t *limit,
                     int level, void *const *dst, const size_t *dst_cap, zipc_hip_stream_result *results) {
  if (!many_pointers_ok(ctx, n, src, src_len, dst, dst_cap, results, true) || level < 0 || level > 3)
    return fill_results(results, n, ZIPC_HIP_ERR_INVALID_ARG);
  if (n == 0) return ZIPC_HIP_OK;
  std::vector<const void *> in_src(src, src + n);
  std::vector<void *> in_dst(dst, dst + n);
  std::vector<size_t> in_len(src_len, src_len + n), in_cap(dst_cap, dst_cap + n);
  std::vector<ZlibPre> pre(n);
  for (size_t i = 0; i < n; i++) {
    const uint8_t *s = (const uint8_t *)src[i];
    ZlibPre &p = pre[i];
    p.expect = 0;
    if (decompress) {
      const bool whole = src_len[i] >= ZLIB_MIN_LEN;
      p.status = zlib_open_status(src_len[i], whole ? s[0] : 0, whole ? s[1] : 0);
      if (p.status == ST_OK) {
        p.expect = zlib_expect(s + src_len[i] - 4);
        in_src[i] = s + zlib_body_off(0);
        in_len[i] = (size_t)zlib_body_len(src_len[i]);
      }
    } else {
      p.status = dst_cap[i] < ZLIB_OVERHEAD ? (uint32_t)ST_DST_TOO_SMALL : (uint32_t)ST_OK;
      if (p.status == ST_OK) {
        in_dst[i] = (uint8_t *)dst[i] + zlib_payload_off(0);
        in_cap[i] = (size_t)zlib_payload_cap(dst_cap[i]);
      }
    }
    if (p.status != ST_OK) { in_len[i] = 0; in_cap[i] = 0; }
  }
  fill_results(results, n, (int)RESULT_UNSET);
  const int st = many_streams(ctx, decompress ? MANY_INFLATE : MANY_DEFLATE, n, in_src.data(), in_len.data(), decompress ? limit : nullptr, level,
                              zlib_crc_op(ctx), in_dst.data(), in_cap.data(), results);
  for (size_t i = 0; i < n; i++) {
    StreamResult inner{results[i].status, results[i].checksum, results[i].out_len};
    if (inner.status == RESULT_UNSET) { inner.status = (uint32_t)(st ? st : ZIPC_HIP_ERR_HIP); inner.checksum = 0; inner.out_len = 0; }
    StreamResult r;
    if (decompress) {
      r = zlib_close_decompress(pre[i].status, pre[i].expect, inner);
    } else {
      bool wrap;
      r = zlib_close_compress(pre[i].status, inner, &wrap);
      if (wrap) {
        uint8_t *o = (uint8_t *)dst[i];
        o[0] = (uint8_t)zlib_cmf();
        o[1] = (uint8_t)zlib_flg(level);
        zlib_put_trailer(o + 2 + inner.out_len, inner.checksum);
      }
    }
    results[i] = zipc_hip_stream_result{r.status, r.checksum, r.out_len};
  }
  return st;
}

extern "C" {

int zipc_hip_deflate_many(zipc_hip_ctx *ctx, size_t n, const void *const *src, const size_t *src_len, int level,
                          int crc_op, void *const *dst, const size_t *dst_cap, zipc_hip_stream_result *results) {
  return many_guarded(ctx, n, results, [&] { return many_streams(ctx, MANY_DEFLATE, n, src, src_len, nullptr, level, crc_op, dst, dst_cap, results); });
}
int zipc_hip_inflate_many(zipc_hip_ctx *ctx, size_t n, const void *const *src, const size_t *src_len,
                          const size_t *limit, int crc_op, void *const *dst, const size_t *dst_cap,
                          zipc_hip_stream_result *results) {
  return many_guarded(ctx, n, results, [&] { return many_streams(ctx, MANY_INFLATE, n, src, src_len, limit, 0, crc_op, dst, dst_cap, results); });
}
int zipc_hip_inflate_many_check(zipc_hip_ctx *ctx, size_t n, const void *const *src, const size_t *src_len,
                                const size_t *limit, int crc_op, const size_t *dst_cap, zipc_hip_stream_result *results) {
  return many_guarded(ctx, n, results, [&] { return many_streams(ctx, MANY_INFLATE, n, src, src_len, limit, 0, crc_op, nullptr, dst_cap, results, false); });
}
int zipc_hip_recode_many(zipc_hip_ctx *ctx, size_t n, const void *const *src, const size_t *src_len, const size_t *limit,
                         const uint32_t *expect_crc32, const size_t *mid_cap, int level, void *const *dst, const size_t *dst_cap,
                         zipc_hip_recode_result *results) {
  return many_guarded(ctx, n, results, [&] { return recode_many(ctx, n, src, src_len, limit, expect_crc32, mid_cap, level, dst, dst_cap, results); });
}
int zipc_hip_checksum_many(zipc_hip_ctx *ctx, size_t n, const void *const *src, const size_t *src_len, int want_crc32, int want_adler32,
                           zipc_hip_checksum_result *results) {
  return many_guarded(ctx, n, results, [&] { return checksum_many(ctx, n, src, src_len, want_crc32, want_adler32, results); });
}
int zipc_hip_zlib_decompress_many(zipc_hip_ctx *ctx, size_t n, const void *const *src, const size_t *src_len, const size_t *limit,
                                  void *const *dst, const size_t *dst_cap, zipc_hip_stream_result *results) {
  return many_guarded(ctx, n, results, [&] { return zlib_many(ctx, true, n, src, src_len, limit, 0, dst, dst_cap, results); });
}
int zipc_hip_zlib_compress_many(zipc_hip_ctx *ctx, size_t n, const void *const *src, const size_t *src_len, int level,
                                void *const *dst, const size_t *dst_cap, zipc_hip_stream_result *results) {
  return many_guarded(ctx, n, results, [&] { return zlib_many(ctx, false, n, src, src_len, nullptr, level, dst, dst_cap, results); });
}

}  // extern "C"
