// api.hip -- the C ABI of include/zipc_hip.h: the context and its scratch, tuning(), the CRC-32 pass and the checksum
// launches, the batch forms as argument checks around launch_deflate / launch_inflate (deflate.hip, inflate.hip), the
// host forms, the many-stream pipeline's device half, the zlib forms and the recode forms.
//
// Host forms stage one stream through device scratch and run the same kernels as
// the batch forms (a batch of one).  Nothing here computes on the CPU: with no
// usable device the calls fail with ZIPC_HIP_ERR_NO_DEVICE / ZIPC_HIP_ERR_HIP.

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <new>
#include <thread>
#include <vector>
#include "ctx.h"
#include "deflate_scratch.h"
#include "host_pipeline.h"
#include "inflate_blocks.h"
#include "recode_rules.h"
#include "tuning.h"
#include "zlib_container.h"

using namespace zd;

static_assert(sizeof(zipc_hip_stream_desc) == sizeof(StreamDesc), "desc layout");
static_assert(sizeof(zipc_hip_stream_result) == sizeof(StreamResult), "result layout");
static_assert(sizeof(zipc_hip_recode_desc) == sizeof(RecodeDesc) && sizeof(RecodeDesc) == 64, "recode desc layout");
static_assert(sizeof(zipc_hip_recode_result) == sizeof(RecodeResult) && sizeof(RecodeResult) == 32, "recode result layout");
static_assert(ZIPC_HIP_STREAM_EXPECT_CRC32 == STREAM_EXPECT_CRC32 && ZIPC_HIP_ERR_CHECKSUM == ST_CHECKSUM, "recode constants");

// ---- context internals -------------------------------------------------------

int zipc_hip_ctx::name_index(const char *name) {
  for (size_t i = 0; i < acc.size(); i++)
    if (acc[i].name == name) return (int)i;
  Acc a;
  a.name = name;
  acc.push_back(a);
  return (int)acc.size() - 1;
}

hipEvent_t zipc_hip_ctx::get_event() {
  if (!event_pool.empty()) {
    hipEvent_t e = event_pool.back();
    event_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}

void zipc_hip_ctx::begin(const char *, hipEvent_t &start) {
  start = get_event();
  (void)hipEventRecord(start, cur);
}

hipError_t zipc_hip_ctx::fork(size_t k) {
  while (side.size() < k) {
    hipStream_t s = nullptr;
    hipEvent_t e = nullptr;
    hipError_t r = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (r != hipSuccess) return r;
    r = hipEventCreateWithFlags(&e, hipEventDisableTiming);
    if (r != hipSuccess) { (void)hipStreamDestroy(s); return r; }
    side.push_back(s);
    side_done.push_back(e);
  }
  if (!fork_ev) {
    const hipError_t r = hipEventCreateWithFlags(&fork_ev, hipEventDisableTiming);
    if (r != hipSuccess) return r;
  }
  hipError_t r = hipEventRecord(fork_ev, stream);
  for (size_t i = 0; i < k && r == hipSuccess; i++) r = hipStreamWaitEvent(side[i], fork_ev, 0);
  return r;
}

hipError_t zipc_hip_ctx::join(size_t k) {
  hipError_t r = hipSuccess;
  for (size_t i = 0; i < k && r == hipSuccess; i++) {
    r = hipEventRecord(side_done[i], side[i]);
    if (r == hipSuccess) r = hipStreamWaitEvent(stream, side_done[i], 0);
  }
  cur = stream;
  return r;
}

void zipc_hip_ctx::end(const char *name, hipEvent_t start) {
  Pending p;
  p.name_idx = name_index(name);
  p.start = start;
  p.stop = get_event();
  (void)hipEventRecord(p.stop, cur);
  pending.push_back(p);
}

hipError_t zipc_hip_ctx::ensure_pinned(Buf &b, size_t bytes) {
  if (bytes <= b.cap && b.p) return hipSuccess;
  if (b.p) {
    hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return e;
    (void)hipHostFree(b.p);
    b.p = nullptr;
    b.cap = 0;
  }
  size_t want = bytes < 4096 ? 4096 : bytes;
  hipError_t e = hipHostMalloc(&b.p, want, hipHostMallocDefault);
  if (e != hipSuccess) { b.p = nullptr; return e; }
  b.cap = want;
  return hipSuccess;
}

hipError_t zipc_hip_ctx::ensure(Buf &b, size_t bytes) {
  if (bytes <= b.cap && b.p) return hipSuccess;
  if (b.p) {
    hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return e;
    (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
  }
  size_t want = bytes < 256 ? 256 : bytes;
  hipError_t e = hipMalloc(&b.p, want);
  if (e != hipSuccess) { b.p = nullptr; return e; }
  b.cap = want;
  return hipSuccess;
}

hipError_t zipc_hip_ctx::collect_times() {
  if (pending.empty()) return hipSuccess;
  hipError_t e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return e;
  for (auto &p : pending) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, p.start, p.stop) == hipSuccess) {
      acc[p.name_idx].launches++;
      acc[p.name_idx].total_ms += ms;
    }
    event_pool.push_back(p.start);
    event_pool.push_back(p.stop);
  }
  pending.clear();
  return hipSuccess;
}

void zd::free_buf(zipc_hip_ctx::Buf &b) {
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.cap = 0;
}

// ---- context API -------------------------------------------------------------

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
// ZIPC_HIP_HOST_CHUNKS: sub-batches a many-stream call is cut into; each goes through gather, copy in, kernels, the
// way back and scatter on its own, so those overlap (1 = one after the other).  Default: by the bytes staged (many_streams).
static size_t host_chunks(uint64_t staged_bytes) {
  long v = zd::tuning().host_chunks;
  if (v < 1) v = staged_bytes >= ((uint64_t)1 << 30) ? 6 : 4;
  return (size_t)(v > 64 ? 64 : v);
}
// The threads behind the host memcpys of the many-stream forms, the copies that go around the cache and the pipeline of a
// call's sub-batches live in host_pipeline.h (no HIP in it: tests/host_sim compiles the same code under the thread and
// address sanitizers with host threads standing in for the device).  The pools are shared by the process's contexts,
// made on first use, and their threads are joined when the last context is destroyed.
static zd_host::Pools &host_pools() {
  static zd_host::Pools *const p = new zd_host::Pools;  // (the object outlives every context; its threads do not)
  return *p;
}
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

namespace zd {
const Tuning &tuning() {
  static const Tuning t = [] {
    auto num = [](const char *name, long dflt) { const char *e = getenv(name); return e ? atol(e) : dflt; };
    auto is = [](const char *name, const char *v) { const char *e = getenv(name); return e && !strcmp(e, v); };
    Tuning x;
    x.chain_peel = is("ZIPC_HIP_CHAIN", "peel");
    x.parse_segments = num("ZIPC_HIP_PARSE_SEGMENTS", -1);
    x.parse_seg = num("ZIPC_HIP_PARSE_SEG", 0);
    x.match_tiles_per_group = num("ZIPC_HIP_MATCH_TILES_PER_GROUP", 0);
    const long form = num("ZIPC_HIP_MATCH_FORM", 0);
    x.match_form = form == 1 || form == 2 ? (int)form : 0;
    const long long group = getenv("ZIPC_HIP_DEFLATE_GROUP_BYTES") ? atoll(getenv("ZIPC_HIP_DEFLATE_GROUP_BYTES")) : 0;
    x.deflate_group_bytes = group > 0 ? (size_t)group : (size_t)8 << 30;
    x.slices = num("ZIPC_HIP_SLICES", 0);
    x.slice_min = num("ZIPC_HIP_SLICE_MIN", 0);
    x.inflate_blocks = num("ZIPC_HIP_INFLATE_BLOCKS", 1) != 0;
    x.inflate_follow = (int)num("ZIPC_HIP_INFLATE_FOLLOW", -1);
    x.explore_stride = (uint64_t)num("ZIPC_HIP_EXPLORE_STRIDE", 16384);
    if (x.explore_stride < 1024) x.explore_stride = 1024;  // (a divisor: never 0 or negative, whatever the environment says)
    x.resolve_hops0 = (int)num("ZIPC_HIP_RESOLVE_HOPS0", 256);
    x.resolve_hops1 = (int)num("ZIPC_HIP_RESOLVE_HOPS1", 256);
    x.host_threads = num("ZIPC_HIP_HOST_THREADS", 0);
    x.host_chunks = num("ZIPC_HIP_HOST_CHUNKS", 0);
    x.host_chunk_min = num("ZIPC_HIP_HOST_CHUNK_MIN", 1024);
    if (x.host_chunk_min < 1) x.host_chunk_min = 1;
    x.host_pack = num("ZIPC_HIP_HOST_PACK", 1) != 0;
    x.host_timing = num("ZIPC_HIP_HOST_TIMING", 0) != 0;
    return x;
  }();
  return t;
}
static long g_slices_override = 0;  // zipc_hip_debug_set_slices: measurements that want every kernel alone on the device
long debug_slices_override() { return g_slices_override; }
size_t crc32_segs(size_t max_len) {
  const size_t segs = (max_len + CRC_SEG_BYTES - 1) / CRC_SEG_BYTES;
  return segs ? segs : 1;
}
hipError_t crc32_segments_launch(zipc_hip_ctx *ctx, const uint8_t *base, int mode, const StreamDesc *d_descs,
                                 const StreamResult *d_results, size_t n_ranges, uint64_t single_off,
                                 uint64_t single_len, size_t max_len, uint32_t *partials) {
  const size_t segs = crc32_segs(max_len);
  if (n_ranges * segs > 0x7FFFFFFFull) return hipErrorInvalidValue;
  ZD_LAUNCH(ctx, "crc32_segments", crc32_segments_kernel, dim3((unsigned)(n_ranges * segs)), dim3(256), 0,
            base, mode, d_descs, d_results, single_off, single_len, (uint32_t)segs, (const uint32_t *)ctx->crc_nib.p,
            partials);
  return hipGetLastError();
}
hipError_t crc32_finish_launch(zipc_hip_ctx *ctx, int mode, const StreamDesc *d_descs, StreamResult *d_results,
                               size_t n_ranges, uint64_t single_len, size_t max_len, const uint32_t *partials,
                               uint32_t *d_single_out) {
  const size_t segs = crc32_segs(max_len);
  if (mode != RANGE_SINGLE && segs <= 16)  // a batch of short streams: one per thread
    ZD_LAUNCH(ctx, "crc32_finish", crc32_finish_streams_kernel, dim3((unsigned)((n_ranges + 255) / 256)), dim3(256), 0,
              mode, d_descs, d_results, (uint32_t)n_ranges, (uint32_t)segs, ctx->crc_consts, partials);
  else
    ZD_LAUNCH(ctx, "crc32_finish", crc32_finish_kernel, dim3((unsigned)n_ranges), dim3(crc_finish_threads(segs)), 0, mode,
              d_descs, d_results, single_len, (uint32_t)segs, ctx->crc_consts, (const uint32_t *)ctx->crc_nib.p,
              partials, d_single_out);
  return hipGetLastError();
}
int crc32_pass(zipc_hip_ctx *ctx, const uint8_t *base, int mode, const StreamDesc *d_descs,
               StreamResult *d_results, size_t n_ranges, uint64_t single_off,
               uint64_t single_len, size_t max_len, uint32_t *d_single_out, size_t partials_at,
               bool ensured) {
  const size_t segs = crc32_segs(max_len);
  if (n_ranges * segs > 0x7FFFFFFFull) return ZIPC_HIP_ERR_INVALID_ARG;
  if (!ensured) HIP_TRY(ctx, ctx->ensure(ctx->crc_partials, (partials_at + n_ranges * segs) * sizeof(uint32_t)));
  uint32_t *partials = (uint32_t *)ctx->crc_partials.p + partials_at;
  HIP_TRY(ctx, crc32_segments_launch(ctx, base, mode, d_descs, (const StreamResult *)d_results, n_ranges, single_off,
                                     single_len, max_len, partials));
  HIP_TRY(ctx, crc32_finish_launch(ctx, mode, d_descs, d_results, n_ranges, single_len, max_len, partials, d_single_out));
  return ZIPC_HIP_OK;
}
}  // namespace zd

extern "C" {

int zipc_hip_abi_version(void) { return ZIPC_HIP_ABI_VERSION; }

int zipc_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char *zipc_hip_strerror(int status) {
  switch (status) {
  case ZIPC_HIP_OK: return "";
  case ZIPC_HIP_ERR_CORRUPTED: return "Corrupted data stream";
  case ZIPC_HIP_ERR_SIZE_EXCEEDED: return "Expected decompression size exceeded";
  case ZIPC_HIP_ERR_ZLIB_METHOD: return "Unknown compression method (%d)";
  case ZIPC_HIP_ERR_ZLIB_WINDOW: return "Window size too large";
  case ZIPC_HIP_ERR_ZLIB_DICT: return "Preset dictionary unsupported";
  case ZIPC_HIP_ERR_CHECKSUM: return "Checksum mismatch, expected %lx found %lx)";
  case ZIPC_HIP_ERR_DST_TOO_SMALL: return "destination buffer too small";
  case ZIPC_HIP_ERR_HIP: return "HIP runtime error";
  case ZIPC_HIP_ERR_INVALID_ARG: return "invalid argument";
  case ZIPC_HIP_ERR_NO_DEVICE: return "no usable HIP device";
  case ZIPC_HIP_ERR_NOMEM: return "out of memory";
  default: return "unknown status";
  }
}

int zipc_hip_create(zipc_hip_ctx **out, int device) {
  if (!out) return ZIPC_HIP_ERR_INVALID_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return ZIPC_HIP_ERR_NO_DEVICE;
  if (device < 0 || device >= n) return ZIPC_HIP_ERR_INVALID_ARG;
  if (hipSetDevice(device) != hipSuccess) return ZIPC_HIP_ERR_HIP;
  zipc_hip_ctx *ctx = new (std::nothrow) zipc_hip_ctx();
  if (!ctx) return ZIPC_HIP_ERR_NOMEM;
  ctx->device = device;
  if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
    delete ctx;
    return ZIPC_HIP_ERR_HIP;
  }
  ctx->cur = ctx->stream;
  host_pools().acquire();  // (released by zipc_hip_destroy: the last context to go joins the staging threads)
  // CRC merge constants (zd_common.h), computed with the same GF(2) routines the
  // kernels use
  uint32_t x = gf2_xpow8n(CRC_PIECE_BYTES);
  for (int k = 0; k < 8; k++) { ctx->crc_consts.xpiece[k] = x; x = gf2_mul(x, x); }
  ctx->crc_consts.xseg = gf2_xpow8n(CRC_SEG_BYTES);
  x = 0x00800000u;  // x^8
  for (int k = 0; k < 48; k++) { ctx->crc_consts.xbyte[k] = x; x = gf2_mul(x, x); }
  {
    std::vector<uint32_t> nib((size_t)CRC_NIB_CONSTS * GF2_NIB_WORDS);
    for (int k = 0; k < 8; k++) gf2_nib_table(ctx->crc_consts.xpiece[k], nib.data() + (size_t)k * GF2_NIB_WORDS);
    gf2_nib_table(ctx->crc_consts.xseg, nib.data() + (size_t)CRC_NIB_XSEG * GF2_NIB_WORDS);
    if (ctx->ensure(ctx->crc_nib, nib.size() * sizeof(uint32_t)) != hipSuccess ||
        hipMemcpy(ctx->crc_nib.p, nib.data(), nib.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) {
      zipc_hip_destroy(ctx);
      return ZIPC_HIP_ERR_HIP;
    }
  }
  ctx->xchg_ordered = zd::xchg_order_probe(ctx);
  *out = ctx;
  return ZIPC_HIP_OK;
}

void zipc_hip_destroy(zipc_hip_ctx *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  for (auto &p : ctx->pending) { (void)hipEventDestroy(p.start); (void)hipEventDestroy(p.stop); }
  for (auto e : ctx->event_pool) (void)hipEventDestroy(e);
  free_buf(ctx->io_src); free_buf(ctx->io_dst); free_buf(ctx->io_desc); free_buf(ctx->io_res);
  free_buf(ctx->io_pack_off);
  free_buf(ctx->io_small); free_buf(ctx->crc_partials); free_buf(ctx->crc_nib); free_buf(ctx->adler_sums);
  free_buf(ctx->deflate_scratch); free_buf(ctx->parse_scratch);
  free_buf(ctx->inflate_scratch);
  free_buf(ctx->blocks_scratch);
  free_buf(ctx->tok_scratch);
  free_buf(ctx->descs_marked);
  free_buf(ctx->zlib_descs); free_buf(ctx->zlib_pre);
  free_buf(ctx->recode_descs); free_buf(ctx->recode_res); free_buf(ctx->recode_verdicts);
  free_buf(ctx->io_mid); free_buf(ctx->io_rdesc); free_buf(ctx->io_rres);
  free_buf(ctx->stored_list);
  free_buf(ctx->chain_check_links);
  if (ctx->chain_check_host) (void)hipHostFree(ctx->chain_check_host);
  if (ctx->pin_src.p) (void)hipHostFree(ctx->pin_src.p);
  if (ctx->pin_dst.p) (void)hipHostFree(ctx->pin_dst.p);
  if (ctx->pin_res.p) (void)hipHostFree(ctx->pin_res.p);
  if (ctx->pin_rres.p) (void)hipHostFree(ctx->pin_rres.p);
  if (ctx->copy_in) (void)hipStreamDestroy(ctx->copy_in);
  if (ctx->copy_out) (void)hipStreamDestroy(ctx->copy_out);
  for (auto s : ctx->side) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
  for (auto e : ctx->side_done) (void)hipEventDestroy(e);
  if (ctx->fork_ev) (void)hipEventDestroy(ctx->fork_ev);
  (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  host_pools().release();
}

void *zipc_hip_stream(zipc_hip_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

int zipc_hip_synchronize(zipc_hip_ctx *ctx) {
  if (!ctx) return ZIPC_HIP_ERR_INVALID_ARG;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return ZIPC_HIP_OK;
}

const char *zipc_hip_last_error(zipc_hip_ctx *ctx) { return ctx ? ctx->last_error.c_str() : ""; }
unsigned zipc_hip_last_inflate_blocks(zipc_hip_ctx *ctx) { return ctx ? ctx->last_inflate_blocks : 0u; }
int zipc_hip_lds_exchange_ordered(zipc_hip_ctx *ctx) { return ctx && ctx->xchg_ordered ? 1 : 0; }
int zipc_hip_chain_check(zipc_hip_ctx *ctx, unsigned long long *compared, unsigned long long *differences) {
  if (!ctx || !compared || !differences) return ZIPC_HIP_ERR_INVALID_ARG;
  *compared = *differences = 0;
  if (!ctx->chain_check_host) return ZIPC_HIP_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *compared = ctx->chain_check_host[1] + ctx->chain_check_host[3];
  *differences = ctx->chain_check_host[0] + ctx->chain_check_host[2];
  return ZIPC_HIP_OK;
}
void zipc_hip_debug_set_slices(long k) { zd::g_slices_override = k; }

int zipc_hip_set_adler_rfc1950(zipc_hip_ctx *ctx, int enabled) {
  if (!ctx) return ZIPC_HIP_ERR_INVALID_ARG;
  ctx->adler_rfc1950 = enabled != 0;
  return ZIPC_HIP_OK;
}

int zipc_hip_set_profiling(zipc_hip_ctx *ctx, int enabled) {
  if (!ctx) return ZIPC_HIP_ERR_INVALID_ARG;
  HIP_TRY(ctx, ctx->collect_times());
  ctx->profiling = enabled != 0;
  return ZIPC_HIP_OK;
}

int zipc_hip_reset_kernel_times(zipc_hip_ctx *ctx) {
  if (!ctx) return ZIPC_HIP_ERR_INVALID_ARG;
  HIP_TRY(ctx, ctx->collect_times());
  for (auto &a : ctx->acc) { a.launches = 0; a.total_ms = 0; }
  return ZIPC_HIP_OK;
}

int zipc_hip_kernel_times(zipc_hip_ctx *ctx, zipc_hip_kernel_time *out, size_t cap, size_t *n) {
  if (!ctx || !n) return ZIPC_HIP_ERR_INVALID_ARG;
  HIP_TRY(ctx, ctx->collect_times());
  size_t k = 0;
  for (auto &a : ctx->acc) {
    if (a.launches == 0) continue;
    if (out && k < cap) {
      memset(&out[k], 0, sizeof out[k]);
      snprintf(out[k].name, sizeof out[k].name, "%s", a.name.c_str());
      out[k].launches = a.launches;
      out[k].total_ms = a.total_ms;
    }
    k++;
  }
  *n = k;
  return ZIPC_HIP_OK;
}

size_t zipc_hip_deflate_bound(size_t len) {
  // all-stored worst case: 5 header bytes per <= 65534 source bytes, +1 per block
  // because the reference's stored-block estimate can be 8 bits high
  // (src/zipc_deflate.ml:1045-1047), so a compressed block may beat it by < 1 byte
  size_t blocks = len / 65534 + 1;
  return len + 6 * blocks + 8;
}
size_t zipc_hip_zlib_bound(size_t len) { return zipc_hip_deflate_bound(len) + 6; }

// ---- batch forms ---------------------------------------------------------------

int zipc_hip_inflate_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena,
                           const zipc_hip_stream_desc *d_descs, zipc_hip_stream_result *d_results,
                           size_t n_streams, size_t max_dst_cap, int crc_op) {
  if (!ctx || !d_descs || !d_results) return ZIPC_HIP_ERR_INVALID_ARG;
  if (crc_op < 0 || crc_op > 3 || n_streams > 0x7FFFFFFFull) return ZIPC_HIP_ERR_INVALID_ARG;
  return launch_inflate(ctx, d_src_arena, d_dst_arena, d_descs, d_results, n_streams, max_dst_cap, crc_op, nullptr, true);
}

int zipc_hip_inflate_size_batch(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs,
                                zipc_hip_stream_result *d_results, size_t n_streams) {
  if (!ctx || !d_descs || !d_results || n_streams > 0x7FFFFFFFull) return ZIPC_HIP_ERR_INVALID_ARG;
  return launch_inflate_size(ctx, d_src_arena, d_descs, d_results, n_streams);
}

int zipc_hip_deflate_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena,
                           const zipc_hip_stream_desc *d_descs, zipc_hip_stream_result *d_results,
                           size_t n_streams, size_t max_src_len, size_t total_src_len, int level,
                           int crc_op) {
  if (!ctx || !d_descs || !d_results) return ZIPC_HIP_ERR_INVALID_ARG;
  if (crc_op < 0 || crc_op > 3 || level < 0 || level > 3 || n_streams > 0x7FFFFFFFull)
    return ZIPC_HIP_ERR_INVALID_ARG;
  if (max_src_len > MAX_STREAM_LEN) return ZIPC_HIP_ERR_INVALID_ARG;
  if (n_streams == 0) return ZIPC_HIP_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, ctx->ensure(ctx->deflate_scratch,
                           deflate_scratch_bytes(n_streams, max_src_len, total_src_len, level, zd::tuning())));
  if (crc_op == ZIPC_HIP_CRC_CRC32) {  // (launch_deflate runs the pass, group by group)
    if (n_streams * crc32_segs(max_src_len) > 0x7FFFFFFFull) return ZIPC_HIP_ERR_INVALID_ARG;
    HIP_TRY(ctx, ctx->ensure(ctx->crc_partials, n_streams * crc32_segs(max_src_len) * sizeof(uint32_t)));
  }
  HIP_TRY(ctx, launch_deflate(ctx, (const uint8_t *)d_src_arena, (uint8_t *)d_dst_arena,
                              (const StreamDesc *)d_descs, (StreamResult *)d_results, n_streams,
                              max_src_len, total_src_len, level, crc_op));
  return ZIPC_HIP_OK;
}

size_t zipc_hip_debug_chain_positions(size_t n_streams, size_t total_src_len) { return zd::debug_chain_positions(n_streams, total_src_len); }
int zipc_hip_debug_chain_links(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs, size_t n_streams,
                               size_t max_src_len, size_t total_src_len, int which, void *d_links, size_t links_cap, void *d_pos_base) {
  if (!ctx || !d_descs || !d_links || which < 0 || which > 1 || n_streams == 0 || n_streams > 0x7FFFFFFFull || max_src_len > MAX_STREAM_LEN)
    return ZIPC_HIP_ERR_INVALID_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, ctx->ensure(ctx->deflate_scratch, deflate_scratch_bytes(n_streams, max_src_len, total_src_len, ZIPC_HIP_LEVEL_DEFAULT, zd::tuning())));
  HIP_TRY(ctx, zd::debug_chain_links(ctx, (const uint8_t *)d_src_arena, (const StreamDesc *)d_descs, n_streams, max_src_len, total_src_len,
                                     which, (uint16_t *)d_links, links_cap, (uint64_t *)d_pos_base));
  return ZIPC_HIP_OK;
}

int zipc_hip_reserve(zipc_hip_ctx *ctx, size_t n_streams, size_t max_src_len, size_t total_src_len) {
  if (!ctx) return ZIPC_HIP_ERR_INVALID_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, ctx->ensure(ctx->deflate_scratch,
                           deflate_scratch_bytes(n_streams, max_src_len, total_src_len, ZIPC_HIP_LEVEL_BEST, zd::tuning())));
  size_t segs = (max_src_len + CRC_SEG_BYTES - 1) / CRC_SEG_BYTES + 1;
  HIP_TRY(ctx, ctx->ensure(ctx->crc_partials, n_streams * segs * sizeof(uint32_t)));
  return ZIPC_HIP_OK;
}

int zipc_hip_checksum_device(zipc_hip_ctx *ctx, const void *d_buf, size_t len, int want_crc32,
                             int want_adler32, uint32_t *d_out) {
  if (!ctx || !d_out || (!d_buf && len)) return ZIPC_HIP_ERR_INVALID_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // Both checksums: ONE pass over the bytes (crc32_adler_segments_kernel leaves the CRC partials and the
  // Adler chunk sums), then the two finishes -- on two queues for a large buffer
  const bool fused = want_crc32 && want_adler32 && len > 0;
  const bool side = fused && len >= (64u << 20);
  if (fused)  // (before any fork: growing a buffer synchronises)
    HIP_TRY(ctx, ctx->ensure(ctx->crc_partials, crc32_segs(len) * sizeof(uint32_t)));
  if (want_crc32 && !fused) {
    const int st = crc32_pass(ctx, (const uint8_t *)d_buf, RANGE_SINGLE, nullptr, nullptr, 1, 0, len, len, d_out);
    if (st != ZIPC_HIP_OK) return st;
  }
  struct Joiner {  // the side queue is joined on every way out of the Adler half
    zipc_hip_ctx *c; bool on;
    ~Joiner() { if (on) { c->cur = c->stream; (void)c->join(1); } }
  } joiner{ctx, false};
  if (want_adler32) {
    const uint64_t n_chunks = adler_n_chunks(len);  // (the chain's shape: adler_chain.h)
    // chunk sums, then the ambiguous-chunk list and the per-run arrays of the chain kernels
    const size_t sums_bytes = ((size_t)(n_chunks + 1) * sizeof(uint2) + 255) / 256 * 256;
    AdlerRuns R;
    R.n_runs = adler_n_runs(n_chunks);
    const size_t run_bytes = (size_t)R.n_runs * sizeof(uint32_t);
    HIP_TRY(ctx, ctx->ensure(ctx->adler_sums, sums_bytes + ADLER_AMB_CAP * 16 + 5 * run_bytes + 256));
    uint2 *sums = (uint2 *)ctx->adler_sums.p;
    uint8_t *q = (uint8_t *)ctx->adler_sums.p + sums_bytes;
    uint32_t *amb = (uint32_t *)q; q += ADLER_AMB_CAP * 16;
    R.sum = (uint32_t *)q; q += run_bytes;
    R.s1_before = (uint32_t *)q; q += run_bytes;
    R.s1_after = (uint32_t *)q; q += run_bytes;
    R.last_hi = (uint32_t *)q; q += run_bytes;
    R.res_before = (uint32_t *)q; q += run_bytes;
    R.amb_count = (uint32_t *)q;
    if (fused) {
      const size_t segs = crc32_segs(len);
      if (segs > 0x7FFFFFFFull) return ZIPC_HIP_ERR_INVALID_ARG;
      uint32_t *partials = (uint32_t *)ctx->crc_partials.p;
      HIP_TRY(ctx, hipMemsetAsync(sums, 0, (size_t)n_chunks * sizeof(uint2), ctx->stream));
      ZD_LAUNCH(ctx, "crc32_adler_segments", crc32_adler_segments_kernel, dim3((unsigned)segs), dim3(256), 0,
                (const uint8_t *)d_buf, (uint64_t)len, (uint32_t)segs, (const uint32_t *)ctx->crc_nib.p, partials,
                sums, n_chunks);
      HIP_TRY(ctx, hipGetLastError());
      if (side) {  // the CRC's finish beside the Adler chain
        HIP_TRY(ctx, ctx->fork(1));
        ctx->cur = ctx->side[0];
        joiner.on = true;
      }
      HIP_TRY(ctx, crc32_finish_launch(ctx, RANGE_SINGLE, nullptr, nullptr, 1, len, len, partials, d_out));
      ctx->cur = ctx->stream;
    } else if (n_chunks) {
      if ((n_chunks + 3) / 4 > 0x7FFFFFFFull) return ZIPC_HIP_ERR_INVALID_ARG;
      ZD_LAUNCH(ctx, "adler_chunks", adler_chunks_kernel, dim3((unsigned)((n_chunks + 3) / 4)), dim3(256), 0,
                (const uint8_t *)d_buf, (uint64_t)len, n_chunks, sums);
    }
    const uint64_t per = adler_per(n_chunks, R.n_runs);
    HIP_TRY(ctx, hipMemsetAsync(R.amb_count, 0, sizeof(uint32_t), ctx->stream));
    ZD_LAUNCH(ctx, "adler_runs_s1", adler_runs_s1_kernel, dim3(R.n_runs / 256), dim3(256), 0, (const uint2 *)sums,
              n_chunks, per, R);
    ZD_LAUNCH(ctx, "adler_scan_runs", adler_scan_runs_kernel, dim3(1), dim3(1024), 0, (const uint32_t *)R.sum,
              R.s1_before, R.n_runs, 1u);
    ZD_LAUNCH(ctx, "adler_runs_a", adler_runs_a_kernel, dim3(R.n_runs / 256), dim3(256), 0, (const uint2 *)sums,
              (uint64_t)len, n_chunks, per, R, amb, ADLER_AMB_CAP);
    ZD_LAUNCH(ctx, "adler_scan_runs", adler_scan_runs_kernel, dim3(1), dim3(1024), 0, (const uint32_t *)R.sum,
              R.res_before, R.n_runs, 0u);
    if (ctx->adler_rfc1950) {  // RFC 1950's arithmetic: the chunk sums combine without the reference's sign cases
      ZD_LAUNCH(ctx, "adler_rfc_finish", adler_rfc_finish_kernel, dim3(1), dim3(1024), 0, (const uint2 *)sums,
                (uint64_t)len, n_chunks, d_out + 1);
      HIP_TRY(ctx, hipGetLastError());
      return ZIPC_HIP_OK;
    }
    ZD_LAUNCH(ctx, "adler_replay", adler_replay_kernel, dim3(1), dim3(1024), 0, (const uint2 *)sums, (uint64_t)len,
              n_chunks, per, R, amb, ADLER_AMB_CAP, d_out + 1);
    HIP_TRY(ctx, hipGetLastError());
  }
  return ZIPC_HIP_OK;
}

// ---- host forms ------------------------------------------------------------------

static int stage_in(zipc_hip_ctx *ctx, const void *src, size_t len) {
  HIP_TRY(ctx, ctx->ensure(ctx->io_src, len + 64));
  if (len) HIP_TRY(ctx, hipMemcpyAsync(ctx->io_src.p, src, len, hipMemcpyHostToDevice, ctx->stream));
  return ZIPC_HIP_OK;
}

static int checksum_host(zipc_hip_ctx *ctx, const void *src, size_t len, int want_crc, uint32_t *out) {
  if (!ctx || !out || (!src && len)) return ZIPC_HIP_ERR_INVALID_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int st = stage_in(ctx, src, len);
  if (st) return st;
  HIP_TRY(ctx, ctx->ensure(ctx->io_small, 64));
  uint32_t *d_out = (uint32_t *)ctx->io_small.p;
  st = zipc_hip_checksum_device(ctx, ctx->io_src.p, len, want_crc, !want_crc, d_out);
  if (st) return st;
  uint32_t h[2] = {0, 0};
  HIP_TRY(ctx, hipMemcpyAsync(h, d_out, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *out = want_crc ? h[0] : h[1];
  return ZIPC_HIP_OK;
}

int zipc_hip_crc32(zipc_hip_ctx *ctx, const void *src, size_t len, uint32_t *crc) {
  return checksum_host(ctx, src, len, 1, crc);
}
int zipc_hip_adler32(zipc_hip_ctx *ctx, const void *src, size_t len, uint32_t *adler) {
  return checksum_host(ctx, src, len, 0, adler);
}

// one stream through the batch kernels; is_inflate selects the direction
static int one_stream(zipc_hip_ctx *ctx, bool is_inflate, const void *src, size_t len, int has_limit,
                      size_t limit, int level, int crc_op, void *dst, size_t dst_cap, size_t *out_len,
                      uint32_t *checksum) {
  if (!ctx || (!src && len) || (!dst && dst_cap) || !out_len) return ZIPC_HIP_ERR_INVALID_ARG;
  *out_len = 0;
  if (checksum) *checksum = 0;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int st = stage_in(ctx, src, len);
  if (st) return st;
  HIP_TRY(ctx, ctx->ensure(ctx->io_dst, dst_cap + 64));
  HIP_TRY(ctx, ctx->ensure(ctx->io_desc, sizeof(StreamDesc)));
  HIP_TRY(ctx, ctx->ensure(ctx->io_res, sizeof(StreamResult)));
  StreamDesc d;
  memset(&d, 0, sizeof d);
  d.src_off = 0; d.src_len = len; d.dst_off = 0; d.dst_cap = dst_cap;
  d.limit = limit; d.flags = has_limit ? STREAM_HAS_LIMIT : 0;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->io_desc.p, &d, sizeof d, hipMemcpyHostToDevice, ctx->stream));
  if (is_inflate)
    st = zipc_hip_inflate_batch(ctx, ctx->io_src.p, ctx->io_dst.p, (zipc_hip_stream_desc *)ctx->io_desc.p,
                                (zipc_hip_stream_result *)ctx->io_res.p, 1, dst_cap, crc_op);
  else
    st = zipc_hip_deflate_batch(ctx, ctx->io_src.p, ctx->io_dst.p, (zipc_hip_stream_desc *)ctx->io_desc.p,
                                (zipc_hip_stream_result *)ctx->io_res.p, 1, len, len, level, crc_op);
  if (st) return st;
  StreamResult r;
  HIP_TRY(ctx, hipMemcpyAsync(&r, ctx->io_res.p, sizeof r, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (r.status != ST_OK) return (int)r.status;
  if (r.out_len > dst_cap) return ZIPC_HIP_ERR_DST_TOO_SMALL;
  if (r.out_len) {
    HIP_TRY(ctx, hipMemcpyAsync(dst, ctx->io_dst.p, r.out_len, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  *out_len = r.out_len;
  if (checksum) *checksum = r.checksum;
  return ZIPC_HIP_OK;
}

int zipc_hip_inflate(zipc_hip_ctx *ctx, const void *src, size_t len, int has_limit, size_t limit,
                     int crc_op, void *dst, size_t dst_cap, size_t *out_len, uint32_t *checksum) {
  return one_stream(ctx, true, src, len, has_limit, limit, 0, crc_op, dst, dst_cap, out_len, checksum);
}

// what one host stream inflates to: a batch of one around a copy in and the result's 16 bytes back
int zipc_hip_inflate_size(zipc_hip_ctx *ctx, const void *src, size_t len, int has_limit, size_t limit, size_t *out_len) {
  if (!ctx || (!src && len) || !out_len) return ZIPC_HIP_ERR_INVALID_ARG;
  *out_len = 0;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int st = stage_in(ctx, src, len);
  if (st) return st;
  HIP_TRY(ctx, ctx->ensure(ctx->io_desc, sizeof(StreamDesc)));
  HIP_TRY(ctx, ctx->ensure(ctx->io_res, sizeof(StreamResult)));
  StreamDesc d;
  memset(&d, 0, sizeof d);
  d.src_len = len;
  d.limit = limit; d.flags = has_limit ? STREAM_HAS_LIMIT : 0;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->io_desc.p, &d, sizeof d, hipMemcpyHostToDevice, ctx->stream));
  st = zipc_hip_inflate_size_batch(ctx, ctx->io_src.p, (const zipc_hip_stream_desc *)ctx->io_desc.p, (zipc_hip_stream_result *)ctx->io_res.p, 1);
  if (st) return st;
  StreamResult r;
  HIP_TRY(ctx, hipMemcpyAsync(&r, ctx->io_res.p, sizeof r, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (r.status != ST_OK) return (int)r.status;
  *out_len = r.out_len;
  return ZIPC_HIP_OK;
}

int zipc_hip_deflate(zipc_hip_ctx *ctx, const void *src, size_t len, int level, int crc_op, void *dst,
                     size_t dst_cap, size_t *out_len, uint32_t *checksum) {
  if (level < 0 || level > 3) return ZIPC_HIP_ERR_INVALID_ARG;
  return one_stream(ctx, false, src, len, 0, 0, level, crc_op, dst, dst_cap, out_len, checksum);
}

// ---- recode on the device (recode_rules.h has the rules; recode.hip the three kernels) ------------------------------

// The context's scratch of a recode of n streams: the descriptors the codec runs with, its results, the verdicts.
static int recode_reserve(zipc_hip_ctx *ctx, size_t n) {
  HIP_TRY(ctx, ctx->ensure(ctx->recode_descs, n * sizeof(StreamDesc)));
  HIP_TRY(ctx, ctx->ensure(ctx->recode_res, n * sizeof(StreamResult)));
  HIP_TRY(ctx, ctx->ensure(ctx->recode_verdicts, n * sizeof(RecodeVerdict)));
  return ZIPC_HIP_OK;
}
// open -> inflate with its CRC-32 pass -> link -> deflate out of the middle arena -> close, all on the context's stream.
// d_plain: null, or n StreamResults for the many-stream pipeline; h_inflate_descs: null, or the host's own copy of what
// recode_open makes of the descriptors (launch_inflate's h_descs); first_of_call: launch_inflate's.
static int recode_sequence(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_mid_arena, void *d_dst_arena, const RecodeDesc *d_descs,
                           RecodeResult *d_results, StreamResult *d_plain, size_t n, size_t max_mid_cap, size_t total_mid_cap, int level,
                           const StreamDesc *h_inflate_descs, bool first_of_call) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int st = recode_reserve(ctx, n);
  if (st) return st;
  StreamDesc *inner = (StreamDesc *)ctx->recode_descs.p;
  StreamResult *inner_res = (StreamResult *)ctx->recode_res.p;
  RecodeVerdict *verdicts = (RecodeVerdict *)ctx->recode_verdicts.p;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  ZD_LAUNCH(ctx, "recode_open", recode_open_kernel, grid, block, 0, d_descs, (uint32_t)n, (uint64_t)max_mid_cap, inner, verdicts);
  HIP_TRY(ctx, hipGetLastError());
  st = launch_inflate(ctx, d_src_arena, d_mid_arena, (const zipc_hip_stream_desc *)inner, (zipc_hip_stream_result *)inner_res, n, max_mid_cap,
                      ZIPC_HIP_CRC_CRC32, h_inflate_descs, first_of_call);
  if (st) return st;
  ZD_LAUNCH(ctx, "recode_link", recode_link_kernel, grid, block, 0, d_descs, (uint32_t)n, (const StreamResult *)inner_res, inner, verdicts);
  HIP_TRY(ctx, hipGetLastError());
  st = zipc_hip_deflate_batch(ctx, d_mid_arena, d_dst_arena, (const zipc_hip_stream_desc *)inner, (zipc_hip_stream_result *)inner_res, n,
                              max_mid_cap, total_mid_cap, level, ZIPC_HIP_CRC_NOP);
  if (st) return st;
  ZD_LAUNCH(ctx, "recode_close", recode_close_kernel, grid, block, 0, (uint32_t)n, (const RecodeVerdict *)verdicts,
            (const StreamResult *)inner_res, d_results, d_plain);
  HIP_TRY(ctx, hipGetLastError());
  return ZIPC_HIP_OK;
}

int zipc_hip_recode_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_mid_arena, void *d_dst_arena,
                          const zipc_hip_recode_desc *d_descs, zipc_hip_recode_result *d_results, size_t n_streams,
                          size_t max_mid_cap, size_t total_mid_cap, int level) {
  if (!ctx || !d_descs || !d_results || n_streams > 0x7FFFFFFFull || level < 0 || level > 3) return ZIPC_HIP_ERR_INVALID_ARG;
  if (max_mid_cap > MAX_STREAM_LEN) return ZIPC_HIP_ERR_INVALID_ARG;  // (deflate takes no longer source; inflate_huge_stream's output is none)
  if (n_streams == 0) return ZIPC_HIP_OK;
  return recode_sequence(ctx, d_src_arena, d_mid_arena, d_dst_arena, (const RecodeDesc *)d_descs, (RecodeResult *)d_results, nullptr,
                         n_streams, max_mid_cap, total_mid_cap, level, nullptr, true);
}

// ---- the many-stream forms' way back: a sub-batch's outputs end to end, written by a kernel ----------------
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
// is as few workgroups as fill the bus.  The host makes the same sums from the results (many_streams below).

// (the host makes the same sums: zd_host::packed_size, host_pipeline.h)
__device__ static inline uint64_t packed_size(uint32_t status, uint64_t out_len, uint64_t dst_cap) {
  return status == ST_OK && out_len <= dst_cap ? (out_len + 15) / 16 * 16 : 0;
}

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

// what the kernels' step of a many-stream call is.  MANY_RECODE: the recode sequence above (crc_op: CRC-32); its middle
// arena is one more buffer of the context, as large as the largest sub-batch needs, and beside the plain results the
// pipeline works with, the call's zipc_hip_recode_results come back into pinned memory of their own (ctx->pin_rres).
enum ManyOp { MANY_DEFLATE = 0, MANY_INFLATE = 1, MANY_RECODE = 2 };
struct RecodeMany {
  const size_t *mid_cap;
  const uint32_t *expect_crc32;  // may be null
};
constexpr uint32_t MANY_RESULT_UNSET = 0xFFFFFFFFu;  // a status no call gives: an entry nothing has written yet

// n host-resident streams through the batch kernels: arenas are the context's
// staging buffers, streams packed at 256-byte aligned offsets
static int many_streams(zipc_hip_ctx *ctx, ManyOp op, size_t n, const void *const *src, const size_t *src_len,
                        const size_t *limit, int level, int crc_op, void *const *dst, const size_t *dst_cap,
                        zipc_hip_stream_result *results, bool want_bytes = true, const RecodeMany *rc = nullptr) {
  const bool is_inflate = op == MANY_INFLATE, recode = op == MANY_RECODE;
  if (!ctx || (n && (!src || !src_len || (!dst && want_bytes) || !dst_cap || !results))) return ZIPC_HIP_ERR_INVALID_ARG;
  if (recode && (!rc || (n && !rc->mid_cap))) return ZIPC_HIP_ERR_INVALID_ARG;
  if (crc_op < 0 || crc_op > 3 || level < 0 || level > 3 || n > 0x7FFFFFFFull) return ZIPC_HIP_ERR_INVALID_ARG;
  if (n == 0) return ZIPC_HIP_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const bool timing = zd::tuning().host_timing;
  const auto t_begin = std::chrono::steady_clock::now();
  auto since = [&](std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
  };
  std::vector<StreamDesc> descs(n);
  uint64_t so = 0, dof = 0;
  size_t max_src = 0, max_cap = 0, max_mid = 0;
  for (size_t i = 0; i < n; i++) {
    if ((!src[i] && src_len[i]) || (want_bytes && !dst[i] && dst_cap[i])) return ZIPC_HIP_ERR_INVALID_ARG;
    StreamDesc &d = descs[i];
    memset(&d, 0, sizeof d);
    d.src_off = so; d.src_len = src_len[i]; d.dst_off = dof; d.dst_cap = dst_cap[i];
    if (limit) { d.limit = limit[i]; d.flags = STREAM_HAS_LIMIT; }
    so += (src_len[i] + 255) / 256 * 256 + 256;
    dof += (dst_cap[i] + 255) / 256 * 256 + 256;
    max_src = src_len[i] > max_src ? src_len[i] : max_src;
    max_cap = dst_cap[i] > max_cap ? dst_cap[i] : max_cap;
    if (recode) max_mid = rc->mid_cap[i] > max_mid ? rc->mid_cap[i] : max_mid;
  }
  if (op == MANY_DEFLATE && max_src > MAX_STREAM_LEN) return ZIPC_HIP_ERR_INVALID_ARG;  // (inflate reports it per stream)
  if (recode && max_mid > MAX_STREAM_LEN) return ZIPC_HIP_ERR_INVALID_ARG;              // (zipc_hip_recode_batch's rule)
  // The batch is cut into K sub-batches, and sub-batch g goes through
  //   gather (host threads, into pinned memory) -> copy in (the engine, queue copy_in, in runs of 16 MiB as they are
  //   gathered) -> kernels (the context's queue) -> the way back (the kernel above, queue copy_out) -> scatter (host threads)
  // on its own, so the bus and the kernels of one sub-batch run under the host memcpys of the others; PCIe is full
  // duplex and the kernels do not touch it.  This thread gathers and feeds the device; a second one (`taker` below)
  // waits for what comes back and scatters it with threads of its own, so the first sub-batch's results are in the
  // caller's buffers while the last one's sources are still being gathered.  Thousands of small pageable copies -- the
  // first version of this function -- cost far more than the kernels.
  // K (ZIPC_HIP_HOST_CHUNKS): 4, or 6 from a GiB of staging on; fewer when sub-batches would get too small to fill the
  // chip (under 1024 streams AND under 64 MiB of sources).  The first and the last sub-batch are half as large as the others: the first is what the bus and the kernels
  // wait for before they have anything to do, the last what the caller waits for when everything else is through.
  // (profiles/r05_host_forms_sweep.txt: 4096 x 64 KiB: 3 / 4 / 5 / 6 sub-batches deflate 9.9 / 9.8 / 9.4 / 10.0 ms,
  // inflate 8.3 / 8.9 / 8.9 / 9.5; 16 384 x 64 KiB: 34.0 / 31.2 / 29.8 / 30.2 and 29.4 / 27.6 / 26.6 / 25.7.)
  size_t K = host_chunks(so + dof);
  {  // a sub-batch holds host_chunk_min streams, or as many source bytes as that many streams of 64 KiB (long members)
    const uint64_t least = (uint64_t)zd::tuning().host_chunk_min;
    while (K > 1 && n / K < least && so / K < least * 65536) K--;
  }
  std::vector<size_t> cut(K + 1, n);
  cut[0] = 0;
  const bool taper = K >= 3;
  const size_t shares = taper ? 2 * K - 2 : K;
  for (size_t g = 1, i = 0; g < K; g++) {
    const size_t before = taper ? 2 * g - 1 : g;  // shares of sub-batches [0, g)
    while (i < n && descs[i].src_off < so / shares * before) i++;
    cut[g] = i;
  }
  size_t n_max = 0, total_max = 0;
  for (size_t g = 0; g < K; g++) {
    size_t t = 0;
    for (size_t i = cut[g]; i < cut[g + 1]; i++) t += src_len[i];
    n_max = cut[g + 1] - cut[g] > n_max ? cut[g + 1] - cut[g] : n_max;
    total_max = t > total_max ? t : total_max;
  }
  const bool packed = zd::tuning().host_pack && want_bytes;  // (false: whole destination slots by the copy engine)
  // recode: every sub-batch's streams get their room in the middle arena from its beginning on; what inflate is handed
  // is known here (recode_open is the kernel's rule), so the block path has nothing to read back
  std::vector<RecodeDesc> rdescs;
  std::vector<StreamDesc> h_inflate;
  uint64_t mid_arena = 0;
  size_t mid_total_max = 0;
  if (recode) {
    rdescs.resize(n);
    h_inflate.resize(n);
    for (size_t g = 0; g < K; g++) {
      uint64_t mo = 0;
      size_t t = 0;
      for (size_t i = cut[g]; i < cut[g + 1]; i++) {
        RecodeDesc &r = rdescs[i];
        memset(&r, 0, sizeof r);
        r.src_off = descs[i].src_off; r.src_len = descs[i].src_len; r.dst_off = descs[i].dst_off; r.dst_cap = descs[i].dst_cap;
        r.mid_off = mo; r.mid_cap = rc->mid_cap[i];
        r.limit = descs[i].limit; r.flags = descs[i].flags;
        if (rc->expect_crc32) { r.expect_crc32 = rc->expect_crc32[i]; r.flags |= STREAM_EXPECT_CRC32; }
        (void)recode_open(r, max_mid, &h_inflate[i]);
        mo += (rc->mid_cap[i] + 255) / 256 * 256 + 256;
        t += rc->mid_cap[i];
      }
      mid_arena = mo > mid_arena ? mo : mid_arena;
      mid_total_max = t > mid_total_max ? t : mid_total_max;
    }
  }
  // everything is allocated before the first sub-batch is under way (growing a buffer
  // synchronises the stream)
  HIP_TRY(ctx, ctx->ensure(ctx->io_src, so + 64));
  HIP_TRY(ctx, ctx->ensure(ctx->io_dst, dof + 64));
  HIP_TRY(ctx, ctx->ensure(ctx->io_desc, n * sizeof(StreamDesc)));
  HIP_TRY(ctx, ctx->ensure(ctx->io_res, n * sizeof(StreamResult)));
  if (packed) HIP_TRY(ctx, ctx->ensure(ctx->io_pack_off, (n + K + 1) * sizeof(uint64_t)));
  HIP_TRY(ctx, ctx->ensure_pinned(ctx->pin_src, so + 64));
  if (want_bytes) HIP_TRY(ctx, ctx->ensure_pinned(ctx->pin_dst, dof + 64));
  HIP_TRY(ctx, ctx->ensure_pinned(ctx->pin_res, n * sizeof(StreamResult)));
  if (recode) {
    HIP_TRY(ctx, ctx->ensure(ctx->io_mid, mid_arena + 64));
    HIP_TRY(ctx, ctx->ensure(ctx->io_rdesc, n * sizeof(RecodeDesc)));
    HIP_TRY(ctx, ctx->ensure(ctx->io_rres, n * sizeof(RecodeResult)));
    HIP_TRY(ctx, ctx->ensure_pinned(ctx->pin_rres, n * sizeof(RecodeResult)));
    memset(ctx->pin_rres.p, 0xFF, n * sizeof(RecodeResult));  // (MANY_RESULT_UNSET: what has not come back says so)
    int st = recode_reserve(ctx, n_max);
    if (st) return st;
    st = zipc_hip_reserve(ctx, n_max, max_mid, mid_total_max);
    if (st) return st;
  }
  if (op == MANY_DEFLATE) {
    const int st = zipc_hip_reserve(ctx, n_max, max_src, total_max);
    if (st) return st;
  } else {
    HIP_TRY(ctx, ctx->ensure(ctx->inflate_scratch, n_max * INFLATE_SCRATCH_PER_STREAM));
  }
  if (crc_op == ZIPC_HIP_CRC_CRC32) {
    const size_t longest = recode ? max_mid : is_inflate ? max_cap : max_src;
    size_t segs = (longest + CRC_SEG_BYTES - 1) / CRC_SEG_BYTES;
    HIP_TRY(ctx, ctx->ensure(ctx->crc_partials, n_max * (segs ? segs : 1) * sizeof(uint32_t)));
  }
  if (!ctx->copy_in) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->copy_in, hipStreamNonBlocking));
  if (!ctx->copy_out) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->copy_out, hipStreamNonBlocking));
  EventSet ev_in, ev_k, ev_out;
  HIP_TRY(ctx, ev_in.make(K, timing));
  HIP_TRY(ctx, ev_k.make(K, timing));
  HIP_TRY(ctx, ev_out.make(K, timing));
  EventSet ev_t;  // timing: the call's begin on the device, a sub-batch's first copy in, its kernels' begin
  if (timing) HIP_TRY(ctx, ev_t.make(1 + 2 * K, true));
  // earlier work of this context (the previous call's kernels read io_src / io_desc; a call that
  // failed half way may have left copies on the two copy streams) first
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->copy_in));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->copy_out));
  const double ms_setup = since(t_begin);
  static_assert(sizeof(StreamResult) == sizeof(zipc_hip_stream_result), "result layout");
  auto dst_end = [&](size_t i) { return i < n ? descs[i].dst_off : dof; };

  // ---- the device's part of the pipeline (host_pipeline.h Device): copies, kernels and events on three queues.  From
  // begin() on, work is in flight that reads `descs` and the pinned buffers and records into the event sets above:
  // many_pipeline returns only when its second thread is through, and after a failure all three queues are waited for
  // below before anything is freed or the next call reuses the buffers.
  struct Dev {
    zipc_hip_ctx *ctx;
    bool is_inflate, timing, packed, want_bytes, first_batch = true;
    size_t n, max_src, max_cap;
    int level, crc_op;
    const size_t *src_len;
    const std::vector<StreamDesc> &descs;
    EventSet &ev_in, &ev_k, &ev_out, &ev_t;
    decltype(dst_end) &dst_end_of;
    std::string error;
    // MANY_RECODE: the call's recode descriptors, what inflate is handed of them, the streams' room and the largest
    const RecodeDesc *rdescs = nullptr;
    const StreamDesc *h_inflate = nullptr;
    const size_t *mid_cap = nullptr;
    size_t max_mid = 0;
#define PIPE_TRY(expr)                                                                   \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess) {                                                              \
      error = std::string(#expr) + ": " + hipGetErrorString(_e);                         \
      return ZIPC_HIP_ERR_HIP;                                                           \
    }                                                                                    \
  } while (0)
    int begin() {
      if (timing) PIPE_TRY(hipEventRecord(ev_t.ev[0], ctx->copy_in));
      PIPE_TRY(hipMemcpyAsync(ctx->io_desc.p, descs.data(), n * sizeof(StreamDesc), hipMemcpyHostToDevice, ctx->copy_in));
      if (rdescs) PIPE_TRY(hipMemcpyAsync(ctx->io_rdesc.p, rdescs, n * sizeof(RecodeDesc), hipMemcpyHostToDevice, ctx->copy_in));
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
      size_t total_g = 0;
      for (size_t i = lo; i < hi; i++) total_g += src_len[i];
      int st;
      if (rdescs) {  // (the plain results the way back works with are recode_close_kernel's second output)
        size_t total_mid = 0;
        for (size_t i = lo; i < hi; i++) total_mid += mid_cap[i];
        st = recode_sequence(ctx, ctx->io_src.p, ctx->io_mid.p, ctx->io_dst.p, (const RecodeDesc *)ctx->io_rdesc.p + lo,
                             (RecodeResult *)ctx->io_rres.p + lo, (StreamResult *)dr, hi - lo, max_mid, total_mid, level, h_inflate + lo,
                             first_batch);
        if (st == ZIPC_HIP_OK)
          PIPE_TRY(hipMemcpyAsync((RecodeResult *)ctx->pin_rres.p + lo, (const RecodeResult *)ctx->io_rres.p + lo,
                                  (hi - lo) * sizeof(RecodeResult), hipMemcpyDeviceToHost, ctx->stream));
      } else if (is_inflate)  // (with the descriptors it has on the host: no read-back, nothing waited for unless a stream goes by blocks)
        st = launch_inflate(ctx, ctx->io_src.p, ctx->io_dst.p, dd, dr, hi - lo, max_cap, crc_op, descs.data() + lo, first_batch);
      else
        st = zipc_hip_deflate_batch(ctx, ctx->io_src.p, ctx->io_dst.p, dd, dr, hi - lo, max_src, total_g, level, crc_op);
      first_batch = false;
      if (st) { error = ctx->last_error; return st; }
      PIPE_TRY(hipMemcpyAsync((StreamResult *)ctx->pin_res.p + lo, dr, (hi - lo) * sizeof(StreamResult),
                              hipMemcpyDeviceToHost, ctx->stream));
      const uint64_t c = dst_end_of(lo), e = dst_end_of(hi);
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
#undef PIPE_TRY
  } dev{ctx, is_inflate, timing, packed, want_bytes, true, n, max_src, max_cap, level, crc_op, src_len, descs, ev_in, ev_k, ev_out, ev_t, dst_end, {}};

  zd_host::ManyJob<StreamDesc> job;
  job.n = n; job.src = src; job.src_len = src_len; job.dst = dst; job.dst_cap = dst_cap; job.results = results;
  job.descs = descs.data(); job.src_arena_end = so; job.dst_arena_end = dof;
  job.cut = cut; job.n_max = n_max; job.packed = packed; job.want_bytes = want_bytes;
  if (recode) { dev.rdescs = rdescs.data(); dev.h_inflate = h_inflate.data(); dev.mid_cap = rc->mid_cap; dev.max_mid = max_mid; }
  job.ahead = (is_inflate && max_cap >= BLOCKS_BATCH_MIN_DST) || (recode && max_mid >= BLOCKS_BATCH_MIN_DST);
  job.h2d_bytes = (uint64_t)16 << 20;  // (sources sent in runs of about 16 MiB as they are gathered)
  job.pin_src = (uint8_t *)ctx->pin_src.p; job.pin_dst = want_bytes ? (const uint8_t *)ctx->pin_dst.p : nullptr;
  job.pin_res = (const zipc_hip_stream_result *)ctx->pin_res.p;
  job.threads = host_threads();
  zd_host::ManyTimes times;
  std::string why;
  const int pst = zd_host::many_pipeline(job, dev, host_pools(), why, timing ? &times : nullptr);
  if (pst) {  // a batch call refused its arguments or a HIP call failed: the call fails as a whole
    (void)hipStreamSynchronize(ctx->copy_in);  // (sub-batches scattered before that stay where they are, with their results;
    (void)hipStreamSynchronize(ctx->stream);   //  every other entry of results[] carries the call's status and no bytes)
    (void)hipStreamSynchronize(ctx->copy_out);
    ctx->last_error = why;
    return pst;
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->copy_in));
  if (timing) {  // where each sub-batch was when: host clock from the call's begin, device clock from the first copy's begin
    fprintf(stderr, "zipc_hip %s_many n=%zu src_arena=%llu dst_arena=%llu ms: setup %.2f feed %.2f (of it gather %.2f) "
                    "scatter %.2f whole %.2f (threads %zu sub-batches %zu)\n",
            recode ? "recode" : is_inflate ? "inflate" : "deflate", n, (unsigned long long)so, (unsigned long long)dof, ms_setup, times.ms_feed,
            times.ms_gather, times.ms_scatter, since(t_begin), host_threads(), K);
    for (size_t g = 0; g < K; g++) {
      if (cut[g] == cut[g + 1]) continue;
      float h0 = 0, h1 = 0, k0 = 0, k1 = 0, o1 = 0;
      (void)hipEventElapsedTime(&h0, ev_t.ev[0], ev_t.ev[1 + 2 * g]);
      (void)hipEventElapsedTime(&h1, ev_t.ev[0], ev_in.ev[g]);
      (void)hipEventElapsedTime(&k0, ev_t.ev[0], ev_t.ev[2 + 2 * g]);
      (void)hipEventElapsedTime(&k1, ev_t.ev[0], ev_k.ev[g]);
      (void)hipEventElapsedTime(&o1, ev_t.ev[0], ev_out.ev[g]);
      fprintf(stderr, "  sub-batch %zu (%zu streams): host gathered at %.2f, scatter %.2f - %.2f | device copy in %.2f - %.2f, "
                      "kernels %.2f - %.2f, back by %.2f\n",
              g, cut[g + 1] - cut[g], times.gathered[g], times.scatter_begin[g], times.scatter_end[g], h0, h1, k0, k1, o1);
    }
  }
  return ZIPC_HIP_OK;
}

// (host vectors sized by n: whatever they throw -- bad_alloc when memory runs out, length_error, system_error from a mutex
// or a thread -- stays on this side of the C boundary: the call fails as out of memory, says so in zipc_hip_last_error, and
// every entry of results[] is defined.  Only the setup before the pipeline can throw: many_pipeline itself does not.)
static int many_threw(zipc_hip_ctx *ctx, size_t n, zipc_hip_stream_result *results) {
  try { if (ctx) ctx->last_error = "zipc_hip: out of memory (or no thread) on the host while setting up a many-stream call"; } catch (...) {}
  if (results) for (size_t i = 0; i < n; i++) results[i] = zipc_hip_stream_result{ZIPC_HIP_ERR_NOMEM, 0, 0};
  return ZIPC_HIP_ERR_NOMEM;
}
int zipc_hip_deflate_many(zipc_hip_ctx *ctx, size_t n, const void *const *src, const size_t *src_len, int level,
                          int crc_op, void *const *dst, const size_t *dst_cap, zipc_hip_stream_result *results) {
  try { return many_streams(ctx, MANY_DEFLATE, n, src, src_len, nullptr, level, crc_op, dst, dst_cap, results); }
  catch (...) { return many_threw(ctx, n, results); }
}
int zipc_hip_inflate_many(zipc_hip_ctx *ctx, size_t n, const void *const *src, const size_t *src_len,
                          const size_t *limit, int crc_op, void *const *dst, const size_t *dst_cap,
                          zipc_hip_stream_result *results) {
  try { return many_streams(ctx, MANY_INFLATE, n, src, src_len, limit, 0, crc_op, dst, dst_cap, results); }
  catch (...) { return many_threw(ctx, n, results); }
}
int zipc_hip_inflate_many_check(zipc_hip_ctx *ctx, size_t n, const void *const *src, const size_t *src_len,
                                const size_t *limit, int crc_op, const size_t *dst_cap, zipc_hip_stream_result *results) {
  try { return many_streams(ctx, MANY_INFLATE, n, src, src_len, limit, 0, crc_op, nullptr, dst_cap, results, false); }
  catch (...) { return many_threw(ctx, n, results); }
}


// zipc_hip_recode_many: many_streams with the recode sequence as its kernels' step.  The pipeline works with plain
// results (status, checksum, out_len); the zipc_hip_recode_results come back beside them into ctx->pin_rres, on the
// context's queue in front of the event the pipeline waits for before it takes a sub-batch.
//  * The call succeeded: every sub-batch was taken, and results[] is what came back.
//  * The call failed: the pipeline has overwritten the plain results of the sub-batches it did not take with the call's
//    status and no bytes, and does not say which those were.  A stream keeps what came back for it only where that says
//    the same as its plain result: an OK stream's plain result is OK only if its sub-batch was taken (its bytes are in
//    the caller's buffer), and a stream that stopped has no bytes either way, so its own verdict is as true as the
//    call's.  Every other entry carries the plain status at stage 0.
static int recode_many(zipc_hip_ctx *ctx, size_t n, const void *const *src, const size_t *src_len, const size_t *limit,
                       const uint32_t *expect_crc32, const size_t *mid_cap, int level, void *const *dst, const size_t *dst_cap,
                       zipc_hip_recode_result *results) {
  auto fail = [&](int st) {
    if (results) for (size_t i = 0; i < n; i++) results[i] = zipc_hip_recode_result{(uint32_t)st, 0, 0, 0, 0, 0};
    return st;
  };
  if (!ctx || (n && (!src || !src_len || !mid_cap || !dst || !dst_cap || !results)) || level < 0 || level > 3) return fail(ZIPC_HIP_ERR_INVALID_ARG);
  for (size_t i = 0; i < n; i++)
    if ((!src[i] && src_len[i]) || (!dst[i] && dst_cap[i])) return fail(ZIPC_HIP_ERR_INVALID_ARG);
  if (n == 0) return ZIPC_HIP_OK;
  std::vector<zipc_hip_stream_result> plain(n, zipc_hip_stream_result{MANY_RESULT_UNSET, 0, 0});
  const RecodeMany rc{mid_cap, expect_crc32};
  const int st = many_streams(ctx, MANY_RECODE, n, src, src_len, limit, level, ZIPC_HIP_CRC_CRC32, dst, dst_cap, plain.data(), true, &rc);
  const zipc_hip_recode_result *back = ctx->pin_rres.cap >= n * sizeof(RecodeResult) ? (const zipc_hip_recode_result *)ctx->pin_rres.p : nullptr;
  if (st == ZIPC_HIP_OK && back) {
    memcpy(results, back, n * sizeof *results);
    return st;
  }
  for (size_t i = 0; i < n; i++) {
    const zipc_hip_stream_result &p = plain[i];
    if (p.status == MANY_RESULT_UNSET) results[i] = zipc_hip_recode_result{(uint32_t)(st ? st : ZIPC_HIP_ERR_HIP), 0, 0, 0, 0, 0};  // (the pipeline never ran)
    else if (back && back[i].status == p.status && back[i].out_len == p.out_len) results[i] = back[i];
    else results[i] = zipc_hip_recode_result{p.status, 0, 0, 0, 0, 0};
  }
  return st;
}
int zipc_hip_recode_many(zipc_hip_ctx *ctx, size_t n, const void *const *src, const size_t *src_len, const size_t *limit,
                         const uint32_t *expect_crc32, const size_t *mid_cap, int level, void *const *dst, const size_t *dst_cap,
                         zipc_hip_recode_result *results) {
  try { return recode_many(ctx, n, src, src_len, limit, expect_crc32, mid_cap, level, dst, dst_cap, results); }
  catch (...) {
    try { if (ctx) ctx->last_error = "zipc_hip: out of memory (or no thread) on the host while setting up a many-stream call"; } catch (...) {}
    if (results) for (size_t i = 0; i < n; i++) results[i] = zipc_hip_recode_result{ZIPC_HIP_ERR_NOMEM, 0, 0, 0, 0, 0};
    return ZIPC_HIP_ERR_NOMEM;
  }
}

// ---- the zlib container (zlib_container.h has the rules; zlib.hip the two kernels of the batch forms) --------------

static int zlib_crc_op(const zipc_hip_ctx *ctx) { return ctx->adler_rfc1950 ? ZIPC_HIP_CRC_ADLER32_RFC1950 : ZIPC_HIP_CRC_ADLER32; }

// zlib_open_kernel over the caller's descriptors: the codec's descriptors and the checks' verdicts, in the context's scratch
static int zlib_open(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs, size_t n, int compress) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, ctx->ensure(ctx->zlib_descs, n * sizeof(StreamDesc)));
  HIP_TRY(ctx, ctx->ensure(ctx->zlib_pre, n * sizeof(ZlibPre)));
  ZD_LAUNCH(ctx, "zlib_open", zlib_open_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (const uint8_t *)d_src_arena,
            (const StreamDesc *)d_descs, (uint32_t)n, compress, (StreamDesc *)ctx->zlib_descs.p, (ZlibPre *)ctx->zlib_pre.p);
  HIP_TRY(ctx, hipGetLastError());
  return ZIPC_HIP_OK;
}
static int zlib_close(zipc_hip_ctx *ctx, void *d_dst_arena, const zipc_hip_stream_desc *d_descs, zipc_hip_stream_result *d_results,
                      size_t n, int compress, int level) {
  ZD_LAUNCH(ctx, "zlib_close", zlib_close_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (uint8_t *)d_dst_arena,
            (const StreamDesc *)d_descs, (const ZlibPre *)ctx->zlib_pre.p, (StreamResult *)d_results, (uint32_t)n, compress, level);
  HIP_TRY(ctx, hipGetLastError());
  return ZIPC_HIP_OK;
}

int zipc_hip_zlib_decompress_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena, const zipc_hip_stream_desc *d_descs,
                                   zipc_hip_stream_result *d_results, size_t n_streams, size_t max_dst_cap) {
  if (!ctx || !d_descs || !d_results || n_streams > 0x7FFFFFFFull) return ZIPC_HIP_ERR_INVALID_ARG;
  if (n_streams == 0) return ZIPC_HIP_OK;
  if (n_streams == 1 && max_dst_cap > MAX_STREAM_LEN) return ZIPC_HIP_ERR_INVALID_ARG;  // (that path has no Adler-32: inflate.hip inflate_huge_stream)
  int st = zlib_open(ctx, d_src_arena, d_descs, n_streams, 0);
  if (st) return st;
  st = zipc_hip_inflate_batch(ctx, d_src_arena, d_dst_arena, (const zipc_hip_stream_desc *)ctx->zlib_descs.p, d_results, n_streams,
                              max_dst_cap, zlib_crc_op(ctx));
  if (st) return st;
  return zlib_close(ctx, d_dst_arena, d_descs, d_results, n_streams, 0, 0);
}

// the sizes of a batch of zlib streams: the container's checks, the size kernel over the bodies, the checks' verdicts over its results
int zipc_hip_zlib_size_batch(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs,
                             zipc_hip_stream_result *d_results, size_t n_streams) {
  if (!ctx || !d_descs || !d_results || n_streams > 0x7FFFFFFFull) return ZIPC_HIP_ERR_INVALID_ARG;
  if (n_streams == 0) return ZIPC_HIP_OK;
  int st = zlib_open(ctx, d_src_arena, d_descs, n_streams, 0);
  if (st) return st;
  st = zipc_hip_inflate_size_batch(ctx, d_src_arena, (const zipc_hip_stream_desc *)ctx->zlib_descs.p, d_results, n_streams);
  if (st) return st;
  ZD_LAUNCH(ctx, "zlib_close_size", zlib_close_size_kernel, dim3((unsigned)((n_streams + 255) / 256)), dim3(256), 0,
            (const ZlibPre *)ctx->zlib_pre.p, (StreamResult *)d_results, (uint32_t)n_streams);
  HIP_TRY(ctx, hipGetLastError());
  return ZIPC_HIP_OK;
}

int zipc_hip_zlib_compress_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena, const zipc_hip_stream_desc *d_descs,
                                 zipc_hip_stream_result *d_results, size_t n_streams, size_t max_src_len, size_t total_src_len,
                                 int level) {
  if (!ctx || !d_descs || !d_results || n_streams > 0x7FFFFFFFull || level < 0 || level > 3) return ZIPC_HIP_ERR_INVALID_ARG;
  if (max_src_len > MAX_STREAM_LEN) return ZIPC_HIP_ERR_INVALID_ARG;
  if (n_streams == 0) return ZIPC_HIP_OK;
  int st = zlib_open(ctx, d_src_arena, d_descs, n_streams, 1);
  if (st) return st;
  st = zipc_hip_deflate_batch(ctx, d_src_arena, d_dst_arena, (const zipc_hip_stream_desc *)ctx->zlib_descs.p, d_results, n_streams,
                              max_src_len, total_src_len, level, zlib_crc_op(ctx));
  if (st) return st;
  return zlib_close(ctx, d_dst_arena, d_descs, d_results, n_streams, 1, level);
}

// The many-stream host forms: the same two steps on the host around many_streams -- the streams' bodies (or the room
// behind their headers) go through it as raw streams, a stream that fails the container's check as one of no bytes and
// no room.  results[] is defined on every return: an entry the pipeline never wrote carries the call's status.
constexpr uint32_t ZLIB_RESULT_UNSET = 0xFFFFFFFFu;
static int zlib_many(zipc_hip_ctx *ctx, bool decompress, size_t n, const void *const *src, const size_t *src_len, const size_t *limit,
                     int level, void *const *dst, const size_t *dst_cap, zipc_hip_stream_result *results) {
  auto fail = [&](int st) {
    if (results) for (size_t i = 0; i < n; i++) results[i] = zipc_hip_stream_result{(uint32_t)st, 0, 0};
    return st;
  };
  if (!ctx || (n && (!src || !src_len || !dst || !dst_cap || !results)) || level < 0 || level > 3) return fail(ZIPC_HIP_ERR_INVALID_ARG);
  for (size_t i = 0; i < n; i++)
    if ((!src[i] && src_len[i]) || (!dst[i] && dst_cap[i])) return fail(ZIPC_HIP_ERR_INVALID_ARG);
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
    results[i] = zipc_hip_stream_result{ZLIB_RESULT_UNSET, 0, 0};
  }
  const int st = many_streams(ctx, decompress ? MANY_INFLATE : MANY_DEFLATE, n, in_src.data(), in_len.data(), decompress ? limit : nullptr, level, zlib_crc_op(ctx),
                              in_dst.data(), in_cap.data(), results);
  for (size_t i = 0; i < n; i++) {
    StreamResult inner{results[i].status, results[i].checksum, results[i].out_len};
    if (inner.status == ZLIB_RESULT_UNSET) { inner.status = (uint32_t)(st ? st : ZIPC_HIP_ERR_HIP); inner.checksum = 0; inner.out_len = 0; }
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
int zipc_hip_zlib_decompress_many(zipc_hip_ctx *ctx, size_t n, const void *const *src, const size_t *src_len, const size_t *limit,
                                  void *const *dst, const size_t *dst_cap, zipc_hip_stream_result *results) {
  try { return zlib_many(ctx, true, n, src, src_len, limit, 0, dst, dst_cap, results); }
  catch (...) { return many_threw(ctx, n, results); }
}
int zipc_hip_zlib_compress_many(zipc_hip_ctx *ctx, size_t n, const void *const *src, const size_t *src_len, int level,
                                void *const *dst, const size_t *dst_cap, zipc_hip_stream_result *results) {
  try { return zlib_many(ctx, false, n, src, src_len, nullptr, level, dst, dst_cap, results); }
  catch (...) { return many_threw(ctx, n, results); }
}

// zlib_decompress src/zipc_deflate.ml:720-740 (start = 0): the container's six bytes on the
// host (zlib_container.h), body through the inflate kernel with Adler-32
int zipc_hip_zlib_decompress(zipc_hip_ctx *ctx, const void *src, size_t len, int has_limit,
                             size_t limit, void *dst, size_t dst_cap, size_t *out_len,
                             uint32_t *adler, uint32_t *expect, uint32_t *found) {
  if (!ctx || (!src && len) || !out_len) return ZIPC_HIP_ERR_INVALID_ARG;
  *out_len = 0;
  const uint8_t *s = (const uint8_t *)src;
  const bool whole = len >= ZLIB_MIN_LEN;
  const uint32_t pre = zlib_open_status(len, whole ? s[0] : 0, whole ? s[1] : 0);
  if (pre != ST_OK) return (int)pre;
  const uint32_t e = zlib_expect(s + len - 4);
  uint32_t f = 0;
  // the reference hands inflate the range [2, len-2) (src/zipc_deflate.ml:732)
  int st = zipc_hip_inflate(ctx, s + zlib_body_off(0), (size_t)zlib_body_len(len), has_limit, limit, zlib_crc_op(ctx), dst, dst_cap,
                            out_len, &f);
  if (st) return st;
  if (expect) *expect = e;
  if (found) *found = f;
  if (e != f) { *out_len = 0; return ZIPC_HIP_ERR_CHECKSUM; }
  if (adler) *adler = f;
  return ZIPC_HIP_OK;
}

// zlib_compress src/zipc_deflate.ml:1262-1277 (start = 0)
int zipc_hip_zlib_compress(zipc_hip_ctx *ctx, const void *src, size_t len, int level, void *dst,
                           size_t dst_cap, size_t *out_len, uint32_t *adler) {
  if (!ctx || !dst || !out_len || level < 0 || level > 3) return ZIPC_HIP_ERR_INVALID_ARG;
  *out_len = 0;
  if (dst_cap < ZLIB_OVERHEAD) return ZIPC_HIP_ERR_DST_TOO_SMALL;
  uint8_t *o = (uint8_t *)dst;
  o[0] = (uint8_t)zlib_cmf();
  o[1] = (uint8_t)zlib_flg(level);
  size_t body = 0;
  uint32_t a = 0;
  int st = zipc_hip_deflate(ctx, src, len, level, zlib_crc_op(ctx), o + zlib_payload_off(0), (size_t)zlib_payload_cap(dst_cap),
                            &body, &a);
  if (st) return st;
  zlib_put_trailer(o + 2 + body, a);
  *out_len = body + ZLIB_OVERHEAD;
  if (adler) *adler = a;
  return ZIPC_HIP_OK;
}

}  // extern "C"
