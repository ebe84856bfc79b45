// api.hip -- the C ABI of include/zipc_hip.h, all of it but the many-stream host forms (many.hip): the context and its
// scratch, tuning(), the CRC-32 pass and the checksum launches, the batch forms as argument checks around the launchers
// of deflate.hip, inflate.hip, zlib.hip, gzip.hip, recode.hip and packed.hip (ctx.h), and the one-stream host forms.
//
// Host forms stage one stream through device scratch and run the same kernels as
// the batch forms (a batch of one).  Nothing here computes on the CPU: with no
// usable device the calls fail with ZIPC_HIP_ERR_NO_DEVICE / ZIPC_HIP_ERR_HIP.

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <vector>
#include "ctx.h"
#include "deflate_packed.h"
#include "deflate_scratch.h"
#include "gzip_container.h"
#include "packed_layout.h"
#include "recode_rules.h"
#include "tuning.h"
#include "inflate_history.h"
#include "zlib_container.h"

using namespace zd;

static_assert(sizeof(zipc_hip_stream_desc) == sizeof(StreamDesc), "desc layout");
static_assert(sizeof(zipc_hip_stream_result) == sizeof(StreamResult), "result layout");
static_assert(ZIPC_HIP_BLOCKS_MIN_SRC == BLOCKS_MIN_SRC, "forms.h");
static_assert(sizeof(zipc_hip_recode_desc) == sizeof(RecodeDesc) && sizeof(RecodeDesc) == 64, "recode desc layout");
static_assert(sizeof(zipc_hip_recode_result) == sizeof(RecodeResult) && sizeof(RecodeResult) == 32, "recode result layout");
static_assert(sizeof(zipc_hip_packed_result) == sizeof(PackedResult) && sizeof(PackedResult) == 32, "packed result layout");
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
// zipc_hip_checksum_batch's scratch, from the declared numbers alone: the plan (its call-wide word in 256 bytes, then
// 8 + 4 bytes per range), segs_bound partials, chunks_bound pairs of chunk sums
int checksum_ranges_reserve(zipc_hip_ctx *ctx, size_t n_ranges, size_t total_len, int want_adler32) {
  HIP_TRY(ctx, ctx->ensure(ctx->ranges_plan, 256 + n_ranges * (sizeof(uint64_t) + sizeof(uint32_t))));
  HIP_TRY(ctx, ctx->ensure(ctx->crc_partials, (size_t)ranges_segs_bound(total_len, n_ranges) * sizeof(uint32_t)));
  if (want_adler32) HIP_TRY(ctx, ctx->ensure(ctx->adler_sums, (size_t)ranges_chunks_bound(total_len, n_ranges) * sizeof(uint2)));
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
  many_pools_acquire();  // (released by zipc_hip_destroy: the last context to go joins the staging threads)
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
  free_buf(ctx->ranges_plan); free_buf(ctx->io_ranges);
  free_buf(ctx->io_small); free_buf(ctx->crc_partials); free_buf(ctx->crc_nib); free_buf(ctx->adler_sums);
  free_buf(ctx->deflate_scratch); free_buf(ctx->parse_scratch);
  free_buf(ctx->inflate_scratch);
  free_buf(ctx->blocks_scratch);
  free_buf(ctx->tok_scratch);
  free_buf(ctx->descs_marked);
  free_buf(ctx->size_descs); free_buf(ctx->size_head); free_buf(ctx->size_rest);
  free_buf(ctx->zlib_descs); free_buf(ctx->zlib_pre); free_buf(ctx->gzip_descs); free_buf(ctx->gzip_pre); free_buf(ctx->prefix_adlers); free_buf(ctx->zlib_hist); free_buf(ctx->dict_adler); free_buf(ctx->io_dict); free_buf(ctx->extent_inner);
  free_buf(ctx->recode_descs); free_buf(ctx->recode_res); free_buf(ctx->recode_verdicts);
  free_buf(ctx->packed_descs); free_buf(ctx->packed_res); free_buf(ctx->packed_verdicts);
  free_buf(ctx->dpacked_staging); free_buf(ctx->dpacked_descs); free_buf(ctx->dpacked_res);
  free_buf(ctx->dpacked_plan); free_buf(ctx->dpacked_verdicts);
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
  many_pools_release();
}

void *zipc_hip_stream(zipc_hip_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

int zipc_hip_synchronize(zipc_hip_ctx *ctx) {
  if (!ctx) return ZIPC_HIP_ERR_INVALID_ARG;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return ZIPC_HIP_OK;
}

const char *zipc_hip_last_error(zipc_hip_ctx *ctx) { return ctx ? ctx->last_error.c_str() : ""; }
unsigned zipc_hip_last_inflate_blocks(zipc_hip_ctx *ctx) { return ctx ? ctx->last_inflate_blocks : 0u; }
unsigned zipc_hip_last_size_blocks(zipc_hip_ctx *ctx) { return ctx ? ctx->last_size_blocks : 0u; }
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

int zipc_hip_inflate_prefix_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena, const zipc_hip_stream_desc *d_descs,
                                  zipc_hip_prefix_result *d_results, size_t n_streams) {
  if (!ctx || !d_descs || !d_results || n_streams > 0x7FFFFFFFull) return ZIPC_HIP_ERR_INVALID_ARG;
  return launch_inflate_prefix(ctx, d_src_arena, d_dst_arena, d_descs, d_results, n_streams, ZIPC_HIP_CRC_NOP, nullptr);
}

// The history forms (inflate_history.h has the rule): the three forms above started from a record per stream
int zipc_hip_inflate_history_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena, const zipc_hip_stream_desc *d_descs,
                                   const zipc_hip_history *d_hist, zipc_hip_stream_result *d_results, size_t n_streams, size_t max_dst_cap,
                                   int crc_op) {
  if (!ctx || !d_descs || !d_results) return ZIPC_HIP_ERR_INVALID_ARG;
  if (crc_op < 0 || crc_op > 3 || n_streams > 0x7FFFFFFFull) return ZIPC_HIP_ERR_INVALID_ARG;
  return launch_inflate_history(ctx, d_src_arena, d_dst_arena, d_descs, d_hist, d_results, n_streams, max_dst_cap, crc_op);
}

int zipc_hip_inflate_prefix_history_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena, const zipc_hip_stream_desc *d_descs,
                                          const zipc_hip_history *d_hist, zipc_hip_prefix_result *d_results, size_t n_streams) {
  if (!ctx || !d_descs || !d_results || n_streams > 0x7FFFFFFFull) return ZIPC_HIP_ERR_INVALID_ARG;
  return launch_inflate_prefix_history(ctx, d_src_arena, d_dst_arena, d_descs, d_hist, d_results, n_streams);
}

int zipc_hip_inflate_size_history_batch(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs,
                                        const zipc_hip_history *d_hist, zipc_hip_stream_result *d_results, size_t n_streams) {
  if (!ctx || !d_descs || !d_results || n_streams > 0x7FFFFFFFull) return ZIPC_HIP_ERR_INVALID_ARG;
  return launch_inflate_size_history(ctx, d_src_arena, d_descs, d_hist, d_results, n_streams);
}

int zipc_hip_inflate_size_blocks_batch(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs,
                                       zipc_hip_stream_result *d_results, size_t n_streams) {
  if (!ctx || !d_descs || !d_results || n_streams > 0x7FFFFFFFull) return ZIPC_HIP_ERR_INVALID_ARG;
  return launch_inflate_size_blocks(ctx, d_src_arena, d_descs, d_results, n_streams, nullptr);
}

// The extent forms (inflate_extent.h has the rule): the forms above with src_used in a 32-byte result
int zipc_hip_inflate_extent_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena, const zipc_hip_stream_desc *d_descs,
                                  zipc_hip_extent_result *d_results, size_t n_streams, size_t max_dst_cap, int crc_op) {
  if (!ctx || !d_descs || !d_results) return ZIPC_HIP_ERR_INVALID_ARG;
  if (crc_op < 0 || crc_op > 3 || n_streams > 0x7FFFFFFFull) return ZIPC_HIP_ERR_INVALID_ARG;
  return launch_inflate_extent(ctx, d_src_arena, d_dst_arena, d_descs, d_results, n_streams, max_dst_cap, crc_op);
}

int zipc_hip_inflate_size_extent_batch(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs,
                                       zipc_hip_extent_result *d_results, size_t n_streams) {
  if (!ctx || !d_descs || !d_results || n_streams > 0x7FFFFFFFull) return ZIPC_HIP_ERR_INVALID_ARG;
  return launch_inflate_size_extent(ctx, d_src_arena, d_descs, d_results, n_streams);
}

int zipc_hip_inflate_size_extent_blocks_batch(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs,
                                              zipc_hip_extent_result *d_results, size_t n_streams) {
  if (!ctx || !d_descs || !d_results || n_streams > 0x7FFFFFFFull) return ZIPC_HIP_ERR_INVALID_ARG;
  return launch_inflate_size_extent_blocks(ctx, d_src_arena, d_descs, d_results, n_streams, nullptr);
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

int zipc_hip_debug_chain_links_form(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs, size_t n_streams,
                                    size_t max_src_len, size_t total_src_len, int chain, size_t seg_positions, void *d_links,
                                    size_t links_cap, void *d_pos_base) {
  if (!ctx || !d_descs || !d_links || chain < 0 || chain > 3 || n_streams == 0 || n_streams > 0x7FFFFFFFull || max_src_len > MAX_STREAM_LEN)
    return ZIPC_HIP_ERR_INVALID_ARG;
  const bool by_segments = chain == zd::CHAIN_XCHG_SEGMENTS || chain == zd::CHAIN_PEEL_SEGMENTS;
  if (by_segments && seg_positions && !zd::chain_seg_known(chain, seg_positions)) return ZIPC_HIP_ERR_INVALID_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, ctx->ensure(ctx->deflate_scratch, deflate_scratch_bytes(n_streams, max_src_len, total_src_len, ZIPC_HIP_LEVEL_DEFAULT, zd::tuning())));
  HIP_TRY(ctx, zd::debug_chain_links_form(ctx, (const uint8_t *)d_src_arena, (const StreamDesc *)d_descs, n_streams, max_src_len, total_src_len,
                                          chain, by_segments ? seg_positions : 0, ZIPC_HIP_DEBUG_LINK_POISON, (uint16_t *)d_links, links_cap,
                                          (uint64_t *)d_pos_base));
  return ZIPC_HIP_OK;
}

int zipc_hip_debug_match_records(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs, size_t n_streams,
                                 size_t max_src_len, size_t total_src_len, int level, int match_form, long tiles_per_group,
                                 void *d_match, void *d_snap, size_t records_cap, void *d_snap_used, void *d_pos_base) {
  if (!ctx || !d_descs || !d_match || !d_snap || !d_snap_used || !d_pos_base || level < 1 || level > 3 || match_form < 0 || match_form > 2 ||
      tiles_per_group < 0 || n_streams == 0 || n_streams > 0x7FFFFFFFull || max_src_len > MAX_STREAM_LEN)
    return ZIPC_HIP_ERR_INVALID_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, ctx->ensure(ctx->deflate_scratch, deflate_scratch_bytes(n_streams, max_src_len, total_src_len, level, zd::tuning())));
  HIP_TRY(ctx, zd::debug_match_records(ctx, (const uint8_t *)d_src_arena, (const StreamDesc *)d_descs, n_streams, max_src_len, total_src_len,
                                       level, match_form, tiles_per_group, (uint32_t *)d_match, (uint32_t *)d_snap, records_cap,
                                       (uint32_t *)d_snap_used, (uint64_t *)d_pos_base));
  return ZIPC_HIP_OK;
}

int zipc_hip_debug_inflate_tokens(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena, const zipc_hip_stream_desc *d_descs,
                                  zipc_hip_stream_result *d_results, size_t n_streams, size_t max_dst_cap, int form, int hops0, int hops1,
                                  void *d_tok_raw, void *d_tok_done, zipc_hip_debug_token_record *records) {
  if (!ctx || !d_descs || !d_results || !d_tok_raw || !d_tok_done || !records || n_streams > 0x7FFFFFFFull) return ZIPC_HIP_ERR_INVALID_ARG;
  if (form < -1 || form > 1 || hops0 < 0 || hops0 > 65536 || hops1 < 0 || hops1 > 65536) return ZIPC_HIP_ERR_INVALID_ARG;
  memset(records, 0, n_streams * sizeof *records);
  zd::BlocksDebug dbg;
  dbg.form = form; dbg.hops0 = hops0; dbg.hops1 = hops1;
  dbg.d_tok_raw = (uint32_t *)d_tok_raw; dbg.d_tok_done = (uint32_t *)d_tok_done;
  dbg.records = records;
  return launch_inflate(ctx, d_src_arena, d_dst_arena, d_descs, d_results, n_streams, max_dst_cap, ZIPC_HIP_CRC_NOP, nullptr, true, &dbg);
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

// The ragged pass (checksum_ranges.h has the rules, checksum.hip the kernels): plan, one pass over the bytes, two finishes
int zipc_hip_checksum_batch(zipc_hip_ctx *ctx, const void *d_arena, size_t arena_len, const zipc_hip_range *d_ranges,
                            zipc_hip_checksum_result *d_results, size_t n_ranges, size_t total_len, int want_crc32,
                            int want_adler32) {
  if (!ctx || !d_ranges || !d_results || (!d_arena && arena_len) || (!want_crc32 && !want_adler32)) return ZIPC_HIP_ERR_INVALID_ARG;
  if (n_ranges > 0x7FFFFFFFull || ranges_segs_bound(total_len, n_ranges) > 0x7FFFFFFFull) return ZIPC_HIP_ERR_INVALID_ARG;
  if (n_ranges == 0) return ZIPC_HIP_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int st = checksum_ranges_reserve(ctx, n_ranges, total_len, want_adler32);
  if (st) return st;
  const uint32_t n = (uint32_t)n_ranges;
  const uint64_t segs_bound = ranges_segs_bound(total_len, n_ranges), chunks_bound = ranges_chunks_bound(total_len, n_ranges);
  RangesPlan P;
  P.call = (RangesCall *)ctx->ranges_plan.p;
  P.chunk_base = (uint64_t *)((uint8_t *)ctx->ranges_plan.p + 256);
  P.seg_base = (uint32_t *)(P.chunk_base + n_ranges);
  const Range *ranges = (const Range *)d_ranges;
  RangeResult *results = (RangeResult *)d_results;
  uint32_t *partials = (uint32_t *)ctx->crc_partials.p;
  uint2 *sums = (uint2 *)ctx->adler_sums.p;
  ZD_LAUNCH(ctx, "checksum_plan", checksum_plan_kernel, dim3(1), dim3(RANGES_PLAN_TILE), 0, ranges, n, (uint64_t)arena_len,
            (uint64_t)total_len, P, results, sums, want_adler32 ? chunks_bound : (uint64_t)0);
  HIP_TRY(ctx, hipGetLastError());
  // Adler-32 alone runs the fused pass too and leaves the CRC partials unused (there is no chunk-list kernel for a batch)
  if (want_adler32) {
    ZD_LAUNCH(ctx, "crc32_adler_ranges", crc32_adler_ranges_kernel, dim3((unsigned)segs_bound), dim3(256), 0, (const uint8_t *)d_arena,
              ranges, n, P, (const uint32_t *)ctx->crc_nib.p, partials, sums);
  } else {
    ZD_LAUNCH(ctx, "crc32_ranges", crc32_ranges_kernel, dim3((unsigned)segs_bound), dim3(256), 0, (const uint8_t *)d_arena, ranges, n,
              P, (const uint32_t *)ctx->crc_nib.p, partials);
  }
  HIP_TRY(ctx, hipGetLastError());
  if (want_crc32)
    ZD_LAUNCH(ctx, "crc32_finish_ranges", crc32_finish_ranges_kernel, dim3((unsigned)((n_ranges + 3) / 4)), dim3(256), 0, ranges, n, P,
              ctx->crc_consts, (const uint32_t *)partials, results);
  if (want_adler32)
    ZD_LAUNCH(ctx, "adler_finish_ranges", adler_finish_ranges_kernel, dim3((unsigned)((n_ranges + 255) / 256)), dim3(256), 0, ranges, n,
              P, (const uint2 *)sums, ctx->adler_rfc1950 ? 1 : 0, results);
  HIP_TRY(ctx, hipGetLastError());
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

// what one host stream inflates to: zipc_hip_inflate_size_blocks_batch of one around a copy in and the result's 16 bytes back
// (the descriptor is handed over with the call: nothing is read back before the path is chosen)
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
  st = launch_inflate_size_blocks(ctx, ctx->io_src.p, (const zipc_hip_stream_desc *)ctx->io_desc.p, (zipc_hip_stream_result *)ctx->io_res.p, 1, &d);
  if (st) return st;
  StreamResult r;
  HIP_TRY(ctx, hipMemcpyAsync(&r, ctx->io_res.p, sizeof r, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (r.status != ST_OK) return (int)r.status;
  *out_len = r.out_len;
  return ZIPC_HIP_OK;
}

// one host stream of unknown length through an extent batch form of one (zlib: the container's form), staged like one_stream
static int one_stream_extent(zipc_hip_ctx *ctx, bool zlib, const void *src, size_t len, int has_limit, size_t limit, void *dst,
                             size_t dst_cap, int crc_op, size_t *out_len, size_t *src_used, uint32_t *checksum) {
  if (!ctx || (!src && len) || (!dst && dst_cap) || !out_len || !src_used) return ZIPC_HIP_ERR_INVALID_ARG;
  *out_len = 0;
  *src_used = 0;
  if (checksum) *checksum = 0;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int st = stage_in(ctx, src, len);
  if (st) return st;
  HIP_TRY(ctx, ctx->ensure(ctx->io_dst, dst_cap + 64));
  HIP_TRY(ctx, ctx->ensure(ctx->io_desc, sizeof(StreamDesc)));
  HIP_TRY(ctx, ctx->ensure(ctx->io_res, sizeof(ExtentResult)));
  StreamDesc d;
  memset(&d, 0, sizeof d);
  d.src_off = 0; d.src_len = len; d.dst_off = 0; d.dst_cap = dst_cap;
  d.limit = limit; d.flags = has_limit ? STREAM_HAS_LIMIT : 0;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->io_desc.p, &d, sizeof d, hipMemcpyHostToDevice, ctx->stream));
  if (zlib)
    st = zipc_hip_zlib_decompress_extent_batch(ctx, ctx->io_src.p, ctx->io_dst.p, (zipc_hip_stream_desc *)ctx->io_desc.p,
                                               (zipc_hip_extent_result *)ctx->io_res.p, 1, dst_cap);
  else
    st = zipc_hip_inflate_extent_batch(ctx, ctx->io_src.p, ctx->io_dst.p, (zipc_hip_stream_desc *)ctx->io_desc.p,
                                       (zipc_hip_extent_result *)ctx->io_res.p, 1, dst_cap, crc_op);
  if (st) return st;
  ExtentResult r;
  HIP_TRY(ctx, hipMemcpyAsync(&r, ctx->io_res.p, sizeof r, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (r.status != ST_OK) {
    if (checksum) *checksum = r.checksum;  // (ZIPC_HIP_ERR_CHECKSUM: the value found; 0 with every other status)
    return (int)r.status;
  }
  if (r.out_len > dst_cap) return ZIPC_HIP_ERR_DST_TOO_SMALL;
  if (r.out_len) {
    HIP_TRY(ctx, hipMemcpyAsync(dst, ctx->io_dst.p, r.out_len, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  *out_len = r.out_len;
  *src_used = r.src_used;
  if (checksum) *checksum = r.checksum;
  return ZIPC_HIP_OK;
}

int zipc_hip_inflate_extent(zipc_hip_ctx *ctx, const void *src, size_t len, int has_limit, size_t limit, void *dst, size_t dst_cap,
                            int crc_op, size_t *out_len, size_t *src_used, uint32_t *checksum) {
  return one_stream_extent(ctx, false, src, len, has_limit, limit, dst, dst_cap, crc_op, out_len, src_used, checksum);
}
int zipc_hip_zlib_decompress_extent(zipc_hip_ctx *ctx, const void *src, size_t len, int has_limit, size_t limit, void *dst,
                                    size_t dst_cap, size_t *out_len, size_t *src_used, uint32_t *adler) {
  return one_stream_extent(ctx, true, src, len, has_limit, limit, dst, dst_cap, 0, out_len, src_used, adler);
}

int zipc_hip_deflate(zipc_hip_ctx *ctx, const void *src, size_t len, int level, int crc_op, void *dst,
                     size_t dst_cap, size_t *out_len, uint32_t *checksum) {
  if (level < 0 || level > 3) return ZIPC_HIP_ERR_INVALID_ARG;
  return one_stream(ctx, false, src, len, 0, 0, level, crc_op, dst, dst_cap, out_len, checksum);
}

// ---- recode on the device (recode_rules.h has the rules; recode.hip the three kernels and their sequence) ---------------

int zipc_hip_recode_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_mid_arena, void *d_dst_arena,
                          const zipc_hip_recode_desc *d_descs, zipc_hip_recode_result *d_results, size_t n_streams,
                          size_t max_mid_cap, size_t total_mid_cap, int level) {
  if (!ctx || !d_descs || !d_results || n_streams > 0x7FFFFFFFull || level < 0 || level > 3) return ZIPC_HIP_ERR_INVALID_ARG;
  if (max_mid_cap > MAX_STREAM_LEN) return ZIPC_HIP_ERR_INVALID_ARG;  // (deflate takes no longer source; inflate_huge_stream's output is none)
  if (n_streams == 0) return ZIPC_HIP_OK;
  return launch_recode(ctx, d_src_arena, d_mid_arena, d_dst_arena, (const RecodeDesc *)d_descs, (RecodeResult *)d_results, nullptr,
                       n_streams, max_mid_cap, total_mid_cap, level, nullptr, true);
}

// ---- the zlib container (zlib_container.h has the rules; zlib.hip the kernels of the batch forms and their launches) --

int zipc_hip_zlib_decompress_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena, const zipc_hip_stream_desc *d_descs,
                                   zipc_hip_stream_result *d_results, size_t n_streams, size_t max_dst_cap) {
  if (!ctx || !d_descs || !d_results || n_streams > 0x7FFFFFFFull) return ZIPC_HIP_ERR_INVALID_ARG;
  if (n_streams == 0) return ZIPC_HIP_OK;
  if (n_streams == 1 && max_dst_cap > MAX_STREAM_LEN) return ZIPC_HIP_ERR_INVALID_ARG;  // (that path has no Adler-32: inflate.hip inflate_huge_stream)
  int st = launch_zlib_open(ctx, d_src_arena, d_descs, n_streams, 0);
  if (st) return st;
  st = zipc_hip_inflate_batch(ctx, d_src_arena, d_dst_arena, (const zipc_hip_stream_desc *)ctx->zlib_descs.p, d_results, n_streams,
                              max_dst_cap, zlib_crc_op(ctx));
  if (st) return st;
  return launch_zlib_close(ctx, d_dst_arena, d_descs, d_results, n_streams, 0, 0);
}

// the sizes of a batch of zlib streams: the container's checks, the size kernel over the bodies, the checks' verdicts over its results
int zipc_hip_zlib_size_batch(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs,
                             zipc_hip_stream_result *d_results, size_t n_streams) {
  if (!ctx || !d_descs || !d_results || n_streams > 0x7FFFFFFFull) return ZIPC_HIP_ERR_INVALID_ARG;
  if (n_streams == 0) return ZIPC_HIP_OK;
  int st = launch_zlib_open(ctx, d_src_arena, d_descs, n_streams, 0);
  if (st) return st;
  st = zipc_hip_inflate_size_batch(ctx, d_src_arena, (const zipc_hip_stream_desc *)ctx->zlib_descs.p, d_results, n_streams);
  if (st) return st;
  return launch_zlib_close_size(ctx, d_results, n_streams);
}

// The first dst_cap bytes of every zlib stream: open as ever, the prefix kernel over the bodies with the context's Adler-32,
// and zlib_container.h's zlib_close_prefix -- an ended stream's Adler-32 is compared, a cut one's is not
int zipc_hip_zlib_decompress_prefix_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena,
                                          const zipc_hip_stream_desc *d_descs, zipc_hip_prefix_result *d_results, size_t n_streams) {
  if (!ctx || !d_descs || !d_results || n_streams > 0x7FFFFFFFull) return ZIPC_HIP_ERR_INVALID_ARG;
  ctx->last_inflate_blocks = 0;
  if (n_streams == 0) return ZIPC_HIP_OK;
  int st = launch_zlib_open(ctx, d_src_arena, d_descs, n_streams, 0);
  if (st) return st;
  HIP_TRY(ctx, ctx->ensure(ctx->prefix_adlers, n_streams * sizeof(uint32_t)));
  st = launch_inflate_prefix(ctx, d_src_arena, d_dst_arena, (const zipc_hip_stream_desc *)ctx->zlib_descs.p, d_results, n_streams,
                             zlib_crc_op(ctx), (uint32_t *)ctx->prefix_adlers.p);
  if (st) return st;
  return launch_zlib_close_prefix(ctx, d_results, n_streams);
}

// The zlib dictionary forms (zlib_container.h zlib_open_dict): RFC 1950's Adler-32 of the dictionary by the checksum kernels
// into the context's scratch, the open that compares every DICTID with it and leaves a history record per stream, (to
// decompress) the seed and the history kernel over the bodies with the context's Adler-32, or the sizing history kernel,
// and the close.  Nothing is read back.
static int zlib_dict_front(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs, size_t n_streams, const void *d_dict,
                           size_t dict_len) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, ctx->ensure(ctx->dict_adler, 2 * sizeof(uint32_t)));
  if (dict_len) {  // (always RFC 1950's: the DICTID is zlib's, whatever flavour this context compares outputs in)
    const bool flavour = ctx->adler_rfc1950;
    ctx->adler_rfc1950 = true;
    const int st = zipc_hip_checksum_device(ctx, d_dict, dict_len, 0, 1, (uint32_t *)ctx->dict_adler.p);
    ctx->adler_rfc1950 = flavour;
    if (st) return st;
  }
  return launch_zlib_open_dict(ctx, d_src_arena, d_descs, n_streams, dict_len, (const uint32_t *)ctx->dict_adler.p + 1);
}
int zipc_hip_zlib_decompress_dict_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena, const zipc_hip_stream_desc *d_descs,
                                        zipc_hip_stream_result *d_results, size_t n_streams, size_t max_dst_cap, const void *d_dict,
                                        size_t dict_len) {
  if (!ctx || !d_descs || !d_results || n_streams > 0x7FFFFFFFull || dict_len > HISTORY_MAX_LEN || (!d_dict && dict_len)) return ZIPC_HIP_ERR_INVALID_ARG;
  ctx->last_inflate_blocks = 0;
  if (n_streams == 0) return ZIPC_HIP_OK;
  int st = zlib_dict_front(ctx, d_src_arena, d_descs, n_streams, d_dict, dict_len);
  if (st) return st;
  st = launch_zlib_seed_dict(ctx, d_dst_arena, d_descs, n_streams, d_dict, dict_len);
  if (st) return st;
  st = launch_inflate_history(ctx, d_src_arena, d_dst_arena, (const zipc_hip_stream_desc *)ctx->zlib_descs.p,
                              (const zipc_hip_history *)ctx->zlib_hist.p, d_results, n_streams, max_dst_cap, zlib_crc_op(ctx));
  if (st) return st;
  return launch_zlib_close_dict(ctx, d_results, n_streams, 0);
}
int zipc_hip_zlib_size_dict_batch(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs,
                                  zipc_hip_stream_result *d_results, size_t n_streams, const void *d_dict, size_t dict_len) {
  if (!ctx || !d_descs || !d_results || n_streams > 0x7FFFFFFFull || dict_len > HISTORY_MAX_LEN || (!d_dict && dict_len)) return ZIPC_HIP_ERR_INVALID_ARG;
  ctx->last_size_blocks = 0;
  if (n_streams == 0) return ZIPC_HIP_OK;
  int st = zlib_dict_front(ctx, d_src_arena, d_descs, n_streams, d_dict, dict_len);
  if (st) return st;
  st = launch_inflate_size_history(ctx, d_src_arena, (const zipc_hip_stream_desc *)ctx->zlib_descs.p, (const zipc_hip_history *)ctx->zlib_hist.p,
                                   d_results, n_streams);
  if (st) return st;
  return launch_zlib_close_dict(ctx, d_results, n_streams, 1);
}

// The host forms of the two: one stream staged as [history | room] in the context's buffers, the batch form of one, the
// result's 16 bytes and then the room alone copied back
static int history_room_back(zipc_hip_ctx *ctx, size_t gap, void *dst, size_t dst_cap, size_t *out_len, uint32_t *checksum) {
  StreamResult r;
  HIP_TRY(ctx, hipMemcpyAsync(&r, ctx->io_res.p, sizeof r, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (r.status != ST_OK) {
    if (checksum) *checksum = r.checksum;  // (ZIPC_HIP_ERR_ZLIB_DICT: the DICTID found, ZIPC_HIP_ERR_CHECKSUM: the value found; else 0)
    return (int)r.status;
  }
  if (r.out_len > dst_cap) return ZIPC_HIP_ERR_DST_TOO_SMALL;
  if (r.out_len) {
    HIP_TRY(ctx, hipMemcpyAsync(dst, (const uint8_t *)ctx->io_dst.p + gap, r.out_len, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  *out_len = r.out_len;
  if (checksum) *checksum = r.checksum;
  return ZIPC_HIP_OK;
}
int zipc_hip_inflate_history(zipc_hip_ctx *ctx, const void *src, size_t len, unsigned start_bit, const void *hist, size_t hist_len,
                             int has_limit, size_t limit, void *dst, size_t dst_cap, int crc_op, size_t *out_len, uint32_t *checksum) {
  if (!ctx || (!src && len) || (!hist && hist_len) || (!dst && dst_cap) || !out_len) return ZIPC_HIP_ERR_INVALID_ARG;
  *out_len = 0;
  if (checksum) *checksum = 0;
  if (history_record_status(hist_len > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)hist_len, start_bit, hist_len, true) != ST_OK)
    return ZIPC_HIP_ERR_INVALID_ARG;  // (before anything is staged: the gap is hist_len bytes)
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int st = stage_in(ctx, src, len);
  if (st) return st;
  HIP_TRY(ctx, ctx->ensure(ctx->io_dst, hist_len + dst_cap + 64));
  HIP_TRY(ctx, ctx->ensure(ctx->io_desc, sizeof(StreamDesc)));
  HIP_TRY(ctx, ctx->ensure(ctx->io_res, sizeof(StreamResult)));
  HIP_TRY(ctx, ctx->ensure(ctx->io_small, 64));
  if (hist_len) HIP_TRY(ctx, hipMemcpyAsync(ctx->io_dst.p, hist, hist_len, hipMemcpyHostToDevice, ctx->stream));
  StreamDesc d;
  memset(&d, 0, sizeof d);
  d.src_off = 0; d.src_len = len; d.dst_off = hist_len; d.dst_cap = dst_cap;
  d.limit = limit; d.flags = has_limit ? STREAM_HAS_LIMIT : 0;
  HistoryRec h;
  h.hist_len = (uint32_t)hist_len; h.start_bit = start_bit;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->io_desc.p, &d, sizeof d, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->io_small.p, &h, sizeof h, hipMemcpyHostToDevice, ctx->stream));
  st = zipc_hip_inflate_history_batch(ctx, ctx->io_src.p, ctx->io_dst.p, (const zipc_hip_stream_desc *)ctx->io_desc.p,
                                      (const zipc_hip_history *)ctx->io_small.p, (zipc_hip_stream_result *)ctx->io_res.p, 1, dst_cap, crc_op);
  if (st) return st;
  return history_room_back(ctx, hist_len, dst, dst_cap, out_len, checksum);
}
int zipc_hip_zlib_decompress_dict(zipc_hip_ctx *ctx, const void *src, size_t len, const void *dict, size_t dict_len, void *dst, size_t dst_cap,
                                  size_t *out_len) {
  if (!ctx || (!src && len) || (!dict && dict_len) || (!dst && dst_cap) || !out_len || dict_len > HISTORY_MAX_LEN) return ZIPC_HIP_ERR_INVALID_ARG;
  *out_len = 0;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int st = stage_in(ctx, src, len);
  if (st) return st;
  HIP_TRY(ctx, ctx->ensure(ctx->io_dst, dict_len + dst_cap + 64));
  HIP_TRY(ctx, ctx->ensure(ctx->io_dict, dict_len + 64));
  HIP_TRY(ctx, ctx->ensure(ctx->io_desc, sizeof(StreamDesc)));
  HIP_TRY(ctx, ctx->ensure(ctx->io_res, sizeof(StreamResult)));
  if (dict_len) HIP_TRY(ctx, hipMemcpyAsync(ctx->io_dict.p, dict, dict_len, hipMemcpyHostToDevice, ctx->stream));
  StreamDesc d;
  memset(&d, 0, sizeof d);
  d.src_off = 0; d.src_len = len; d.dst_off = dict_len; d.dst_cap = dst_cap;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->io_desc.p, &d, sizeof d, hipMemcpyHostToDevice, ctx->stream));
  st = zipc_hip_zlib_decompress_dict_batch(ctx, ctx->io_src.p, ctx->io_dst.p, (const zipc_hip_stream_desc *)ctx->io_desc.p,
                                           (zipc_hip_stream_result *)ctx->io_res.p, 1, dst_cap, ctx->io_dict.p, dict_len);
  if (st) return st;
  return history_room_back(ctx, dict_len, dst, dst_cap, out_len, nullptr);
}

// The zlib extent forms: open as ever (its `expect`, read at src_len - 4, is not used), the extent kernel over the bodies, and
// zlib_container.h's zlib_close_extent, which finds the trailer behind the body's extent
int zipc_hip_zlib_decompress_extent_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena, const zipc_hip_stream_desc *d_descs,
                                          zipc_hip_extent_result *d_results, size_t n_streams, size_t max_dst_cap) {
  if (!ctx || !d_descs || !d_results || n_streams > 0x7FFFFFFFull) return ZIPC_HIP_ERR_INVALID_ARG;
  ctx->last_inflate_blocks = 0;
  if (n_streams == 0) return ZIPC_HIP_OK;
  int st = launch_zlib_open(ctx, d_src_arena, d_descs, n_streams, 0);
  if (st) return st;
  st = launch_inflate_extent(ctx, d_src_arena, d_dst_arena, (const zipc_hip_stream_desc *)ctx->zlib_descs.p, d_results, n_streams,
                             max_dst_cap, zlib_crc_op(ctx));
  if (st) return st;
  return launch_zlib_close_extent(ctx, d_src_arena, d_descs, d_results, n_streams, 1);
}
int zipc_hip_zlib_size_extent_batch(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs,
                                    zipc_hip_extent_result *d_results, size_t n_streams) {
  if (!ctx || !d_descs || !d_results || n_streams > 0x7FFFFFFFull) return ZIPC_HIP_ERR_INVALID_ARG;
  ctx->last_size_blocks = 0;
  if (n_streams == 0) return ZIPC_HIP_OK;
  int st = launch_zlib_open(ctx, d_src_arena, d_descs, n_streams, 0);
  if (st) return st;
  st = launch_inflate_size_extent(ctx, d_src_arena, (const zipc_hip_stream_desc *)ctx->zlib_descs.p, d_results, n_streams);
  if (st) return st;
  return launch_zlib_close_extent(ctx, d_src_arena, d_descs, d_results, n_streams, 0);
}
int zipc_hip_zlib_size_extent_blocks_batch(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs,
                                           zipc_hip_extent_result *d_results, size_t n_streams) {
  if (!ctx || !d_descs || !d_results || n_streams > 0x7FFFFFFFull) return ZIPC_HIP_ERR_INVALID_ARG;
  ctx->last_size_blocks = 0;
  if (n_streams == 0) return ZIPC_HIP_OK;
  int st = launch_zlib_open(ctx, d_src_arena, d_descs, n_streams, 0);
  if (st) return st;
  st = launch_inflate_size_extent_blocks(ctx, d_src_arena, (const zipc_hip_stream_desc *)ctx->zlib_descs.p, d_results, n_streams, nullptr);
  if (st) return st;
  return launch_zlib_close_extent(ctx, d_src_arena, d_descs, d_results, n_streams, 0);
}

// ... with the long bodies sized by blocks: the same open and close around launch_inflate_size_blocks over the body descriptors
int zipc_hip_zlib_size_blocks_batch(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs,
                                    zipc_hip_stream_result *d_results, size_t n_streams) {
  if (!ctx || !d_descs || !d_results || n_streams > 0x7FFFFFFFull) return ZIPC_HIP_ERR_INVALID_ARG;
  ctx->last_size_blocks = 0;
  if (n_streams == 0) return ZIPC_HIP_OK;
  int st = launch_zlib_open(ctx, d_src_arena, d_descs, n_streams, 0);
  if (st) return st;
  st = launch_inflate_size_blocks(ctx, d_src_arena, (const zipc_hip_stream_desc *)ctx->zlib_descs.p, d_results, n_streams, nullptr);
  if (st) return st;
  return launch_zlib_close_size(ctx, d_results, n_streams);
}

// ---- decode into one arena laid out on the device (packed_layout.h has the rules; packed.hip the two kernels and the sequence) --

int zipc_hip_inflate_packed_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena, size_t dst_arena_len,
                                  const zipc_hip_stream_desc *d_descs, zipc_hip_packed_result *d_results, size_t n_streams,
                                  size_t max_out_len, size_t align, int crc_op, uint64_t *d_need) {
  if (!ctx || !d_descs || !d_results) return ZIPC_HIP_ERR_INVALID_ARG;
  if (const uint32_t st = packed_call_status(d_dst_arena == nullptr, dst_arena_len, n_streams, max_out_len, align, crc_op)) return (int)st;
  if (n_streams == 0) return ZIPC_HIP_OK;
  return launch_inflate_packed(ctx, d_src_arena, d_dst_arena, dst_arena_len, d_descs, d_results, n_streams, max_out_len, align, crc_op,
                               d_need, false);
}

int zipc_hip_zlib_decompress_packed_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena, size_t dst_arena_len,
                                          const zipc_hip_stream_desc *d_descs, zipc_hip_packed_result *d_results, size_t n_streams,
                                          size_t max_out_len, size_t align, uint64_t *d_need) {
  if (!ctx || !d_descs || !d_results) return ZIPC_HIP_ERR_INVALID_ARG;
  if (const uint32_t st = packed_call_status(d_dst_arena == nullptr, dst_arena_len, n_streams, max_out_len, align, zlib_crc_op(ctx))) return (int)st;
  if (n_streams == 0) return ZIPC_HIP_OK;
  return launch_inflate_packed(ctx, d_src_arena, d_dst_arena, dst_arena_len, d_descs, d_results, n_streams, max_out_len, align,
                               zlib_crc_op(ctx), d_need, true);
}

int zipc_hip_zlib_compress_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena, const zipc_hip_stream_desc *d_descs,
                                 zipc_hip_stream_result *d_results, size_t n_streams, size_t max_src_len, size_t total_src_len,
                                 int level) {
  if (!ctx || !d_descs || !d_results || n_streams > 0x7FFFFFFFull || level < 0 || level > 3) return ZIPC_HIP_ERR_INVALID_ARG;
  if (max_src_len > MAX_STREAM_LEN) return ZIPC_HIP_ERR_INVALID_ARG;
  if (n_streams == 0) return ZIPC_HIP_OK;
  int st = launch_zlib_open(ctx, d_src_arena, d_descs, n_streams, 1);
  if (st) return st;
  st = zipc_hip_deflate_batch(ctx, d_src_arena, d_dst_arena, (const zipc_hip_stream_desc *)ctx->zlib_descs.p, d_results, n_streams,
                              max_src_len, total_src_len, level, zlib_crc_op(ctx));
  if (st) return st;
  return launch_zlib_close(ctx, d_dst_arena, d_descs, d_results, n_streams, 1, level);
}

// ---- deflate into one arena laid out on the device (deflate_packed.h has the rules; deflate_packed.hip the four kernels and the sequence) --

size_t zipc_hip_deflate_packed_bound(size_t n_streams, size_t total_src_len, size_t align) {
  return (size_t)dpacked_arena_bound(n_streams, total_src_len, align, false);
}
size_t zipc_hip_zlib_compress_packed_bound(size_t n_streams, size_t total_src_len, size_t align) {
  return (size_t)dpacked_arena_bound(n_streams, total_src_len, align, true);
}

int zipc_hip_deflate_packed_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena, size_t dst_arena_len,
                                  const zipc_hip_stream_desc *d_descs, zipc_hip_packed_result *d_results, size_t n_streams,
                                  size_t max_src_len, size_t total_src_len, int level, int crc_op, size_t align, uint64_t *d_need) {
  if (!ctx || !d_descs || !d_results) return ZIPC_HIP_ERR_INVALID_ARG;
  if (const uint32_t st = dpacked_call_status(d_dst_arena == nullptr, dst_arena_len, n_streams, max_src_len, total_src_len, level, crc_op, align, false))
    return (int)st;
  if (n_streams == 0) return ZIPC_HIP_OK;
  return launch_deflate_packed(ctx, d_src_arena, d_dst_arena, dst_arena_len, d_descs, d_results, n_streams, max_src_len, total_src_len, level,
                               crc_op, align, d_need, false);
}

int zipc_hip_zlib_compress_packed_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena, size_t dst_arena_len,
                                        const zipc_hip_stream_desc *d_descs, zipc_hip_packed_result *d_results, size_t n_streams,
                                        size_t max_src_len, size_t total_src_len, int level, size_t align, uint64_t *d_need) {
  if (!ctx || !d_descs || !d_results) return ZIPC_HIP_ERR_INVALID_ARG;
  if (const uint32_t st = dpacked_call_status(d_dst_arena == nullptr, dst_arena_len, n_streams, max_src_len, total_src_len, level, zlib_crc_op(ctx), align, true))
    return (int)st;
  if (n_streams == 0) return ZIPC_HIP_OK;
  return launch_deflate_packed(ctx, d_src_arena, d_dst_arena, dst_arena_len, d_descs, d_results, n_streams, max_src_len, total_src_len, level,
                               zlib_crc_op(ctx), align, d_need, true);
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

// ---- the gzip container (gzip_container.h has the rules; gzip.hip the three kernels and their launches) ---------------
// Each batch form is the mirrored extent form (or zipc_hip_deflate_batch) between gzip.hip's open and close.

static_assert(sizeof(zipc_hip_gzip_result) == sizeof(GzipResult) && sizeof(GzipResult) == sizeof(zipc_hip_extent_result), "gzip result layout");
static_assert(ZIPC_HIP_GZIP_PLAIN == GZIP_PLAIN && ZIPC_HIP_GZIP_BGZF == GZIP_BGZF, "gzip flavours");

int zipc_hip_gzip_decompress_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena, const zipc_hip_stream_desc *d_descs,
                                   zipc_hip_gzip_result *d_results, size_t n_streams, size_t max_dst_cap) {
  if (!ctx || !d_descs || !d_results || n_streams > 0x7FFFFFFFull) return ZIPC_HIP_ERR_INVALID_ARG;
  ctx->last_inflate_blocks = 0;
  if (n_streams == 0) return ZIPC_HIP_OK;
  int st = launch_gzip_open(ctx, d_src_arena, d_descs, n_streams, 0, 0);
  if (st) return st;
  st = launch_inflate_extent(ctx, d_src_arena, d_dst_arena, (const zipc_hip_stream_desc *)ctx->gzip_descs.p, (zipc_hip_extent_result *)d_results,
                             n_streams, max_dst_cap, ZIPC_HIP_CRC_CRC32);
  if (st) return st;
  return launch_gzip_close_extent(ctx, d_src_arena, d_descs, d_results, n_streams, 1);
}
int zipc_hip_gzip_size_batch(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs, zipc_hip_gzip_result *d_results,
                             size_t n_streams) {
  if (!ctx || !d_descs || !d_results || n_streams > 0x7FFFFFFFull) return ZIPC_HIP_ERR_INVALID_ARG;
  ctx->last_size_blocks = 0;
  if (n_streams == 0) return ZIPC_HIP_OK;
  int st = launch_gzip_open(ctx, d_src_arena, d_descs, n_streams, 0, 0);
  if (st) return st;
  st = launch_inflate_size_extent(ctx, d_src_arena, (const zipc_hip_stream_desc *)ctx->gzip_descs.p, (zipc_hip_extent_result *)d_results, n_streams);
  if (st) return st;
  return launch_gzip_close_extent(ctx, d_src_arena, d_descs, d_results, n_streams, 0);
}
int zipc_hip_gzip_size_blocks_batch(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs,
                                    zipc_hip_gzip_result *d_results, size_t n_streams) {
  if (!ctx || !d_descs || !d_results || n_streams > 0x7FFFFFFFull) return ZIPC_HIP_ERR_INVALID_ARG;
  ctx->last_size_blocks = 0;
  if (n_streams == 0) return ZIPC_HIP_OK;
  int st = launch_gzip_open(ctx, d_src_arena, d_descs, n_streams, 0, 0);
  if (st) return st;
  st = launch_inflate_size_extent_blocks(ctx, d_src_arena, (const zipc_hip_stream_desc *)ctx->gzip_descs.p, (zipc_hip_extent_result *)d_results,
                                         n_streams, nullptr);
  if (st) return st;
  return launch_gzip_close_extent(ctx, d_src_arena, d_descs, d_results, n_streams, 0);
}

size_t zipc_hip_gzip_bound(size_t len, int flavour) {
  return zipc_hip_deflate_bound(len) + (size_t)gzip_overhead(flavour == ZIPC_HIP_GZIP_BGZF ? GZIP_BGZF : GZIP_PLAIN);
}

int zipc_hip_gzip_compress_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena, const zipc_hip_stream_desc *d_descs,
                                 zipc_hip_stream_result *d_results, size_t n_streams, size_t max_src_len, size_t total_src_len, int level,
                                 int flavour) {
  if (!ctx || !d_descs || !d_results || n_streams > 0x7FFFFFFFull || level < 0 || level > 3) return ZIPC_HIP_ERR_INVALID_ARG;
  if (flavour != ZIPC_HIP_GZIP_PLAIN && flavour != ZIPC_HIP_GZIP_BGZF) return ZIPC_HIP_ERR_INVALID_ARG;
  if (max_src_len > MAX_STREAM_LEN) return ZIPC_HIP_ERR_INVALID_ARG;
  if (n_streams == 0) return ZIPC_HIP_OK;
  int st = launch_gzip_open(ctx, d_src_arena, d_descs, n_streams, 1, flavour);
  if (st) return st;
  st = zipc_hip_deflate_batch(ctx, d_src_arena, d_dst_arena, (const zipc_hip_stream_desc *)ctx->gzip_descs.p, d_results, n_streams, max_src_len,
                              total_src_len, level, ZIPC_HIP_CRC_CRC32);
  if (st) return st;
  return launch_gzip_close_compress(ctx, d_dst_arena, d_descs, d_results, n_streams, level, flavour);
}

// One member from host memory: the batch form of one around a copy in and a copy back
int zipc_hip_gzip_compress(zipc_hip_ctx *ctx, const void *src, size_t len, int level, int flavour, void *dst, size_t dst_cap, size_t *out_len) {
  if (!ctx || (!src && len) || (!dst && dst_cap) || !out_len) return ZIPC_HIP_ERR_INVALID_ARG;
  *out_len = 0;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int st = stage_in(ctx, src, len);
  if (st) return st;
  HIP_TRY(ctx, ctx->ensure(ctx->io_dst, dst_cap + 64));
  HIP_TRY(ctx, ctx->ensure(ctx->io_desc, sizeof(StreamDesc)));
  HIP_TRY(ctx, ctx->ensure(ctx->io_res, sizeof(StreamResult)));
  StreamDesc d;
  memset(&d, 0, sizeof d);
  d.src_len = len; d.dst_cap = dst_cap;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->io_desc.p, &d, sizeof d, hipMemcpyHostToDevice, ctx->stream));
  st = zipc_hip_gzip_compress_batch(ctx, ctx->io_src.p, ctx->io_dst.p, (zipc_hip_stream_desc *)ctx->io_desc.p, (zipc_hip_stream_result *)ctx->io_res.p,
                                    1, len, len, level, flavour);
  if (st) return st;
  StreamResult r;
  HIP_TRY(ctx, hipMemcpyAsync(&r, ctx->io_res.p, sizeof r, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (r.status != ST_OK) return (int)r.status;
  if (r.out_len > dst_cap) return ZIPC_HIP_ERR_DST_TOO_SMALL;
  HIP_TRY(ctx, hipMemcpyAsync(dst, ctx->io_dst.p, r.out_len, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *out_len = r.out_len;
  return ZIPC_HIP_OK;
}

// A whole FILE of members from host memory (zipc_hip_gzip_size, zipc_hip_gzip_decompress): staged once and walked with
// gzip_next; the outputs lie end to end in the context's staging room and come back in one copy.
struct GzipWalk {
  zipc_hip_ctx *ctx;
  bool decode;
  const uint8_t *file;
  uint64_t len, dst_cap;
  uint64_t off = 0, total = 0, members = 0;  // where the next member begins, the output so far, the members read
  uint32_t crc_found = 0;                     // of the member that is ZIPC_HIP_ERR_CHECKSUM
  std::vector<StreamDesc> descs;
  std::vector<GzipResult> res;
};

// descs -> the context's descriptor slot; room for n results of 32 bytes
static int gzip_walk_put(GzipWalk &w, size_t n) {
  zipc_hip_ctx *ctx = w.ctx;
  HIP_TRY(ctx, ctx->ensure(ctx->io_desc, n * sizeof(StreamDesc)));
  HIP_TRY(ctx, ctx->ensure(ctx->io_res, n * sizeof(GzipResult)));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->io_desc.p, w.descs.data(), n * sizeof(StreamDesc), hipMemcpyHostToDevice, ctx->stream));
  return ZIPC_HIP_OK;
}
static int gzip_walk_get(GzipWalk &w, void *into, size_t bytes) {
  zipc_hip_ctx *ctx = w.ctx;
  HIP_TRY(ctx, hipMemcpyAsync(into, ctx->io_res.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return ZIPC_HIP_OK;
}

// The run of members of known length that begins at w.off (consecutive BGZF members): ONE batch call, src_len exact, the
// destinations laid out from the ISIZEs.  A member that is not OK reports its status; one whose src_used is not its
// BSIZE + 1, or whose body does not fit the room its own ISIZE promised, is corrupted.
static int gzip_walk_run(GzipWalk &w) {
  zipc_hip_ctx *ctx = w.ctx;
  uint64_t at = w.off, room = w.total, max_cap = 0;
  w.descs.clear();
  for (;;) {
    const GzipStep s = gzip_next(w.file, w.len, at);
    if (s.end_of_members || s.status != ST_OK || !s.known) break;
    StreamDesc d;
    memset(&d, 0, sizeof d);
    d.src_off = at; d.src_len = s.bsize; d.dst_off = room; d.dst_cap = s.isize;
    w.descs.push_back(d);
    at += s.bsize;
    room += s.isize;
    if (s.isize > max_cap) max_cap = s.isize;
  }
  const size_t n = w.descs.size();
  if (n > 0x7FFFFFFFull) return ZIPC_HIP_ERR_INVALID_ARG;
  // (a run that promises more than the caller's room is only sized: a member that lies about itself says so first)
  const bool no_room = w.decode && room > w.dst_cap;
  int st = gzip_walk_put(w, n);
  if (st) return st;
  const zipc_hip_stream_desc *dd = (const zipc_hip_stream_desc *)ctx->io_desc.p;
  zipc_hip_gzip_result *dr = (zipc_hip_gzip_result *)ctx->io_res.p;
  st = w.decode && !no_room ? zipc_hip_gzip_decompress_batch(ctx, ctx->io_src.p, ctx->io_dst.p, dd, dr, n, (size_t)max_cap)
                            : zipc_hip_gzip_size_batch(ctx, ctx->io_src.p, dd, dr, n);
  if (st) return st;
  w.res.resize(n);
  st = gzip_walk_get(w, w.res.data(), n * sizeof(GzipResult));
  if (st) return st;
  for (size_t i = 0; i < n; i++) {
    const GzipResult &r = w.res[i];
    if (r.status == ST_DST_TOO_SMALL) return ZIPC_HIP_ERR_CORRUPTED;
    if (r.status != ST_OK) { w.crc_found = r.checksum; return (int)r.status; }
    if (r.src_used != w.descs[i].src_len) return ZIPC_HIP_ERR_CORRUPTED;
  }
  if (no_room) return ZIPC_HIP_ERR_DST_TOO_SMALL;
  w.off = at; w.total = room; w.members += n;  // (every member OK: out_len is the ISIZE its room was laid out from)
  return ZIPC_HIP_OK;
}

// A member of unknown length at w.off: sized by the size-by-blocks form of one over the rest of the file, decoded by
// zipc_hip_inflate_batch's path over its body with src_len := the extent and CRC-32 (a long member goes by blocks), closed
// here by the same gzip_close.  (The bound is clipped to the longest stream there is: a longer member is not read.)
static int gzip_walk_member(GzipWalk &w) {
  zipc_hip_ctx *ctx = w.ctx;
  StreamDesc d;
  memset(&d, 0, sizeof d);
  d.src_off = w.off;
  d.src_len = w.len - w.off > MAX_STREAM_LEN ? MAX_STREAM_LEN : w.len - w.off;
  w.descs.assign(1, d);
  int st = gzip_walk_put(w, 1);
  if (st) return st;
  st = zipc_hip_gzip_size_blocks_batch(ctx, ctx->io_src.p, (const zipc_hip_stream_desc *)ctx->io_desc.p, (zipc_hip_gzip_result *)ctx->io_res.p, 1);
  if (st) return st;
  GzipResult sized;
  st = gzip_walk_get(w, &sized, sizeof sized);
  if (st) return st;
  if (sized.status != ST_OK) return (int)sized.status;
  if (w.decode) {
    if (w.total + sized.out_len > w.dst_cap) return ZIPC_HIP_ERR_DST_TOO_SMALL;
    const uint64_t u = sized.src_used - sized.hdr_len - 8u;
    StreamDesc body;
    memset(&body, 0, sizeof body);
    body.src_off = gzip_body_off(w.off, sized.hdr_len); body.src_len = u;
    body.dst_off = w.total; body.dst_cap = sized.out_len;
    w.descs.assign(1, body);
    st = gzip_walk_put(w, 1);
    if (st) return st;
    st = launch_inflate(ctx, ctx->io_src.p, ctx->io_dst.p, (const zipc_hip_stream_desc *)ctx->io_desc.p, (zipc_hip_stream_result *)ctx->io_res.p, 1,
                        (size_t)sized.out_len, ZIPC_HIP_CRC_CRC32, &body, true);
    if (st) return st;
    StreamResult sr;
    st = gzip_walk_get(w, &sr, sizeof sr);
    if (st) return st;
    ExtentResult inner;
    inner.status = sr.status; inner.checksum = sr.checksum; inner.out_len = sr.out_len; inner.src_used = u; inner.reserved = 0;
    const GzipResult closed = gzip_close(ST_OK, d.src_len, w.file + w.off, sized.hdr_len, sized.flg, inner, true);
    if (closed.status != ST_OK) { w.crc_found = closed.checksum; return (int)closed.status; }
  }
  w.off += sized.src_used; w.total += sized.out_len; w.members += 1;
  return ZIPC_HIP_OK;
}

static int gzip_file(zipc_hip_ctx *ctx, bool decode, const void *src, size_t len, void *dst, size_t dst_cap, size_t *out_len, size_t *src_used,
                     size_t *n_members, uint32_t *crc_found) {
  if (!ctx || (!src && len) || (decode && !dst && dst_cap) || !out_len || !src_used) return ZIPC_HIP_ERR_INVALID_ARG;
  *out_len = 0;
  *src_used = 0;
  if (n_members) *n_members = 0;
  if (crc_found) *crc_found = 0;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int st = stage_in(ctx, src, len);
  if (st) return st;
  if (decode) HIP_TRY(ctx, ctx->ensure(ctx->io_dst, dst_cap + 64));  // (before anything is in flight: growing it would lose what it holds)
  GzipWalk w;
  w.ctx = ctx; w.decode = decode; w.file = (const uint8_t *)src; w.len = len; w.dst_cap = dst_cap;
  for (;;) {
    const GzipStep step = gzip_next(w.file, w.len, w.off);
    if (step.end_of_members) break;  // (what lies behind the last member is ignored: *src_used says where it begins)
    if (step.status != ST_OK) return (int)step.status;
    st = step.known ? gzip_walk_run(w) : gzip_walk_member(w);
    if (st) {
      if (st == ZIPC_HIP_ERR_CHECKSUM && crc_found) *crc_found = w.crc_found;
      return st;
    }
  }
  if (decode && w.total) {
    HIP_TRY(ctx, hipMemcpyAsync(dst, ctx->io_dst.p, w.total, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  *out_len = (size_t)w.total;
  *src_used = (size_t)w.off;
  if (n_members) *n_members = (size_t)w.members;
  return ZIPC_HIP_OK;
}

int zipc_hip_gzip_size(zipc_hip_ctx *ctx, const void *src, size_t len, size_t *out_len, size_t *src_used, size_t *n_members) {
  return gzip_file(ctx, false, src, len, nullptr, 0, out_len, src_used, n_members, nullptr);
}
int zipc_hip_gzip_decompress(zipc_hip_ctx *ctx, const void *src, size_t len, void *dst, size_t dst_cap, size_t *out_len, size_t *src_used,
                             size_t *n_members, uint32_t *crc_found) {
  return gzip_file(ctx, true, src, len, dst, dst_cap, out_len, src_used, n_members, crc_found);
}

}  // extern "C"
