// ctx.h -- the context behind zipc_hip_ctx (host side, internal).
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/zipc_hip.h"
#include "kernels.h"
#include "recode_rules.h"

struct zipc_hip_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  // The stream ZD_LAUNCH enqueues on: `stream`, or one of `side` while a batch call has its
  // slices in flight (fork()/join() below).
  hipStream_t cur = nullptr;
  // Side streams of the batch forms (two slices by default, ZIPC_HIP_SLICES overrides: forms.h batch_slices
  // has the measurement).  A large batch is cut into slices of consecutive streams and every slice's kernels
  // go to a queue of their own.  Work is still ordered behind everything enqueued on `stream` before
  // the call (fork) and everything enqueued on `stream` after the call is ordered behind the slices (join).
  std::vector<hipStream_t> side;
  std::vector<hipEvent_t> side_done;
  hipEvent_t fork_ev = nullptr;
  bool profiling = false;
  bool xchg_ordered = false;   // deflate.hip xchg_order_probe: one LDS exchange serves lanes on one address in ascending lane order
  bool adler_rfc1950 = false;  // zipc_hip_set_adler_rfc1950: the zlib forms and checksum_device use RFC 1950's Adler-32
  std::string last_error;
  zd::CrcConsts crc_consts;

  // ---- per-kernel timing (HIP events on `stream`)
  struct Pending { int name_idx; hipEvent_t start, stop; };
  struct Acc { std::string name; uint64_t launches = 0; double total_ms = 0; };
  std::vector<Pending> pending;
  std::vector<hipEvent_t> event_pool;
  std::vector<Acc> acc;

  // ---- device scratch, grown on demand, reused across calls
  struct Buf {
    void *p = nullptr;
    size_t cap = 0;
  };
  Buf io_src, io_dst, io_desc, io_res, io_small;  // staging of the host forms
  Buf pin_src, pin_dst, pin_res;                  // pinned host memory of the many-stream host forms
  Buf io_pack_off;                                // ... where each output of a sub-batch begins once they lie end to end (many.hip pack_offsets_kernel)
  hipStream_t copy_in = nullptr, copy_out = nullptr;  // their H2D / D2H queues (made on first use)
  Buf crc_partials, adler_sums;                   // checksum kernels
  Buf crc_nib;                                    // nibble tables of the CRC merge constants (kernels.h)
  Buf ranges_plan;                                // the ragged checksum pass: the call-wide word, every range's bases (kernels.h RangesPlan)
  Buf io_ranges;                                  // ... of host streams: the call's ranges in the source arena
  Buf deflate_scratch;                            // deflate pipeline (deflate.hip)
  Buf parse_scratch;                              // lz_parse by segments: their symbols, paths and verdicts (deflate.hip ParseSegs)
  Buf inflate_scratch;                            // inflate: the span decoder's index, 2304 bytes per stream
  Buf stored_list;                                // inflate of one stream beyond 4 GiB: the stored blocks a walk listed
  Buf blocks_scratch, tok_scratch;                // inflate of streams by a wave per block: candidates, chains; a word per output byte
  Buf descs_marked;                               // ... a call's descriptors with those streams marked as done, for the one waves of the rest
  Buf size_descs, size_head, size_rest;                      // sizing by blocks: the call's descriptors with no destination (dst_off 0, dst_cap the longest stream's), the heads' results and span slots, the one-wave results of the streams left
  Buf zlib_descs, zlib_pre;                       // the zlib batch forms: the descriptors the codec runs with, the container checks' verdicts (zlib.hip)
  Buf gzip_descs, gzip_pre;                       // the gzip batch forms: the descriptors the codec runs with, the headers' verdicts, lengths and FLGs (gzip.hip)
  Buf zlib_hist, dict_adler, io_dict;             // the zlib dictionary forms: the history record of every stream (zlib.hip zlib_open_dict_kernel), the dictionary's Adler-32 (two words: zipc_hip_checksum_device's), the host form's copy of the dictionary
  Buf prefix_adlers;                              // the zlib prefix form: the Adler-32 of every stream that ended within its room (inflate.hip inflate_prefix_kernel)
  Buf extent_inner;                               // the extent decode form with CRC-32: a StreamResult per stream for the checksum pass (inflate.hip launch_inflate_extent)
  Buf recode_descs, recode_res, recode_verdicts;  // the recode forms: the descriptors inflate, then deflate run with, their results, what is known of a stream between the steps (recode.hip)
  Buf packed_descs, packed_res, packed_verdicts;  // the packed decode forms: the descriptors inflate runs with, the sizing pass's results and then inflate's, the layout's verdicts (packed.hip)
  Buf dpacked_staging, dpacked_descs, dpacked_res;  // the packed encode forms: the staging arena of the slots, the descriptors deflate runs with, its results (deflate_packed.hip)
  Buf dpacked_plan, dpacked_verdicts;             // ... the call-wide word, the stage's statuses and the segment bases; the layout's verdicts
  Buf io_mid, io_rdesc, io_rres;                  // ... of host streams: the middle arena of a sub-batch, the call's recode descriptors and results
  Buf pin_rres;                                   // ... the results as they come back (pinned)
  Buf chain_check_links;                          // lz_chain's run-time check: the links the exchange kernel made of a batch's first streams
  unsigned long long *chain_check_host = nullptr; // ... [0] differences, [1] positions compared in the context's first batch; [2], [3]: the same for the create-time probe (device-visible host memory)
  bool chain_checked = false;                     // ... that first batch has been seen
  uint32_t last_inflate_blocks = 0;               // blocks of the last one-stream inflate that went that way (0: it did not)
  uint32_t last_size_blocks = 0;                  // blocks of the chains (and heads) that sized streams of the last sizing call by blocks (0: every stream by its one wave)

  int name_index(const char *name);
  hipEvent_t get_event();
  void begin(const char *name, hipEvent_t &start);
  void end(const char *name, hipEvent_t start);
  hipError_t ensure(Buf &b, size_t bytes);
  hipError_t ensure_pinned(Buf &b, size_t bytes);
  hipError_t collect_times();
  // side streams [0, k) wait for what `stream` holds now / `stream` waits for side streams [0, k)
  // (join also points `cur` back at `stream`; every fork is followed by a join on every path)
  hipError_t fork(size_t k);
  hipError_t join(size_t k);
  // slice i of a batch call goes to: `stream` for i = 0, side[i] above
  void use_slice_stream(size_t i) { cur = i == 0 ? stream : side[i]; }
};

// Launch `kernel<<<grid, block, lds, ctx->stream>>>(args...)`, bracketed by HIP
// events on the same stream when profiling is on.
#define ZD_LAUNCH(ctx, name, kernel, grid, block, lds, ...)                       \
  do {                                                                            \
    hipEvent_t _zd_start = nullptr;                                               \
    if ((ctx)->profiling) (ctx)->begin(name, _zd_start);                          \
    hipLaunchKernelGGL(kernel, grid, block, lds, (ctx)->cur, __VA_ARGS__);        \
    if ((ctx)->profiling) (ctx)->end(name, _zd_start);                            \
  } while (0)

// a HIP call of a function that returns a ZIPC_HIP_* status: a failure is written down and ends it
#define HIP_TRY(ctx, expr)                                                             \
  do {                                                                                 \
    hipError_t _e = (expr);                                                            \
    if (_e != hipSuccess) {                                                            \
      (ctx)->last_error = std::string(#expr) + ": " + hipGetErrorString(_e);           \
      return ZIPC_HIP_ERR_HIP;                                                         \
    }                                                                                  \
  } while (0)

namespace zd {
// api.hip: a buffer of the context's scratch goes back to the device (the stream must be idle)
void free_buf(zipc_hip_ctx::Buf &b);
// api.hip: zipc_hip_debug_set_slices' number of slices for forms.h batch_slices (0: none set)
long debug_slices_override();
// api.hip: the two halves of the CRC-32 pass over n_ranges ranges of up to max_len bytes, on ctx->cur.
// partials: n_ranges * crc32_segs(max_len) words.
size_t crc32_segs(size_t max_len);
hipError_t crc32_segments_launch(zipc_hip_ctx *ctx, const uint8_t *base, int mode, const StreamDesc *d_descs,
                                 const StreamResult *d_results, size_t n_ranges, uint64_t single_off,
                                 uint64_t single_len, size_t max_len, uint32_t *partials);
hipError_t crc32_finish_launch(zipc_hip_ctx *ctx, int mode, const StreamDesc *d_descs, StreamResult *d_results,
                               size_t n_ranges, uint64_t single_len, size_t max_len, const uint32_t *partials,
                               uint32_t *d_single_out);
// ... and the whole pass (a ZIPC_HIP_* status); partials: the context's buffer from word `partials_at` on, grown here unless `ensured`
int crc32_pass(zipc_hip_ctx *ctx, const uint8_t *base, int mode, const StreamDesc *d_descs, StreamResult *d_results,
               size_t n_ranges, uint64_t single_off, uint64_t single_len, size_t max_len, uint32_t *d_single_out,
               size_t partials_at = 0, bool ensured = false);
// api.hip: the scratch zipc_hip_checksum_batch takes for n_ranges ranges of total_len bytes, for a caller that wants it
// grown before anything is in flight (a ZIPC_HIP_* status)
int checksum_ranges_reserve(zipc_hip_ctx *ctx, size_t n_ranges, size_t total_len, int want_adler32);
// deflate.hip: the probe behind ctx->xchg_ordered
bool xchg_order_probe(zipc_hip_ctx *ctx);
// deflate.hip (tests): the links one of the two chain kernels makes of a batch, and how many link slots that takes
hipError_t debug_chain_links(zipc_hip_ctx *ctx, const uint8_t *d_src, const StreamDesc *d_descs, size_t n, size_t max_src_len,
                             size_t total_src_len, int which, uint16_t *d_links, size_t links_cap, uint64_t *d_pos_base);
size_t debug_chain_positions(size_t n, size_t total_src_len);
// deflate.hip (tests): the links any of the four chain forms (forms.h ChainKernel) makes of a batch, through the pipeline's
// own launch_lz_chain, over links filled with `fill`; seg_positions: 0 for the shape's own, else one the forms can produce
hipError_t debug_chain_links_form(zipc_hip_ctx *ctx, const uint8_t *d_src, const StreamDesc *d_descs, size_t n, size_t max_src_len,
                                  size_t total_src_len, int chain, size_t seg_positions, uint16_t fill, uint16_t *d_links,
                                  size_t links_cap, uint64_t *d_pos_base);
// deflate.hip (tests): lz_match's tables of a batch after deflate_offsets, lz_chain_kernel and lz_match alone, the latter
// launched as the pipeline launches it under that match_form and tiles_per_group
hipError_t debug_match_records(zipc_hip_ctx *ctx, const uint8_t *d_src, const StreamDesc *d_descs, size_t n, size_t max_src_len,
                               size_t total_src_len, int level, int match_form, long tiles_per_group, uint32_t *d_match,
                               uint32_t *d_snap, size_t records_cap, uint32_t *d_snap_used, uint64_t *d_pos_base);
// deflate.hip: the pipeline itself (the scratch it needs: deflate_scratch.h deflate_scratch_bytes)
hipError_t launch_deflate(zipc_hip_ctx *ctx, const uint8_t *d_src, uint8_t *d_dst,
                          const StreamDesc *d_descs, StreamResult *d_results, size_t n_streams,
                          size_t max_src_len, size_t total_src_len, int level, int crc_op);
// inflate.hip: zipc_hip_inflate_batch behind its argument checks (a ZIPC_HIP_* status).  h_descs: the caller's own host copy
// of the descriptors, or null: the block path reads them back; first_of_call: zipc_hip_last_inflate_blocks counts from zero
// (the many-stream host forms' sub-batches add up).  dbg: zipc_hip_debug_inflate_tokens' wishes (tests), null for every other
// caller: the token form (-1: blocks_follow's rule) and the hops of the first / a later resolve round (0: the tuning's), where
// the tokens go, the records (host memory, one per stream, zeroed by the caller) -- and every stream that fits goes by blocks
struct BlocksDebug {
  int form, hops0, hops1;
  uint32_t *d_tok_raw, *d_tok_done;
  zipc_hip_debug_token_record *records;
};
int launch_inflate(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena, const zipc_hip_stream_desc *d_descs,
                   zipc_hip_stream_result *d_results, size_t n_streams, size_t max_dst_cap, int crc_op, const StreamDesc *h_descs,
                   bool first_of_call, const BlocksDebug *dbg = nullptr);
// inflate.hip: zipc_hip_inflate_size_batch behind its argument checks (a ZIPC_HIP_* status): inflate_size_kernel, a wave per
// stream, one launch on ctx->cur
int launch_inflate_size(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs, zipc_hip_stream_result *d_results,
                        size_t n_streams);
// inflate.hip: zipc_hip_inflate_prefix_batch behind its argument checks (a ZIPC_HIP_* status): inflate_prefix_kernel, a wave
// per stream whatever its room, one launch on ctx->cur; crc_op: ZIPC_HIP_CRC_NOP, or zlib_crc_op's with d_adlers a word per
// stream for the Adler-32 of those that ended (the zlib form)
int launch_inflate_prefix(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena, const zipc_hip_stream_desc *d_descs,
                          zipc_hip_prefix_result *d_results, size_t n_streams, int crc_op, uint32_t *d_adlers);
// inflate.hip: the history forms behind their argument checks (a ZIPC_HIP_* status each; inflate_history.h has the rule):
// inflate_history_kernel / inflate_prefix_history_kernel / inflate_size_history_kernel, a wave per stream whatever its room,
// one launch on ctx->cur, nothing read back; d_hist: null (no stream has history), or a record per stream.
// launch_inflate_history with ZIPC_HIP_CRC_CRC32: the checksum pass behind it, over d_descs' rooms.
int launch_inflate_history(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena, const zipc_hip_stream_desc *d_descs,
                           const zipc_hip_history *d_hist, zipc_hip_stream_result *d_results, size_t n_streams, size_t max_dst_cap,
                           int crc_op);
int launch_inflate_prefix_history(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena, const zipc_hip_stream_desc *d_descs,
                                  const zipc_hip_history *d_hist, zipc_hip_prefix_result *d_results, size_t n_streams);
int launch_inflate_size_history(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs, const zipc_hip_history *d_hist,
                                zipc_hip_stream_result *d_results, size_t n_streams);
// inflate.hip: the extent forms behind their argument checks (a ZIPC_HIP_* status each; inflate_extent.h has the rule).
// launch_inflate_extent: inflate_extent_kernel, a wave per stream whatever max_dst_cap, one launch on ctx->cur, and for
// ZIPC_HIP_CRC_CRC32 the checksum pass behind it; launch_inflate_size_extent: inflate_size_extent_kernel, one launch;
// launch_inflate_size_extent_blocks: launch_inflate_size_blocks' path, decision for decision, with the extent forms of the
// verdict and of the one wave -- it synchronises where that one does.
int launch_inflate_extent(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena, const zipc_hip_stream_desc *d_descs,
                          zipc_hip_extent_result *d_results, size_t n_streams, size_t max_dst_cap, int crc_op);
int launch_inflate_size_extent(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs,
                               zipc_hip_extent_result *d_results, size_t n_streams);
int launch_inflate_size_extent_blocks(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs,
                                      zipc_hip_extent_result *d_results, size_t n_streams, const StreamDesc *h_descs);
// inflate.hip: zipc_hip_inflate_size_blocks_batch behind its argument checks: the call's long streams (forms.h size_blocks_pick)
// by the block path's first half and a head walk, the rest by inflate_size_kernel's wave; h_descs: the caller's host copy of
// the descriptors, or null: they are read back.  Synchronises ctx->stream unless no stream of the call is long.
int launch_inflate_size_blocks(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs, zipc_hip_stream_result *d_results,
                               size_t n_streams, const StreamDesc *h_descs);
// recode.hip: zipc_hip_recode_batch behind its argument checks, and the kernels' step of zipc_hip_recode_many (a ZIPC_HIP_*
// status): open -> inflate with its CRC-32 pass -> link -> deflate -> close on ctx->stream.  d_plain: null, or n StreamResults
// for the many-stream pipeline; h_inflate_descs, first_of_call: launch_inflate's.  recode_reserve: its scratch for n streams,
// for a caller that wants it grown before anything is in flight
int recode_reserve(zipc_hip_ctx *ctx, size_t n);
int launch_recode(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_mid_arena, void *d_dst_arena, const RecodeDesc *d_descs,
                  RecodeResult *d_results, StreamResult *d_plain, size_t n, size_t max_mid_cap, size_t total_mid_cap, int level,
                  const StreamDesc *h_inflate_descs, bool first_of_call);
// packed.hip: zipc_hip_inflate_packed_batch / zipc_hip_zlib_decompress_packed_batch behind their argument checks (a ZIPC_HIP_*
// status): (zlib: open ->) the sizing pass packed_layout.h names -> layout -> inflate -> close on ctx->stream; crc_op: the
// caller's, or zlib_crc_op's.  packed_reserve: its scratch for n streams, for a caller that wants it grown before anything
// is in flight
int packed_reserve(zipc_hip_ctx *ctx, size_t n);
int launch_inflate_packed(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena, size_t dst_arena_len,
                          const zipc_hip_stream_desc *d_descs, zipc_hip_packed_result *d_results, size_t n, size_t max_out_len,
                          size_t align, int crc_op, uint64_t *d_need, bool zlib);
// deflate_packed.hip: zipc_hip_deflate_packed_batch / zipc_hip_zlib_compress_packed_batch behind their argument checks (a
// ZIPC_HIP_* status): stage -> (zlib: open ->) deflate (-> zlib close) -> layout -> copy -> close on ctx->stream; crc_op: the
// caller's, or zlib_crc_op's.  dpacked_reserve: its scratch beside deflate's own for n streams of total_src_len bytes, for
// a caller that wants it grown before anything is in flight
int dpacked_reserve(zipc_hip_ctx *ctx, size_t n, size_t total_src_len, bool zlib);
int launch_deflate_packed(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena, size_t dst_arena_len,
                          const zipc_hip_stream_desc *d_descs, zipc_hip_packed_result *d_results, size_t n, size_t max_src_len,
                          size_t total_src_len, int level, int crc_op, size_t align, uint64_t *d_need, bool zlib);
// zlib.hip: the checksum the zlib forms of this context ask the codec for, and the container's kernels around the codec's
// (a ZIPC_HIP_* status each): open leaves the codec's descriptors in ctx->zlib_descs and the checks' verdicts in ctx->zlib_pre
int zlib_crc_op(const zipc_hip_ctx *ctx);
int launch_zlib_open(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs, size_t n, int compress);
int launch_zlib_close(zipc_hip_ctx *ctx, void *d_dst_arena, const zipc_hip_stream_desc *d_descs, zipc_hip_stream_result *d_results,
                      size_t n, int compress, int level);
int launch_zlib_close_size(zipc_hip_ctx *ctx, zipc_hip_stream_result *d_results, size_t n);
int launch_zlib_close_prefix(zipc_hip_ctx *ctx, zipc_hip_prefix_result *d_results, size_t n);  // (the Adler-32s: ctx->prefix_adlers)
// ... of the dictionary forms (zlib_container.h zlib_open_dict): the open also leaves a history record per stream in
// ctx->zlib_hist (d_dict_adler: a device word, RFC 1950's Adler-32 of the dictionary; not read when dict_len is 0); the seed
// copies the dictionary in front of the room of every stream opened with FDICT; size 1: the sizing form's close
int launch_zlib_open_dict(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs, size_t n, size_t dict_len,
                          const uint32_t *d_dict_adler);
int launch_zlib_seed_dict(zipc_hip_ctx *ctx, void *d_dst_arena, const zipc_hip_stream_desc *d_descs, size_t n, const void *d_dict, size_t dict_len);
int launch_zlib_close_dict(zipc_hip_ctx *ctx, zipc_hip_stream_result *d_results, size_t n, int size);
// ... of the extent forms: d_descs the caller's (the trailer is read at 2 + the body's extent); compare 0: the sizing form's
int launch_zlib_close_extent(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs,
                             zipc_hip_extent_result *d_results, size_t n, int compare);
// gzip.hip: the gzip container's kernels around the codec's (a ZIPC_HIP_* status each): open leaves the codec's descriptors in
// ctx->gzip_descs and the headers' verdicts in ctx->gzip_pre (compress: the room behind the header to be; flavour: ZIPC_HIP_GZIP_*);
// the extent close reads the trailer behind the body's extent (d_descs the caller's; compare_crc 0: the sizing forms')
int launch_gzip_open(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs, size_t n, int compress, int flavour);
int launch_gzip_close_extent(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs, zipc_hip_gzip_result *d_results,
                             size_t n, int compare_crc);
int launch_gzip_close_compress(zipc_hip_ctx *ctx, void *d_dst_arena, const zipc_hip_stream_desc *d_descs, zipc_hip_stream_result *d_results,
                               size_t n, int level, int flavour);
// many.hip: the staging threads' pools, shared by the process's contexts (zipc_hip_create / zipc_hip_destroy)
void many_pools_acquire();
void many_pools_release();
}  // namespace zd
