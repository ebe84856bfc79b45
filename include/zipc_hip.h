/* zipc_hip.h -- C ABI of the MI355X-native Zipc_deflate hot path.
 *
 * This is the drop-in boundary for the reference's src/zipc_deflate.ml: every
 * entry point below replaces one value of the reference's module signature
 * src/zipc_deflate.mli (cited per function).  The reference has no FFI of its
 * own -- the seam is that OCaml signature -- so an OCaml shim
 * (bindings/ocaml/, shown in INTEGRATION.md) marshals strings to these calls,
 * applies ?start as a pointer offset, supplies the reference's default level
 * (`Best, zipc_deflate.ml:817) and maps status codes to the reference's error
 * strings (zipc_hip_strerror).
 *
 * Plain C: pointers and sizes only, no C++/torch types.  Status codes, never
 * exceptions.  The library never frees or retains caller memory.
 *
 * Two families:
 *   - host forms   (zipc_hip_crc32 ... zipc_hip_zlib_decompress): host
 *     pointers in, host buffers out; one stream = a batch of one.  They copy
 *     H2D/D2H around the same kernels as the batch forms.
 *   - batch forms  (zipc_hip_*_batch, zipc_hip_checksum_device): descriptors
 *     over DEVICE-resident arenas; nothing crosses PCIe.  These are what
 *     bench.py times.
 *
 * All compute happens in HIP kernels on gfx950.  There is no CPU fallback: with
 * no usable device every call returns ZIPC_HIP_ERR_NO_DEVICE / _HIP.
 */
#ifndef ZIPC_HIP_H
#define ZIPC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZIPC_HIP_ABI_VERSION 1

/* Longest single stream, and largest destination capacity, in bytes: 4 GiB - 64 KiB (positions are
 * 32-bit inside the kernels).  The reference's own limit is OCaml's string length.
 * One exception, for inflate: a batch of ONE stream that begins with stored blocks -- what the
 * reference's encoder makes of incompressible data -- may be of any size (zipc_hip_inflate_batch with
 * max_dst_cap above this limit; checksum none or CRC-32): stored blocks of any lengths are copied with
 * 64-bit offsets (a run of equal blocks all at once, others by a walk over their headers), with the
 * reference's messages for a damaged header and for a block beyond ?decompressed_size; the first block
 * of another kind and what follows it has to fit the limit as a stream of its own. */
#define ZIPC_HIP_MAX_STREAM_LEN 0xFFFF0000ull

/* ---- status codes --------------------------------------------------------
 * 1..6 are the reference's Failure messages (zipc_deflate.ml:233,29,728-730,104) */
enum {
  ZIPC_HIP_OK = 0,
  ZIPC_HIP_ERR_CORRUPTED = 1,     /* "Corrupted data stream" */
  ZIPC_HIP_ERR_SIZE_EXCEEDED = 2, /* "Expected decompression size exceeded" */
  ZIPC_HIP_ERR_ZLIB_METHOD = 3,   /* "Unknown compression method (%d)" */
  ZIPC_HIP_ERR_ZLIB_WINDOW = 4,   /* "Window size too large" */
  ZIPC_HIP_ERR_ZLIB_DICT = 5,     /* "Preset dictionary unsupported" */
  ZIPC_HIP_ERR_CHECKSUM = 6,      /* "Checksum mismatch, expected %lx found %lx)" */
  /* boundary-only conditions (no reference counterpart) */
  ZIPC_HIP_ERR_DST_TOO_SMALL = 16, /* dst_cap too small and no decompressed_size
                                      limit was given: retry with a larger dst */
  ZIPC_HIP_ERR_HIP = 17,           /* a HIP runtime call failed */
  ZIPC_HIP_ERR_INVALID_ARG = 18,
  ZIPC_HIP_ERR_NO_DEVICE = 19,
  ZIPC_HIP_ERR_NOMEM = 20
};

/* crc_op (zipc_deflate.ml:210): which checksum the reference updates once per deflate block inside
 * inflate (over the output) / deflate (over the input).  Here Adler-32 is computed inside the codec
 * kernels block by block (its value depends on that chunking, see below); CRC-32, whose value does
 * not, is a separate pass of the checksum kernels over the same bytes once the codec kernel is done
 * (one more read of them; the result is the same word for word). */
enum {
  ZIPC_HIP_CRC_NOP = 0,
  ZIPC_HIP_CRC_CRC32 = 1,
  ZIPC_HIP_CRC_ADLER32 = 2,         /* Zipc_deflate.Adler_32 as the reference computes it (below) */
  ZIPC_HIP_CRC_ADLER32_RFC1950 = 3  /* RFC 1950's Adler-32: what zlib and everybody else computes */
};
/* The reference's Adler-32 takes a SIGNED 32-bit remainder after every 5552-byte chunk
 * (src/zipc_deflate.ml:95,196) and restarts its chunking at every deflate block (:688,1084): on
 * data whose running sum crosses 2^31 -- bytes above 0x7F in bulk: 6 KB of random bytes do -- its
 * value differs from RFC 1950's, and depends on how the bytes were cut into calls.  A drop-in has
 * to reproduce that (ZIPC_HIP_CRC_ADLER32, the default everywhere): zlib_compress then writes
 * trailers standard zlib REJECTS for such data, and zlib_decompress reports a checksum mismatch on
 * valid RFC 1950 streams of such data, exactly as the reference does.  Where interoperation with
 * zlib matters more than equality with the reference, ask for RFC 1950's value instead: crc_op
 * ZIPC_HIP_CRC_ADLER32_RFC1950 in the inflate / deflate forms, zipc_hip_set_adler_rfc1950() for the
 * zlib forms and zipc_hip_checksum_device of a context. */

/* type level (zipc_deflate.mli:123-125) */
enum {
  ZIPC_HIP_LEVEL_NONE = 0,
  ZIPC_HIP_LEVEL_FAST = 1,
  ZIPC_HIP_LEVEL_DEFAULT = 2,
  ZIPC_HIP_LEVEL_BEST = 3
};

/* ---- context ---------------------------------------------------------------
 * Owns a HIP stream, constant tables and device scratch (grown on demand and
 * reused).  One context per host thread; contexts are independent (the
 * reference is re-entrant with no shared state). */
typedef struct zipc_hip_ctx zipc_hip_ctx;

int zipc_hip_abi_version(void);
int zipc_hip_device_count(void);
int zipc_hip_create(zipc_hip_ctx **ctx, int device);
void zipc_hip_destroy(zipc_hip_ctx *ctx);
/* the hipStream_t all of this context's work is enqueued on */
void *zipc_hip_stream(zipc_hip_ctx *ctx);
int zipc_hip_synchronize(zipc_hip_ctx *ctx);
/* text of the last HIP runtime error seen by this context ("" if none) */
const char *zipc_hip_last_error(zipc_hip_ctx *ctx);
/* how the last inflate of ONE stream ran: the number of blocks it was decoded by, a wave per block (inflate.hip),
 * or 0 when the stream's one wave decoded it (short streams, streams that are not a chain of dynamic blocks,
 * anything that reports an error).  For tests and measurements; the results are the same either way. */
unsigned zipc_hip_last_inflate_blocks(zipc_hip_ctx *ctx);
/* the same for sizing: the blocks of the chains that the last sizing call (zipc_hip_inflate_size, any _size_batch form)
 * sized streams by, a wave per block, or 0 when every stream of it was sized by its one wave.  zipc_hip_last_inflate_blocks
 * is not touched by a sizing call.  For tests and measurements; the results are the same either way. */
unsigned zipc_hip_last_size_blocks(zipc_hip_ctx *ctx);
/* the source length from which one stream goes by a wave per block, to be decoded (given the room) or sized */
#define ZIPC_HIP_BLOCKS_MIN_SRC ((size_t)40 << 10)
/* 1 when this context builds hash chains by ordered LDS exchange (deflate.hip lz_chain_xchg_kernel): the probe run
 * by zipc_hip_create found that one LDS exchange instruction serves the lanes that hit one address in ascending lane
 * order, which is the order insert_hash (zipc_deflate.ml:1150-1152) inserts positions in.  0: the probe failed and the
 * context keeps the kernel that orders them itself (same links either way).  For tests and measurements. */
int zipc_hip_lds_exchange_ordered(zipc_hip_ctx *ctx);
/* What the guards of that property have seen so far (round 6): positions whose links BOTH chain kernels made and were
 * compared -- the create-time probe runs lz_chain_xchg_kernel itself, whole and by segments, on a stream made of runs,
 * short periods and few-symbol alphabets; the context's first deflate batch has its first 32 streams (at most
 * 16 MiB) chained by both kernels under that batch's load -- and how many differed.  A difference in
 * the first batch fails that batch's streams with ZIPC_HIP_ERR_HIP and moves the context to the ordering kernel.
 * Synchronises the context's stream. */
int zipc_hip_chain_check(zipc_hip_ctx *ctx, unsigned long long *compared, unsigned long long *differences);
/* Measurements only: the number of slices the batch forms cut a call into (side queues, forms.h batch_slices), for
 * every context of the process from now on; 0 = the default again (two slices of at least 2048 streams, or
 * ZIPC_HIP_SLICES).  bench.py times a kernel alone on the device with 1.  Results are the same for every value. */
void zipc_hip_debug_set_slices(long k);
/* the reference's message for a status (format strings kept verbatim) */
const char *zipc_hip_strerror(int status);

/* ---- per-kernel timing -----------------------------------------------------
 * With profiling on, every kernel launch is bracketed by HIP events on the
 * context stream; zipc_hip_kernel_times reports, per kernel name, launches and
 * total milliseconds since the last reset.  bench.py uses this for the
 * roofline's live per-launch duration. */
typedef struct {
  char name[48];
  uint64_t launches;
  double total_ms;
} zipc_hip_kernel_time;
int zipc_hip_set_profiling(zipc_hip_ctx *ctx, int enabled);
/* enabled != 0: the zlib forms (single, _many and _batch) and zipc_hip_checksum_device's Adler-32 of this
 * context follow RFC 1950 (see ZIPC_HIP_CRC_ADLER32_RFC1950); 0 (the default): the reference's. */
int zipc_hip_set_adler_rfc1950(zipc_hip_ctx *ctx, int enabled);
int zipc_hip_reset_kernel_times(zipc_hip_ctx *ctx);
int zipc_hip_kernel_times(zipc_hip_ctx *ctx, zipc_hip_kernel_time *out, size_t cap,
                          size_t *n);

/* ---- host forms ------------------------------------------------------------ */

/* Crc_32.string  (zipc_deflate.mli:46; zipc_deflate.ml:161) */
int zipc_hip_crc32(zipc_hip_ctx *ctx, const void *src, size_t len, uint32_t *crc);
/* Adler_32.string (zipc_deflate.mli:72; zipc_deflate.ml:203), signed-remainder
 * behaviour of zipc_deflate.ml:95,196 included */
int zipc_hip_adler32(zipc_hip_ctx *ctx, const void *src, size_t len, uint32_t *adler);

/* inflate / inflate_and_crc_32 / inflate_and_adler_32
 * (zipc_deflate.mli:79-102; zipc_deflate.ml:692-718).
 * has_limit != 0  <=>  ?decompressed_size = limit.  dst_cap >= limit required
 * then.  With has_limit == 0 the reference grows its buffer without bound; here
 * ZIPC_HIP_ERR_DST_TOO_SMALL asks the caller to retry with a larger dst. */
int zipc_hip_inflate(zipc_hip_ctx *ctx, const void *src, size_t len, int has_limit,
                     size_t limit, int crc_op, void *dst, size_t dst_cap,
                     size_t *out_len, uint32_t *checksum);
/* What one host stream inflates to, with nothing inflated: zipc_hip_inflate_size_blocks_batch (below) of a batch of one,
 * around a copy of the stream to the device and 16 bytes back.  Returns the stream's status -- what zipc_hip_inflate
 * (ZIPC_HIP_CRC_NOP) returns for the same src, len, has_limit and limit into a dst of ZIPC_HIP_MAX_STREAM_LEN bytes --
 * and on ZIPC_HIP_OK its decompressed length in *out_len (0 otherwise): the dst_cap that call needs.  A stream of 40 KiB
 * and more is sized by a wave per block -- the first half of the launches zipc_hip_inflate decodes it by, and less than
 * that decode costs -- a shorter one, and any stream the block path does not show to be ZIPC_HIP_OK, by its one wave:
 * the results are the same either way (zipc_hip_last_size_blocks tells which it was). */
int zipc_hip_inflate_size(zipc_hip_ctx *ctx, const void *src, size_t len, int has_limit,
                          size_t limit, size_t *out_len);

/* zlib_decompress (zipc_deflate.mli:104-118; zipc_deflate.ml:720-740).  On
 * ZIPC_HIP_ERR_CHECKSUM, *expect and *found hold the two Adler-32 values. */
int zipc_hip_zlib_decompress(zipc_hip_ctx *ctx, const void *src, size_t len,
                             int has_limit, size_t limit, void *dst, size_t dst_cap,
                             size_t *out_len, uint32_t *adler, uint32_t *expect,
                             uint32_t *found);

/* upper bound of the deflate output for len input bytes, any level */
size_t zipc_hip_deflate_bound(size_t len);
size_t zipc_hip_zlib_bound(size_t len);

/* deflate / crc_32_and_deflate / adler_32_and_deflate
 * (zipc_deflate.mli:128-150; zipc_deflate.ml:1247-1260).  level is explicit
 * here; the shim passes ZIPC_HIP_LEVEL_BEST when ?level is absent, which is
 * what the reference does (zipc_deflate.ml:817).  dst_cap: the rule stated at
 * zipc_hip_deflate_batch decides whether the stream fits (it is not "the output
 * fits"; zipc_hip_deflate_bound(len) always does); ZIPC_HIP_ERR_DST_TOO_SMALL
 * leaves *out_len = 0, *checksum = 0 and dst as it was. */
int zipc_hip_deflate(zipc_hip_ctx *ctx, const void *src, size_t len, int level,
                     int crc_op, void *dst, size_t dst_cap, size_t *out_len,
                     uint32_t *checksum);

/* zlib_compress (zipc_deflate.mli:152-162; zipc_deflate.ml:1262-1277) */
int zipc_hip_zlib_compress(zipc_hip_ctx *ctx, const void *src, size_t len, int level,
                           void *dst, size_t dst_cap, size_t *out_len,
                           uint32_t *adler);

/* Many independent streams held in HOST memory through the batch kernels in one
 * go: stream i is src[i][0 .. src_len[i]) -> dst[i] (capacity dst_cap[i]);
 * results[i] (host memory, declared below) gets its status, length and checksum.
 * This is what a caller that handles the members of an archive together uses
 * instead of n calls of the single-stream forms -- Zipc.File.deflate_of_binary_string
 * / to_binary_string over all members (src/zipc.ml:180-186,208-231).  limit may
 * be NULL (no ?decompressed_size for any stream); a stream whose output does not
 * fit (to deflate: by the dst_cap rule stated at zipc_hip_deflate_batch) reports
 * ZIPC_HIP_ERR_DST_TOO_SMALL (or the reference's size message when a
 * limit is given) in its own result.  The call itself fails only for bad
 * arguments or HIP errors.
 * Staging: the call runs as a pipeline of a few sub-batches.  Each is gathered into
 * pinned memory the context keeps (sized to the batch; the first call of a size pays
 * for pinning it) by a few host threads the library keeps, copied to the device as
 * it is gathered, run, brought back -- the outputs end to end, by a kernel that
 * writes the pinned memory -- and scattered to the caller's buffers by a second
 * thread, so bus copies and kernels of one sub-batch run under the host memcpys of
 * the others.  A call that FAILS (bad arguments, a HIP error, no memory or thread on the host) may have filled some of
 * the caller's buffers, and results[] is defined all the same: the streams of sub-batches that had come back keep their
 * results, every other stream carries the call's status and out_len 0; zipc_hip_last_error says what happened.  No C++
 * exception crosses this boundary.  The staging threads are shared by the process's contexts and joined when the last
 * context is destroyed; a forked child makes its own (csrc/host_pipeline.h, which tests/test_sanitizers.py runs under
 * the thread and address sanitizers with host threads standing in for the device).
 * Environment, read once per process: ZIPC_HIP_HOST_THREADS (default 8 or the core
 * count), ZIPC_HIP_HOST_CHUNKS (sub-batches, default 4, 6 from a GiB of staging on;
 * fewer when a sub-batch would hold under 1024 streams), ZIPC_HIP_HOST_TIMING=1
 * (where each sub-batch was when, on stderr); csrc/tuning.h has the rest. */
struct zipc_hip_stream_result_s;
int zipc_hip_deflate_many(zipc_hip_ctx *ctx, size_t n, const void *const *src, const size_t *src_len,
                          int level, int crc_op, void *const *dst, const size_t *dst_cap,
                          struct zipc_hip_stream_result_s *results);
int zipc_hip_inflate_many(zipc_hip_ctx *ctx, size_t n, const void *const *src, const size_t *src_len,
                          const size_t *limit, int crc_op, void *const *dst, const size_t *dst_cap,
                          struct zipc_hip_stream_result_s *results);
/* The same decode with nothing brought back but the results: every stream is inflated into the context's device arena
 * (dst_cap[i] bytes of room each), its checksum taken there, and results[i] = {status, checksum, out_len}.  What a caller
 * that TESTS an archive needs -- File.to_binary_string of every member for its Ok / Error alone, the reference's
 * `zipc unzip -t` (test/zipc_tool.ml:635-660 check_archive) -- without the decompressed bytes crossing the bus. */
int zipc_hip_inflate_many_check(zipc_hip_ctx *ctx, size_t n, const void *const *src, const size_t *src_len,
                                const size_t *limit, int crc_op, const size_t *dst_cap,
                                struct zipc_hip_stream_result_s *results);

/* The zlib container around many host streams: zlib_decompress / zlib_compress (zipc_deflate.ml:720-740, 1262-1277,
 * start = 0) of every stream in one go, through the same pipeline as zipc_hip_inflate_many / _deflate_many.  The six
 * container bytes of a stream are read and written on the host (csrc/zlib_container.h: the reference's checks in its
 * order, the body range [2, len-2), the big-endian Adler-32); the bodies go through the kernels with the context's
 * Adler-32 flavour (zipc_hip_set_adler_rfc1950).  results[i]: ZIPC_HIP_OK, the checksum and the length -- to compress,
 * of the whole zlib stream in dst[i] -- or the stream's own error: the reference's header messages,
 * ZIPC_HIP_ERR_CHECKSUM with checksum = the Adler-32 FOUND and out_len 0 (the expected one is the stream's last four
 * bytes, big-endian), inflate's statuses, ZIPC_HIP_ERR_DST_TOO_SMALL for a dst_cap under 6 or under what the stream
 * takes (zipc_hip_zlib_bound).  A stream that fails its header check never reaches the device and leaves dst[i] as it
 * was.  results[] is defined on every return, bad arguments included (every entry then carries the call's status), and
 * no C++ exception crosses the boundary. */
int zipc_hip_zlib_decompress_many(zipc_hip_ctx *ctx, size_t n, const void *const *src, const size_t *src_len,
                                  const size_t *limit, void *const *dst, const size_t *dst_cap,
                                  struct zipc_hip_stream_result_s *results);
int zipc_hip_zlib_compress_many(zipc_hip_ctx *ctx, size_t n, const void *const *src, const size_t *src_len, int level,
                                void *const *dst, const size_t *dst_cap, struct zipc_hip_stream_result_s *results);

/* ---- batch forms (device-resident) ----------------------------------------- */

/* One independent stream: bytes [src_off, src_off+src_len) of the source arena
 * go to [dst_off, dst_off+dst_cap) of the destination arena.  For inflate,
 * limit is ?decompressed_size when flags & ZIPC_HIP_STREAM_HAS_LIMIT. */
typedef struct {
  uint64_t src_off;
  uint64_t src_len;
  uint64_t dst_off;
  uint64_t dst_cap;
  uint64_t limit;
  uint32_t flags;
  uint32_t reserved;
} zipc_hip_stream_desc;
#define ZIPC_HIP_STREAM_HAS_LIMIT 1u

typedef struct zipc_hip_stream_result_s {
  uint32_t status;   /* ZIPC_HIP_OK or an error code */
  uint32_t checksum; /* per crc_op, finished (0 for NOP) */
  uint64_t out_len;  /* bytes produced at dst_off */
} zipc_hip_stream_result;

/* All pointers are DEVICE pointers (descs and results too).  Work is enqueued
 * on the context stream and NOT synchronised: call zipc_hip_synchronize (or
 * synchronise the stream) before reading results.  Two exceptions, both zipc_hip_inflate_batch: ONE stream with
 * max_dst_cap above ZIPC_HIP_MAX_STREAM_LEN (a stream of stored blocks beyond 4 GiB, below), and a call whose
 * max_dst_cap is 256 KiB and more (one stream: 40 KiB of input and more): the library reads the descriptors back, and
 * the call's long streams -- all of a few, the long ones among many short ones, none of thousands of equal ones: chosen
 * by what each way costs -- are decoded by a wave per BLOCK, side by side: block starts searched for, the blocks walked
 * at once, copies resolved afterwards (a MiB in 1.3-1.9 ms instead of 10-30, 64 of them in 5 instead of 17).  That path
 * reads a few words back between its steps and so synchronises the stream itself.
 * Results, messages and limits are the same whichever way a stream is decoded (zipc_hip_last_inflate_blocks tells how
 * many blocks of the last call went that way; ZIPC_HIP_INFLATE_BLOCKS=0 in the environment keeps every stream on its
 * one wave).  Bits of flags other than ZIPC_HIP_STREAM_HAS_LIMIT must be zero: a stream whose descriptor has one set
 * reports ZIPC_HIP_ERR_INVALID_ARG and nothing is written to its destination. */
/* max_dst_cap: upper bound of dst_cap over the batch (sizes the CRC-32 pass). A stream
 * whose output is longer than that reports ZIPC_HIP_ERR_INVALID_ARG in its result when a
 * CRC-32 is asked for (its checksum would cover only a part). A descriptor with src_len or
 * dst_cap above ZIPC_HIP_MAX_STREAM_LEN reports ZIPC_HIP_ERR_INVALID_ARG in its own result.
 * dst_cap, the room of a stream -- the same in every form the library takes (a wave per stream, a wave per block) and in
 * every call that inflates (the host forms, the zlib forms, zipc_hip_inflate_packed_batch, zipc_hip_recode_batch with its
 * mid_cap): nothing is written in front of dst_off or behind dst_off + dst_cap, whatever the status.  Bytes between
 * out_len (or limit) and dst_cap may be written.  A stream that inflates to N bytes fits iff N <= R, R = min(limit,
 * dst_cap) (no limit: dst_cap); one that does not fit reports, with out_len 0 (what lies in its room is
 * unspecified):
 *     limit     dst_cap     status when R < N
 *     none      R           ZIPC_HIP_ERR_DST_TOO_SMALL
 *     R         R           ZIPC_HIP_ERR_SIZE_EXCEEDED
 *     R         above R     ZIPC_HIP_ERR_SIZE_EXCEEDED
 *     above N   R           ZIPC_HIP_ERR_DST_TOO_SMALL
 * (a limit in R < limit < N with dst_cap = R: ZIPC_HIP_ERR_SIZE_EXCEEDED where the symbol that does not fit ends behind
 * the limit, else ZIPC_HIP_ERR_DST_TOO_SMALL).  tests/test_gpu_inflate_room.py holds every form to this with guard bytes. */
int zipc_hip_inflate_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena,
                           const zipc_hip_stream_desc *d_descs,
                           zipc_hip_stream_result *d_results, size_t n_streams,
                           size_t max_dst_cap, int crc_op);

/* max_src_len: upper bound of src_len over the batch (sizes the kernels' grids);
 * total_src_len: sum of src_len over the batch (sizes the scratch). Both are checked on the
 * device against the descriptors: if a stream is longer than max_src_len or the sum exceeds
 * total_src_len, EVERY stream of the batch reports ZIPC_HIP_ERR_INVALID_ARG and nothing is
 * compressed. max_src_len above ZIPC_HIP_MAX_STREAM_LEN fails the call; a single descriptor
 * with src_len or dst_cap above it reports ZIPC_HIP_ERR_INVALID_ARG in its own result only.
 * dst_cap, the rule by which a stream fits -- the same in every form the library takes (a wave per stream, a wave per
 * block) and in every call that deflates (the host forms, the zlib forms with the room their container leaves,
 * zipc_hip_recode_batch); it is NOT "the output fits":
 *   a compressing level: the blocks are tested one by one, in order, each before it is written.  A block passes when the
 *     bits of the blocks in front of it plus its own size, rounded up to whole bytes, do not exceed dst_cap.  The size of a
 *     fixed or a stored block is its real size; the size of a dynamic block is the reference's ESTIMATE of it
 *     (bit_length_of_dynamic_huffman_block, zipc_deflate.ml:1071-1079), which counts the code-length symbols of every
 *     block so far -- the reference never resets those counts -- and so is exact for a stream's first block and high
 *     from the second on.  Hence a dst_cap that holds the whole output can be refused (70 000 zero bytes: 97 bytes of
 *     output, 101 needed), and a block in the middle of a stream can be the one that decides;
 *   ZIPC_HIP_LEVEL_NONE: the stream fits iff src_len + 5 * nblocks <= dst_cap, nblocks = 1 for an empty stream and
 *     ceil(src_len / 65534) otherwise;
 *   dst_cap = zipc_hip_deflate_bound(src_len) always fits.
 * A stream that does not fit reports ZIPC_HIP_ERR_DST_TOO_SMALL with out_len 0.  Nothing is written behind dst_cap, nor at
 * or behind the first whole byte of the first block that did not pass; in front of that, whole bytes of the blocks that
 * passed may have been written (of a stream whose first block does not pass, and at ZIPC_HIP_LEVEL_NONE: nothing).  Its
 * checksum is 0 with either Adler-32, and with ZIPC_HIP_CRC_CRC32 the CRC-32 of its source: that pass runs over the source
 * whatever the verdict.  (zipc_hip_deflate hands out no checksum with an error status.) */
int zipc_hip_deflate_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena,
                           const zipc_hip_stream_desc *d_descs,
                           zipc_hip_stream_result *d_results, size_t n_streams,
                           size_t max_src_len, size_t total_src_len, int level,
                           int crc_op);

/* The zlib container on the device: stream i of the source arena is a WHOLE zlib stream (decompress), or becomes one
 * in its destination slot (compress; dst_cap of zipc_hip_zlib_bound(src_len) always fits).  Same descriptors, results
 * and contract as the two forms above -- all pointers are device pointers, the work is enqueued on the context's stream
 * and not synchronised, except where zipc_hip_inflate_batch itself synchronises (max_dst_cap of 256 KiB and more) -- and
 * the same kernels, between two small ones that handle the container, a lane per stream (csrc/zlib.hip):
 *   before: the reference's checks in its order (zipc_deflate.ml:723-730; to compress: dst_cap < 6 is
 *     ZIPC_HIP_ERR_DST_TOO_SMALL), a flag bit other than ZIPC_HIP_STREAM_HAS_LIMIT is ZIPC_HIP_ERR_INVALID_ARG; a stream
 *     that fails reports that status with checksum 0 and out_len 0, and nothing is written to its destination.  The
 *     codec is handed the reference's body range [2, len-2) / the room [2, dst_cap-4) (the descriptors it runs with
 *     live in the context's scratch);
 *   behind: to decompress, the Adler-32 of the output (the reference's, or RFC 1950's after
 *     zipc_hip_set_adler_rfc1950) against the stream's last four bytes: a stream whose checksum differs reports
 *     ZIPC_HIP_ERR_CHECKSUM with checksum = the value FOUND and out_len 0 -- the value EXPECTED is not in the result:
 *     it is the big-endian word in the stream's own last four bytes.  To compress, CMF / FLG and the Adler-32 are
 *     stored around deflate's bytes, out_len counts them and checksum is the Adler-32.  Every other result is the
 *     codec's (the batch-wide ZIPC_HIP_ERR_INVALID_ARG of zipc_hip_deflate_batch's declared sizes among them).
 * level outside 0..3 fails the call.  ONE stream with max_dst_cap above ZIPC_HIP_MAX_STREAM_LEN fails the call with
 * ZIPC_HIP_ERR_INVALID_ARG: inflate's path for stored streams beyond 4 GiB computes no Adler-32. */
int zipc_hip_zlib_decompress_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena,
                                   const zipc_hip_stream_desc *d_descs, zipc_hip_stream_result *d_results,
                                   size_t n_streams, size_t max_dst_cap);
int zipc_hip_zlib_compress_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena,
                                 const zipc_hip_stream_desc *d_descs, zipc_hip_stream_result *d_results,
                                 size_t n_streams, size_t max_src_len, size_t total_src_len, int level);

/* Sizing: what every stream of a batch inflates to, and whether it does, before there is a destination -- a raw deflate
 * stream carries no decompressed size and a zlib stream only an Adler-32, and every decode form above needs a dst_cap.
 * Same descriptors and results as zipc_hip_inflate_batch, all pointers DEVICE pointers; ONE kernel launch, a wave per
 * stream, enqueued on the context's stream and never synchronised (no path of it reads anything back).
 * The defining property: for every stream, status and out_len are what zipc_hip_inflate_batch (ZIPC_HIP_CRC_NOP) reports
 * for the same src_off, src_len, limit and flags with dst_cap = ZIPC_HIP_MAX_STREAM_LEN; checksum is 0.  No byte of any
 * arena is written -- there is no destination arena; the source is only read -- and dst_off and dst_cap of the
 * descriptors are not looked at (a dst_cap above ZIPC_HIP_MAX_STREAM_LEN is no error here).  Hence:
 *   - ZIPC_HIP_ERR_DST_TOO_SMALL appears only for a stream that inflates beyond ZIPC_HIP_MAX_STREAM_LEN.  (That path is
 *     not tested: a wave would have to walk 4 GiB of output.)
 *   - with ZIPC_HIP_STREAM_HAS_LIMIT, a stream that inflates beyond its limit is ZIPC_HIP_ERR_SIZE_EXCEEDED, out_len 0;
 *     one that ends below it is ZIPC_HIP_OK with its true length, as with the reference's ?decompressed_size.
 *   - every message of inflate is made with inflate's checks in inflate's order (a distance beyond the output so far
 *     is checked against the true output position): an empty source is ZIPC_HIP_ERR_CORRUPTED, as the reference says.
 *   - a flag bit other than ZIPC_HIP_STREAM_HAS_LIMIT, or src_len above ZIPC_HIP_MAX_STREAM_LEN, is
 *     ZIPC_HIP_ERR_INVALID_ARG in that stream's own result.
 *   - null ctx, d_descs or d_results, or n_streams above 0x7FFFFFFF, fails the call with ZIPC_HIP_ERR_INVALID_ARG;
 *     n_streams == 0 is ZIPC_HIP_OK and nothing is enqueued.
 *   - in THIS form a stream is always sized by its one wave, so a long stream costs what one wave takes to walk it --
 *     4.5 to 7 ms a MiB of text -- while a batch of many streams is sized in less time than it is decoded (DESIGN.md
 *     section 6).  A call that holds long streams is for zipc_hip_inflate_size_blocks_batch (below), which sizes those
 *     by a wave per block and synchronises; this form stays one launch, never synchronised.
 * The use: size the batch, read the results, lay the destinations out with dst_cap = out_len, call
 * zipc_hip_inflate_batch (INTEGRATION.md has the recipe). */
int zipc_hip_inflate_size_batch(zipc_hip_ctx *ctx, const void *d_src_arena,
                                const zipc_hip_stream_desc *d_descs,
                                zipc_hip_stream_result *d_results, size_t n_streams);
/* The same for WHOLE zlib streams (stream i of the source arena as in zipc_hip_zlib_decompress_batch): the container's
 * checks before (csrc/zlib.hip, unchanged), the size kernel over the bodies [2, len-2), and a close, a lane per stream:
 * a stream that fails its header check (or has a flag bit other than ZIPC_HIP_STREAM_HAS_LIMIT) reports that status with
 * out_len 0, every other stream what the size kernel says of its body.  checksum is 0.  The Adler-32 is NOT compared --
 * there are no bytes to take it of -- so a stream that is sized ZIPC_HIP_OK can still be ZIPC_HIP_ERR_CHECKSUM when it is
 * decompressed.  Enqueued on the context's stream, never synchronised; the same argument rules as above. */
int zipc_hip_zlib_size_batch(zipc_hip_ctx *ctx, const void *d_src_arena,
                             const zipc_hip_stream_desc *d_descs,
                             zipc_hip_stream_result *d_results, size_t n_streams);

/* A prefix: the first dst_cap bytes of every stream of a batch -- for a caller who wants the beginning of each stream (a
 * magic number, a header line, a first record) and neither the time nor the room of the whole.  Every other decode form
 * is all or nothing: a stream that does not fit its room is ZIPC_HIP_ERR_DST_TOO_SMALL with nothing to show. */
typedef struct {            /* 16 bytes, the layout of zipc_hip_stream_result */
  uint32_t status;   /* ZIPC_HIP_OK or the stream's own error */
  uint32_t ended;    /* 1: the stream's final block ended within the room; 0: cut at dst_cap, or an error */
  uint64_t out_len;  /* bytes at dst_off; 0 unless OK */
} zipc_hip_prefix_result;
/* All pointers are DEVICE pointers.  The descriptors are zipc_hip_inflate_batch's, every field with the meaning it has
 * there, limit and ZIPC_HIP_STREAM_HAS_LIMIT included.
 * The defining property, the one rule: for every stream let (s, n) be the status and out_len that zipc_hip_inflate_batch
 * (ZIPC_HIP_CRC_NOP) reports for the same descriptor.
 *   s == ZIPC_HIP_OK: the result is {ZIPC_HIP_OK, ended 1, n} and the room holds the same bytes.
 *   s == ZIPC_HIP_ERR_DST_TOO_SMALL: the result is {ZIPC_HIP_OK, ended 0, out_len = dst_cap} and the room holds the first
 *     dst_cap bytes of the serial decode: the whole symbols before the one that did not fit and, of a match or a stored
 *     block that straddles the end, the bytes that fit.  Nothing behind the cut is read or judged: an error of the stream
 *     that lies behind the symbol that was cut is not reported.
 *   any other s: that status, ended 0, out_len 0 -- ZIPC_HIP_ERR_CORRUPTED, ZIPC_HIP_ERR_SIZE_EXCEEDED (also where a limit
 *     lies inside the straddling symbol, exactly as the table at zipc_hip_inflate_batch says) and the
 *     ZIPC_HIP_ERR_INVALID_ARG of a flag bit or of a length above ZIPC_HIP_MAX_STREAM_LEN.
 * What follows from it:
 *   - symbols with no output still count: an end of block, a block header, an empty stored block behind a full room are
 *     still read, and their errors reported;
 *   - the exact fit: a stream whose output is exactly dst_cap is ended 1 iff its final block ends before a symbol needs room;
 *   - dst_cap == 0 is legal: {ZIPC_HIP_OK, 0, 0} for a stream that has output;
 *   - nothing is written in front of dst_off or behind dst_off + dst_cap, whatever the status.
 * Always a wave per stream, whatever dst_cap: this form has no by-blocks path and reads nothing back
 * (zipc_hip_last_inflate_blocks is 0 behind it).  One launch, enqueued on the context's stream and never synchronised;
 * growing the context's scratch may synchronise, as everywhere.  A wave that is cut has read only the source it needed.
 * No checksum is offered: zipc_hip_checksum_batch over the prefixes is the way to one.
 * Null ctx, d_descs or d_results, or n_streams above 0x7FFFFFFF, fails the call with ZIPC_HIP_ERR_INVALID_ARG;
 * n_streams == 0 is ZIPC_HIP_OK and nothing is enqueued.  INTEGRATION.md has the recipe "peek, then decide". */
int zipc_hip_inflate_prefix_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena,
                                  const zipc_hip_stream_desc *d_descs, zipc_hip_prefix_result *d_results,
                                  size_t n_streams);
/* The same for WHOLE zlib streams (stream i of the source arena as in zipc_hip_zlib_decompress_batch): the container's
 * checks before (csrc/zlib.hip, unchanged) -- a stream that fails them reports that status, ended 0, out_len 0, and
 * nothing of it is written -- the prefix kernel over the bodies with the context's Adler-32 flavour, and a close, a lane
 * per stream: a stream that ENDED within its room has its Adler-32 compared as zipc_hip_zlib_decompress_batch compares
 * it, and on a mismatch reports ZIPC_HIP_ERR_CHECKSUM, ended 0, out_len 0 (the value found is not reported: there is no
 * field for it); a stream that was cut is {ZIPC_HIP_OK, 0, dst_cap} with nothing compared -- its trailer has not been
 * reached; every other status is the body's.  Enqueued and never synchronised; the same argument rules. */
int zipc_hip_zlib_decompress_prefix_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena,
                                          const zipc_hip_stream_desc *d_descs, zipc_hip_prefix_result *d_results,
                                          size_t n_streams);

/* Inflate with HISTORY: a stream that does not start at bit 0 of its input with nothing in front of its output -- a raw
 * deflate piece whose encoder kept its window across a flush (permessage-deflate messages, pigz-style chunks, the records
 * of a log written with Z_SYNC_FLUSH), a chunk of a long stream read from an access point (the zran / indexed-gzip idea:
 * an index holds a bit position and the 32 KiB of output in front of it), a zlib stream with a preset dictionary.  Every
 * other inflate form calls a match that reaches in front of the output ZIPC_HIP_ERR_CORRUPTED. */
typedef struct {            /* 8 bytes, one per stream */
  uint32_t hist_len;   /* bytes of history, <= 32768: they lie at [dst_off - hist_len, dst_off) of the DESTINATION arena */
  uint32_t start_bit;  /* the bit of the byte at src_off at which the first block header starts, 0..7, 0 the lowest */
} zipc_hip_history;
/* All pointers are DEVICE pointers.  The descriptors are zipc_hip_inflate_batch's; d_hist: a record per stream, or null:
 * every record is {0, 0}.  The CALLER has put the history where the record says (the zlib dictionary forms below do it
 * themselves); it is read, never written: the bytes at [dst_off - hist_len, dst_off) are unchanged after every call,
 * whatever the status.
 * The verdict on a record, in this order, each the stream's own result with out_len 0: hist_len > 32768, start_bit > 7,
 * hist_len > dst_off (the sizing form has no destination and skips this one) are ZIPC_HIP_ERR_INVALID_ARG; then the
 * descriptor's own tests as ever, on the caller's values.
 * The defining property: a match is legal iff its distance <= hist_len + (bytes produced so far).  Everything else is
 * what zipc_hip_inflate_batch says with positions counted from dst_off: the room table, the limit rule (a limit counts
 * the stream's own bytes, not the history), the statuses, the order of checks, out_len.  With a null d_hist, or a record
 * of {0, 0}, every history form IS the form it mirrors: same status, out_len, checksum and bytes.
 * Checksums: ZIPC_HIP_CRC_ADLER32 / _RFC1950 are of the stream's own output (the history is not summed);
 * ZIPC_HIP_CRC_CRC32 is the pass over [dst_off, dst_off + out_len).  The checksums of pieces are not combined here.
 * Always a wave per stream: no by-blocks path, no stored-chain path, nothing read back, never synchronised
 * (zipc_hip_last_inflate_blocks is 0 behind them).  The layout is the caller's duty ("decode from an
 * access point"): streams of ONE call need rooms of their own with their histories in front, and a stream's history must
 * not be the room another stream of the same call is written to (a copy may store up to 7 transient bytes past a match);
 * pieces decoded in successive calls may lie end to end, hist_len = min(32768, bytes so far).
 * Null ctx, d_descs or d_results, crc_op outside 0..3, or n_streams above 0x7FFFFFFF, fails the call with
 * ZIPC_HIP_ERR_INVALID_ARG; n_streams == 0 is ZIPC_HIP_OK and nothing is enqueued.
 * Out of scope: deflating against a dictionary or a kept window; building an index of access points; history in the
 * extent, packed, gzip and recode forms; a by-blocks path for long streams with history; combining checksums of pieces.
 *
 * zipc_hip_inflate_history_batch: from the start point to the end of the final block, all or nothing. */
int zipc_hip_inflate_history_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena,
                                   const zipc_hip_stream_desc *d_descs, const zipc_hip_history *d_hist,
                                   zipc_hip_stream_result *d_results, size_t n_streams, size_t max_dst_cap, int crc_op);
/* The first dst_cap bytes from the start point: zipc_hip_inflate_prefix_batch's one rule, word for word, over the
 * statuses above.  This is the read from an access point: a chunk of a long stream is cut at its room, and nothing
 * behind the cut is read or judged. */
int zipc_hip_inflate_prefix_history_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena,
                                          const zipc_hip_stream_desc *d_descs, const zipc_hip_history *d_hist,
                                          zipc_hip_prefix_result *d_results, size_t n_streams);
/* Sizing: no arena is written or read, the record serves the distance test alone; status and out_len are what
 * zipc_hip_inflate_history_batch reports with dst_cap = ZIPC_HIP_MAX_STREAM_LEN, checksum 0. */
int zipc_hip_inflate_size_history_batch(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs,
                                        const zipc_hip_history *d_hist, zipc_hip_stream_result *d_results,
                                        size_t n_streams);
/* WHOLE zlib streams against ONE preset dictionary on the device (RFC 1950's FDICT, as deflateSetDictionary makes them):
 * d_dict, dict_len <= 32768 bytes (more, or a null d_dict with dict_len != 0, fails the call).
 * zipc_hip_zlib_decompress_batch keeps answering ZIPC_HIP_ERR_ZLIB_DICT for such streams; these forms open them:
 *   - the container's checks in their order up to the FDICT test (length, FCHECK, method, window);
 *   - a stream WITHOUT FDICT is opened exactly as there and decoded with no history, as zlib does;
 *   - a stream with FDICT: shorter than 10 bytes is ZIPC_HIP_ERR_CORRUPTED; dict_len == 0, or a DICTID (bytes 2..5,
 *     big-endian) that is not RFC 1950's Adler-32 of the dictionary -- whatever the context's flavour -- is
 *     ZIPC_HIP_ERR_ZLIB_DICT with checksum = the DICTID found, so that a caller can look the right dictionary up, and
 *     out_len 0; otherwise the body is [6, len - 4) and the dictionary its history.
 * The dictionary's Adler-32 is made once per call on the device; nothing is read back, the call is never synchronised.
 * The decompress form then COPIES THE DICTIONARY to [dst_off - dict_len, dst_off) of every stream opened with FDICT:
 * the one place where a form of this library writes in front of dst_off.  That gap belongs to the call; dst_off <
 * dict_len is the stream's ZIPC_HIP_ERR_INVALID_ARG.  The gap of a stream without FDICT, or of one that failed its open,
 * is not written; nothing is written in front of the gap or behind dst_off + dst_cap.  The sizing form writes nothing.
 * The close: the Adler-32 of the output alone (the context's flavour) against the trailer, as
 * zipc_hip_zlib_decompress_batch compares it; the sizing form compares nothing, as zipc_hip_zlib_size_batch. */
int zipc_hip_zlib_decompress_dict_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena,
                                        const zipc_hip_stream_desc *d_descs, zipc_hip_stream_result *d_results,
                                        size_t n_streams, size_t max_dst_cap, const void *d_dict, size_t dict_len);
int zipc_hip_zlib_size_dict_batch(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs,
                                  zipc_hip_stream_result *d_results, size_t n_streams, const void *d_dict,
                                  size_t dict_len);
/* Host forms, thin: ONE stream from host memory, staged as [history | room] in the context's buffers, through the batch
 * form of one, and only the room copied back.  They synchronise.  The return value is the stream's status.
 * zipc_hip_inflate_history: hist_len bytes at `hist` are the history (hist_len > 32768 or start_bit > 7 is
 * ZIPC_HIP_ERR_INVALID_ARG); checksum may be null.  zipc_hip_zlib_decompress_dict: a whole zlib stream against `dict`. */
int zipc_hip_inflate_history(zipc_hip_ctx *ctx, const void *src, size_t len, unsigned start_bit, const void *hist,
                             size_t hist_len, int has_limit, size_t limit, void *dst, size_t dst_cap, int crc_op,
                             size_t *out_len, uint32_t *checksum);
int zipc_hip_zlib_decompress_dict(zipc_hip_ctx *ctx, const void *src, size_t len, const void *dict, size_t dict_len,
                                  void *dst, size_t dst_cap, size_t *out_len);

/* Sizing with the long streams of the call BY BLOCKS: descriptors, results, argument rules and the defining property of
 * zipc_hip_inflate_size_batch / zipc_hip_zlib_size_batch, word for word -- status and out_len are what
 * zipc_hip_inflate_batch (ZIPC_HIP_CRC_NOP) reports with dst_cap = ZIPC_HIP_MAX_STREAM_LEN, checksum is 0, no arena is
 * written, dst_off and dst_cap are not looked at.  The one difference: the call reads the descriptors and a few counts
 * back, so it SYNCHRONISES the context's stream (as zipc_hip_inflate_batch does from 256 KiB on), and streams of 40 KiB
 * to 512 MiB of source -- the longest of the call, as many as the model of csrc/forms.h size_blocks_pick says pay:
 * all of a few long streams, the few long ones among many short ones, none of thousands of equal ones -- are sized by the
 * first half of the launches that decode a long stream (csrc/inflate.hip: block headers found, a dry run a block, the
 * chain of the blocks' sizes) and one short walk of the stream's first 32 KiB of output, which makes the one check the
 * dry runs leave out (a match distance against the true output position).  A stream is sized that way only where those
 * steps show it to be ZIPC_HIP_OK; every other stream -- any error, a limit exceeded, a stream of fixed or stored
 * blocks nobody could chain -- is sized by its one wave, which owns every message.  ZIPC_HIP_INFLATE_BLOCKS=0 keeps every
 * stream on its one wave.  The zlib form: zipc_hip_zlib_size_batch's open and close around this path over the bodies. */
int zipc_hip_inflate_size_blocks_batch(zipc_hip_ctx *ctx, const void *d_src_arena,
                                       const zipc_hip_stream_desc *d_descs,
                                       zipc_hip_stream_result *d_results, size_t n_streams);
int zipc_hip_zlib_size_blocks_batch(zipc_hip_ctx *ctx, const void *d_src_arena,
                                    const zipc_hip_stream_desc *d_descs,
                                    zipc_hip_stream_result *d_results, size_t n_streams);

/* Streams of UNKNOWN COMPRESSED LENGTH: where each one ends.  Every decode form ignores what lies behind the final block, as
 * the reference does, so src_len may already be an upper bound of the stream's length -- but a raw deflate stream carries
 * no length of its own and a zlib stream only an Adler-32 (objects of a git pack, Flate streams of a PDF, zlib streams in
 * other containers, any run of streams stored back to back).  The extent forms are the forms they mirror, with one more
 * answer: src_used, the source bytes the stream took.  Nothing of an existing form changes. */
typedef struct {            /* 32 bytes: zipc_hip_stream_result's three fields, then the extent */
  uint32_t status;    /* as in the mirrored form */
  uint32_t checksum;  /* as in the mirrored form; 0 unless OK */
  uint64_t out_len;   /* as in the mirrored form; 0 unless OK */
  uint64_t src_used;  /* source bytes from src_off up to and including the byte that holds the last bit of the final block --
                         behind the end-of-block symbol of a compressed block, behind the last data byte of a stored one
                         (LEN == 0 included); the zlib forms: the whole stream, header and trailer too.  0 unless OK: a
                         stream that is refused has no extent.  src_used <= src_len for every OK stream. */
  uint64_t reserved;  /* 0 */
} zipc_hip_extent_result;
/* All pointers are DEVICE pointers.  The descriptors are zipc_hip_stream_desc, every field as in the form each mirrors;
 * src_len may be any upper bound of the stream's length that lies inside the arena: nothing behind src_off + src_len is read.
 * The defining properties:
 *   raw, decode (zipc_hip_inflate_extent_batch): status, checksum, out_len and the destination bytes are what
 *     zipc_hip_inflate_batch gives for the same descriptor and crc_op -- the table of room rules and the guard-byte contract
 *     there included.  src_used is 0 unless OK.  For an OK stream, zipc_hip_inflate_batch with src_len := src_used gives the
 *     same result and bytes.  With ZIPC_HIP_CRC_CRC32 a stream whose output is longer than max_dst_cap is
 *     ZIPC_HIP_ERR_INVALID_ARG as it is there (its checksum would cover only a part), with checksum, out_len and src_used 0
 *     like every status but OK (zipc_hip_inflate_batch leaves the length in that one record).
 *   raw, size (zipc_hip_inflate_size_extent_batch, zipc_hip_inflate_size_extent_blocks_batch): the same with
 *     zipc_hip_inflate_size_batch / zipc_hip_inflate_size_blocks_batch; checksum is 0, no arena but the source is touched.
 *     The blocks form synchronises where zipc_hip_inflate_size_blocks_batch does, picks the streams it picks, and
 *     zipc_hip_last_size_blocks says what it says there; the wave form never synchronises.
 *   zlib (zipc_hip_zlib_decompress_extent_batch, zipc_hip_zlib_size_extent_batch, zipc_hip_zlib_size_extent_blocks_batch):
 *     header failures are the reference's, in its order; src_len < 6 is ZIPC_HIP_ERR_CORRUPTED and nothing of the stream is
 *     read.  The body handed to the codec is the reference's range [2, src_len - 2).  With u the body's extent, the trailer
 *     is the four bytes at src_off + 2 + u, big-endian, NOT those at src_len - 4; if 2 + u + 4 > src_len the trailer is not
 *     inside the declared bytes: ZIPC_HIP_ERR_CORRUPTED, nothing compared.  Otherwise the Adler-32 is compared as
 *     zipc_hip_zlib_decompress_batch compares it: a mismatch is ZIPC_HIP_ERR_CHECKSUM with the value found, out_len 0 and
 *     src_used 0.  On OK src_used = u + 6, and zipc_hip_zlib_decompress_batch (or zipc_hip_zlib_size_batch) with
 *     src_len := src_used gives the same status, checksum, out_len and bytes.  The sizing forms compare no checksum, like
 *     zipc_hip_zlib_size_batch, but hold the same "trailer inside src_len" rule, so a stream they size OK has the src_used
 *     the decode form reports.
 * The decode forms are ALWAYS a wave per stream, whatever max_dst_cap: one launch (and for ZIPC_HIP_CRC_CRC32 the checksum
 * pass over the produced bytes, which max_dst_cap sizes as in zipc_hip_inflate_batch), enqueued on the context's stream and
 * never synchronised (growing the context's scratch may synchronise, as everywhere); there is no by-blocks path and
 * zipc_hip_last_inflate_blocks is 0 behind them.  A long stream then costs what its one wave costs: 4.5 - 6.9 ms a MiB of
 * output (the sizing form's figure), where zipc_hip_inflate_batch decodes it by blocks in 0.13 - 1.8.  A
 * caller with long streams sizes them with zipc_hip_inflate_size_extent_blocks_batch and decodes with
 * zipc_hip_inflate_batch over src_len := src_used.
 * Null ctx, d_descs or d_results, n_streams above 0x7FFFFFFF, or a crc_op outside the ZIPC_HIP_CRC_* values, fails the call
 * with ZIPC_HIP_ERR_INVALID_ARG; n_streams == 0 is ZIPC_HIP_OK and nothing is enqueued.  A flag bit other than
 * ZIPC_HIP_STREAM_HAS_LIMIT, or a length above ZIPC_HIP_MAX_STREAM_LEN, is ZIPC_HIP_ERR_INVALID_ARG in the stream's own
 * result.  Walking a run of back-to-back streams is the caller's loop (each start depends on the end before it):
 * INTEGRATION.md has the recipe "streams whose compressed length you do not know". */
int zipc_hip_inflate_extent_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena,
                                  const zipc_hip_stream_desc *d_descs, zipc_hip_extent_result *d_results,
                                  size_t n_streams, size_t max_dst_cap, int crc_op);
int zipc_hip_zlib_decompress_extent_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena,
                                          const zipc_hip_stream_desc *d_descs, zipc_hip_extent_result *d_results,
                                          size_t n_streams, size_t max_dst_cap);
int zipc_hip_inflate_size_extent_batch(zipc_hip_ctx *ctx, const void *d_src_arena,
                                       const zipc_hip_stream_desc *d_descs,
                                       zipc_hip_extent_result *d_results, size_t n_streams);
int zipc_hip_zlib_size_extent_batch(zipc_hip_ctx *ctx, const void *d_src_arena,
                                    const zipc_hip_stream_desc *d_descs,
                                    zipc_hip_extent_result *d_results, size_t n_streams);
int zipc_hip_inflate_size_extent_blocks_batch(zipc_hip_ctx *ctx, const void *d_src_arena,
                                              const zipc_hip_stream_desc *d_descs,
                                              zipc_hip_extent_result *d_results, size_t n_streams);
int zipc_hip_zlib_size_extent_blocks_batch(zipc_hip_ctx *ctx, const void *d_src_arena,
                                           const zipc_hip_stream_desc *d_descs,
                                           zipc_hip_extent_result *d_results, size_t n_streams);
/* One stream from HOST memory, staged like zipc_hip_inflate / zipc_hip_zlib_decompress: `len` is an upper bound, *src_used
 * the bytes of src the stream took (0 unless ZIPC_HIP_OK); everything else as in those two.  The stream's one wave decodes
 * it whatever its length (see above).  On ZIPC_HIP_ERR_CHECKSUM *adler is the value found, with every other error 0.
 * Many-stream host forms (_many) of the extent forms are out of scope: there are none. */
int zipc_hip_inflate_extent(zipc_hip_ctx *ctx, const void *src, size_t len, int has_limit, size_t limit,
                            void *dst, size_t dst_cap, int crc_op, size_t *out_len, size_t *src_used,
                            uint32_t *checksum);
int zipc_hip_zlib_decompress_extent(zipc_hip_ctx *ctx, const void *src, size_t len, int has_limit, size_t limit,
                                    void *dst, size_t dst_cap, size_t *out_len, size_t *src_used,
                                    uint32_t *adler);

/* GZIP MEMBERS (RFC 1952): .gz files, HTTP bodies, and BGZF (bgzip, BAM, tabix) -- a file of back-to-back members of at
 * most 64 KiB each, every one carrying its own length in an extra field.  The reference has no gzip; the rules are RFC
 * 1952's as zlib reads them, in csrc/gzip_container.h.  A member's length is not known up front, so the forms below are
 * the extent forms above between an open and a close of a lane per member.  Nothing of an existing form changes.
 * The defining properties:
 *   - for an OK member, zipc_hip_inflate_batch over [src_off + hdr_len, src_off + src_used - 8) with ZIPC_HIP_CRC_CRC32
 *     gives the same bytes, length and checksum;
 *   - a member produced by zipc_hip_gzip_compress_batch is ten (BGZF: eighteen) header bytes, then exactly the bytes
 *     zipc_hip_deflate_batch writes for that source and level, then the trailer.
 * The header (src_len: any upper bound of the member's length inside the arena; every index is checked against it before
 * it is read), in this order: src_len < 18 is ZIPC_HIP_ERR_CORRUPTED and nothing is read; ID1, ID2 other than 1f 8b
 * CORRUPTED; CM other than 8 ZIPC_HIP_ERR_ZLIB_METHOD; a reserved bit of FLG (0xE0) CORRUPTED, FTEXT is ignored; FEXTRA:
 * XLEN and its bytes inside src_len or CORRUPTED -- the first subfield 'B','C' of length 2 is BGZF's BSIZE, a subfield that
 * overruns XLEN ends the walk and is no error; FNAME, then FCOMMENT: the zero inside src_len and at most 65 535 bytes in
 * front of it or CORRUPTED -- a LIMIT OF THIS LIBRARY (zlib scans without bound) that keeps a lane's walk over a hostile
 * member bounded; FHCRC: the low 16 bits of the CRC-32 of the header bytes in front of it, or CORRUPTED.
 * The body handed to the codec is [hdr_len, src_len).  With u the body's extent, the trailer -- CRC32, then ISIZE,
 * little-endian -- is the eight bytes at src_off + hdr_len + u; hdr_len + u + 8 > src_len is CORRUPTED with nothing read.
 * A CRC-32 that differs is ZIPC_HIP_ERR_CHECKSUM with the value FOUND in checksum; then an ISIZE other than out_len mod
 * 2^32 is CORRUPTED (the CRC comes first, as in zlib: a member with both wrong is CHECKSUM).  The sizing forms compare no
 * CRC-32 (there are no bytes to take it of) but compare ISIZE and hold the same bound, so a member they size OK has the
 * src_used the decode form reports.  On OK src_used = hdr_len + u + 8; what lies behind it is not looked at. */
typedef struct {            /* 32 bytes, the layout of zipc_hip_extent_result */
  uint32_t status;
  uint32_t checksum;  /* CRC-32 of the output (decode), 0 (size); with ZIPC_HIP_ERR_CHECKSUM the value found; else 0 unless OK */
  uint64_t out_len;   /* 0 unless OK */
  uint64_t src_used;  /* whole member: header, body, trailer; 0 unless OK */
  uint32_t hdr_len;   /* 0 unless OK */
  uint32_t flg;       /* the member's FLG byte; 0 unless OK */
} zipc_hip_gzip_result;
enum { ZIPC_HIP_GZIP_PLAIN = 0, ZIPC_HIP_GZIP_BGZF = 1 };
/* All pointers are DEVICE pointers.  The descriptors are zipc_hip_stream_desc with every field as in the mirrored extent
 * form (zipc_hip_inflate_extent_batch with ZIPC_HIP_CRC_CRC32, zipc_hip_inflate_size_extent_batch,
 * zipc_hip_inflate_size_extent_blocks_batch); limit and ZIPC_HIP_STREAM_HAS_LIMIT apply to the member's output.
 * The decode form is ALWAYS a wave per member, whatever max_dst_cap: the open, one launch and the CRC-32 pass over the
 * produced bytes, which max_dst_cap sizes as in zipc_hip_inflate_batch (a member whose output is longer is
 * ZIPC_HIP_ERR_INVALID_ARG), then the close -- enqueued on the context's stream and never synchronised (growing the
 * context's scratch may synchronise, as everywhere); zipc_hip_last_inflate_blocks is 0 behind it.  The size form never
 * synchronises; the size-by-blocks form synchronises where zipc_hip_inflate_size_blocks_batch does, picks the members it
 * picks, and zipc_hip_last_size_blocks says what it says there.  A caller with long members sizes them by blocks and
 * decodes with zipc_hip_inflate_batch over the body (the first property), as zipc_hip_gzip_decompress does.
 * Null ctx, d_descs or d_results, or n_streams above 0x7FFFFFFF, fails the call with ZIPC_HIP_ERR_INVALID_ARG;
 * n_streams == 0 is ZIPC_HIP_OK and nothing is enqueued.  A flag bit other than ZIPC_HIP_STREAM_HAS_LIMIT, or a length
 * above ZIPC_HIP_MAX_STREAM_LEN, is ZIPC_HIP_ERR_INVALID_ARG in the member's own result. */
int zipc_hip_gzip_decompress_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena,
                                   const zipc_hip_stream_desc *d_descs, zipc_hip_gzip_result *d_results,
                                   size_t n_streams, size_t max_dst_cap);
int zipc_hip_gzip_size_batch(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs,
                             zipc_hip_gzip_result *d_results, size_t n_streams);
int zipc_hip_gzip_size_blocks_batch(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs,
                                    zipc_hip_gzip_result *d_results, size_t n_streams);
/* Compress: zipc_hip_deflate_batch with ZIPC_HIP_CRC_CRC32 between the open and the close, arguments and results as
 * zipc_hip_zlib_compress_batch's (out_len counts the container's bytes, checksum is the CRC-32 of the source).  The header
 * is 1f 8b 08 00 00000000 XFL ff: MTIME 0 and OS 255, so the output is a function of the input alone; XFL is 2 at
 * ZIPC_HIP_LEVEL_BEST, 4 at ZIPC_HIP_LEVEL_FAST, 0 otherwise.  The trailer is the CRC-32 of the source and src_len mod
 * 2^32.  ZIPC_HIP_GZIP_BGZF writes FLG = 4, XLEN = 6 and the subfield 42 43 02 00 BSIZE (the member's length - 1): an
 * 18-byte header; the room is first clipped to 65 536 bytes, so a member can never exceed what BSIZE can say (a source
 * that does not deflate into it is ZIPC_HIP_ERR_DST_TOO_SMALL: BGZF callers cut their input at 65 280 bytes).  The
 * library writes members only: BGZF's 28-byte end-of-file block is the caller's to append.
 * dst_cap below the overhead (18 bytes, BGZF 26) is ZIPC_HIP_ERR_DST_TOO_SMALL; zipc_hip_gzip_bound(len, flavour) always
 * suffices for the plain flavour.  A level outside 0..3 or a flavour other than the two fails the call. */
size_t zipc_hip_gzip_bound(size_t len, int flavour);
int zipc_hip_gzip_compress_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena,
                                 const zipc_hip_stream_desc *d_descs, zipc_hip_stream_result *d_results,
                                 size_t n_streams, size_t max_src_len, size_t total_src_len, int level, int flavour);
/* From HOST memory.  zipc_hip_gzip_compress writes ONE member.  zipc_hip_gzip_size and zipc_hip_gzip_decompress take a
 * whole FILE: every member is read and the outputs are concatenated (RFC 1952 section 2.2); *src_used says where the last
 * member ended, *n_members how many there were.  The file is staged once.  A run of consecutive members whose headers say
 * their length (BGZF) goes to the device as ONE batch call with exact lengths and destinations laid out from the ISIZEs --
 * a BAM file costs one launch sequence, not a round trip per 64 KiB; a member of such a run that is not OK reports its
 * status, one whose src_used differs from its BSIZE + 1, or whose body does not fit the room its own ISIZE promised, is
 * ZIPC_HIP_ERR_CORRUPTED.  A member of unknown length is sized by the size-by-blocks form, decoded by
 * zipc_hip_inflate_batch over its body (so a long .gz goes by blocks) and closed by the same rule.  Bytes behind the
 * last member that do not begin with 1f 8b end the walk with ZIPC_HIP_OK.  Total output above dst_cap is
 * ZIPC_HIP_ERR_DST_TOO_SMALL.  Any error returns with *out_len = *src_used = 0; on ZIPC_HIP_ERR_CHECKSUM *crc_found is the
 * value found.  n_members and crc_found may be null.  There are no many-stream (_many) forms of gzip. */
int zipc_hip_gzip_compress(zipc_hip_ctx *ctx, const void *src, size_t len, int level, int flavour,
                           void *dst, size_t dst_cap, size_t *out_len);
int zipc_hip_gzip_size(zipc_hip_ctx *ctx, const void *src, size_t len, size_t *out_len, size_t *src_used,
                       size_t *n_members);
int zipc_hip_gzip_decompress(zipc_hip_ctx *ctx, const void *src, size_t len, void *dst, size_t dst_cap,
                             size_t *out_len, size_t *src_used, size_t *n_members, uint32_t *crc_found);

/* Decode into ONE arena laid out on the device: size-then-decode (above) as one call, for a batch that is on the device
 * and whose caller has no destinations of their own.  The call sizes every stream, lays the outputs end to end in
 * d_dst_arena, decodes them there and says where each one went; nothing is read back for the layout.  All pointers are
 * DEVICE pointers.  Of a descriptor src_off, src_len, limit and flags are read; dst_off and dst_cap are not looked at, as
 * in the sizing forms.  The two arenas must not overlap.
 * The layout rule (csrc/packed_layout.h):
 *   - a stream TAKES ROOM iff it is sized ZIPC_HIP_OK (the sizing forms' checks of flags and src_len included) and its
 *     size is at most max_out_len.  A stream sized above max_out_len reports ZIPC_HIP_ERR_INVALID_ARG, one that is not
 *     sized OK that status; neither takes room, both report out_len 0 and dst_off 0.
 *   - the streams that take room lie in index order: dst_off[i] = the sum over the roomed streams j < i of
 *     align_up(out_len[j], align).  align: a power of two in 1..4096.  Every sum is 64-bit.  Padding is never written.
 *   - a roomed stream FITS iff dst_off[i] + out_len[i] <= dst_arena_len.  One that does not reports
 *     ZIPC_HIP_ERR_DST_TOO_SMALL with out_len 0 and the dst_off the rule gave it; nothing of it is decoded, and nothing
 *     is written at or behind dst_arena_len.
 *   - d_need[0], if d_need is given, receives the end (dst_off + out_len) of the last roomed stream, whether it fit or
 *     not, and 0 if no stream took room: the arena length with which every roomed stream fits.  A caller that came up
 *     short retries once with exactly that.
 * The defining property: a roomed stream that fits gets status, checksum, out_len and the bytes in the arena that
 * zipc_hip_inflate_batch gives for the same src_off, src_len, limit and flags with that dst_off, dst_cap = out_len and
 * this call's crc_op.
 * Launches: below max_out_len = 256 KiB the streams are sized by zipc_hip_inflate_size_batch's one launch and the whole
 * call is enqueued on the context's stream and never synchronised (a call of ONE stream: below 40 KiB, where
 * zipc_hip_inflate_batch's own block path begins for one stream); from 256 KiB on they are sized as
 * zipc_hip_inflate_size_blocks_batch sizes them and decoded as zipc_hip_inflate_batch decodes from there on, and the call
 * synchronises where those two do.  zipc_hip_last_size_blocks and zipc_hip_last_inflate_blocks say what they say after
 * those calls.
 * A null ctx, d_descs or d_results, a null d_dst_arena with dst_arena_len != 0, n_streams above 0x7FFFFFFF, an align that
 * is no power of two in 1..4096, max_out_len above ZIPC_HIP_MAX_STREAM_LEN (one stored stream beyond 4 GiB is not offered
 * here) or a crc_op outside the enum fails the call with ZIPC_HIP_ERR_INVALID_ARG.  n_streams == 0 is ZIPC_HIP_OK,
 * enqueues nothing and does not write d_need. */
typedef struct {            /* 32 bytes */
  uint32_t status;    /* ZIPC_HIP_OK or the stream's own error */
  uint32_t checksum;  /* per crc_op, as zipc_hip_inflate_batch reports it */
  uint64_t out_len;   /* decompressed bytes at dst_off; 0 unless OK */
  uint64_t dst_off;   /* where the stream's room begins in the destination arena; 0 if it was given none */
  uint64_t reserved;  /* 0 */
} zipc_hip_packed_result;
int zipc_hip_inflate_packed_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena, size_t dst_arena_len,
                                  const zipc_hip_stream_desc *d_descs, zipc_hip_packed_result *d_results,
                                  size_t n_streams, size_t max_out_len, size_t align, int crc_op,
                                  uint64_t *d_need /* may be NULL */);
/* The same for WHOLE zlib streams, through the container's open and close of zipc_hip_zlib_decompress_batch, with the
 * context's Adler-32 flavour: a stream that fails its header check (or is shorter than 6 bytes) reports that status and
 * takes no room; one that inflates to another Adler-32 than it says reports ZIPC_HIP_ERR_CHECKSUM with checksum = the
 * value FOUND, out_len 0 and the dst_off it was given -- its bytes were decoded. */
int zipc_hip_zlib_decompress_packed_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena, size_t dst_arena_len,
                                          const zipc_hip_stream_desc *d_descs, zipc_hip_packed_result *d_results,
                                          size_t n_streams, size_t max_out_len, size_t align,
                                          uint64_t *d_need /* may be NULL */);

/* Deflate into ONE arena laid out on the device: the counterpart of the packed decode forms above, for a batch that is on
 * the device and whose caller wants the compressed streams contiguous -- an archive's body, bytes for a wire, the input
 * of another kernel -- without reading n results back, laying offsets out on the host and running n copies.  All pointers
 * are DEVICE pointers.  Of a descriptor src_off, src_len and flags are read (flags as zipc_hip_deflate_batch, or for the
 * zlib form zipc_hip_zlib_compress_batch, treats them); dst_off and dst_cap are not looked at.  The two arenas must not
 * overlap.
 * Staging: nobody knows a deflate output's size in advance, so every stream is deflated into a staging slot in the
 * context's scratch -- zipc_hip_deflate_bound(src_len) bytes (the zlib form: zipc_hip_zlib_bound(src_len)), the slots on
 * 16-byte boundaries in index order, their offsets from a scan on the device -- and copied from there.  That scratch is
 * sized from n_streams and total_src_len alone: zipc_hip_deflate_packed_bound(n_streams, total_src_len, 16) bytes (the zlib
 * form: the zlib helper's) beside deflate's own, and 88 bytes per stream of descriptors, results and plan.
 * Declared sizes: zipc_hip_deflate_batch's device-side check of max_src_len and total_src_len applies, and the stage step
 * makes it itself before any slot is used (the slots are sized from it): if a stream is longer than max_src_len or the
 * sum of src_len exceeds total_src_len, EVERY result is ZIPC_HIP_ERR_INVALID_ARG with out_len 0 and dst_off 0, need is 0,
 * nothing is staged and nothing is written to the destination.  A descriptor with src_len above ZIPC_HIP_MAX_STREAM_LEN
 * counts in neither: it is ZIPC_HIP_ERR_INVALID_ARG in its own result only.
 * The layout rule (csrc/deflate_packed.h; the packed decode forms' rule with "deflated OK" in the place of "sized OK"):
 *   - a stream TAKES ROOM iff its deflate result is ZIPC_HIP_OK.  One that is not OK reports that status (with the
 *     checksum zipc_hip_deflate_batch reports beside it), out_len 0 and dst_off 0, and takes no room.
 *   - the streams that take room lie in index order: dst_off[i] = the sum over the roomed streams j < i of
 *     align_up(out_len[j], align).  align: a power of two in 1..4096.  Every sum is 64-bit.  Padding is never written.
 *   - a roomed stream FITS iff dst_off[i] + out_len[i] <= dst_arena_len.  One that does not reports
 *     ZIPC_HIP_ERR_DST_TOO_SMALL with out_len 0 and the dst_off the rule gave it; none of its bytes is written.  Its
 *     checksum is what zipc_hip_deflate_batch reports with that status: the CRC-32 of the source with
 *     ZIPC_HIP_CRC_CRC32, else 0.
 *   - d_need[0], if d_need is given, receives the end (dst_off + out_len) of the last roomed stream, whether it fit or
 *     not, and 0 if no stream took room: the arena length with which every roomed stream fits.
 * The suffix property: offsets never fall with the index and neither do the ends of the roomed streams, so the roomed
 * streams that do not fit are exactly those from the first one that does not fit onwards.  A caller that came up short
 * keeps every stream in front of that one and re-runs only the streams from it on, into an arena of need - its dst_off
 * bytes (its dst_off is a multiple of align, so the second call's offsets continue the first's): a retry of the whole
 * batch would cost a whole deflate, not a cheap sizing pass.
 * The defining property: a roomed stream that fits gets the status, checksum, out_len and the bytes at dst_off that
 * zipc_hip_deflate_batch (the zlib form: zipc_hip_zlib_compress_batch) gives for the same source, level and crc_op with
 * dst_cap equal to the bound.  Nothing is written in front of d_dst_arena, at or behind dst_arena_len, or outside
 * [dst_off, dst_off + out_len) of a stream that fits.
 * The bound helpers (host arithmetic only) return an arena length with which every stream fits:
 *     total_src_len + 6 * (total_src_len / 65534) + 14 * n_streams + (align - 1) * n_streams      (zlib: + 6 * n_streams)
 * which follows from zipc_hip_deflate_bound(len) = len + 6 * (len / 65534 + 1) + 8: the floors of the streams sum to at
 * most the floor of the total, and a stream's padding is below align.
 * Launches: a stage step (one workgroup: the check, the slots, the descriptors deflate runs with), zipc_hip_deflate_batch's
 * (zipc_hip_zlib_compress_batch's) own kernels over the slots, a layout step (one workgroup), a ragged device-to-device
 * copy by one workgroup per 32 KiB segment that exists on a grid of staging bytes / 32768 + n_streams, and a close, a lane
 * per stream.  The call is enqueued on the context's stream; it synchronises only where zipc_hip_deflate_batch does
 * (growing the context's scratch, and the check of a context's first batch).
 * A null ctx, d_descs or d_results, a null d_dst_arena with dst_arena_len != 0, n_streams above 0x7FFFFFFF, a copy grid
 * bound above 0x7FFFFFFF, an align that is no power of two in 1..4096, a level outside 0..3, a crc_op outside the enum or
 * max_src_len above ZIPC_HIP_MAX_STREAM_LEN fails the call with ZIPC_HIP_ERR_INVALID_ARG.  n_streams == 0 is ZIPC_HIP_OK,
 * enqueues nothing and does not write d_need. */
size_t zipc_hip_deflate_packed_bound(size_t n_streams, size_t total_src_len, size_t align);
size_t zipc_hip_zlib_compress_packed_bound(size_t n_streams, size_t total_src_len, size_t align);
int zipc_hip_deflate_packed_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena, size_t dst_arena_len,
                                  const zipc_hip_stream_desc *d_descs, zipc_hip_packed_result *d_results,
                                  size_t n_streams, size_t max_src_len, size_t total_src_len, int level, int crc_op,
                                  size_t align, uint64_t *d_need /* may be NULL */);
/* The same with every stream a WHOLE zlib stream in the arena (the container's open and close of
 * zipc_hip_zlib_compress_batch around the slots, the context's Adler-32 flavour): out_len counts the six container
 * bytes, checksum is the Adler-32, and a flag bit other than ZIPC_HIP_STREAM_HAS_LIMIT is ZIPC_HIP_ERR_INVALID_ARG in
 * the stream's own result. */
int zipc_hip_zlib_compress_packed_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena, size_t dst_arena_len,
                                        const zipc_hip_stream_desc *d_descs, zipc_hip_packed_result *d_results,
                                        size_t n_streams, size_t max_src_len, size_t total_src_len, int level,
                                        size_t align, uint64_t *d_need /* may be NULL */);

/* Recode on the device: every stream of the source arena -- a raw deflate stream, a ZIP member's bytes -- is inflated
 * into its room in a MIDDLE arena, its CRC-32 taken there and compared where the descriptor expects one, and what it
 * inflated to is deflated at `level` into its destination slot: Zipc_deflate.inflate_and_crc_32, Crc_32.check and
 * Zipc_deflate.deflate of every member (the reference's `recode`, test/zipc_tool.ml:437-545) in one call, with nothing
 * read back in between and the decompressed bytes never leaving the device.  The codec's kernels are the ones of the
 * two batch forms above, between three small ones, a lane per stream (csrc/recode.hip, rules: csrc/recode_rules.h):
 *   open: a flag bit other than ZIPC_HIP_STREAM_HAS_LIMIT and ZIPC_HIP_STREAM_EXPECT_CRC32, or mid_cap above the call's
 *     max_mid_cap, is ZIPC_HIP_ERR_INVALID_ARG at stage 0 and nothing of the stream is read or written;
 *   link: a stream inflate refused stops with inflate's status at stage 1; one whose CRC-32 is not expect_crc32 stops
 *     with ZIPC_HIP_ERR_CHECKSUM at stage 2, checksum = the value FOUND;
 *   close: deflate's status (ZIPC_HIP_ERR_DST_TOO_SMALL, or the batch-wide ZIPC_HIP_ERR_INVALID_ARG of its declared
 *     sizes) at stage 3, or ZIPC_HIP_OK with the recoded length.
 * The CRC-32 is taken once, over inflate's output; it is the CRC-32 the recoded member has. */
#define ZIPC_HIP_STREAM_EXPECT_CRC32 2u
typedef struct {            /* 64 bytes */
  uint64_t src_off, src_len;   /* the deflate stream, in the source arena */
  uint64_t mid_off, mid_cap;   /* room for its decompressed bytes, in the middle arena */
  uint64_t dst_off, dst_cap;   /* room for the recoded stream, in the destination arena */
  uint64_t limit;              /* ?decompressed_size when flags & ZIPC_HIP_STREAM_HAS_LIMIT */
  uint32_t flags;
  uint32_t expect_crc32;       /* compared when flags & ZIPC_HIP_STREAM_EXPECT_CRC32 */
} zipc_hip_recode_desc;
typedef struct {            /* 32 bytes */
  uint32_t status;    /* ZIPC_HIP_OK or the failing step's status */
  uint32_t checksum;  /* CRC-32 of the decompressed bytes (stage 2, 3 and OK); else 0 */
  uint64_t out_len;   /* bytes of the recoded stream at dst_off; 0 unless OK */
  uint64_t mid_len;   /* decompressed length; 0 at stage 0 and 1 */
  uint32_t stage;     /* 0 OK or refused before any work, 1 inflate, 2 CRC check, 3 deflate */
  uint32_t reserved;  /* 0 */
} zipc_hip_recode_result;
/* All pointers are DEVICE pointers.  The work is enqueued on the context's stream and not synchronised, except where
 * zipc_hip_inflate_batch itself synchronises (max_mid_cap of 256 KiB and more).  max_mid_cap: upper bound of mid_cap
 * over the batch; total_mid_cap: their sum -- inflate's max_dst_cap and deflate's max_src_len / total_src_len, whose
 * device-side check of the declared sizes applies unchanged (if it trips, the streams that got as far as deflate report
 * its ZIPC_HIP_ERR_INVALID_ARG at stage 3).  level outside 0..3, or max_mid_cap above ZIPC_HIP_MAX_STREAM_LEN (one
 * stream's included: inflate's path for stored streams beyond 4 GiB has nothing deflate could take), fails the call
 * with ZIPC_HIP_ERR_INVALID_ARG.  Nothing is written behind any stream's dst_cap or mid_cap, and nothing to the
 * destination slot of a stream that stops at stage 0, 1 or 2; one that stops at stage 3 did not fit by the dst_cap rule
 * stated at zipc_hip_deflate_batch, and has what that call leaves of such a stream: nothing of the block that did not fit
 * nor of those behind it (of a stream of one block: nothing).
 * The defining property: for every stream, the result and the destination bytes are what the caller gets from
 * zipc_hip_inflate_batch (ZIPC_HIP_CRC_CRC32) into the middle arena, the link rule above applied on the host, and
 * zipc_hip_deflate_batch (level, ZIPC_HIP_CRC_NOP) of the streams that go on. */
int zipc_hip_recode_batch(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_mid_arena, void *d_dst_arena,
                          const zipc_hip_recode_desc *d_descs, zipc_hip_recode_result *d_results,
                          size_t n_streams, size_t max_mid_cap, size_t total_mid_cap, int level);
/* The same for streams held in HOST memory, through the pipeline of zipc_hip_inflate_many / _deflate_many (gather, copy
 * in, kernels, copy back end to end, scatter): stream i is src[i][0 .. src_len[i]), recoded into dst[i] (capacity
 * dst_cap[i]; zipc_hip_deflate_bound(mid_cap[i]) always fits), with mid_cap[i] bytes of room for its decompressed bytes
 * in a middle arena the context keeps on the device, sized to the largest sub-batch.  What crosses the bus is the old
 * stream on the way in and the new one on the way back.  limit may be NULL (no ?decompressed_size for any stream: a
 * stream that inflates to more than mid_cap[i] reports ZIPC_HIP_ERR_DST_TOO_SMALL at stage 1), expect_crc32 may be NULL
 * (no stream's CRC-32 is compared).  Like the other _many forms: results[] (host memory) is defined on every return,
 * bad arguments included -- the streams of sub-batches that had come back keep their results, every other one carries
 * the call's status at stage 0 -- and no C++ exception crosses the boundary. */
int zipc_hip_recode_many(zipc_hip_ctx *ctx, size_t n, const void *const *src, const size_t *src_len,
                         const size_t *limit /* may be NULL */, const uint32_t *expect_crc32 /* may be NULL */,
                         const size_t *mid_cap, int level, void *const *dst, const size_t *dst_cap,
                         zipc_hip_recode_result *results);

/* CRC-32 and Adler-32 of one device buffer (Crc_32.string + Adler_32.string).  Both asked for: ONE pass over the bytes
 * leaves the CRC-32 partials and the Adler-32 chunk sums (len bytes of traffic), then the two short finishes.  d_out receives {crc32, adler32}.  Either selector may be 0 to
 * skip that checksum. */
int zipc_hip_checksum_device(zipc_hip_ctx *ctx, const void *d_buf, size_t len,
                             int want_crc32, int want_adler32, uint32_t *d_out);

/* CRC-32 and Adler-32 of MANY ranges of one device arena per call, ragged: range i is d_arena[off, off + len).  All
 * pointers are device pointers; the work is enqueued on the context's stream and not synchronised (growing the
 * context's scratch may synchronise, as everywhere), and nothing is read back.
 * For every OK range, crc32 and adler32 are what zipc_hip_checksum_device gives for the same bytes with the same
 * context flavour (zipc_hip_set_adler_rfc1950); an empty range gives crc32 = 0, adler32 = 1; a checksum not asked for
 * is 0.  Ranges may overlap, repeat, touch, be empty, start at any byte and be of any length the arena holds (no 4 GiB
 * limit per range).  A range that lies outside [0, arena_len), or whose end overflows 64 bits, reports
 * ZIPC_HIP_ERR_INVALID_ARG in its own result with both checksums 0, and none of its bytes is read.
 * total_len: the sum of len over the call, an upper bound.  It sizes grids and scratch and is checked on the device: if
 * the OK ranges sum to more, EVERY result is ZIPC_HIP_ERR_INVALID_ARG and no byte of the arena is read.
 * The call itself fails with ZIPC_HIP_ERR_INVALID_ARG for a null ctx / d_ranges / d_results, a null d_arena with
 * arena_len > 0, both selectors 0, or where n_ranges or total_len / 32768 + n_ranges exceeds 0x7FFFFFFF;
 * n_ranges == 0 is OK and enqueues nothing.
 * The work is one pass over the ranges' bytes by one workgroup per 32 KiB segment THAT EXISTS (a grid of
 * total_len / 32768 + n_ranges workgroups, whatever the longest range), between a plan and two finishes: four kernel
 * launches whatever n_ranges is.  Scratch, all in the context and sized from the declared numbers alone:
 * total_len / 32768 + n_ranges words of CRC partials, total_len / 5552 + n_ranges pairs of Adler-32 chunk sums (zeroed
 * per call), 12 bytes per range of plan (csrc/checksum_ranges.h has every rule). */
typedef struct { uint64_t off, len; } zipc_hip_range;                                   /* 16 bytes */
typedef struct { uint32_t status, crc32, adler32, reserved; } zipc_hip_checksum_result; /* 16 bytes */
int zipc_hip_checksum_batch(zipc_hip_ctx *ctx, const void *d_arena, size_t arena_len,
                            const zipc_hip_range *d_ranges, zipc_hip_checksum_result *d_results,
                            size_t n_ranges, size_t total_len, int want_crc32, int want_adler32);
/* The same for streams held in HOST memory, through the pipeline of the other _many forms (gather into pinned memory,
 * copy in, kernels, results back) with nothing but the 16-byte results coming back: results[i] is the result of
 * src[i][0 .. src_len[i]).  Like the other _many forms: results[] (host memory) is defined on every return, bad
 * arguments included (every entry then carries the call's status and no checksum), and no C++ exception crosses the
 * boundary.  The call fails with ZIPC_HIP_ERR_INVALID_ARG for a null src[i] with src_len[i] > 0 or both selectors 0. */
int zipc_hip_checksum_many(zipc_hip_ctx *ctx, size_t n, const void *const *src, const size_t *src_len,
                           int want_crc32, int want_adler32, zipc_hip_checksum_result *results);

/* Tests only: the hash-chain links (zipc_deflate.ml:1150-1152, insert_hash: per position the distance to the previous
 * position of equal hash, 0 beyond 32768) of a batch of device-resident streams as ONE of the library's two chain
 * kernels makes them -- which = 0: by ordered LDS exchange (ZIPC_HIP_ERR_HIP where the context's probe failed), 1: by
 * the kernel that orders equal hashes itself -- copied to d_links (links_cap 16-bit slots, at least
 * zipc_hip_debug_chain_positions(n_streams, total_src_len); slots no kernel writes are zero) with every stream's first
 * slot in d_pos_base (n_streams 64-bit words, may be null).  The batch must fit one pass (8 GiB of source).  The
 * suite requires the two kernels' links to be equal over the benchmark's whole batches (tests/test_gpu_limits.py). */
size_t zipc_hip_debug_chain_positions(size_t n_streams, size_t total_src_len);
int zipc_hip_debug_chain_links(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs,
                               size_t n_streams, size_t max_src_len, size_t total_src_len, int which, void *d_links,
                               size_t links_cap, void *d_pos_base);
/* Tests only: the same links as ANY of the four chain forms makes them, launched by the pipeline's own launch site.
 * chain (csrc/forms.h ChainKernel): 0 ordered LDS exchange, a workgroup per stream; 1 the same by segments of a stream;
 * 2 the kernel that orders equal hashes itself, a workgroup per stream; 3 the same by segments.  seg_positions, for the
 * two forms by segments: 0 for the segment size a deflate call of this shape gets (whole streams where it gets no
 * segments), else one of the sizes the launch rules can produce -- 32768, 65536 or 131072 for chain 3, 98304 << k for
 * chain 1; anything else is ZIPC_HIP_ERR_INVALID_ARG.  The whole-stream forms ignore it.  chain 0 or 1 on a context whose
 * probe failed reports ZIPC_HIP_ERR_HIP.  d_links, links_cap and d_pos_base as above, but every slot is filled with
 * ZIPC_HIP_DEBUG_LINK_POISON before the kernels run: no link exceeds 32768, so a slot nobody wrote shows.
 * tests/test_gpu_chain_links.py holds every link of every form to a serial insert_hash. */
#define ZIPC_HIP_DEBUG_LINK_POISON 0xFFFFu
int zipc_hip_debug_chain_links_form(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs,
                                    size_t n_streams, size_t max_src_len, size_t total_src_len, int chain,
                                    size_t seg_positions, void *d_links, size_t links_cap, void *d_pos_base);

/* Tests only: the match finder's tables of a batch of device-resident streams.  Runs deflate_offsets, lz_chain (the
 * kernel that orders equal hashes itself) and lz_match and nothing else, lz_match launched exactly as a deflate call of
 * this shape at `level` (1..3) launches it, but with match_form (0: the walk chosen per tile, 1 / 2: always the first /
 * second form) and tiles_per_group (0: by the grid) in place of ZIPC_HIP_MATCH_FORM and ZIPC_HIP_MATCH_TILES_PER_GROUP,
 * which are read once per process.  Copied out: d_match and d_snap (records_cap 32-bit slots each, at least
 * zipc_hip_debug_chain_positions(n_streams, total_src_len)), d_snap_used (n_streams 32-bit words) and d_pos_base
 * (n_streams 64-bit words: every stream's first slot).  Position p of stream i is slot pos_base[i] + p: match holds the
 * best of the first K chain candidates as dist << 9 | len (0: none), with bit 31 set where the best of the first K / 4
 * is another one, which is then in snap; snap_used[i] is 1 iff stream i has such a position.  Both tables are filled
 * with ZIPC_HIP_DEBUG_MATCH_POISON before the kernels run, so a slot nobody wrote shows.  The batch must fit one pass
 * (8 GiB of source).  tests/test_gpu_match_records.py holds every record to a serial find_backref. */
#define ZIPC_HIP_DEBUG_MATCH_POISON 0x5A5A5A5Au
int zipc_hip_debug_match_records(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs,
                                 size_t n_streams, size_t max_src_len, size_t total_src_len, int level, int match_form,
                                 long tiles_per_group, void *d_match, void *d_snap, size_t records_cap, void *d_snap_used,
                                 void *d_pos_base);

/* Tests only: zipc_hip_inflate_batch (no checksum) with the second half of the block path laid open.  Every stream that
 * passes the length, capacity and 64x conditions of the block path is handed to it -- the cost rule that picks the k
 * longest is the one thing bypassed; the call's gate (max_dst_cap) and ZIPC_HIP_INFLATE_BLOCKS hold as ever -- and the
 * token run is launched by the pipeline's own launch site with
 *   form   0: a wave per interval, the span decoder writing a match byte's source down as it is; 1: a wave per block, the span
 *          decoder following sources as far as they are known (`follow`).  In BOTH forms the wide turn's store and wave_match
 *          look the source's own word up, so a raw word is the byte's source or an earlier byte of the same chain of copies;
 *          -1: whichever the call's own rule gives the stream;
 *   hops0, hops1   the links a thread follows in the first / a later resolve round, 0: the tuning value; the number of
 *          rounds follows from them as in the ordinary call.
 * Anything else (form outside -1..1, hops outside 0..65536) is ZIPC_HIP_ERR_INVALID_ARG.
 * d_tok_raw, d_tok_done: device arrays of as many 32-bit words as the destination arena has bytes.  The words of a
 * stream that went into the token run lie at [dst_off, dst_off + out_len): tok[] copied once behind the token run (raw)
 * and once behind the last resolve round (done) -- word i is the stream's output position byte i is a copy of, i
 * itself for a literal.  No other word is touched.
 * records: n_streams entries of HOST memory, one per stream.
 * Behind the captures the call goes on as zipc_hip_inflate_batch does: gather, results, the one waves for every stream
 * not done; status, length and bytes of every stream are the ordinary call's.
 * tests/test_gpu_inflate_tokens.py holds every word to a serial decode. */
#define ZIPC_HIP_DEBUG_TOKEN_ROUNDS 12
typedef struct zipc_hip_debug_token_record {
  uint32_t taken;        /* 1: the stream went into the token run (everything below is 0 otherwise) */
  int32_t form;          /* the form it ran in: 0 or 1 */
  uint32_t n_blocks;     /* blocks of its chain */
  uint32_t n_intervals;  /* intervals of those blocks (form 0: waves of the token run) */
  uint32_t token_bad;    /* waves that did not end as the dry run said */
  uint32_t rounds;       /* resolve rounds launched */
  uint32_t more[ZIPC_HIP_DEBUG_TOKEN_ROUNDS]; /* more[r], r < rounds: bytes round r left short of a literal */
  uint32_t blocks_done;  /* 1: the block path's output stands; 0: left to the stream's one wave */
  uint32_t reserved;
} zipc_hip_debug_token_record;
int zipc_hip_debug_inflate_tokens(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_dst_arena,
                                  const zipc_hip_stream_desc *d_descs, zipc_hip_stream_result *d_results,
                                  size_t n_streams, size_t max_dst_cap, int form, int hops0, int hops1, void *d_tok_raw,
                                  void *d_tok_done, zipc_hip_debug_token_record *records);

/* grow the context scratch up front (keeps hipMalloc out of timed regions) */
int zipc_hip_reserve(zipc_hip_ctx *ctx, size_t n_streams, size_t max_src_len,
                     size_t total_src_len);

#ifdef __cplusplus
}
#endif
#endif
