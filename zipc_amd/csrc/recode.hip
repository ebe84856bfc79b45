// recode.hip -- a batch of device-resident deflate streams recoded in place on the device (zipc_hip_recode_batch and
// the kernels' step of zipc_hip_recode_many): inflate, the CRC-32 check and deflate of every stream with nothing read
// back between them.
//
// Three kernels around the codec's and the checksum's, a lane per stream each; none of them touches a stream's bytes:
//   recode_open_kernel   reads a stream's descriptor, applies the call's checks and writes the descriptor inflate is to
//                        run with -- the stream into its room in the middle arena -- with the verdict so far;
//   recode_link_kernel   reads inflate's result (the CRC-32 pass has been over it), compares the CRC-32 where one is
//                        expected, and writes the descriptor deflate is to run with: the bytes inflate left, as many as
//                        it said, into the caller's destination slot;
//   recode_close_kernel  puts the verdict and deflate's result together into the caller's result.
// Inner descriptors, inner results and verdicts live in the context's scratch (launch_recode below, the one way to the
// kernels: ctx.h).  The rules themselves are recode_rules.h's (the host form and the tests compile the same functions).
#include "ctx.h"
#include "recode_rules.h"

namespace zd {

__global__ __launch_bounds__(256) void recode_open_kernel(const RecodeDesc *__restrict__ descs, uint32_t n_streams, uint64_t max_mid_cap,
                                                          StreamDesc *__restrict__ inner, RecodeVerdict *__restrict__ verdicts) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_streams) return;
  StreamDesc in;
  verdicts[i] = recode_open(descs[i], max_mid_cap, &in);
  inner[i] = in;
}

__global__ __launch_bounds__(256) void recode_link_kernel(const RecodeDesc *__restrict__ descs, uint32_t n_streams,
                                                          const StreamResult *__restrict__ inflated, StreamDesc *__restrict__ inner,
                                                          RecodeVerdict *__restrict__ verdicts) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_streams) return;
  StreamDesc in;
  verdicts[i] = recode_link(descs[i], verdicts[i], inflated[i], &in);
  inner[i] = in;
}

// plain: null, or where the many-stream pipeline reads {status, checksum, out_len} of every stream (many.hip pack_offsets_kernel)
__global__ __launch_bounds__(256) void recode_close_kernel(uint32_t n_streams, const RecodeVerdict *__restrict__ verdicts,
                                                           const StreamResult *__restrict__ deflated, RecodeResult *__restrict__ results,
                                                           StreamResult *__restrict__ plain) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_streams) return;
  const RecodeResult r = recode_close(verdicts[i], deflated[i]);
  results[i] = r;
  if (plain) plain[i] = recode_plain_result(r);
}

// The context's scratch of a recode of n streams: the descriptors the codec runs with, its results, the verdicts.
int recode_reserve(zipc_hip_ctx *ctx, size_t n) {
  HIP_TRY(ctx, ctx->ensure(ctx->recode_descs, n * sizeof(StreamDesc)));
  HIP_TRY(ctx, ctx->ensure(ctx->recode_res, n * sizeof(StreamResult)));
  HIP_TRY(ctx, ctx->ensure(ctx->recode_verdicts, n * sizeof(RecodeVerdict)));
  return ZIPC_HIP_OK;
}
// open -> inflate with its CRC-32 pass -> link -> deflate out of the middle arena -> close, all on the context's stream.
// d_plain: null, or n StreamResults for the many-stream pipeline; h_inflate_descs: null, or the host's own copy of what
// recode_open makes of the descriptors (launch_inflate's h_descs); first_of_call: launch_inflate's.
int launch_recode(zipc_hip_ctx *ctx, const void *d_src_arena, void *d_mid_arena, void *d_dst_arena, const RecodeDesc *d_descs,
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

}  // namespace zd
