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
// Inner descriptors, inner results and verdicts live in the context's scratch (api.hip recode_sequence).  The rules
// themselves are recode_rules.h's (the host form and the tests compile the same functions).
#include "kernels.h"
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

// plain: null, or where the many-stream pipeline reads {status, checksum, out_len} of every stream (api.hip pack_offsets_kernel)
__global__ __launch_bounds__(256) void recode_close_kernel(uint32_t n_streams, const RecodeVerdict *__restrict__ verdicts,
                                                           const StreamResult *__restrict__ deflated, RecodeResult *__restrict__ results,
                                                           StreamResult *__restrict__ plain) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_streams) return;
  const RecodeResult r = recode_close(verdicts[i], deflated[i]);
  results[i] = r;
  if (plain) plain[i] = recode_plain_result(r);
}

}  // namespace zd
