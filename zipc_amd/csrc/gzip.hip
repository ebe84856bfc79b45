// gzip.hip -- the gzip container of a batch of device-resident members (zipc_hip_gzip_decompress_batch / _size_batch /
// _size_blocks_batch / _compress_batch).
//
// Three kernels around the codec's, a lane per member each; they keep no logic of their own:
//   gzip_open_kernel            reads a member's descriptor (and, to decompress, its header), applies gzip_container.h's
//                               checks and writes the descriptor the codec is to run with -- the body behind the header, an
//                               upper bound, or the room behind the header to be -- into the context's scratch, with the
//                               header's verdict, length and FLG;
//   gzip_close_extent_kernel    puts that verdict and the extent decoder's record together (gzip_close): the trailer found
//                               behind the body's extent, the CRC-32 compared (decode) or not (size), ISIZE compared;
//   gzip_close_compress_kernel  stores the header, BSIZE where asked, and the trailer around what deflate wrote.
// Nothing is read back: the calls enqueue and return like the raw batch forms.  The launches at the end of this file are
// the one way to the kernels (ctx.h).
#include "ctx.h"
#include "gzip_container.h"

namespace zd {

// A member the codec is not to touch: nothing to read, no room to write (zlib.hip zlib_no_stream: inflate reports a
// corrupted stream for it, deflate a destination too small, neither stores a byte; the close puts the container's verdict
// in its place).
__device__ __forceinline__ StreamDesc gzip_no_stream(const StreamDesc &sd) {
  StreamDesc in = sd;
  in.src_len = 0;
  in.dst_cap = 0;
  in.flags = 0;
  return in;
}

__global__ __launch_bounds__(256) void gzip_open_kernel(const uint8_t *__restrict__ src_arena, const StreamDesc *__restrict__ descs,
                                                        uint32_t n_streams, int compress, int flavour, StreamDesc *__restrict__ inner,
                                                        GzipPre *__restrict__ pre) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_streams) return;
  const StreamDesc sd = descs[i];
  GzipPre p;
  p.status = ST_OK; p.hdr_len = 0; p.flg = 0;
  StreamDesc in = sd;
  if ((sd.flags & ~STREAM_HAS_LIMIT) != 0 || (!compress && sd.src_len > MAX_STREAM_LEN)) {
    p.status = ST_INVALID_ARG;
  } else if (compress) {
    p.status = gzip_open_compress_status(sd.dst_cap, flavour);
    if (p.status == ST_OK) {
      in.dst_off = gzip_payload_off(sd.dst_off, flavour);
      in.dst_cap = gzip_payload_cap(sd.dst_cap, flavour);
    }
  } else {
    const GzipHeader h = gzip_parse_header(src_arena + sd.src_off, sd.src_len);  // (reads inside [src_off, src_off + src_len) alone)
    p.status = h.status;
    if (h.status == ST_OK) {
      p.hdr_len = h.hdr_len; p.flg = h.flg;
      in.src_off = gzip_body_off(sd.src_off, h.hdr_len);
      in.src_len = gzip_body_len(sd.src_len, h.hdr_len);
    }
  }
  if (p.status != ST_OK) in = gzip_no_stream(sd);
  inner[i] = in;
  pre[i] = p;
}

// The closes of the decode form (compare_crc) and of the two sizing forms: d_descs are the caller's, the trailer is read
// from the source arena at hdr_len + the body's extent, if it lies inside the declared bytes (gzip_container.h gzip_close).
__global__ __launch_bounds__(256) void gzip_close_extent_kernel(const uint8_t *__restrict__ src_arena, const StreamDesc *__restrict__ descs,
                                                                const GzipPre *__restrict__ pre, GzipResult *__restrict__ results,
                                                                uint32_t n_streams, int compare_crc) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_streams) return;
  const GzipPre p = pre[i];
  const ExtentResult inner = ((const ExtentResult *)results)[i];  // (the extent kernels wrote the records in place: same 32 bytes)
  results[i] = gzip_close(p.status, descs[i].src_len, src_arena + descs[i].src_off, p.hdr_len, p.flg, inner, compare_crc != 0);
}

__global__ __launch_bounds__(256) void gzip_close_compress_kernel(uint8_t *__restrict__ dst_arena, const StreamDesc *__restrict__ descs,
                                                                  const GzipPre *__restrict__ pre, StreamResult *__restrict__ results,
                                                                  uint32_t n_streams, int level, int flavour) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_streams) return;
  const StreamResult inner = results[i];
  bool wrap;
  const StreamResult r = gzip_close_compress(pre[i].status, inner, flavour, &wrap);
  if (wrap) {  // (inner.out_len <= gzip_payload_cap: deflate said its bytes fit, so header, payload and trailer lie inside dst_cap)
    uint8_t *o = dst_arena + descs[i].dst_off;
    gzip_put_header(o, level, flavour, r.out_len);
    gzip_put_trailer(o + gzip_header_len(flavour) + inner.out_len, inner.checksum, descs[i].src_len);
  }
  results[i] = r;
}

// gzip_open_kernel over the caller's descriptors: the codec's descriptors and the headers' verdicts, in the context's scratch
int launch_gzip_open(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs, size_t n, int compress, int flavour) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, ctx->ensure(ctx->gzip_descs, n * sizeof(StreamDesc)));
  HIP_TRY(ctx, ctx->ensure(ctx->gzip_pre, n * sizeof(GzipPre)));
  ZD_LAUNCH(ctx, "gzip_open", gzip_open_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (const uint8_t *)d_src_arena,
            (const StreamDesc *)d_descs, (uint32_t)n, compress, flavour, (StreamDesc *)ctx->gzip_descs.p, (GzipPre *)ctx->gzip_pre.p);
  HIP_TRY(ctx, hipGetLastError());
  return ZIPC_HIP_OK;
}
int launch_gzip_close_extent(zipc_hip_ctx *ctx, const void *d_src_arena, const zipc_hip_stream_desc *d_descs, zipc_hip_gzip_result *d_results,
                             size_t n, int compare_crc) {
  ZD_LAUNCH(ctx, "gzip_close_extent", gzip_close_extent_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (const uint8_t *)d_src_arena,
            (const StreamDesc *)d_descs, (const GzipPre *)ctx->gzip_pre.p, (GzipResult *)d_results, (uint32_t)n, compare_crc);
  HIP_TRY(ctx, hipGetLastError());
  return ZIPC_HIP_OK;
}
int launch_gzip_close_compress(zipc_hip_ctx *ctx, void *d_dst_arena, const zipc_hip_stream_desc *d_descs, zipc_hip_stream_result *d_results,
                               size_t n, int level, int flavour) {
  ZD_LAUNCH(ctx, "gzip_close_compress", gzip_close_compress_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (uint8_t *)d_dst_arena,
            (const StreamDesc *)d_descs, (const GzipPre *)ctx->gzip_pre.p, (StreamResult *)d_results, (uint32_t)n, level, flavour);
  HIP_TRY(ctx, hipGetLastError());
  return ZIPC_HIP_OK;
}

}  // namespace zd
