// sim_gzip.cpp -- the gzip forms on the CPU (zipc_hip_gzip_decompress_batch, _size_batch, _compress_batch, and the host
// forms' plan): gzip_container.h's rules around the extent model of tests/extent_sim/sim_extent.cpp -- inflate_lane.h's
// plain lane step run serially -- compiled with g++ for tests/test_gzip_rules.py.  One member: gzip_parse_header as
// gzip.hip's open kernel applies it, the body [hdr_len, src_len) through raw_extent, then gzip_close.  The CRC-32 of the
// output is not this model's subject (the checksum tests'): the caller hands it in.  The compress side is the rules
// around deflate's bytes, which the caller hands in too (the oracle's, by deflate's own capacity rule).
// Nothing is read outside [src, src + src_len) or written outside [dst, dst + dst_cap).  Test tooling only.
#include "../extent_sim/sim_extent.cpp"
#include "../../zipc_amd/csrc/gzip_container.h"

// form: 0 decode, 1 size.  crc: the CRC-32 of the bytes the body inflates to.  out: status, checksum, out_len, src_used,
// hdr_len, flg.
extern "C" void sim_gzip(const uint8_t *src, uint64_t src_len, uint8_t *dst, uint64_t dst_cap, int has_limit, uint64_t limit,
                         uint32_t flags_extra, int form, uint32_t crc, int budget, uint64_t *out) {
  const bool size = form != 0;
  GzipResult r;
  if (flags_extra != 0 || src_len > MAX_STREAM_LEN) {
    r = gzip_refusal(ST_INVALID_ARG, 0);  // (gzip.hip gzip_open_kernel)
  } else {
    const GzipHeader h = gzip_parse_header(src, src_len);
    ExtentResult inner = extent_result(ST_CORRUPTED, 0, 0, 0);  // (gzip_no_stream: inflate of nothing)
    if (h.status == ST_OK)
      inner = raw_extent(src + gzip_body_off(0, h.hdr_len), gzip_body_len(src_len, h.hdr_len), dst, dst_cap, has_limit, limit, 0, size,
                         size ? 0u : crc, budget);
    r = gzip_close(h.status, src_len, src, h.hdr_len, h.flg, inner, !size);
  }
  out[0] = r.status; out[1] = r.checksum; out[2] = r.out_len; out[3] = r.src_used; out[4] = r.hdr_len; out[5] = r.flg;
}

extern "C" void sim_gzip_header(const uint8_t *src, uint64_t src_len, uint32_t *out) {
  const GzipHeader h = gzip_parse_header(src, src_len);
  out[0] = h.status; out[1] = h.hdr_len; out[2] = h.flg; out[3] = h.bsize;
}

// the compress form's open: out = the verdict, where deflate's bytes go in a destination at 0, how many there may be
extern "C" void sim_gzip_open_compress(uint64_t dst_cap, int flavour, uint64_t *out) {
  out[0] = gzip_open_compress_status(dst_cap, flavour);
  out[1] = out[2] = 0;
  if (out[0] == ST_OK) { out[1] = gzip_payload_off(0, flavour); out[2] = gzip_payload_cap(dst_cap, flavour); }
}
// ... and its close over deflate's result (inner_status, the CRC-32 of the source, n_body bytes at body): the member in dst
// (of dst_cap bytes), out = status, checksum, out_len
extern "C" void sim_gzip_close_compress(uint32_t pre, uint32_t inner_status, uint32_t crc, const uint8_t *body, uint64_t n_body, uint64_t src_len,
                                        int level, int flavour, uint8_t *dst, uint64_t *out) {
  StreamResult inner;
  inner.status = inner_status; inner.checksum = crc; inner.out_len = inner_status == ST_OK ? n_body : 0;
  if (pre == ST_OK && inner_status == ST_OK) memcpy(dst + gzip_payload_off(0, flavour), body, n_body);  // (what deflate wrote)
  bool wrap;
  const StreamResult r = gzip_close_compress(pre, inner, flavour, &wrap);
  if (wrap) {
    gzip_put_header(dst, level, flavour, r.out_len);
    gzip_put_trailer(dst + gzip_header_len(flavour) + inner.out_len, inner.checksum, src_len);
  }
  out[0] = r.status; out[1] = r.checksum; out[2] = r.out_len;
}
extern "C" unsigned long long sim_gzip_overhead(int flavour) { return gzip_overhead(flavour); }

// the host plan's step: out = status, end_of_members, known, hdr_len, flg, bsize, isize
extern "C" void sim_gzip_next(const uint8_t *file, uint64_t len, uint64_t off, uint32_t *out) {
  const GzipStep s = gzip_next(file, len, off);
  out[0] = s.status; out[1] = s.end_of_members; out[2] = s.known; out[3] = s.hdr_len; out[4] = s.flg; out[5] = s.bsize; out[6] = s.isize;
}
