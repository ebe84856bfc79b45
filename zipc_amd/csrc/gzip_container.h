// gzip_container.h -- the header and the eight trailer bytes RFC 1952 puts around a deflate stream: free of HIP.
//
// The reference has no gzip; the rules below are RFC 1952's, held to zlib's reading of it (Python's
// zlib.decompressobj(wbits=31)) for verdict and extent, and to the project's own decoder for the body.  They are pure
// functions of plain numbers and bytes, so the same code is compiled three times:
//   * into gzip.hip's three kernels (zipc_hip_gzip_*_batch: a lane per member opens and closes the container on the device);
//   * into the host forms (api.hip zipc_hip_gzip_compress / _size / _decompress, which plan a whole file with gzip_next);
//   * into tests/gzip_sim/sim_gzip.cpp with g++, where tests/test_gzip_rules.py holds the catalogue of tests/gzip_cases.py to them.
// A member's length is not known up front: src_len is an upper bound, the body handed to the codec is [hdr_len, src_len),
// and the trailer is found behind the body's extent (inflate_extent.h), as zlib_close_extent finds a zlib stream's.
// One limit is this library's own: a name or a comment is at most GZIP_MAX_TEXT bytes before its zero (zlib scans without
// bound); it keeps a lane's walk over a hostile member bounded.
#pragma once

#include "inflate_extent.h"
#include "zd_common.h"
#include "zlib_container.h"

namespace zd {

constexpr uint64_t GZIP_MIN_LEN = 18;        // ten header bytes and the eight of the trailer
constexpr uint64_t GZIP_MAX_TEXT = 65535;    // FNAME, FCOMMENT: bytes in front of the zero
constexpr uint64_t GZIP_BGZF_MAX = 65536;    // the longest member BSIZE can say
enum : uint32_t { GZIP_FTEXT = 1, GZIP_FHCRC = 2, GZIP_FEXTRA = 4, GZIP_FNAME = 8, GZIP_FCOMMENT = 16 };
enum : int { GZIP_PLAIN = 0, GZIP_BGZF = 1 };  // include/zipc_hip.h ZIPC_HIP_GZIP_*

// what gzip_parse_header says of a member: its verdict; on ST_OK where the body begins, FLG, and the member's whole length
// if an extra subfield 'B','C' says it (BGZF), else 0
struct GzipHeader { uint32_t status, hdr_len, flg, bsize; };
// what is kept of a member between open and close (gzip.hip's kernels)
struct GzipPre { uint32_t status, hdr_len, flg; };
// zipc_hip_gzip_result (include/zipc_hip.h): the layout of ExtentResult, the last word split
struct GzipResult {
  uint32_t status, checksum;
  uint64_t out_len, src_used;
  uint32_t hdr_len, flg;
};
static_assert(sizeof(GzipResult) == 32, "include/zipc_hip.h");

// a member that is refused: every field but the status (and, for ST_CHECKSUM, the value found) is 0
ZD_HD GzipResult gzip_refusal(uint32_t status, uint32_t found) {
  GzipResult r;
  r.status = status; r.checksum = found; r.out_len = 0; r.src_used = 0; r.hdr_len = 0; r.flg = 0;
  return r;
}

ZD_HD uint32_t gzip_u16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
ZD_HD uint32_t gzip_u32(const uint8_t *p) { return gzip_u16(p) | (gzip_u16(p + 2) << 16); }

// the CRC-32 of the n header bytes at s, bit by bit: no table, headers are short
ZD_HD uint32_t gzip_header_crc(const uint8_t *s, uint64_t n) {
  uint32_t c = 0xFFFFFFFFu;
  for (uint64_t i = 0; i < n; i++) {
    c ^= s[i];
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (CRC_POLY & (0u - (c & 1u)));
  }
  return ~c;
}

// The extra field's subfields, walked as SI1, SI2, SLEN, data: the first 'B','C' of SLEN 2 gives BSIZE + 1.  A subfield
// that overruns the field ends the walk: it is no error (zlib does not look either).
ZD_HD uint32_t gzip_bsize_of_extra(const uint8_t *x, uint64_t xlen) {
  uint64_t at = 0;
  while (at + 4 <= xlen) {
    const uint64_t slen = gzip_u16(x + at + 2);
    if (at + 4 + slen > xlen) break;
    if (x[at] == 'B' && x[at + 1] == 'C' && slen == 2) return gzip_u16(x + at + 4) + 1u;
    at += 4 + slen;
  }
  return 0;
}

// a zero-terminated field at s + pos: the zero is searched inside len and within GZIP_MAX_TEXT bytes -> the position
// behind the zero, or 0: there is none
ZD_HD uint64_t gzip_skip_text(const uint8_t *s, uint64_t len, uint64_t pos) {
  for (uint64_t n = 0; n <= GZIP_MAX_TEXT; n++) {
    if (pos + n >= len) return 0;
    if (s[pos + n] == 0) return pos + n + 1;
  }
  return 0;
}

// The header of the member in the `len` bytes at s (len: an upper bound of the member's length).  Every index is checked
// against len before it is read; the checks run in RFC 1952's field order.
ZD_HD GzipHeader gzip_parse_header(const uint8_t *s, uint64_t len) {
  GzipHeader h;
  h.status = ST_CORRUPTED; h.hdr_len = 0; h.flg = 0; h.bsize = 0;
  if (len < GZIP_MIN_LEN) return h;  // (nothing is read of a shorter one)
  if (s[0] != 0x1Fu || s[1] != 0x8Bu) return h;
  if (s[2] != 8u) { h.status = ST_ZLIB_METHOD; return h; }
  const uint32_t flg = s[3];
  if ((flg & 0xE0u) != 0) return h;  // (reserved bits; FTEXT says nothing a decoder needs)
  uint64_t pos = 10;                 // MTIME, XFL and OS are not looked at
  uint32_t bsize = 0;
  if (flg & GZIP_FEXTRA) {
    if (pos + 2 > len) return h;
    const uint64_t xlen = (uint64_t)s[pos] | ((uint64_t)s[pos + 1] << 8);
    pos += 2;
    if (pos + xlen > len) return h;
    bsize = gzip_bsize_of_extra(s + pos, xlen);
    pos += xlen;
  }
  if (flg & GZIP_FNAME) {
    pos = gzip_skip_text(s, len, pos);
    if (pos == 0) return h;
  }
  if (flg & GZIP_FCOMMENT) {
    pos = gzip_skip_text(s, len, pos);
    if (pos == 0) return h;
  }
  if (flg & GZIP_FHCRC) {  // the low 16 bits of the CRC-32 of every header byte in front of them
    if (pos + 2 > len) return h;
    if (((gzip_header_crc(s, pos) ^ gzip_u16(s + pos)) & 0xFFFFu) != 0) return h;
    pos += 2;
  }
  h.status = ST_OK; h.hdr_len = (uint32_t)pos; h.flg = flg; h.bsize = bsize;
  return h;
}

// what the codec is handed of a member at [off, off + len) whose header is hdr_len bytes: everything behind the header,
// an upper bound -- the extent decoder says where the body ends (hdr_len <= len: gzip_parse_header read that far)
ZD_HD uint64_t gzip_body_off(uint64_t off, uint32_t hdr_len) { return off + hdr_len; }
ZD_HD uint64_t gzip_body_len(uint64_t len, uint32_t hdr_len) { return len - hdr_len; }

// A member's result from the header's verdict (pre, with hdr_len and flg) and the extent decoder's record of the body
// (inner: u = inner.src_used bytes of body).  The trailer -- CRC32, then ISIZE, little-endian -- is the eight bytes at
// hdr_len + u of the member and has to lie inside the declared bytes, or the member is ST_CORRUPTED with nothing read.
// compare_crc: the decode forms, whose inner.checksum is the CRC-32 of the output; a mismatch reports the value FOUND and
// nothing else.  The sizing forms compare no CRC (there are no bytes to take it of) but hold the same bound and compare
// ISIZE, so a member they size OK has the src_used the decode forms report.  The CRC comes before ISIZE, as in zlib: a
// member with both wrong is ST_CHECKSUM.  `stream`: the member's first byte; only [hdr_len + u, hdr_len + u + 8) is read.
ZD_HD GzipResult gzip_close(uint32_t pre, uint64_t src_len, const uint8_t *stream, uint32_t hdr_len, uint32_t flg, ExtentResult inner,
                            bool compare_crc) {
  if (pre != ST_OK) return gzip_refusal(pre, 0);
  if (inner.status != ST_OK) return gzip_refusal(inner.status, 0);
  const uint64_t u = inner.src_used;
  if (hdr_len + u + 8u > src_len) return gzip_refusal(ST_CORRUPTED, 0);
  const uint8_t *trailer = stream + hdr_len + u;
  const uint32_t crc = gzip_u32(trailer), isize = gzip_u32(trailer + 4);
  const bool crc_bad = compare_crc && inner.checksum != crc;
  const bool isize_bad = isize != (uint32_t)inner.out_len;
  if (crc_bad) return gzip_refusal(ST_CHECKSUM, inner.checksum);
  if (isize_bad) return gzip_refusal(ST_CORRUPTED, 0);
  GzipResult r;
  r.status = ST_OK;
  r.checksum = compare_crc ? inner.checksum : 0u;
  r.out_len = inner.out_len;
  r.src_used = hdr_len + u + 8u;
  r.hdr_len = hdr_len; r.flg = flg;
  return r;
}

// ---- compress: the header 1f 8b 08 FLG 00000000 XFL ff (MTIME 0 and OS 255: the output is a function of the input alone),
// in the BGZF flavour FLG = 4, XLEN = 6 and the subfield 42 43 02 00 BSIZE behind it; then deflate's bytes; then the
// CRC-32 of the source and its length mod 2^32
ZD_HD uint32_t gzip_xfl(int level) { return level == LEVEL_BEST ? 2u : level == LEVEL_FAST ? 4u : 0u; }
ZD_HD uint64_t gzip_header_len(int flavour) { return flavour == GZIP_BGZF ? 18u : 10u; }
ZD_HD uint64_t gzip_overhead(int flavour) { return gzip_header_len(flavour) + 8u; }
// the room a member may take of a destination of `cap` bytes: a BGZF member can never exceed what BSIZE can say
ZD_HD uint64_t gzip_room(uint64_t cap, int flavour) { return flavour == GZIP_BGZF && cap > GZIP_BGZF_MAX ? GZIP_BGZF_MAX : cap; }
// where deflate's bytes go in a destination at [off, off + cap), and how many there may be (cap >= gzip_overhead)
ZD_HD uint64_t gzip_payload_off(uint64_t off, int flavour) { return off + gzip_header_len(flavour); }
ZD_HD uint64_t gzip_payload_cap(uint64_t cap, int flavour) { return gzip_room(cap, flavour) - gzip_overhead(flavour); }
// the header of a member of member_len bytes in all
ZD_HD void gzip_put_header(uint8_t *o, int level, int flavour, uint64_t member_len) {
  o[0] = 0x1Fu; o[1] = 0x8Bu; o[2] = 8u;
  o[3] = flavour == GZIP_BGZF ? (uint8_t)GZIP_FEXTRA : (uint8_t)0;
  o[4] = o[5] = o[6] = o[7] = 0;
  o[8] = (uint8_t)gzip_xfl(level);
  o[9] = 0xFFu;
  if (flavour != GZIP_BGZF) return;
  const uint64_t bsize = member_len - 1u;
  o[10] = 6u; o[11] = 0;
  o[12] = 'B'; o[13] = 'C'; o[14] = 2u; o[15] = 0;
  o[16] = (uint8_t)bsize; o[17] = (uint8_t)(bsize >> 8);
}
ZD_HD void gzip_put_trailer(uint8_t *p, uint32_t crc, uint64_t src_len) {
  for (int k = 0; k < 4; k++) {
    p[k] = (uint8_t)(crc >> (8 * k));
    p[4 + k] = (uint8_t)(src_len >> (8 * k));
  }
}
// the compress form's open: the destination's verdict in front of deflate
ZD_HD uint32_t gzip_open_compress_status(uint64_t dst_cap, int flavour) { return dst_cap < gzip_overhead(flavour) ? ST_DST_TOO_SMALL : ST_OK; }
// ... and its close: `inner` is deflate's, the result counts the container's bytes too.  *wrap: the caller has to put the
// header and the trailer (inner.checksum, behind inner.out_len bytes of payload) around what deflate wrote.  A member that
// is not OK has no checksum and no length.
ZD_HD StreamResult gzip_close_compress(uint32_t pre, StreamResult inner, int flavour, bool *wrap) {
  *wrap = false;
  if (pre != ST_OK) inner.status = pre;
  if (inner.status != ST_OK) { inner.checksum = 0; inner.out_len = 0; }
  else { inner.out_len += gzip_overhead(flavour); *wrap = true; }
  return inner;
}

// ---- the host plan: a file is a run of members back to back (RFC 1952 section 2.2)
// What stands at `off` of a file of `len` bytes.  end_of_members: the bytes there do not begin with 1f 8b and a member has
// been seen (off > 0) -- what lies behind the last member is ignored.  Otherwise status is the header's verdict, and on
// ST_OK: known -- the header has BSIZE and the member lies inside the file, so its length (bsize) is known without
// decoding it and isize is read from its last four bytes; else bsize and isize are 0 and the member has to be sized.
struct GzipStep {
  uint32_t status, end_of_members, known, hdr_len, flg, bsize, isize, reserved;
};
ZD_HD GzipStep gzip_next(const uint8_t *file, uint64_t len, uint64_t off) {
  GzipStep st;
  st.status = ST_OK; st.end_of_members = 0; st.known = 0; st.hdr_len = 0; st.flg = 0; st.bsize = 0; st.isize = 0; st.reserved = 0;
  const uint64_t left = len - off;
  if (off > 0 && (left < 2 || file[off] != 0x1Fu || file[off + 1] != 0x8Bu)) { st.end_of_members = 1; return st; }
  const GzipHeader h = gzip_parse_header(file + off, left);
  st.status = h.status;
  if (h.status != ST_OK) return st;
  st.hdr_len = h.hdr_len; st.flg = h.flg;
  if (h.bsize != 0 && h.bsize >= h.hdr_len + 8u && h.bsize <= left) {
    st.known = 1; st.bsize = h.bsize;
    st.isize = gzip_u32(file + off + h.bsize - 4u);
  }
  return st;
}

}  // namespace zd
