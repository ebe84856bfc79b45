// zlib_container.h -- the six bytes RFC 1950 puts around a deflate stream, as the reference reads and writes them: free
// of HIP.
//
// zlib_decompress (src/zipc_deflate.ml:720-740) and zlib_compress (:1262-1277) are inflate / deflate with Adler-32 plus
// the rules below.  They are pure functions of plain numbers, so the same code is compiled three times:
//   * into zlib.hip's two kernels (zipc_hip_zlib_*_batch: a lane per stream opens and closes the container on the device);
//   * into the host forms (api.hip zipc_hip_zlib_compress / _decompress, many.hip the *_many forms);
//   * into tests/zlib_sim/sim_zlib.cpp with g++, where tests/test_zlib_rules.py holds every (CMF, FLG) pair to the oracle.
#pragma once

#include "inflate_extent.h"
#include "inflate_prefix.h"
#include "zd_common.h"

namespace zd {

// the statuses of include/zipc_hip.h that only the container has (zd_common.h has the codec's)
enum : uint32_t { ST_ZLIB_METHOD = 3, ST_ZLIB_WINDOW = 4, ST_ZLIB_DICT = 5, ST_CHECKSUM = 6 };

constexpr uint64_t ZLIB_MIN_LEN = 6;   // CMF, FLG and the Adler-32: zd.ml:723
constexpr uint64_t ZLIB_OVERHEAD = 6;  // what zlib_compress adds to deflate's bytes

// what is kept of a stream between open and close (zlib.hip's kernels, many.hip zlib_many): the container check's
// verdict; to decompress, the Adler-32 the stream says it has
struct ZlibPre { uint32_t status, expect; };

// The reference's checks of a stream of `len` bytes that begins with cmf, flg, in the reference's order (zd.ml:723-730).
// (len < ZLIB_MIN_LEN: the two bytes are not looked at -- callers that cannot read them pass anything.)
ZD_HD uint32_t zlib_open_status(uint64_t len, uint32_t cmf, uint32_t flg) {
  if (len < ZLIB_MIN_LEN) return ST_CORRUPTED;
  if ((256u * cmf + flg) % 31u != 0) return ST_CORRUPTED;
  if ((cmf & 0x0Fu) != 8u) return ST_ZLIB_METHOD;
  if ((cmf >> 4) > 7u) return ST_ZLIB_WINDOW;
  if ((flg & 0x20u) != 0) return ST_ZLIB_DICT;
  return ST_OK;
}

// What inflate is handed of a stream at [off, off + len): the range [2, len - 2) (zd.ml:732).  It ends two bytes
// short of the stream, not four: the first two bytes of the trailer are inside it, and a deflate stream that runs into
// them reads them as the reference does.  (len >= ZLIB_MIN_LEN.)
ZD_HD uint64_t zlib_body_off(uint64_t off) { return off + 2; }
ZD_HD uint64_t zlib_body_len(uint64_t len) { return len - 4; }

// the Adler-32 a stream says it has: its last four bytes, big-endian (zd.ml:731)
ZD_HD uint32_t zlib_expect(const uint8_t *last4) {
  return ((uint32_t)last4[0] << 24) | ((uint32_t)last4[1] << 16) | ((uint32_t)last4[2] << 8) | (uint32_t)last4[3];
}

// what zlib_compress writes in front (zd.ml:1266-1270): deflate with a 32 KiB window, the level in FLG's top bits,
// FCHECK making the two bytes a multiple of 31
ZD_HD uint32_t zlib_cmf() { return (7u << 4) | 8u; }
ZD_HD uint32_t zlib_flg(int level) {
  const uint32_t header = (zlib_cmf() << 8) | ((uint32_t)level << 6);
  return (header + 31u - header % 31u) & 0xFFu;
}
// where deflate's bytes go in a destination at [off, off + cap), and how many there may be (cap >= ZLIB_OVERHEAD)
ZD_HD uint64_t zlib_payload_off(uint64_t off) { return off + 2; }
ZD_HD uint64_t zlib_payload_cap(uint64_t cap) { return cap - ZLIB_OVERHEAD; }
// ... and behind them (zd.ml:1274)
ZD_HD void zlib_put_trailer(uint8_t *p, uint32_t adler) {
  p[0] = (uint8_t)(adler >> 24);
  p[1] = (uint8_t)(adler >> 16);
  p[2] = (uint8_t)(adler >> 8);
  p[3] = (uint8_t)adler;
}

// ---- a stream's result, from what the container check said before the codec ran (pre) and what the codec said (inner)
// zlib_decompress: a stream that failed its own check says so; one that inflated to another Adler-32 than it says
// reports the one found and no bytes (zd.ml:735-737); everything else is inflate's.
ZD_HD StreamResult zlib_close_decompress(uint32_t pre, uint32_t expect, StreamResult inner) {
  if (pre != ST_OK) { inner.status = pre; inner.checksum = 0; inner.out_len = 0; }
  else if (inner.status == ST_OK && inner.checksum != expect) { inner.status = ST_CHECKSUM; inner.out_len = 0; }
  return inner;
}
// Sizing a zlib stream (zipc_hip_zlib_size_batch): `inner` is the size kernel's verdict of the body.  A stream that failed
// its own check says so; every other one is the body's -- its status, and on ST_OK what it inflates to.  The Adler-32 is
// NOT compared (there are no bytes to take it of): a stream sized ST_OK can still be ST_CHECKSUM when it is decompressed.
ZD_HD StreamResult zlib_close_size(uint32_t pre, StreamResult inner) {
  if (pre != ST_OK) { inner.status = pre; inner.out_len = 0; }
  inner.checksum = 0;
  return inner;
}
// The prefix of a zlib stream (zipc_hip_zlib_decompress_prefix_batch): `inner` is the prefix kernel's record of the body,
// `adler` the Adler-32 of its bytes where it ended.  A stream that failed its own check says so; one that ENDED within its
// room is compared as zlib_close_decompress compares it (the value found is not reported: the record has no field for
// it); one that was cut has not been read to its end and nothing of it is compared; everything else is inflate's.
ZD_HD PrefixResult zlib_close_prefix(uint32_t pre, uint32_t expect, uint32_t adler, PrefixResult inner) {
  if (pre != ST_OK) { inner.status = pre; inner.ended = 0; inner.out_len = 0; }
  else if (inner.status == ST_OK && inner.ended != 0 && adler != expect) { inner.status = ST_CHECKSUM; inner.ended = 0; inner.out_len = 0; }
  return inner;
}
// A zlib stream of unknown length (zipc_hip_zlib_decompress_extent_batch, zipc_hip_zlib_size_extent_batch): src_len is an
// upper bound, so the trailer is not at src_len - 4.  The body handed to the codec is still [2, src_len - 2); with u the
// body's extent (inner.src_used) the trailer is the four bytes at 2 + u of the stream, and it has to lie inside the
// declared bytes: 2 + u + 4 > src_len is ST_CORRUPTED with nothing read or compared.  `stream`: the stream's first byte;
// only [2 + u, 2 + u + 4) is read, and only when `compare` (the sizing form compares nothing, like zlib_close_size, but
// holds the same bound, so that a stream it sizes OK has the src_used the decode form reports).  The Adler-32 is compared
// as zlib_close_decompress compares it; a mismatch reports the value found and no bytes.  OK: the whole stream, 6 more.
ZD_HD ExtentResult zlib_close_extent(uint32_t pre, uint64_t src_len, const uint8_t *stream, ExtentResult inner, bool compare) {
  if (pre != ST_OK) return extent_result(pre, 0, 0, 0);
  if (inner.status != ST_OK) return extent_result(inner.status, 0, 0, 0);
  const uint64_t u = inner.src_used;
  if (2u + u + 4u > src_len) return extent_result(ST_CORRUPTED, 0, 0, 0);
  if (!compare) inner.checksum = 0;
  else if (inner.checksum != zlib_expect(stream + 2u + u)) {
    inner.status = ST_CHECKSUM; inner.out_len = 0; inner.src_used = 0;
    return inner;
  }
  inner.src_used = u + 6u;
  return inner;
}
// ---- zlib streams with a preset dictionary (zipc_hip_zlib_decompress_dict_batch, zipc_hip_zlib_size_dict_batch): RFC 1950's
// FDICT, as deflateSetDictionary makes them.  One dictionary of dict_len bytes serves the call; dict_adler is RFC 1950's
// Adler-32 of it, whatever flavour the context compares outputs in (the DICTID is the encoder's, and zlib's is RFC 1950's).
constexpr uint64_t ZLIB_DICT_MIN_LEN = 10;  // CMF, FLG, the DICTID and the Adler-32
// what the open says of a stream: the verdict; on ST_ZLIB_DICT the DICTID found (a caller can look the right dictionary
// up), else 0; on ST_OK the body as [body_off, body_off + body_len) of the stream and the history it decodes with
struct ZlibDictOpen {
  uint32_t status, dictid;
  uint64_t body_off, body_len;
  uint32_t hist_len;
};
// the DICTID: bytes 2..5, big-endian
ZD_HD uint32_t zlib_dictid(const uint8_t *at2) {
  return ((uint32_t)at2[0] << 24) | ((uint32_t)at2[1] << 16) | ((uint32_t)at2[2] << 8) | (uint32_t)at2[3];
}
// zlib_open_status's checks in their order up to the FDICT test.  A stream without FDICT is opened exactly as
// zipc_hip_zlib_decompress_batch opens it and decodes with no history (zlib does the same).  One with FDICT: len < 10 is
// ST_CORRUPTED; no dictionary, or another DICTID than the dictionary's, is ST_ZLIB_DICT; otherwise the body is [6, len - 4)
// and the whole dictionary is its history.  dictid: the stream's (read only when len >= 10 and FDICT is set: callers
// that cannot read it pass anything).
ZD_HD ZlibDictOpen zlib_open_dict(uint64_t len, uint32_t cmf, uint32_t flg, uint32_t dictid, uint64_t dict_len, uint32_t dict_adler) {
  ZlibDictOpen o;
  o.status = zlib_open_status(len, cmf, flg); o.dictid = 0; o.body_off = 0; o.body_len = 0; o.hist_len = 0;
  if (o.status == ST_OK) { o.body_off = zlib_body_off(0); o.body_len = zlib_body_len(len); return o; }
  if (o.status != ST_ZLIB_DICT) return o;
  if (len < ZLIB_DICT_MIN_LEN) { o.status = ST_CORRUPTED; return o; }
  if (dict_len == 0 || dictid != dict_adler) { o.dictid = dictid; return o; }
  o.status = ST_OK; o.body_off = 6; o.body_len = len - ZLIB_DICT_MIN_LEN; o.hist_len = (uint32_t)dict_len;
  return o;
}
// The seed: the dictionary is copied to [dst_off - hist_len, dst_off) of a stream that was opened with FDICT and has the
// gap (a stream without it is ST_INVALID_ARG by inflate_history.h's rule).  The gap of a stream without FDICT, or of one
// that failed its open, is not written.
ZD_HD bool zlib_dict_seeds(uint32_t pre, uint32_t hist_len, uint64_t dst_off) { return pre == ST_OK && hist_len != 0 && dst_off >= hist_len; }
// The closes: zlib_close_decompress / zlib_close_size, but a stream whose dictionary is not the call's reports the
// DICTID it asks for (`expect` holds it then: the trailer was not read)
ZD_HD StreamResult zlib_close_dict(uint32_t pre, uint32_t expect, StreamResult inner, bool size) {
  if (pre == ST_ZLIB_DICT) { inner.status = pre; inner.checksum = expect; inner.out_len = 0; return inner; }
  return size ? zlib_close_size(pre, inner) : zlib_close_decompress(pre, expect, inner);
}

// zlib_compress: `inner` is deflate's, the result counts the container's bytes too.  *wrap: the caller has to put the
// header and the trailer (inner.checksum, behind inner.out_len bytes of payload) around what deflate wrote.
ZD_HD StreamResult zlib_close_compress(uint32_t pre, StreamResult inner, bool *wrap) {
  *wrap = false;
  if (pre != ST_OK) { inner.status = pre; inner.checksum = 0; inner.out_len = 0; }
  else if (inner.status == ST_OK) { inner.out_len += ZLIB_OVERHEAD; *wrap = true; }
  return inner;
}

}  // namespace zd
