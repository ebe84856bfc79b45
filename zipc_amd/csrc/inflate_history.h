// inflate_history.h -- the rule of the history forms (zipc_hip_inflate_history_batch, zipc_hip_inflate_prefix_history_batch,
// zipc_hip_inflate_size_history_batch, and the zlib dictionary forms around the first and the last): free of HIP, pure
// functions of plain numbers.
//
// Every other inflate form starts at bit 0 of a stream and at output position 0, and a match that reaches in front of the
// output is ST_CORRUPTED (inflate_lane.h lane_match_commit: dist > d.out_pos, zd.ml:614).  A history form is handed, per
// stream, a record {hist_len, start_bit}: hist_len bytes of history lie at [dst_off - hist_len, dst_off) of the
// DESTINATION arena (a preset dictionary, the 32 KiB in front of an access point, the end of the piece before), and the
// first block header starts at bit start_bit of the byte at src_off.  Every copy site of the decoder addresses its source
// as dst + out_pos - dist, so the wave is told that its room begins hist_len bytes earlier and that hist_len bytes of it
// are written already: the bias below.  No instruction of the lane step, the span decoder or the copies changes; the
// wave applies the bias once behind lane_init and takes it off once at its result store (inflate.hip inflate_wave,
// HISTORY).  The defining property: a match is legal iff dist <= hist_len + (bytes produced so far); everything else is
// zipc_hip_inflate_batch's, with positions counted from dst_off.  A record of {0, 0} is the form without history.
// The kernels, api.hip and the host model (tests/history_sim/sim_history.cpp) compile this text.
//
// Out of scope here and in the forms built on it: deflating against a dictionary or a kept window, building an index of
// access points, history in the extent, packed, gzip and recode forms, a by-blocks path for long streams with history,
// combining the checksums of pieces.
#pragma once

#include "inflate_prefix.h"
#include "zd_common.h"

namespace zd {

// zipc_hip_history (include/zipc_hip.h)
struct HistoryRec {
  uint32_t hist_len;   // bytes of history in front of dst_off
  uint32_t start_bit;  // the bit of the byte at src_off at which the first block header starts, 0 the lowest
};
static_assert(sizeof(HistoryRec) == 8, "zipc_hip_history");

constexpr uint32_t HISTORY_MAX_LEN = 32768;  // deflate's window: no distance is longer
constexpr uint32_t HISTORY_MAX_BIT = 7;
// the biased room still fits the lane's 32-bit positions
static_assert(MAX_STREAM_LEN + HISTORY_MAX_LEN == 0xFFFF8000ull, "the longest room plus the longest history");
static_assert(MAX_STREAM_LEN + HISTORY_MAX_LEN <= 0xFFFFFFFFull, "InflateLane's positions are 32-bit");

// The verdict on a record, in this order, before the descriptor's own tests (a flag bit, a length above MAX_STREAM_LEN:
// those keep their statuses and are made on the caller's values, before any bias).  has_dst: the sizing form has no
// destination and does not look at dst_off.
ZD_HD uint32_t history_record_status(uint32_t hist_len, uint32_t start_bit, uint64_t dst_off, bool has_dst) {
  if (hist_len > HISTORY_MAX_LEN) return ST_INVALID_ARG;
  if (start_bit > HISTORY_MAX_BIT) return ST_INVALID_ARG;
  if (has_dst && (uint64_t)hist_len > dst_off) return ST_INVALID_ARG;
  return ST_OK;
}

// ---- the bias: the caller's numbers (as lane_init read them) -> what the wave runs with
ZD_HD uint64_t history_dst_off(uint64_t dst_off, uint32_t hist_len) { return dst_off - hist_len; }
ZD_HD uint32_t history_cap(uint32_t dst_cap, uint32_t hist_len) { return dst_cap + hist_len; }  // (<= 0xFFFF8000)
// a limit counts the stream's own bytes: it goes up with them, saturating where lane_init saturates
ZD_HD uint32_t history_limit(uint32_t limit, uint32_t hist_len) { return limit > 0xFFFFFFFFu - hist_len ? 0xFFFFFFFFu : limit + hist_len; }
ZD_HD uint32_t history_out_pos(uint32_t hist_len) { return hist_len; }
ZD_HD uint32_t history_bit(uint32_t start_bit) { return start_bit; }
// ... applied to a lane behind lane_init / lane_init_size that left it ST_OK (Lane: inflate_lane.h InflateLane).
// has_dst false: IM_SIZE, whose dst_off is 0 and never forms an address.
template <class Lane>
ZD_HD void history_start(Lane &d, uint32_t hist_len, uint32_t start_bit, bool has_dst) {
  if (has_dst) d.dst_off = history_dst_off(d.dst_off, hist_len);
  d.hard_cap = history_cap(d.hard_cap, hist_len);
  d.limit = history_limit(d.limit, hist_len);
  d.cap_min = d.limit < d.hard_cap ? d.limit : d.hard_cap;
  d.in_word = history_bit(start_bit) >> 5;
  d.boff = history_bit(start_bit) & 31u;
  d.ring_wr = d.in_word;
  d.out_pos = history_out_pos(hist_len);
  d.blk_out_start = d.out_pos;
}

// ---- the unbias: the wave's position (or, on a cut, its room) -> the caller's out_len
ZD_HD uint64_t history_out_len(uint32_t pos, uint32_t hist_len) { return (uint64_t)(pos - hist_len); }
// the result of the all-or-nothing forms (adler: of the stream's own output, the chain started at 1 at dst_off)
ZD_HD StreamResult history_result(uint32_t status, uint32_t adler, uint32_t out_pos, uint32_t hist_len) {
  StreamResult r;
  r.status = status;
  r.checksum = status == ST_OK ? adler : 0u;
  r.out_len = status == ST_OK ? history_out_len(out_pos, hist_len) : 0u;
  return r;
}
// ... and of the prefix form: prefix_result's record with both of its lengths -- an ended stream's out_pos, a cut one's
// cap_min -- counted from dst_off
ZD_HD PrefixResult history_prefix_result(uint32_t status, uint32_t out_pos, uint32_t cap_min, uint32_t hist_len) {
  PrefixResult r = prefix_result(status, out_pos, cap_min);
  if (r.status == ST_OK) r.out_len = history_out_len((uint32_t)r.out_len, hist_len);
  return r;
}

}  // namespace zd
