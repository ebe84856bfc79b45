// checksum_ranges.h -- the rules of the ragged checksum pass (zipc_hip_checksum_batch): free of HIP.
//
// A call hands over n ranges {off, len} of one arena and a declared total of their lengths.  Every number a kernel of
// that pass uses as an index, a bound or a grid size is a function here, so that the same code is compiled twice:
//   * into libzipc_hip.so (checksum.hip's checksum_plan / crc32_ranges / crc32_finish_ranges / adler_finish_ranges
//     kernels, api.hip's zipc_hip_checksum_batch);
//   * into tests/checksum_ranges_sim/sim_ranges.cpp with g++, where the launches run as loops over every workgroup of
//     the grid bound and every index is checked before it is used (tests/test_checksum_ranges_rules.py holds a mutation
//     table over this file; tests/checksum_ranges_sim/audit_main.cpp is the same model under the address sanitizer).
// Arrays come as anything with operator[]: pointers on the device, checking wrappers in the model.
#pragma once

#include "adler_chain.h"
#include "zd_common.h"

namespace zd {

constexpr uint32_t RANGES_SEG_BYTES = 32768;   // a workgroup's segment (checksum.hip CRC_SEG)
constexpr uint32_t RANGES_PLAN_TILE = 1024;    // ranges the plan's one workgroup scans at a time, one per thread
constexpr uint32_t RANGES_FINISH_LANES = 64;   // the CRC finish: a wave per range, a column of partials per lane

// binary-identical to zipc_hip_range / zipc_hip_checksum_result of include/zipc_hip.h
struct Range { uint64_t off, len; };
struct RangeResult { uint32_t status, crc32, adler32, reserved; };

// ---- a range
// INVALID_ARG: its end overflows 64 bits or lies beyond the arena.  Such a range counts as empty everywhere below.
ZD_HD uint32_t range_verdict(const Range &r, uint64_t arena_len) {
  const uint64_t end = r.off + r.len;
  if (end < r.off) return ST_INVALID_ARG;
  if (end > arena_len) return ST_INVALID_ARG;
  return ST_OK;
}
ZD_HD uint64_t range_segs(uint64_t len) {
  if (len == 0) return 0;
  return (len - 1) / RANGES_SEG_BYTES + 1;
}
// what a range adds to the three running sums of the plan
struct RangeCounts { uint64_t len, segs, chunks; };
ZD_HD RangeCounts range_counts(const Range &r, uint64_t arena_len) {
  RangeCounts c;
  c.len = range_verdict(r, arena_len) == ST_OK ? r.len : 0;
  c.segs = range_segs(c.len);
  c.chunks = adler_n_chunks(c.len);
  return c;
}
// (the lengths saturate: overlapping ranges of a large arena may sum past 2^64, and a saturated sum is past every declared total
// but 2^64 - 1 itself, whose grid no call gets to launch; saturating addition is associative, so any scan gives the same sums)
ZD_HD uint64_t ranges_sat_add(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }
ZD_HD RangeCounts ranges_counts_add(const RangeCounts &a, const RangeCounts &b) {
  RangeCounts c;
  c.len = ranges_sat_add(a.len, b.len);
  c.segs = a.segs + b.segs;      // (below 2^64 / 32768 * 2^31: no wrap for n < 2^31)
  c.chunks = a.chunks + b.chunks;
  return c;
}
// per range, from the sums of the ranges BEFORE it.  seg_base is 32 bits: where the call is not bad the total is at most
// segs_bound, which the call checks against 2^31; in a bad call nothing reads it.
ZD_HD uint32_t ranges_seg_base(const RangeCounts &before) { return (uint32_t)before.segs; }
ZD_HD uint64_t ranges_chunk_base(const RangeCounts &before) { return before.chunks; }

// ---- the call
// Grid and scratch sizes from the declared numbers alone: sum ceil(len / S) <= sum (len / S + 1) <= total / S + n, and
// adler_n_chunks(len) <= len / 5552 + 1 likewise, wherever the lengths sum to at most total_len.
ZD_HD uint64_t ranges_segs_bound(uint64_t total_len, uint64_t n_ranges) { return total_len / RANGES_SEG_BYTES + n_ranges; }
ZD_HD uint64_t ranges_chunks_bound(uint64_t total_len, uint64_t n_ranges) { return total_len / ADLER_CHUNK + n_ranges; }
// the call-wide word the plan leaves for every later kernel
struct RangesCall {
  uint64_t sum_len;       // of the OK ranges (saturated)
  uint64_t total_chunks;
  uint32_t total_segs;    // (meaningless in a bad call)
  uint32_t bad;           // the OK ranges sum to more than the declared total: the bounds above do not hold
  uint32_t reserved[2];
};
static_assert(sizeof(RangesCall) == 32, "the plan's scratch begins with 32 bytes of it");
ZD_HD RangesCall ranges_call_word(const RangeCounts &total, uint64_t total_len) {
  RangesCall c;
  c.sum_len = total.len;
  c.total_chunks = total.chunks;
  c.total_segs = (uint32_t)total.segs;
  c.bad = total.len > total_len ? 1u : 0u;
  c.reserved[0] = c.reserved[1] = 0;
  return c;
}
// what a range's result says before the finishes fill in the checksums
ZD_HD uint32_t ranges_status(const RangesCall &call, uint32_t verdict) { return call.bad != 0 ? (uint32_t)ST_INVALID_ARG : verdict; }
// a workgroup of the segment pass (the grid is segs_bound of them) has nothing to do
ZD_HD bool ranges_wg_idle(const RangesCall &call, uint64_t w) { return call.bad != 0 || w >= call.total_segs; }

// ---- workgroup -> work.  The range of workgroup w < total_segs: the last i with seg_base[i] <= w.  (seg_base never
// falls, seg_base[0] = 0, and a range without segments shares its base with the next one, so that last i has segments:
// were it empty, i + 1 would qualify too, or, at the end, total_segs = seg_base[i] <= w.)
template <class A>
ZD_HD uint32_t ranges_find(const A &seg_base, uint32_t n_ranges, uint32_t w) {
  uint32_t lo = 0, hi = n_ranges;  // the first i of [lo, hi] whose base is above w (hi: none)
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (seg_base[mid] <= w) lo = mid + 1;
    else hi = mid;
  }
  return lo - 1;
}
struct RangeWork {
  uint32_t range;     // whose bytes
  uint32_t seg;       // which 32 KiB segment of its right-aligned grid
  uint32_t slot;      // of the partials
  uint64_t chunk_at;  // where the range's chunk sums begin
};
template <class A, class B>
ZD_HD RangeWork ranges_work(const A &seg_base, const B &chunk_base, uint32_t n_ranges, uint32_t w) {
  RangeWork k;
  k.range = ranges_find(seg_base, n_ranges, w);
  k.seg = w - seg_base[k.range];
  k.slot = w;
  k.chunk_at = chunk_base[k.range];
  return k;
}
// the bytes [lo, hi) of a range of len bytes that segment seg of its grid holds: the grid is right-aligned (nseg * 32 KiB
// end at len), so the first segment is the short one
ZD_HD void ranges_seg_interval(uint64_t len, uint64_t seg, uint64_t &lo, uint64_t &hi) {
  const uint64_t pad = range_segs(len) * RANGES_SEG_BYTES - len;
  hi = (seg + 1) * RANGES_SEG_BYTES - pad;
  lo = seg == 0 ? 0 : hi - RANGES_SEG_BYTES;
}
// the chunk of the reference's grid (first chunk = len mod 5552) that holds byte pos of a range, and where that chunk ends
ZD_HD uint64_t ranges_chunk_of(uint64_t len, uint64_t pos, uint64_t &chunk_end) {
  const uint64_t r = len % ADLER_CHUNK;
  if (pos < r) { chunk_end = r; return 0; }
  const uint64_t k = (pos - r) / ADLER_CHUNK + 1;
  chunk_end = r + k * ADLER_CHUNK;
  return k;
}

// ---- the CRC-32 finish of a range: nseg partials from partials[base] on, by one wave.  Up to CRC_FINISH_HORNER_MAX
// of them: Horner by one lane.  More: adler_chain.h's right-aligned grid with 64 columns, a column per lane (its Horner
// step shifts by a whole row), then a tree over the lanes that shifts by 1, 2, 4 .. 32 segments.
ZD_HD bool ranges_crc_by_one_lane(uint64_t nseg) { return crc_finish_by_one_thread(nseg); }
template <class A>
ZD_HD uint32_t ranges_crc_horner(const A &partials, uint64_t base, uint64_t nseg, uint32_t xseg) {
  uint32_t raw = 0;
  for (uint64_t j = 0; j < nseg; j++) raw = gf2_mul(raw, xseg) ^ partials[base + j];
  return raw;
}
template <class A>
ZD_HD uint32_t ranges_crc_column(const A &partials, uint64_t base, uint64_t nseg, uint32_t lane, uint32_t xrow) {
  const uint64_t R = crc_finish_rows(nseg, RANGES_FINISH_LANES);
  const uint64_t padp = crc_finish_padp(nseg, RANGES_FINISH_LANES);
  uint32_t c = 0;
  for (uint64_t row = 0; row < R; row++) {
    const int64_t idx = crc_finish_index(row, RANGES_FINISH_LANES, lane, padp);
    const uint32_t w = partials[base + crc_finish_load_index(idx, row, R)];  // (clamped: the value is selected afterwards)
    c = gf2_mul(c, xrow) ^ (idx >= 0 ? w : 0u);
  }
  return c;
}
// step s = 1, 2 .. 32 of the tree: lane t (t a multiple of 2 s) takes lane t + s's value; xr = x^(8 * 32 KiB * s)
ZD_HD uint32_t ranges_crc_tree_step(uint32_t mine, uint32_t other, uint32_t xr) { return gf2_mul(mine, xr) ^ other; }
// init and final xor (zd.ml:135-136) around the raw CRC of len bytes; xlen = x^(8 len)
ZD_HD uint32_t ranges_crc_value(uint32_t raw, uint32_t xlen) { return crc_state_advance(0xFFFFFFFFu, raw, xlen) ^ 0xFFFFFFFFu; }

// ---- the Adler-32 finish of a range: the walk over its chunk sums from sums[base] on, by one lane -- adler_plain_walk's
// loop (the reference's signed remainder), or RFC 1950's arithmetic and packing where the context asks for it
template <class A>
ZD_HD uint32_t ranges_adler_walk(const A &sums, uint64_t base, uint64_t len, bool rfc) {
  const uint64_t n_chunks = adler_n_chunks(len);
  const uint32_t r = (uint32_t)(len % ADLER_CHUNK);
  uint32_t a1, a2;
  adler_unpack(1u, a1, a2);
  for (uint64_t k = 0; k < n_chunks; k++) adler_chunk_step(a1, a2, adler_chunk_len(k, r), sums[base + k].x, sums[base + k].y, rfc);
  return rfc ? (a2 << 16) | a1 : adler_pack(a1, a2);
}

}  // namespace zd
