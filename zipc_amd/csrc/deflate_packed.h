// deflate_packed.h -- the rules of the packed encode forms (zipc_hip_deflate_packed_batch / zipc_hip_zlib_compress_packed_batch):
// free of HIP.
//
// A packed encode call deflates every stream of a batch into a STAGING slot of the context's scratch (nobody knows a
// deflate output's size in advance: a slot holds the bound), lays the results end to end in ONE destination arena, copies
// them there and says where each one went, with nothing read back between the steps.  The codec's kernels are not touched:
// a stage step stands in front of deflate, and a layout, a copy and a close step behind it (deflate_packed.hip).  Every
// number those steps use as an index, a bound, a verdict or a grid size is a pure function of plain numbers here, so that
// the same code is compiled three times:
//   * into deflate_packed.hip's four kernels (dpacked_stage / dpacked_layout: one workgroup, tiles of DPACKED_TILE streams;
//     dpacked_copy: a workgroup per 32 KiB segment that exists; dpacked_close: a lane per stream) and their launcher;
//   * into api.hip (the call's checks, the bound helpers);
//   * into tests/deflate_packed_sim/sim_deflate_packed.cpp with g++, where the tiles, waves and workgroups run as loops over
//     real byte arrays with every index checked (tests/test_deflate_packed_rules.py holds a mutation table over this file;
//     tests/deflate_packed_sim/audit_main.cpp is the same model under the address sanitizer).
// Arrays come as anything with operator[]: pointers on the device, checking wrappers in the model.
//
// The rule.  A stream TAKES ROOM iff its deflate result is ST_OK.  The streams that take room lie in index order:
// dst_off[i] = the sum, over the roomed streams j < i, of align_up(out_len[j], align) -- packed_layout.h's rule, whose
// functions (packed_align_up, packed_next_off, packed_fits, packed_end, the scan's halves, the need join) are used as they
// are.  A roomed stream FITS iff dst_off + out_len <= dst_arena_len, and `need` is the end of the last roomed stream.
#pragma once

#include "checksum_ranges.h"  // ranges_find: the workgroup -> (stream, segment) search of the ragged passes
#include "packed_layout.h"

namespace zd {

constexpr uint32_t DPACKED_TILE = PACKED_TILE;   // streams the stage's and the layout's one workgroup scan at a time
constexpr uint32_t DPACKED_WAVE = PACKED_WAVE;
constexpr uint64_t DPACKED_SLOT_ALIGN = 16;      // staging slots begin on these boundaries: the copy's source side is aligned
constexpr uint32_t DPACKED_SEG_BYTES = 32768;    // a copy workgroup's segment of one stream's output
constexpr uint32_t DPACKED_COPY_THREADS = 256;
constexpr uint32_t DPACKED_UNIT = 16;            // the body goes by aligned stores of this many bytes
constexpr uint32_t DPACKED_IN_FLIGHT = 4;        // units a thread loads before it stores them

// the call-wide word the stage and the layout leave for the kernels behind them (the context's scratch begins with it)
struct DpackedCall {
  uint64_t need;        // the layout's
  uint32_t total_segs;  // the layout's: segments of the streams that fit
  uint32_t bad;         // the stage's: the descriptors exceed what the call declared
  uint64_t reserved[2];
};
static_assert(sizeof(DpackedCall) == 32, "the plan's scratch begins with 32 bytes of it");

// ---- the bounds.  zipc_hip_deflate_bound(len) = len + 6 * (len / 65534 + 1) + 8 (api.hip) = len + 6 * (len / 65534) + 14,
// six more around a zlib stream; the floors of the streams sum to at most the floor of the total, so n slots whose sources
// sum to at most `total`, each padded to `align`, take at most the arena bound below.
ZD_HD uint64_t dpacked_slot_bytes(uint64_t src_len, bool zlib) { return src_len + 6 * (src_len / MAX_BLOCK_SRC_LEN + 1) + 8 + (zlib ? ZLIB_OVERHEAD : 0); }
ZD_HD uint64_t dpacked_arena_bound(uint64_t n_streams, uint64_t total_src_len, uint64_t align, bool zlib) {
  return total_src_len + 6 * (total_src_len / MAX_BLOCK_SRC_LEN) + 14 * n_streams + (align - 1) * n_streams + (zlib ? ZLIB_OVERHEAD * n_streams : 0);
}
// the staging arena: the slots on DPACKED_SLOT_ALIGN boundaries
ZD_HD uint64_t dpacked_staging_bound(uint64_t n_streams, uint64_t total_src_len, bool zlib) {
  return dpacked_arena_bound(n_streams, total_src_len, DPACKED_SLOT_ALIGN, zlib);
}
// the copy's grid, from the declared numbers alone: sum ceil(out_len / S) <= sum (slot / S + 1) <= staging / S + n
ZD_HD uint64_t dpacked_copy_grid(uint64_t n_streams, uint64_t total_src_len, bool zlib) {
  return dpacked_staging_bound(n_streams, total_src_len, zlib) / DPACKED_SEG_BYTES + n_streams;
}

// ---- the call's own arguments (every pointer but the arenas has been looked at): a status
ZD_HD uint32_t dpacked_call_status(bool dst_arena_null, uint64_t dst_arena_len, uint64_t n_streams, uint64_t max_src_len, uint64_t total_src_len,
                                   int level, int crc_op, uint64_t align, bool zlib) {
  if (dst_arena_null && dst_arena_len != 0) return ST_INVALID_ARG;
  if (n_streams > 0x7FFFFFFFull) return ST_INVALID_ARG;
  if (!packed_align_ok(align)) return ST_INVALID_ARG;
  if (level < LEVEL_NONE || level > LEVEL_BEST) return ST_INVALID_ARG;
  if (crc_op < CRC_NOP || crc_op > CRC_ADLER32_RFC) return ST_INVALID_ARG;
  if (max_src_len > MAX_STREAM_LEN) return ST_INVALID_ARG;
  if (total_src_len > (1ull << 48)) return ST_INVALID_ARG;  // (far beyond any grid: keeps the bounds' sums from wrapping)
  if (dpacked_copy_grid(n_streams, total_src_len, zlib) > 0x7FFFFFFFull) return ST_INVALID_ARG;
  return ST_OK;
}

// ---- stage: a stream, from its descriptor.  A descriptor beyond the format's range is refused on its own: it counts
// neither in the declared-size check nor among the slots.
ZD_HD bool dpacked_in_range(uint64_t src_len) { return src_len <= MAX_STREAM_LEN; }
ZD_HD uint64_t dpacked_declared_len(uint64_t src_len) { return dpacked_in_range(src_len) ? src_len : 0; }
ZD_HD bool dpacked_over_max(uint64_t src_len, uint64_t max_src_len) { return dpacked_in_range(src_len) && src_len > max_src_len; }
// the declared-size verdict of the whole call (zipc_hip_deflate_batch's device-side check, made before any slot is used)
ZD_HD uint32_t dpacked_declared_bad(bool any_over_max, uint64_t sum_len, uint64_t total_src_len) {
  return (any_over_max || sum_len > total_src_len) ? 1u : 0u;
}
// what a stream adds to the running sum of the slot offsets: its slot, padded -- the LENGTH is padded, as in the arena
ZD_HD uint64_t dpacked_slot_room(uint64_t src_len, bool zlib) {
  return dpacked_in_range(src_len) ? packed_align_up(dpacked_slot_bytes(src_len, zlib), DPACKED_SLOT_ALIGN) : 0;
}
// ST_OK: the stream is to run
ZD_HD uint32_t dpacked_stage_status(uint32_t call_bad, uint64_t src_len) {
  if (call_bad != 0) return ST_INVALID_ARG;
  return dpacked_in_range(src_len) ? (uint32_t)ST_OK : (uint32_t)ST_INVALID_ARG;
}
// The descriptor deflate (the zlib form: its open) runs with.  A stream that is to run: into exactly its slot.  Every
// other one goes through as a stream of no bytes and no room (packed_layout.h packed_inner_desc): deflate reports a
// destination too small for it and stores nothing, and the stage's status stands in its place.
ZD_HD StreamDesc dpacked_inner_desc(const StreamDesc &sd, uint32_t stage_status, uint64_t slot_off, bool zlib) {
  StreamDesc in;
  in.src_off = sd.src_off; in.reserved = 0;
  if (stage_status == ST_OK) { in.src_len = sd.src_len; in.dst_off = slot_off; in.dst_cap = dpacked_slot_bytes(sd.src_len, zlib); in.limit = sd.limit; in.flags = sd.flags; }
  else { in.src_len = 0; in.dst_off = 0; in.dst_cap = 0; in.limit = 0; in.flags = 0; }
  return in;
}

// ---- layout: a stream, from the stage's status and what deflate (the zlib form: its close) said of it in its slot
ZD_HD bool dpacked_takes_room(uint32_t stage_status, const StreamResult &staged) { return stage_status == ST_OK && staged.status == ST_OK; }
ZD_HD uint32_t dpacked_own_status(uint32_t stage_status, const StreamResult &staged) { return stage_status != ST_OK ? stage_status : staged.status; }
ZD_HD uint64_t dpacked_room(uint32_t stage_status, const StreamResult &staged, uint64_t align) {
  return dpacked_takes_room(stage_status, staged) ? packed_next_off(0, staged.out_len, align) : 0;
}
ZD_HD PackedVerdict dpacked_verdict(uint32_t stage_status, const StreamResult &staged, uint64_t off, uint64_t dst_arena_len) {
  PackedVerdict v;
  v.status = dpacked_own_status(stage_status, staged);
  v.roomed = dpacked_takes_room(stage_status, staged) ? 1u : 0u;
  v.dst_off = v.roomed ? off : 0;
  if (v.roomed && !packed_fits(off, staged.out_len, dst_arena_len)) v.status = ST_DST_TOO_SMALL;
  return v;
}
// where a stream ends, for `need`: the end of its bytes, not of its padding (0: it took no room)
ZD_HD uint64_t dpacked_end(const PackedVerdict &v, uint64_t out_len) { return packed_end(v.roomed != 0, v.dst_off, out_len); }
// the copy's segments of a stream of len bytes, and of a stream by its verdict: only one that fits is copied
ZD_HD uint64_t dpacked_segs(uint64_t len) {
  if (len == 0) return 0;
  return (len - 1) / DPACKED_SEG_BYTES + 1;
}
ZD_HD uint64_t dpacked_copy_segs(const PackedVerdict &v, uint64_t out_len) { return v.roomed && v.status == ST_OK ? dpacked_segs(out_len) : 0; }

// ---- copy: workgroup -> work.  seg_base[i]: the segments of the fitting streams before i (it never falls, and a stream
// without segments shares its base with the next one: checksum_ranges.h ranges_find).  w < total_segs.
ZD_HD bool dpacked_wg_idle(const DpackedCall &call, uint64_t w) { return call.bad != 0 || w >= call.total_segs; }
struct DpackedWork { uint32_t stream, seg; };
template <class A>
ZD_HD DpackedWork dpacked_work(const A &seg_base, uint32_t n_streams, uint32_t w) {
  DpackedWork k;
  k.stream = ranges_find(seg_base, n_streams, w);
  k.seg = w - seg_base[k.stream];
  return k;
}
// Segment seg of a stream of len bytes whose first byte goes to an address that is dst_at modulo DPACKED_UNIT (the arena's
// base plus dst_off): the bytes [lo, lo + count) of the stream, as `head` single bytes up to the destination's first unit
// boundary, `units` whole aligned units, `tail` single bytes.  The staging slot and lo are multiples of the unit, so the
// source of the body is off its boundaries by `head`.  A unit of the arena that is not wholly this segment's is reached
// by byte stores only: a neighbour -- another stream with align below 16, the next segment of this one -- writes the rest.
struct DpackedSpan { uint64_t lo; uint32_t count, head, units, tail; };
ZD_HD DpackedSpan dpacked_span(uint64_t len, uint64_t seg, uint64_t dst_at) {
  DpackedSpan s;
  s.lo = seg * DPACKED_SEG_BYTES;
  const uint64_t left = len - s.lo;
  s.count = left < DPACKED_SEG_BYTES ? (uint32_t)left : DPACKED_SEG_BYTES;
  const uint32_t to_boundary = (DPACKED_UNIT - (uint32_t)((dst_at + s.lo) & (DPACKED_UNIT - 1))) & (DPACKED_UNIT - 1);
  s.head = to_boundary < s.count ? to_boundary : s.count;
  s.units = (s.count - s.head) / DPACKED_UNIT;
  s.tail = s.count - s.head - s.units * DPACKED_UNIT;
  return s;
}
// the unit thread t takes as the k-th of the DPACKED_IN_FLIGHT it holds in round r (consecutive threads, consecutive units)
ZD_HD uint32_t dpacked_unit_of(uint32_t r, uint32_t k, uint32_t t) { return (r * DPACKED_IN_FLIGHT + k) * DPACKED_COPY_THREADS + t; }
ZD_HD uint32_t dpacked_rounds(uint32_t units) { return (units + DPACKED_IN_FLIGHT * DPACKED_COPY_THREADS - 1) / (DPACKED_IN_FLIGHT * DPACKED_COPY_THREADS); }
// where the parts lie, from the segment's first byte
ZD_HD uint32_t dpacked_unit_at(const DpackedSpan &s, uint32_t u) { return s.head + u * DPACKED_UNIT; }
ZD_HD uint32_t dpacked_tail_at(const DpackedSpan &s) { return s.head + s.units * DPACKED_UNIT; }

// ---- close: the caller's result.  A stream that fits: what deflate said of it in its slot.  One with room that does not
// fit: the dst_off the rule gave it, no bytes, and the checksum zipc_hip_deflate_batch reports with ST_DST_TOO_SMALL -- the
// CRC-32 of the source (that pass runs whatever the verdict), 0 with either Adler-32.  One without room: its own status.
ZD_HD uint32_t dpacked_short_checksum(int crc_op, uint32_t staged_checksum) { return crc_op == CRC_CRC32 ? staged_checksum : 0u; }
ZD_HD PackedResult dpacked_close(const PackedVerdict &v, uint32_t stage_status, const StreamResult &staged, int crc_op) {
  PackedResult r;
  r.dst_off = v.dst_off; r.reserved = 0; r.out_len = 0;
  if (v.roomed && v.status == ST_OK) { r.status = ST_OK; r.checksum = staged.checksum; r.out_len = staged.out_len; }
  else if (v.roomed) { r.status = v.status; r.checksum = dpacked_short_checksum(crc_op, staged.checksum); }
  else { r.status = v.status; r.checksum = stage_status != ST_OK ? 0u : staged.checksum; }
  return r;
}

}  // namespace zd
