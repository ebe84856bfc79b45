// packed_layout.h -- the rules of the packed decode forms (zipc_hip_inflate_packed_batch / zipc_hip_zlib_decompress_packed_batch):
// free of HIP.
//
// A packed call sizes every stream of a batch, lays the outputs end to end in ONE destination arena, decodes them there
// and says where each one went, with nothing read back between the steps.  The codec's kernels are not touched: a
// layout step stands between sizing and decode and a close step behind decode (packed.hip).  Which streams take room,
// where, whether they fit, what the decoder is handed and what the caller is told are pure functions of plain numbers
// here, so that the same code is compiled three times:
//   * into packed.hip's two kernels (packed_layout_kernel: one workgroup, tiles of PACKED_TILE streams; packed_close_kernel:
//     a lane per stream);
//   * into the launcher (packed.hip launch_inflate_packed: the call's checks and which sizing pass runs);
//   * into tests/packed_sim/sim_packed.cpp with g++, where the layout kernel's tiles and waves run as loops with every
//     index checked (tests/test_packed_rules.py holds a mutation table over this file).
//
// The rule.  A stream TAKES ROOM iff it was sized ST_OK and its size is at most the call's max_out_len.  The streams that
// take room lie in index order: dst_off[i] = the sum, over the roomed streams j < i, of align_up(out_len[j], align) -- the
// LENGTHS are padded, so every roomed stream begins on a multiple of align and the padding lies behind a stream's bytes,
// where nothing is ever written.  A roomed stream FITS iff dst_off + out_len <= dst_arena_len.  `need` is the end
// (dst_off + out_len, without padding) of the last roomed stream, fitting or not, and 0 if none took room: the arena
// length with which every roomed stream fits.  Every sum is 64-bit (n < 2^31 streams of at most 2^32 bytes: no wrap).
#pragma once

#include "forms.h"           // BLOCKS_BATCH_MIN_DST: from where zipc_hip_inflate_batch itself enters the block path
#include "zlib_container.h"  // (ST_CHECKSUM and the container's verdicts: the zlib form's close goes through here)

namespace zd {

constexpr uint32_t PACKED_TILE = 1024;       // streams the layout's one workgroup scans at a time, one per thread
constexpr uint32_t PACKED_WAVE = 64;         // ... in waves of this many: a wave scan each, the waves' totals through LDS
constexpr uint64_t PACKED_ALIGN_MAX = 4096;  // align: a power of two in 1..4096

// binary-identical to zipc_hip_packed_result of include/zipc_hip.h
struct PackedResult {
  uint32_t status, checksum;
  uint64_t out_len, dst_off, reserved;
};
// What the layout knows of a stream (the context's scratch holds one per stream): ST_OK for a stream that has room and
// fits -- the decoder's word counts -- or why it has none; where its room begins (0: it was given none).
struct PackedVerdict {
  uint32_t status, roomed;
  uint64_t dst_off;
};

// ---- the call
ZD_HD bool packed_align_ok(uint64_t align) { return align >= 1 && align <= PACKED_ALIGN_MAX && (align & (align - 1)) == 0; }
// the call's own arguments (every pointer but the arenas has been looked at): a status
ZD_HD uint32_t packed_call_status(bool dst_arena_null, uint64_t dst_arena_len, uint64_t n_streams, uint64_t max_out_len, uint64_t align,
                                  int crc_op) {
  if (dst_arena_null && dst_arena_len != 0) return ST_INVALID_ARG;
  if (n_streams > 0x7FFFFFFFull) return ST_INVALID_ARG;
  if (!packed_align_ok(align)) return ST_INVALID_ARG;
  if (max_out_len > MAX_STREAM_LEN) return ST_INVALID_ARG;  // (one stored stream beyond 4 GiB, inflate_batch's exception, is not offered)
  if (crc_op < CRC_NOP || crc_op > CRC_ADLER32_RFC) return ST_INVALID_ARG;
  return ST_OK;
}
// Which sizing pass runs: inflate_size_kernel's one wave per stream, enqueued and never waited for, while no stream of the
// call may be as long as the block path takes them in a batch; from there on the sizing by blocks, which synchronises
// (inflate.hip launch_inflate_size_blocks) -- as the decode behind it then does by itself (launch_inflate: inflate_blocks_gate).
// (A call of ONE stream: launch_inflate's gate opens at BLOCKS_MIN_SRC of room already, and such a call's decode reads
// its descriptor back.)
enum : int { PACKED_SIZE_ONE_WAVE = 0, PACKED_SIZE_BY_BLOCKS = 1 };
ZD_HD int packed_size_form(uint64_t max_out_len) { return max_out_len < BLOCKS_BATCH_MIN_DST ? PACKED_SIZE_ONE_WAVE : PACKED_SIZE_BY_BLOCKS; }

// ---- a stream, from what the sizing pass said of it
ZD_HD uint64_t packed_align_up(uint64_t len, uint64_t align) { return (len + align - 1) & ~(align - 1); }
ZD_HD uint64_t packed_add(uint64_t a, uint64_t b) { return a + b; }
ZD_HD bool packed_takes_room(const StreamResult &sized, uint64_t max_out_len) { return sized.status == ST_OK && sized.out_len <= max_out_len; }
// what it says of itself when it takes none: its own error, or a size the call did not declare
ZD_HD uint32_t packed_sized_status(const StreamResult &sized, uint64_t max_out_len) {
  if (sized.status != ST_OK) return sized.status;
  return sized.out_len > max_out_len ? (uint32_t)ST_INVALID_ARG : (uint32_t)ST_OK;
}
// where the room behind a stream of len bytes at off begins: the length is padded, not the offset
ZD_HD uint64_t packed_next_off(uint64_t off, uint64_t len, uint64_t align) { return packed_add(off, packed_align_up(len, align)); }
// what a stream adds to the running sum of the offsets
ZD_HD uint64_t packed_room(const StreamResult &sized, uint64_t max_out_len, uint64_t align) {
  return packed_takes_room(sized, max_out_len) ? packed_next_off(0, sized.out_len, align) : 0;
}
ZD_HD bool packed_fits(uint64_t off, uint64_t len, uint64_t dst_arena_len) { return packed_add(off, len) <= dst_arena_len; }
// where a stream ends, for `need`: the ends of the roomed streams never fall with the index, so the last one's is their
// maximum, and a stream without room adds nothing to it
ZD_HD uint64_t packed_end(bool roomed, uint64_t off, uint64_t len) { return roomed ? packed_add(off, len) : 0; }
ZD_HD uint64_t packed_need_join(uint64_t a, uint64_t b) { return a > b ? a : b; }

// ---- the scan.  A room is below 2^32, so a wave's 64-bit inclusive scan is two 32-bit ones (wave_ops.h wave_scan_incl)
// over its halves of 16 bits: 64 x 0xFFFF stays far below 2^32 in each.
ZD_HD uint32_t packed_scan_lo(uint64_t room) { return (uint32_t)(room & 0xFFFFu); }
ZD_HD uint32_t packed_scan_hi(uint64_t room) { return (uint32_t)(room >> 16); }
ZD_HD uint64_t packed_scan_join(uint32_t lo_sum, uint32_t hi_sum) { return packed_add(lo_sum, (uint64_t)hi_sum << 16); }
// the base the next tile's offsets begin at: what was carried into this tile and what its streams added
ZD_HD uint64_t packed_tile_base(uint64_t carried, uint64_t tile_total) { return packed_add(carried, tile_total); }

// ---- the layout's verdict of a stream whose room, if it takes any, begins at off
ZD_HD PackedVerdict packed_verdict(const StreamResult &sized, uint64_t off, uint64_t max_out_len, uint64_t dst_arena_len) {
  PackedVerdict v;
  v.status = packed_sized_status(sized, max_out_len);
  v.roomed = packed_takes_room(sized, max_out_len) ? 1u : 0u;
  v.dst_off = v.roomed ? off : 0;
  if (v.roomed && !packed_fits(off, sized.out_len, dst_arena_len)) v.status = ST_DST_TOO_SMALL;
  return v;
}
// The descriptor inflate runs with.  `sd`: the stream as inflate is to read it (the caller's descriptor; the zlib form: the
// body's, zlib.hip zlib_open_kernel).  A stream with room that fits: into exactly its room, dst_cap = its size.  Every
// other one goes through as a stream of no bytes and no room (zlib.hip zlib_no_stream, recode_rules.h recode_no_stream):
// inflate reports a corrupted stream for it and stores nothing, and the verdict stands in its place.
ZD_HD StreamDesc packed_inner_desc(const StreamDesc &sd, const PackedVerdict &v, uint64_t out_len) {
  StreamDesc in;
  in.src_off = sd.src_off; in.limit = sd.limit; in.reserved = 0;
  if (v.status == ST_OK) { in.src_len = sd.src_len; in.dst_off = v.dst_off; in.dst_cap = out_len; in.flags = sd.flags; }
  else { in.src_len = 0; in.dst_off = 0; in.dst_cap = 0; in.flags = 0; in.limit = 0; }
  return in;
}

// ---- close: the caller's result.  The decoder's word counts for a stream that reached it; a stream without room, or
// with room that did not fit, says so and has no bytes -- the latter still says where the rule put it.
ZD_HD PackedResult packed_close(const PackedVerdict &v, const StreamResult &decoded) {
  PackedResult r;
  r.dst_off = v.dst_off; r.reserved = 0;
  if (v.status == ST_OK) { r.status = decoded.status; r.checksum = decoded.checksum; r.out_len = decoded.out_len; }
  else { r.status = v.status; r.checksum = 0; r.out_len = 0; }
  return r;
}

}  // namespace zd
