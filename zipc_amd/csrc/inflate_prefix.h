// inflate_prefix.h -- the rule of the prefix forms (zipc_hip_inflate_prefix_batch, zipc_hip_zlib_decompress_prefix_batch):
// free of HIP, pure functions of plain numbers.
//
// The stream's wave in its prefix form (inflate.hip inflate_prefix_kernel) is the decoder of zipc_hip_inflate_batch up to
// the one symbol that does not fit the room.  That symbol is met by the plain lane step at four places of inflate_lane.h
// -- a stored block, a match, a literal of either symbol step -- each of which has made the reference's checks of the
// symbol by then (a distance beyond the output is ST_CORRUPTED before the room is looked at, zd.ml:614) and asks here,
// with the symbol's length still at hand: cut, or fail as ever?  A cut writes the part of the symbol that fits and ends
// the stream, status OK and not ended; nothing behind it is read.  The kernel and the host model
// (tests/prefix_sim/sim_prefix.cpp) compile this text.
#pragma once

#include "zd_common.h"

namespace zd {

// zipc_hip_prefix_result (include/zipc_hip.h): the layout of StreamResult with `ended` where the checksum is
struct PrefixResult {
  uint32_t status;
  uint32_t ended;
  uint64_t out_len;
};

// A stream that was cut, while its wave is still running (InflateLane::status): never stored in a result
constexpr uint32_t ST_PREFIX_CUT = 0x100u;

// The symbol needs the output to reach `need` bytes and the room (cap_min = min(limit, dst_cap)) ends before that.
// zipc_hip_inflate_batch reports ST_SIZE_EXCEEDED when need > limit and ST_DST_TOO_SMALL otherwise (InflateLane::overflow);
// the prefix form cuts exactly where that is ST_DST_TOO_SMALL.  (Then limit >= need > cap_min: the room is dst_cap.)
ZD_HD bool prefix_cuts(uint64_t need, uint32_t limit) { return need <= (uint64_t)limit; }
// bytes of the cut symbol that fit: the room behind the whole symbols before it (0 for a literal: out_pos == cap_min there)
ZD_HD uint32_t prefix_cut_len(uint32_t out_pos, uint32_t cap_min) { return cap_min - out_pos; }
// where they come from: a match's `dist` bytes back in the output (the periodic copy of Buf.recopy, cut short), a stored
// block's at its first byte in the input
ZD_HD uint32_t prefix_match_from(uint32_t out_pos, uint32_t dist) { return out_pos - dist; }
ZD_HD uint32_t prefix_stored_from(uint32_t block_pos) { return block_pos; }

// The stream's result from what its wave ended with: ended -- the final block's end was read with room to spare or none
// needed; cut -- the room is full, to its last byte; anything else is the stream's own error and no bytes.
ZD_HD PrefixResult prefix_result(uint32_t status, uint32_t out_pos, uint32_t cap_min) {
  PrefixResult r;
  if (status == ST_OK) { r.status = ST_OK; r.ended = 1; r.out_len = out_pos; }
  else if (status == ST_PREFIX_CUT) { r.status = ST_OK; r.ended = 0; r.out_len = cap_min; }
  else { r.status = status; r.ended = 0; r.out_len = 0; }
  return r;
}

}  // namespace zd
