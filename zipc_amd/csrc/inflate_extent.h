// inflate_extent.h -- the rule of the extent forms (zipc_hip_inflate_extent_batch, zipc_hip_inflate_size_extent_batch,
// zipc_hip_inflate_size_extent_blocks_batch and their zlib forms): free of HIP, pure functions of plain numbers.
//
// Every decode form ignores what lies behind the final block, as the reference does (inflate_and_crc returns at the BFINAL
// block, zd.ml:692-709), so src_len may be an upper bound of the stream's length -- and a raw deflate stream carries no
// length of its own.  The extent forms say where the stream ended: src_used, the count of source bytes from src_off up
// to and including the byte that holds the last bit of the final block.
//
// The decoder already ends with that bit.  The stream's wave (inflate.hip inflate_wave) leaves InflateLane::in_word /
// boff exactly behind the final block in every way such a block ends:
//   a stored block      lane_block_header sets the position behind the block's last data byte when it reads LEN
//                       (LEN == 0: behind NLEN), before the cooperative copy; lane_after_copy moves the output only;
//   an end-of-block     is decoded by lane_one_symbol or lane_one_symbol_fixed alone (the wide turns' tables, the strided
//                       turn and the span decoder stop IN FRONT of it: inflate_span.h), which advance() by its bits;
//   the span's commit   ends in front of the first symbol it must not decode, so never behind an end-of-block;
//   a fixed block       whose tables were built after its table-free symbols ends through lane_one_symbol as above.
// InflateLane::advance carries into in_word when boff wraps, so the pair is one number: in_word * 32 + boff, returned
// as BlockEnd::end_bit.  By blocks, the chain walks from true end bit to true end bit (inflate_blocks.h), and the head
// returns the same BlockEnd.  The kernels and the host model (tests/extent_sim/sim_extent.cpp) compile this text.
#pragma once

#include "zd_common.h"

namespace zd {

// zipc_hip_extent_result (include/zipc_hip.h): StreamResult's three fields, then the extent
struct ExtentResult {
  uint32_t status;
  uint32_t checksum;
  uint64_t out_len;
  uint64_t src_used;
  uint64_t reserved;  // 0
};
static_assert(sizeof(ExtentResult) == 32, "include/zipc_hip.h");

// end_bit: the first bit behind the final block -- behind the end-of-block symbol of a compressed block, behind the last
// data byte of a stored one (LEN == 0 included).  The bytes that hold the bits in front of it:
ZD_HD uint64_t extent_bytes(uint64_t end_bit) { return (end_bit + 7u) / 8u; }

// The stream's result from what its decoder ended with.  A stream that is refused has no extent, and nothing may be read
// into a partial one: every field but the status is 0.
ZD_HD ExtentResult extent_result(uint32_t status, uint32_t checksum, uint64_t out_len, uint64_t end_bit) {
  ExtentResult r;
  r.status = status; r.checksum = 0; r.out_len = 0; r.src_used = 0; r.reserved = 0;
  if (status == ST_OK) { r.checksum = checksum; r.out_len = out_len; r.src_used = extent_bytes(end_bit); }
  return r;
}

// The decode form with CRC-32: the checksum pass behind the kernel ran over a StreamResult of the stream's (its status and
// length) and left there the CRC-32 -- or its own refusal: a stream whose output is longer than the call's max_dst_cap is
// ST_INVALID_ARG, as in zipc_hip_inflate_batch (its checksum would cover only a part).  A refusal of the pass is the
// stream's status like any other: no checksum, no length, no extent.  A record that was not OK stays as it is.
ZD_HD ExtentResult extent_with_crc(ExtentResult r, uint32_t pass_status, uint32_t crc) {
  if (r.status != ST_OK) return r;
  if (pass_status != ST_OK) return extent_result(pass_status, 0, 0, 0);
  r.checksum = crc;
  return r;
}

// Sizing by blocks (inflate_blocks.h size_blocks_verdict): a stream that is sized by a head that saw the final block ends
// where the head ended; every other sized stream ends where its chain's last block -- the final one: chain_ok -- ended.
ZD_HD uint64_t size_blocks_end_bit(uint32_t head_final, uint64_t head_end_bit, uint64_t chain_last_end_bit) {
  return head_final != 0u ? head_end_bit : chain_last_end_bit;
}

}  // namespace zd
