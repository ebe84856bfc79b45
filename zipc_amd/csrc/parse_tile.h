// parse_tile.h -- which of its two forms lz_parse_wave (deflate.hip) runs a tile of 64 positions in.  HIP-free: the kernel
// and tests/test_parse_tile_form.py (g++) compile the same predicate.
#pragma once

#include "zd_common.h"

namespace zd {

// One past the last source byte a tile's own loads touch: the literal word of lane 63, three tiles ahead of the tile's
// first position (3 * 64 + 63 + 4 bytes).  The table loads of the same tile end 3 * 64 + 64 entries behind it, inside
// PARSE_PAD whatever the length.
constexpr uint32_t PARSE_TILE_REACH = 4u * 64u + 3u;
// The furthest a macro step advances: 255 deferral literals and a match of MAX_MATCH_LEN.
constexpr uint32_t PARSE_STEP_MAX = 255u + (uint32_t)MAX_MATCH_LEN;

// The interior form of the tile at B (a multiple of 64, below len): every lane's position lies in the stream and has a table
// entry, the look-ahead loads need no clamp and the lanes' literal bytes are the low bytes of their words (B + 259 <= len),
// and -- where the wave cuts blocks (cuts: one wave per stream; blk_start: the open block's first position, at most
// B + 63 + 255) -- no step of the tile can end past the block's 65534 bytes: the last lane's step ends at most
// B + 63 + 513 - blk_start bytes into it.  Everything else is the edge form, which is the general one.
// (32-bit arithmetic: B < len <= MAX_STREAM_LEN leaves 64 KiB of headroom, and blk_start <= B + 318 keeps the
// difference positive)
ZD_HD bool parse_tile_interior(uint32_t B, uint32_t len, uint32_t blk_start, bool cuts) {
  if (B + PARSE_TILE_REACH > len) return false;
  return !cuts || B + 63u + PARSE_STEP_MAX - blk_start <= (uint32_t)MAX_BLOCK_SRC_LEN;
}

// The same condition as ONE bound, for a loop that asks it per tile: the tiles B < parse_interior_end(..) are the interior
// ones (both halves of the predicate only grow with B).  The bound changes where blk_start does: at a block cut.
ZD_HD uint32_t parse_interior_end(uint32_t len, uint32_t blk_start, bool cuts) {
  const uint32_t by_len = len >= PARSE_TILE_REACH ? len - PARSE_TILE_REACH + 1u : 0u;
  const uint32_t by_cut = blk_start + ((uint32_t)MAX_BLOCK_SRC_LEN - 63u - PARSE_STEP_MAX) + 1u;  // (<= MAX_STREAM_LEN + 64 Ki: no wrap)
  return !cuts || by_len < by_cut ? by_len : by_cut;
}

}  // namespace zd
