// deflate_scratch.h -- the layout of the deflate pipeline's scratch (ctx->deflate_scratch), free of HIP: deflate.hip
// carves it, api.hip sizes it, tests/host_sim/sim_forms.cpp holds the sizes to the sums written out in its test.
#pragma once

#include <type_traits>

#include "deflate_lane.h"
#include "forms.h"

namespace zd {

struct DeflateScratch {
  uint64_t *pos_base;   // [n] first position slot of stream i
  uint64_t *blk_base;   // [n] first BlockDesc slot of stream i
  uint32_t *n_blocks;   // [n]
  uint32_t *error;      // [1] != 0: the batch does not fit what the caller declared (total_src_len too small,
                        //     or a stream longer than max_src_len: the grids are sized from it)
  uint16_t *prev;       // [P] chain links
  uint32_t *match;      // [P] lz_match_position's best of the first K candidates (dist << 9 | len, 0: none) | MATCH_SNAP when the best of the
                        //     first K/4 is another: that one is then in snap[] (round 5: 4 bytes a position where 8 were written and read)
  uint32_t *snap;       // [P] the best of the first K/4, written for positions with MATCH_SNAP only
  uint32_t *snap_used;  // [n] != 0: the stream has such positions (its parse then reads both tables side by side; zeroed by deflate_offsets_kernel)
  uint32_t *syms;       // [P]
  BlockDesc *blocks;    // [Bk]
  uint64_t cap_positions, cap_blocks;
};

// The scratch of a group of n streams of total_src_len bytes (forms.h deflate_grouping), each array on a 256-byte boundary.
// Carves them from base and returns the end: from 0, that is the size to allocate -- ONE layout for the size and the pointers.
inline uintptr_t carve_deflate_scratch(uintptr_t base, size_t n, size_t total_src_len, int level, DeflateScratch &s) {
  uintptr_t q = base;
  auto take = [&q](auto *&p, size_t bytes) {
    p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(q);
    q += align_up(bytes, 256);
  };
  s = DeflateScratch{};
  scratch_caps(n, total_src_len, s.cap_positions, s.cap_blocks);
  const uint64_t P = s.cap_positions;
  take(s.pos_base, n * 8);
  take(s.blk_base, n * 8);
  take(s.n_blocks, n * 4);
  take(s.snap_used, n * 4);
  take(s.error, 256);
  if (level != LEVEL_NONE) {
    take(s.prev, P * 2);
    take(s.match, P * 4);
    take(s.snap, P * 4);
    take(s.syms, P * 4);
    take(s.blocks, s.cap_blocks * sizeof(BlockDesc));
  }
  return q;
}

// bytes of scratch a call needs: its largest group's, and a KiB to spare
inline size_t deflate_scratch_bytes(size_t n_all, size_t max_src_len, size_t total_all, int level, const Tuning &t) {
  size_t n, total_src_len;
  deflate_grouping(n_all, max_src_len, total_all, t, n, total_src_len);
  DeflateScratch s;
  return (size_t)carve_deflate_scratch(0, n, total_src_len, level, s) + 1024;
}

}  // namespace zd
