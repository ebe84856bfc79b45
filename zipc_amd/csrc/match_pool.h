// match_pool.h -- how a wave of lz_match_runs_pool (deflate_lane.h) hands the positions of its chunk to the run slots that
// finish, and while it may run its loop in the STEADY form.  HIP-free: the kernel and tests/test_match_pool_form.py (g++,
// tests/match_pool_sim) compile the same rules.
#pragma once

#include "zd_common.h"

namespace zd {

constexpr uint32_t POOL_CHUNK = 256;  // >= 64 * NP: a fresh chunk serves any one handout.  Measured, same box, 128 / 256 / 512:
                                      // C2 5.58 / 5.44-5.48 / 5.83 ms, real text 145.5 / 150.1 / 167.5 ms

// Is every position of a chunk that ends at cend (one past its last position) MAX_MATCH_LEN or more from the stream's end:
// cend - 1 + MAX_MATCH_LEN <= len.  Such a position's matches are capped by MAX_MATCH_LEN alone, never by the end.  (The
// subtraction is on len's side and guarded: nothing wraps for a stream near 4 GiB.)
ZD_HD bool match_chunk_steady(uint32_t cend, uint32_t len) {
  return len >= (uint32_t)MAX_MATCH_LEN - 1u && cend <= len - ((uint32_t)MAX_MATCH_LEN - 1u);
}

// One handout: `taken` run slots of a wave finish in the same iteration, the rank-th of them (0 .. taken - 1) asks.  The
// wave's chunk has [next, cend) left.  fresh: the chunk runs out within this handout (taken > cend - next) and the pool
// was asked for another, [c, ce) -- empty (c == ce) once the pool is.  np: the position the slot takes if np < lim; else
// it gets none and lim is where it parks.  next, cend: the wave's chunk afterwards.
// (positions are formed as "start + offset if offset < what is left, else the limit": a stream may end within a chunk of
// 2^32 and a sum must not wrap into a position that looks valid)
struct MatchHandout { uint32_t np, lim, next, cend; };
ZD_HD MatchHandout match_handout(uint32_t rank, uint32_t taken, uint32_t next, uint32_t cend, bool fresh, uint32_t c, uint32_t ce) {
  const uint32_t rem = cend - next;
  MatchHandout h{rank < rem ? next + rank : cend, cend, 0u, cend};
  if (fresh) {
    if (rank >= rem) { h.np = rank - rem < ce - c ? c + (rank - rem) : ce; h.lim = ce; }
    h.next = ce - c > taken - rem ? c + (taken - rem) : ce;
    h.cend = ce;
  } else {
    h.next = rem > taken ? next + taken : cend;
  }
  return h;
}

// Does a wave in the steady form stay in it over this handout?  Its invariant: every run slot holds a real position whose
// maxlen is MAX_MATCH_LEN.  So every finishing slot must get a position -- the old chunk serves them all, or the fresh one
// is a whole chunk (which holds more than a handout's 64 NP can take) -- and the fresh chunk's positions must be steady
// ones.  The old chunk's are: the wave was steady when it took it.
ZD_HD bool match_handout_steady(uint32_t taken, uint32_t next, uint32_t cend, bool fresh, uint32_t c, uint32_t ce, uint32_t len) {
  if (!fresh) return taken <= cend - next;
  return ce - c == POOL_CHUNK && match_chunk_steady(ce, len);
}

// The steady form's common case (!fresh, and match_handout_steady said yes): match_handout is an add.
ZD_HD MatchHandout match_handout_within(uint32_t rank, uint32_t taken, uint32_t next, uint32_t cend) {
  return MatchHandout{next + rank, cend, next + taken, cend};
}

}  // namespace zd
