// How many iterations of the walk's loop every position of a stream takes: deflate_lane.h's match_run_start and
// match_run_step_to -- the step the device's loop is written after -- run position by position over the links given (the
// test passes sim_chain_serial's).  TEST TOOLING ONLY: what tests/match_pool_sim/sim_match_pool.cpp's model of the pool
// lets a run spend on a position.  Every position's record is held to lz_match_position on the way.
#include "../../zipc_amd/csrc/deflate_lane.h"

// steps[p] for p = 0 .. len - 4.  Returns the number of positions whose record is not lz_match_position's.
extern "C" uint32_t sim_match_steps(const uint8_t *src, uint32_t len, const uint16_t *links, int K, int Kq, uint32_t *steps) {
  uint32_t wrong = 0;
  if (len < 4) return 0;
  for (uint32_t p = 0; p + 4 <= len; p++) {
    zd::MatchRun r;
    zd::match_run_start<false>(r, src, len, p, len - 3u, links);
    uint64_t rec = ~0ull;
    uint32_t n = 0;
    bool fin = false;
    while (!fin) {
      fin = zd::match_run_step_to<false>(r, src, links, (uint32_t)K, (uint32_t)Kq, [&](uint32_t at, uint32_t best, uint32_t snap) {
        rec = at == p ? (uint64_t)best | ((uint64_t)snap << 32) : ~0ull;
      });
      n++;
    }
    steps[p] = n;
    wrong += rec != zd::lz_match_position(src, len, p, links, K, Kq);
  }
  return wrong;
}
