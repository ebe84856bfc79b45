// zipc_amd/csrc/match_pool.h behind a C view, and a serial model of one tile's pool built on it.  TEST TOOLING ONLY: the
// very rules by which a wave of lz_match_runs_pool (deflate_lane.h) hands out its chunk's positions and stays in, or
// leaves, the steady form of its loop -- so that tests/test_match_pool_form.py can enumerate the predicate and walk whole
// tiles through the handouts.  The header's path can be set from outside (the test's mutants compile a changed copy).
#include <stdint.h>

#include <random>
#include <vector>

#ifndef MATCH_POOL_H
#define MATCH_POOL_H "../../zipc_amd/csrc/match_pool.h"
#endif
#include MATCH_POOL_H

extern "C" int sim_match_chunk_steady(uint32_t cend, uint32_t len) { return zd::match_chunk_steady(cend, len) ? 1 : 0; }
extern "C" uint32_t sim_pool_chunk(void) { return zd::POOL_CHUNK; }

// One handout by match_handout, for every rank: out[4 rank ..] = np, lim, next, cend
extern "C" void sim_match_handout(uint32_t taken, uint32_t next, uint32_t cend, int fresh, uint32_t c, uint32_t ce, uint32_t *out) {
  for (uint32_t rank = 0; rank < taken; rank++) {
    const zd::MatchHandout h = zd::match_handout(rank, taken, next, cend, fresh != 0, c, ce);
    out[4 * rank] = h.np; out[4 * rank + 1] = h.lim; out[4 * rank + 2] = h.next; out[4 * rank + 3] = h.cend;
  }
}

namespace {
constexpr int WAVES = 16, LANES = 64, NP = 2;  // deflate.hip MATCHW_THREADS / 64, MATCHW_NP
struct Run { uint32_t p; bool alive; uint32_t left; };  // left: iterations until the position is finished
struct Wave {
  uint32_t next = 0, cend = 0;
  bool empty = false, steady = false, done = false;
  Run r[NP][LANES];
};
struct Tile {
  uint32_t len, pbeg, pend, pool_next = 0;
  const uint32_t *steps;
  uint32_t *handed;
  uint64_t *stats;
  uint32_t take() {  // TilePool::take without a taper
    const uint32_t c = pool_next;
    pool_next += zd::POOL_CHUNK;
    return c < pend - pbeg ? pbeg + c : pend;
  }
  uint32_t chunk_end(uint32_t c) const { return pend - c > zd::POOL_CHUNK ? c + zd::POOL_CHUNK : pend; }
  void give(Run &r, uint32_t p) {  // the run takes position p
    r.p = p;
    if (p >= pbeg && p < pend) { handed[p]++; r.left = steps[p] ? steps[p] : 1u; }
    else { stats[4]++; r.left = 1u; }  // not a position of the tile: only a broken rule gets here
  }
  void start(Wave &w) {
    w.next = take();
    w.cend = chunk_end(w.next);
    w.empty = w.next >= pend;
    w.steady = w.cend - w.next == zd::POOL_CHUNK && zd::match_chunk_steady(w.cend, len);
    stats[2] += w.steady;
    for (int i = 0; i < NP; i++)
      for (int l = 0; l < LANES; l++) {
        const uint32_t off = (uint32_t)l + 64u * (uint32_t)i;
        const uint32_t p = off < w.cend - w.next ? w.next + off : w.cend;
        Run &r = w.r[i][l];
        r.alive = p < w.cend;
        r.p = p; r.left = 1u;
        if (r.alive) give(r, p);
      }
    w.next = w.cend - w.next > 64u * NP ? w.next + 64u * NP : w.cend;
  }
  // one iteration of the wave's loop: a step of both run slots, each with its handout
  void iterate(Wave &w) {
    stats[1]++;
    stats[0] += w.steady;
    for (int i = 0; i < NP; i++) {
      if (w.steady)  // the steady form's invariant: every run holds a real position whose maxlen is MAX_MATCH_LEN
        for (int l = 0; l < LANES; l++) {
          const Run &r = w.r[i][l];
          if (!(r.alive && r.p >= pbeg && r.p < pend && len - r.p >= (uint32_t)zd::MAX_MATCH_LEN)) stats[3]++;
        }
      bool fin[LANES];
      uint32_t rank[LANES], taken = 0;
      for (int l = 0; l < LANES; l++) {
        Run &r = w.r[i][l];
        fin[l] = r.alive && --r.left == 0;
        rank[l] = taken;
        taken += fin[l];
      }
      if (!taken) continue;
      bool given = false;
      uint32_t gc = 0;
      if (w.steady) {
        bool stay = true, fresh = false;
        uint32_t c = 0, ce = 0;
        if (!zd::match_handout_steady(taken, w.next, w.cend, false, 0u, 0u, len)) {
          c = take();
          ce = chunk_end(c);
          fresh = true;
          stay = zd::match_handout_steady(taken, w.next, w.cend, true, c, ce, len);
        }
        if (stay) {
          zd::MatchHandout h{};
          for (int l = 0; l < LANES; l++) {
            h = fresh ? zd::match_handout((uint32_t)rank[l], taken, w.next, w.cend, true, c, ce)
                      : zd::match_handout_within((uint32_t)rank[l], taken, w.next, w.cend);
            if (fin[l]) give(w.r[i][l], h.np);  // (no test of np: the steady form makes none)
          }
          w.next = h.next;
          w.cend = h.cend;
          continue;
        }
        w.steady = false;  // this handout, with its chunk fetched, and the rest of the iteration are the general form's
        stats[5]++;
        given = true;
        gc = c;
      }
      const bool fresh = taken > w.cend - w.next && !w.empty;
      uint32_t c = 0, ce = 0;
      if (fresh) {
        c = given ? gc : take();
        ce = chunk_end(c);
        w.empty = c >= pend;
      } else if (given) {
        stats[4]++;  // a fetched chunk the general handout does not take would be lost
      }
      zd::MatchHandout h{};
      for (int l = 0; l < LANES; l++) {
        h = zd::match_handout(rank[l], taken, w.next, w.cend, fresh, c, ce);
        if (!fin[l]) continue;
        Run &r = w.r[i][l];
        r.alive = h.np < h.lim;
        if (r.alive) give(r, h.np);
      }
      w.next = h.next;
      w.cend = h.cend;
    }
    if (!w.steady) {
      bool alive = false;
      for (int i = 0; i < NP; i++)
        for (int l = 0; l < LANES; l++) alive |= w.r[i][l].alive;
      w.done = !alive;
    }
  }
};
}  // namespace

// The pool of the tile [pbeg, pend) of a stream of len bytes, its 16 waves served one iteration at a time in an order drawn
// from seed.  steps[p]: the iterations position p takes.  handed[p] (len entries, zeroed by the caller) counts how often p
// was handed to a run.  stats: [0] iterations a wave began in the steady form  [1] iterations  [2] waves that entered the
// steady form  [3] runs met in the steady form without a real position of maxlen MAX_MATCH_LEN  [4] handouts of something
// that is no position of the tile (or a fetched chunk lost)  [5] waves that left the steady form.  Returns 0, or 1 when the
// waves do not come to an end.
extern "C" int sim_match_pool_tile(uint32_t len, uint32_t pbeg, uint32_t pend, const uint32_t *steps, uint32_t seed, uint32_t *handed,
                                   uint64_t *stats) {
  Tile t{len, pbeg, pend, 0u, steps, handed, stats};
  for (int i = 0; i < 6; i++) stats[i] = 0;
  std::vector<Wave> waves(WAVES);
  std::mt19937 rng(seed);
  {  // the waves take their first chunks before any of them iterates, in an order of the seed's
    int order[WAVES];
    for (int w = 0; w < WAVES; w++) order[w] = w;
    for (int w = WAVES - 1; w > 0; w--) std::swap(order[w], order[rng() % (uint32_t)(w + 1)]);
    for (int w = 0; w < WAVES; w++) t.start(waves[order[w]]);
  }
  uint64_t budget = 64ull * WAVES + 1000ull;  // every iteration but a wave's last brings some position a step nearer its end
  for (uint32_t p = pbeg; p < pend; p++) budget += steps[p] ? steps[p] : 1u;
  for (;;) {
    int live[WAVES], n = 0;
    for (int w = 0; w < WAVES; w++)
      if (!waves[w].done) live[n++] = w;
    if (!n) return 0;
    if (!budget--) return 1;
    t.iterate(waves[live[rng() % (uint32_t)n]]);
  }
}
