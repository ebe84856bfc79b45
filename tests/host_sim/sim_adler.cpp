// Host model of the Adler-32 chunk chain (zipc_amd/csrc/checksum.hip: adler_runs_s1, adler_scan_runs, adler_runs_a,
// adler_scan_runs, adler_replay; adler_rfc_finish) and of crc32_finish_kernel's grid over the partials.
// TEST TOOLING ONLY.  Every decision is zipc_amd/csrc/adler_chain.h, the file the kernels compile; here the launches
// are loops over "threads", the two scans are plain exclusive prefixes mod p, and the ambiguous records -- which the
// device appends in the order its atomics happen to land -- are appended in a shuffled order.  n_runs and REPLAY_MAX
// can be set small, so that tens of chunks reach every branch.
#include <stdint.h>
#include <algorithm>
#include <random>
#include <vector>
#include "../../zipc_amd/csrc/adler_chain.h"

using namespace zd;

namespace {
struct Sums { uint32_t x, y; };
std::vector<Sums> pack(const uint32_t *S1, const uint32_t *S2, uint64_t n) {
  std::vector<Sums> v(n);
  for (uint64_t k = 0; k < n; k++) v[k] = Sums{S1[k], S2[k]};
  return v;
}
}  // namespace

enum { ADLER_PATH_REPLAY = 0, ADLER_PATH_WALK = 1 };

// api.hip's shape of the chain for a buffer of len bytes: out = n_chunks, n_runs, per
extern "C" void sim_adler_shape(uint64_t len, uint64_t *out) {
  out[0] = adler_n_chunks(len);
  out[1] = adler_n_runs(out[0]);
  out[2] = adler_per(out[0], (uint32_t)out[1]);
}

// The five launches over the chunk sums of a buffer of len bytes (n_chunks must be adler_n_chunks(len): -1 otherwise).
// n_runs, replay_max, amb_cap: 0 for the product's.  info = path, ambiguous chunks counted, n_runs, per.
extern "C" int sim_adler_chain(const uint32_t *S1, const uint32_t *S2, uint64_t n_chunks, uint64_t len, uint32_t n_runs,
                               uint32_t replay_max, uint32_t amb_cap, uint32_t seed, uint32_t *value, uint64_t *info) {
  if (n_chunks != adler_n_chunks(len)) return -1;
  const std::vector<Sums> sums = pack(S1, S2, n_chunks);
  const uint32_t r = (uint32_t)(len % ADLER_CHUNK);
  if (!n_runs) n_runs = adler_n_runs(n_chunks);
  if (!replay_max) replay_max = REPLAY_MAX;
  if (!amb_cap) amb_cap = ADLER_AMB_CAP;
  const uint64_t per = adler_per(n_chunks, n_runs);
  // the per-run arrays (kernels.h AdlerRuns).  The device's hold n_runs entries, all written; the slack behind them
  // reads as empty runs, so that a mutant of the run arithmetic gives a wrong value, not a wild read
  const size_t slots = (size_t)n_runs + n_chunks + 2;
  std::vector<uint32_t> sum(slots, 0), s1_before(slots, 0), s1_after(slots, 0), last_hi(slots, 0xFFFFFFFFu), res_before(slots, 0);
  // adler_runs_s1
  for (uint32_t run = 0; run < n_runs; run++) {
    uint64_t lo, hi, acc = 0;
    adler_run_bounds(run, per, n_chunks, lo, hi);
    for (uint64_t k = lo; k < hi; k++) acc += sums[k].x;
    sum[run] = (uint32_t)(acc % ADLER_BASE);
  }
  // adler_scan_runs, first = 1
  uint32_t pre = 1u % ADLER_BASE;
  for (uint32_t run = 0; run < n_runs; run++) { s1_before[run] = pre; pre = addmod(pre, sum[run]); }
  // adler_runs_a
  std::vector<AmbRecord> found;
  for (uint32_t run = 0; run < n_runs; run++) {
    uint64_t lo, hi;
    adler_run_bounds(run, per, n_chunks, lo, hi);
    uint64_t s1 = s1_before[run], a_acc = 0;
    uint32_t lh = 0xFFFFFFFFu;
    for (uint64_t k = lo; k < hi; k++) {
      AmbRecord rec;
      if (adler_runs_a_step(k, adler_chunk_len(k, r), sums[k].x, sums[k].y, s1, a_acc, lh, rec)) found.push_back(rec);
    }
    sum[run] = (uint32_t)a_acc;
    last_hi[run] = lh;
    s1_after[run] = (uint32_t)s1;
  }
  std::mt19937 rng(seed);
  std::shuffle(found.begin(), found.end(), rng);  // the atomics' order
  const uint32_t n_amb = (uint32_t)found.size();  // amb_count counts them all; the list keeps amb_cap
  std::vector<AmbRecord> amb(found.begin(), found.begin() + std::min<size_t>(found.size(), amb_cap));
  // adler_scan_runs, first = 0
  pre = 0;
  for (uint32_t run = 0; run < n_runs; run++) { res_before[run] = pre; pre = addmod(pre, sum[run]); }
  // adler_replay
  info[1] = n_amb; info[2] = n_runs; info[3] = per;
  if (adler_replay_falls_back(n_amb, amb_cap, replay_max)) {
    info[0] = ADLER_PATH_WALK;
    *value = adler_plain_walk(sums.data(), n_chunks, r);
    return 0;
  }
  info[0] = ADLER_PATH_REPLAY;
  std::vector<ReplayRecord> rec(n_amb);
  for (uint32_t i = 0; i < n_amb; i++) {  // rank sort (chunk indices are distinct)
    uint32_t rank = 0;
    for (uint32_t j = 0; j < n_amb; j++) rank += amb[j].k < amb[i].k ? 1u : 0u;
    rec[rank] = adler_replay_prepare(amb[i], r, sums[amb[i].k].y, per, res_before.data(), last_hi.data());
  }
  ReplayState st;
  for (uint32_t i = 0; i < n_amb; i++) adler_replay_step(st, rec[i].k, rec[i].res, rec[i].C, rec[i].pc, rec[i].prev != 0);
  *value = adler_replay_final(st, n_chunks, per, res_before.data(), sum.data(), last_hi.data(), s1_after.data());
  return 0;
}

// the serial walk with adler_chunk_step (zd_common.h), the reference's order
extern "C" int sim_adler_serial(const uint32_t *S1, const uint32_t *S2, uint64_t n_chunks, uint64_t len, uint32_t *value) {
  if (n_chunks != adler_n_chunks(len)) return -1;
  const std::vector<Sums> sums = pack(S1, S2, n_chunks);
  *value = adler_plain_walk(sums.data(), n_chunks, (uint32_t)(len % ADLER_CHUNK));
  return 0;
}

// adler_rfc_finish_kernel: a run per thread, chained by thread 0
extern "C" int sim_adler_rfc(const uint32_t *S1, const uint32_t *S2, uint64_t n_chunks, uint64_t len, uint32_t *value) {
  if (n_chunks != adler_n_chunks(len)) return -1;
  const std::vector<Sums> sums = pack(S1, S2, n_chunks);
  std::vector<uint32_t> a1(ADLER_RFC_THREADS), a2(ADLER_RFC_THREADS);
  std::vector<uint64_t> nb(ADLER_RFC_THREADS);
  for (uint32_t t = 0; t < ADLER_RFC_THREADS; t++) {
    uint64_t lo, hi;
    adler_run_bounds(t, adler_rfc_per(n_chunks), n_chunks, lo, hi);
    adler_rfc_fold_run(sums.data(), lo, hi, (uint32_t)(len % ADLER_CHUNK), a1[t], a2[t], nb[t]);
  }
  *value = adler_rfc_chain(a1.data(), a2.data(), nb.data(), ADLER_RFC_THREADS);
  return 0;
}

// crc32_finish_kernel's reads of a range of nseg partials, launched for `segs` declared segments (NT: 0 for the
// launch's rule).  used[q] is the partial that enters the fold at place q (-1: a virtual zero), places in the order
// the fold shifts them: a Horner step over a row shifts by NT places, the tree over the threads by 1, 2, 4 ...  so
// place q = row * NT + t.  loaded[] are the words the threads fetch, rows of a batch of eight behind the last row
// included.  info = NT, rows, padp, 1 if one thread folds the range.  -> places (0: nothing to fold)
extern "C" uint64_t sim_crc_finish_grid(uint64_t nseg, uint64_t segs, uint32_t NT, int64_t *used, uint64_t used_cap, uint64_t *loaded,
                                        uint64_t loaded_cap, uint64_t *n_loaded, uint64_t *info) {
  if (!NT) NT = crc_finish_threads(segs);
  info[0] = NT; info[1] = 0; info[2] = 0; info[3] = 0;
  *n_loaded = 0;
  uint64_t nu = 0, nl = 0;
  if (nseg <= 1 || crc_finish_by_one_thread(nseg)) {
    info[3] = 1;
    for (uint64_t j = 0; j < nseg; j++) {
      if (nu < used_cap) used[nu] = (int64_t)j;
      if (nl < loaded_cap) loaded[nl] = j;
      nu++; nl++;
    }
    *n_loaded = nl;
    return nu;
  }
  const uint64_t R = crc_finish_rows(nseg, NT), padp = crc_finish_padp(nseg, NT);
  info[1] = R; info[2] = padp;
  for (uint64_t j0 = 0; j0 < R; j0 += CRC_FINISH_ROWS_AT_ONCE)
    for (uint64_t u = 0; u < CRC_FINISH_ROWS_AT_ONCE; u++)
      for (uint32_t t = 0; t < NT; t++) {
        const int64_t idx = crc_finish_index(j0 + u, NT, t, padp);
        if (nl < loaded_cap) loaded[nl] = crc_finish_load_index(idx, j0 + u, R);
        nl++;
        if (j0 + u < R) {  // the rows the fold takes
          if (nu < used_cap) used[nu] = idx >= 0 ? idx : -1;
          nu++;
        }
      }
  *n_loaded = nl;
  return nu;
}
