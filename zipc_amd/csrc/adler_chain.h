// adler_chain.h -- every arithmetic decision of the Adler-32 chunk chain and of the CRC-32 finish's index grid: free of HIP.
//
// checksum.hip keeps the launches, the LDS staging, the rank sort and the scans; what a thread DECIDES between them is a
// function here, so that the same code is compiled twice:
//   * into libzipc_hip.so (checksum.hip's adler_* and crc32_finish kernels, api.hip's zipc_hip_checksum_device);
//   * into tests/host_sim/sim_adler.cpp with g++, where tests/test_adler_chain_sim.py runs the five launches as loops
//     against the serial walk and holds a mutation table over this file.
// The sums of a chunk come as any struct with members x (S1) and y (S2): uint2 on the device.
#pragma once

#include "zd_common.h"

namespace zd {

// The chunk chain (src/zipc_deflate.ml:196: s1/s2 := SIGNED rem after every chunk)
// for hundreds of thousands of chunks, without walking them one by one.
//   s1 never goes negative, so s1 before chunk k is (1 + sum of S1) mod 65521: a scan.
//   s2: with x = s2 before the chunk (|x| < 65521) the reference computes
//   srem32(wrap32(x + C)), C = n * s1 + S2 < 2^32.  Unless C lies within 65521 of 0
//   or of 2^31 the branch taken depends on C alone: below 2^31 the result is
//   (x + C) mod p >= 0, above it is congruent to x + C - 225 (2^32 mod 65521 = 225)
//   with a non-positive representative.  So the residues follow from a second scan
//   of a_k = C_k - 225 * hi_k; the few chunks whose branch does depend on x
//   ("ambiguous", about 6e-5 of them on random data) are then replayed exactly, in
//   order, by one thread, each replay shifting all later residues by a constant.
constexpr uint32_t ADLER_AMB_CAP = 8192;  // ambiguous-chunk records (16 bytes each)
constexpr uint32_t ADLER_MAX_RUNS = 65536;
constexpr uint32_t REPLAY_MAX = 4096;  // ambiguous chunks replayed out of LDS; more: plain walk

// chunk k of the reference's grid for a buffer of n bytes: chunk 0 is
// [0, n mod 5552) (possibly empty), chunk k >= 1 is 5552 bytes
ZD_HD uint64_t adler_n_chunks(uint64_t len) { return len ? len / ADLER_CHUNK + 1 : 0; }
ZD_HD uint32_t adler_chunk_len(uint64_t k, uint32_t r) { return k == 0 ? r : ADLER_CHUNK; }

// The chain runs over R runs of `per` consecutive chunks (R 1024 times a power of two, up to 64 Ki: a thread per run)
ZD_HD uint32_t adler_n_runs(uint64_t n_chunks) {
  uint32_t n_runs = 1024;  // one thread per run; at least ~8 chunks per run
  while (n_runs < ADLER_MAX_RUNS && (uint64_t)n_runs * 8 < n_chunks) n_runs *= 2;
  return n_runs;
}
ZD_HD uint64_t adler_per(uint64_t n_chunks, uint32_t n_runs) { return n_chunks ? (n_chunks + n_runs - 1) / n_runs : 1; }
// chunks [lo, hi) of a run (empty behind the last chunk)
ZD_HD void adler_run_bounds(uint64_t run, uint64_t per, uint64_t n_chunks, uint64_t &lo, uint64_t &hi) {
  lo = run * per < n_chunks ? run * per : n_chunks;
  hi = lo + per < n_chunks ? lo + per : n_chunks;
}

// (a + b) mod p for a, b <= p
ZD_HD uint32_t addmod(uint32_t a, uint32_t b) {
  const uint32_t s = a + b;
  return s >= ADLER_BASE ? s - ADLER_BASE : s;
}

// what pass 2 already knows about an ambiguous chunk, kept for the replay
struct AmbRecord {
  uint32_t k;          // chunk index
  uint32_t s1;         // s1 before the chunk
  uint32_t a_partial;  // sum of a_j over the chunks of its run before it (mod p)
  uint32_t prev_hi;    // branch of chunk k-1 as C_{k-1} alone decides it
};
static_assert(sizeof(AmbRecord) == 16, "the list is sized with 16 bytes per entry");

// ---- a chunk as adler_runs_a_kernel sees it: s1 before it (< p) and its sums
ZD_HD uint64_t adler_chunk_C(uint32_t len, uint64_t s1, uint32_t S2) { return (uint64_t)len * s1 + S2; }  // < 2^32
ZD_HD bool adler_chunk_hi(uint64_t C) { return C >= 0x80000000ull; }
ZD_HD bool adler_chunk_ambiguous(uint64_t C) {
  return C < ADLER_BASE || (C > 0x80000000ull - ADLER_BASE && C < 0x80000000ull + ADLER_BASE);
}
// a_k mod p: what the chunk adds to the residue of s2 if C alone decides its branch
ZD_HD uint32_t adler_chunk_a(uint64_t C, bool hi_k) {
  return addmod((uint32_t)(C % ADLER_BASE), hi_k ? ADLER_BASE - 225u : 0u);
}
ZD_HD AmbRecord adler_amb_record(uint64_t k, uint64_t s1, uint64_t a_acc, uint32_t last_hi) {
  AmbRecord rec;
  rec.k = (uint32_t)k;
  rec.s1 = (uint32_t)s1;
  rec.a_partial = (uint32_t)a_acc;
  rec.prev_hi = last_hi;
  return rec;
}
// one chunk of a run: -> whether it is ambiguous (`rec` is then its record); the run's state moves on
ZD_HD bool adler_runs_a_step(uint64_t k, uint32_t len, uint32_t S1, uint32_t S2, uint64_t &s1, uint64_t &a_acc,
                             uint32_t &last_hi, AmbRecord &rec) {
  const uint64_t C = adler_chunk_C(len, s1, S2);
  const bool hi_k = adler_chunk_hi(C);
  const bool ambiguous = adler_chunk_ambiguous(C);
  if (ambiguous) rec = adler_amb_record(k, s1, a_acc, last_hi);
  a_acc = (a_acc + adler_chunk_a(C, hi_k)) % ADLER_BASE;
  s1 = (s1 + S1) % ADLER_BASE;
  last_hi = hi_k ? 1u : 0u;
  return ambiguous;
}

// ---- adler_replay_kernel
// more ambiguous chunks than recorded, or than worth sorting: the plain walk
ZD_HD bool adler_replay_falls_back(uint32_t n_amb, uint32_t amb_cap, uint32_t replay_max) {
  return n_amb > amb_cap || n_amb > replay_max;
}
template <class Sums>
ZD_HD uint32_t adler_plain_walk(const Sums *sums, uint64_t n_chunks, uint32_t r) {
  uint32_t a1, a2;
  adler_unpack(1u, a1, a2);
  for (uint64_t k = 0; k < n_chunks; k++) adler_chunk_step(a1, a2, adler_chunk_len(k, r), sums[k].x, sums[k].y);
  return adler_pack(a1, a2);
}
// branch of the chunk before position k when k opens a run: last chunk of the
// nearest earlier non-empty run
ZD_HD bool adler_prev_branch(uint64_t k, uint32_t rec_prev_hi, uint64_t per, const uint32_t *run_last_hi) {
  if (rec_prev_hi != 0xFFFFFFFFu) return rec_prev_hi != 0;
  if (k == 0) return false;
  int64_t run = (int64_t)((k - 1) / per);
  while (run >= 0 && run_last_hi[run] == 0xFFFFFFFFu) run--;
  return run >= 0 && run_last_hi[run] != 0;
}
// the representative of a residue of s2 that the reference holds behind a chunk of that branch
ZD_HD int32_t adler_signed_s2(uint32_t rr, bool prev_hi) {
  return prev_hi ? (rr == 0 ? 0 : (int32_t)rr - (int32_t)ADLER_BASE) : (int32_t)rr;
}
// everything about a record that does not depend on the chunks before it: worked out by the thread that ranks it
struct ReplayRecord {
  uint32_t k;    // the chunk,
  uint32_t res;  // the predicted residue of s2 before it,
  uint32_t C;    // C = n * s1 + S2 (< 2^32),
  uint32_t pc;   // what the prediction adds for the chunk: (C - 225 * hi) mod p,
  uint8_t prev;  // the branch of the chunk before it as C alone decides it
};
ZD_HD ReplayRecord adler_replay_prepare(const AmbRecord &rec, uint32_t r, uint32_t S2, uint64_t per, const uint32_t *run_res,
                                        const uint32_t *run_last_hi) {
  ReplayRecord p;
  const uint32_t len = adler_chunk_len(rec.k, r);
  const uint32_t C = len * rec.s1 + S2;  // < 2^32
  p.k = rec.k;
  p.res = addmod(run_res[rec.k / per], rec.a_partial);
  p.C = C;
  p.pc = adler_chunk_a(C, adler_chunk_hi(C));
  p.prev = adler_prev_branch(rec.k, rec.prev_hi, per, run_last_hi) ? 1 : 0;
  return p;
}
struct ReplayState {
  uint32_t delta = 0;         // correction (mod p) of every predicted residue from here on
  int32_t exact_next = 0;     // exact s2 after the last replayed chunk ...
  uint64_t exact_at = ~0ull;  // ... valid as the input of chunk `exact_at`
};
// replay of one ambiguous chunk (they come in order)
ZD_HD void adler_replay_step(ReplayState &st, uint32_t k, uint32_t res, uint32_t C, uint32_t pc, bool prev) {
  const uint32_t rr = addmod(res, st.delta);
  const int32_t x = k == st.exact_at ? st.exact_next : adler_signed_s2(rr, prev);
  const uint32_t t2 = C + (uint32_t)x;                     // wraps like the reference's int32
  const int32_t outv = (int32_t)t2 % (int32_t)ADLER_BASE;  // the reference's signed rem
  const uint32_t ro = (uint32_t)(outv < 0 ? outv + (int32_t)ADLER_BASE : outv);
  const uint32_t predicted = addmod(rr, pc);
  st.delta = addmod(addmod(st.delta, ro), ADLER_BASE - predicted);
  st.exact_next = outv;
  st.exact_at = (uint64_t)k + 1;
}
// state after the last chunk, packed
ZD_HD uint32_t adler_replay_final(const ReplayState &st, uint64_t n_chunks, uint64_t per, const uint32_t *run_res,
                                  const uint32_t *run_a, const uint32_t *run_last_hi, const uint32_t *run_s1_after) {
  uint32_t final_s2;
  if (st.exact_at == n_chunks) final_s2 = (uint32_t)st.exact_next;
  else {
    const uint64_t last_run = n_chunks ? (n_chunks - 1) / per : 0;
    const uint64_t total_res = n_chunks ? ((uint64_t)run_res[last_run] + run_a[last_run]) % ADLER_BASE : 0;
    const uint32_t rr = (uint32_t)((total_res + st.delta) % ADLER_BASE);
    const bool ph = n_chunks ? adler_prev_branch(n_chunks, 0xFFFFFFFFu, per, run_last_hi) : false;
    final_s2 = (uint32_t)adler_signed_s2(rr, ph);
  }
  const uint64_t lr = n_chunks ? (n_chunks - 1) / per : 0;
  const uint64_t s1_all = n_chunks ? run_s1_after[lr] : 1;
  return adler_pack((uint32_t)s1_all, final_s2);
}

// ---- adler_rfc_finish_kernel.  RFC 1950's Adler-32 of the buffer from its chunk sums: with the unsigned remainder the
// chunk steps are an affine map mod 65521 in (s1, s2), so chunks combine in any grouping: every thread folds a run of
// chunks starting from (0, 0), then the runs are chained by one thread
// (s1' = s1 + A1, s2' = s2 + bytes_of_run * s1 + A2 for a run that maps (0, 0) to (A1, A2)).
constexpr uint32_t ADLER_RFC_THREADS = 1024;
ZD_HD uint64_t adler_rfc_per(uint64_t n_chunks) { return (n_chunks + ADLER_RFC_THREADS - 1) / ADLER_RFC_THREADS; }
template <class Sums>
ZD_HD void adler_rfc_fold_run(const Sums *sums, uint64_t lo, uint64_t hi, uint32_t r, uint32_t &s1, uint32_t &s2, uint64_t &bytes) {
  s1 = 0; s2 = 0; bytes = 0;
  for (uint64_t k = lo; k < hi; k++) {
    const uint32_t len = adler_chunk_len(k, r);
    adler_chunk_step(s1, s2, len, sums[k].x, sums[k].y, true);
    bytes += len;
  }
}
ZD_HD uint32_t adler_rfc_chain(const uint32_t *a1, const uint32_t *a2, const uint64_t *nb, uint32_t n) {
  uint64_t c1 = 1, c2 = 0;  // Adler-32 starts at (1, 0)
  for (uint32_t i = 0; i < n; i++) {
    c2 = (c2 + (nb[i] % ADLER_BASE) * c1 + a2[i]) % ADLER_BASE;
    c1 = (c1 + a1[i]) % ADLER_BASE;
  }
  return (uint32_t)((c2 << 16) | c1);
}

// ---- crc32_finish_kernel: the grid over a range's 32 KiB partials.  One partial: itself.  Up to 16: Horner by one
// thread.  More: a right-aligned grid of R rows of NT partials (padp virtual zero partials in front), thread t takes
// column t, eight rows requested together; partial (row, t) is index row * NT + t - padp.
constexpr uint32_t CRC_FINISH_HORNER_MAX = 16;
constexpr uint32_t CRC_FINISH_ROWS_AT_ONCE = 8;
ZD_HD uint32_t crc_finish_threads(uint64_t segs) { return segs > 4096 ? 1024u : 256u; }
ZD_HD bool crc_finish_by_one_thread(uint64_t nseg) { return nseg <= CRC_FINISH_HORNER_MAX; }
ZD_HD uint64_t crc_finish_rows(uint64_t nseg, uint32_t NT) { return (nseg + NT - 1) / NT; }
ZD_HD uint64_t crc_finish_padp(uint64_t nseg, uint32_t NT) { return NT * crc_finish_rows(nseg, NT) - nseg; }
ZD_HD int64_t crc_finish_index(uint64_t row, uint32_t NT, uint32_t t, uint64_t padp) {
  return (int64_t)(row * NT + (uint64_t)t) - (int64_t)padp;
}
// the word a thread loads for (row, t): clamped, the value selected afterwards by crc_finish_index >= 0
ZD_HD uint64_t crc_finish_load_index(int64_t idx, uint64_t row, uint64_t R) { return idx >= 0 && row < R ? (uint64_t)idx : 0; }

}  // namespace zd
