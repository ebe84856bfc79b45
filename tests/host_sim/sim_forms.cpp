// The launch rules of zipc_amd/csrc/forms.h and inflate_blocks.h and the scratch layout of deflate_scratch.h behind a C view.
// TEST TOOLING ONLY: the very headers deflate.hip, inflate.hip, api.hip and many.hip compile, so that tests/test_host_sim.py can hold
// every threshold to rows written out by hand.
#include <string.h>

#include "../../zipc_amd/csrc/deflate_scratch.h"
#include "../../zipc_amd/csrc/forms.h"
#include "../../zipc_amd/csrc/inflate_blocks.h"

using namespace zd;

// tun[8]: chain_peel is the caller's business (xchg_ok); parse_segments, parse_seg, match_tiles_per_group,
// deflate_group_bytes, slices, slice_min, the debug override of the slices, segments_ok
static Tuning tuning_of(const long long *tun) {
  Tuning t;
  memset(&t, 0, sizeof t);
  t.parse_segments = (long)tun[0];
  t.parse_seg = (long)tun[1];
  t.match_tiles_per_group = (long)tun[2];
  t.deflate_group_bytes = (size_t)tun[3];
  t.slices = (long)tun[4];
  t.slice_min = (long)tun[5];
  return t;
}

extern "C" void sim_deflate_grouping(uint64_t n, uint64_t max_src_len, uint64_t total_src_len, const long long *tun, uint64_t *out2) {
  size_t per_group, group_total;
  deflate_grouping(n, max_src_len, total_src_len, tuning_of(tun), per_group, group_total);
  out2[0] = per_group;
  out2[1] = group_total;
}

extern "C" uint64_t sim_deflate_scratch_bytes(uint64_t n, uint64_t max_src_len, uint64_t total_src_len, int level, const long long *tun) {
  return deflate_scratch_bytes(n, max_src_len, total_src_len, level, tuning_of(tun));
}

// out[20]: grid_too_large, K, slices, tps, cps, tpg, gps, segmented, segments_required, segp, sps, bps, n_slots, tiles,
// seg_syms, xchg_chain, chain_seg, csegs, xseg, xsegs;
// slice[12] for a slice of m streams: chain, chain_grid, match_window, match_grid, gpw, streams, segments, blocks, ppb,
// bits_grid, pack_grid, seal_grid
extern "C" void sim_deflate_forms(uint64_t n, uint64_t max_src_len, uint64_t total_src_len, int level, const long long *tun,
                                  int xchg_ok, uint64_t m, uint64_t *out, uint64_t *slice) {
  const DeflateForms f = deflate_forms(n, max_src_len, total_src_len, level, tuning_of(tun), xchg_ok != 0, (long)tun[6], tun[7] != 0);
  const uint64_t o[20] = {f.grid_too_large, (uint64_t)f.K, f.slices, f.tps, f.cps, f.tpg, f.gps, f.segmented, f.segments_required, f.segp,
                          f.sps, f.bps, f.n_slots, f.tiles, f.seg_syms, f.xchg_chain, f.chain_seg, f.csegs, f.xseg, f.xsegs};
  memcpy(out, o, sizeof o);
  const DeflateSliceForms s = deflate_slice_forms(f, m);
  const uint64_t q[12] = {(uint64_t)s.chain, s.chain_grid, s.match_window, s.match_grid, s.gpw, s.streams, s.segments, s.blocks, s.ppb,
                          s.bits_grid, s.pack_grid, s.seal_grid};
  memcpy(slice, q, sizeof q);
}

extern "C" int sim_chain_seg_known(int chain, uint64_t seg_positions) { return chain_seg_known(chain, seg_positions) ? 1 : 0; }

extern "C" int sim_inflate_blocks_gate(uint64_t n_streams, uint64_t max_dst_cap) { return inflate_blocks_gate(n_streams, max_dst_cap) ? 1 : 0; }
extern "C" int sim_inflate_few_streams(uint64_t n_streams) { return inflate_few_streams(n_streams) ? 1 : 0; }

// src_len[n], dst_cap[n] -> picked[] (at most n), group_ends[] (at most n); returns how many were picked
extern "C" uint64_t sim_inflate_blocks_pick(const uint64_t *src_len, const uint64_t *dst_cap, uint64_t n, uint32_t *picked,
                                            uint64_t *group_ends, uint64_t *n_groups) {
  std::vector<StreamDesc> sds(n);
  for (uint64_t i = 0; i < n; i++) {
    memset(&sds[i], 0, sizeof(StreamDesc));
    sds[i].src_len = src_len[i];
    sds[i].dst_cap = dst_cap[i];
  }
  const std::vector<uint32_t> p = inflate_blocks_pick(sds.data(), n);
  const std::vector<size_t> e = inflate_blocks_groups(sds.data(), p);
  for (size_t i = 0; i < p.size(); i++) picked[i] = p[i];
  for (size_t i = 0; i < e.size(); i++) group_ends[i] = e[i];
  *n_groups = e.size();
  return p.size();
}

// ---- inflate_blocks.h

// out[4]: first_cap, cand_cap, max_explorers, rec_cap
extern "C" void sim_blocks_caps(uint64_t src_len, uint64_t explore_stride, uint64_t *out) {
  const BlocksJob J = blocks_job(0, src_len, explore_stride);
  const uint64_t o[4] = {J.first_cap, J.cand_cap, blocks_max_explorers(src_len, explore_stride), J.rec_cap};
  if (J.chain_cap != J.rec_cap) return;  // (one length for both lists: the rows would miss an unset out[])
  memcpy(out, o, sizeof o);
}

extern "C" int sim_blocks_read_candidates(uint64_t nj, uint64_t src_len_of_first, uint64_t explore_stride) {
  return blocks_read_candidates(nj, blocks_job(0, src_len_of_first, explore_stride).cand_cap) ? 1 : 0;
}

// the layout of a group of n streams carved from base: head[2] = counts, the job list; lists[11 * j ..]: stream j's counts,
// first, cand, recs, sorted, sorted_src, chain, chain_end, chain_iv, cks, and the stream the job says it is; returns the end
extern "C" uint64_t sim_blocks_scratch(uint64_t base, const uint64_t *src_len, uint64_t n, uint64_t explore_stride, uint64_t *head,
                                       uint64_t *lists) {
  std::vector<BlocksJob> jobs(n);
  for (uint64_t j = 0; j < n; j++) jobs[j] = blocks_job((uint32_t)(100 + j), src_len[j], explore_stride);
  FindCounts *counts;
  BlocksJob *job_list;
  const uint64_t end = carve_blocks_scratch((uintptr_t)base, jobs, counts, job_list);
  head[0] = (uintptr_t)counts;
  head[1] = (uintptr_t)job_list;
  for (uint64_t j = 0; j < n; j++) {
    const BlocksJob &J = jobs[j];
    const uint64_t o[11] = {(uintptr_t)J.counts, (uintptr_t)J.first, (uintptr_t)J.cand, (uintptr_t)J.recs, (uintptr_t)J.sorted,
                            (uintptr_t)J.sorted_src, (uintptr_t)J.chain, (uintptr_t)J.chain_end, (uintptr_t)J.chain_iv, (uintptr_t)J.cks,
                            J.stream};
    memcpy(lists + 11 * j, o, sizeof o);
  }
  return end;
}

// One stream's counts as the host reads them back.  in[11]: src_len, explore_stride, n_cand, chain_ok, miss_bit, n_recs,
// n_blocks, out_len, token_bad, the resolve round whose more[] is set (or -1), rounds;
// out[6]: found, chained (0 dropped, 1 kept, 2 lost), explorers and waves of the explore launch, taken into the token run, done
extern "C" void sim_blocks_verdicts(const uint64_t *in, uint64_t *out) {
  BlocksJob J = blocks_job(0, in[0], in[1]);
  FindCounts c;
  memset(&c, 0, sizeof c);
  c.n_cand = (uint32_t)in[2];
  c.chain_ok = (uint32_t)in[3];
  c.miss_bit = in[4];
  c.n_recs = (uint32_t)in[5];
  c.n_blocks = (uint32_t)in[6];
  c.out_len = in[7];
  c.token_bad = (uint32_t)in[8];
  if ((int64_t)in[9] >= 0) c.more[in[9]] = 1;
  const uint64_t found = blocks_found(c, J), chained = (uint64_t)blocks_chained(c, J);
  blocks_explore_waves(c, J, in[0], in[1]);
  const uint64_t o[6] = {found, chained, J.n_blocks, J.n, blocks_token_taken(c), blocks_done(c, (int)in[10])};
  memcpy(out, o, sizeof o);
}

// The token run of n streams.  per stream in[5 * j ..]: src_len, chain_ok, n_blocks, out_len, n_intervals;
// out[5 * j ..]: taken, follow, n (its waves), where its tok[] begins in bytes, its output bytes as the job has them;
// total[2]: call_out, tok_bytes
extern "C" void sim_blocks_token_plan(const uint64_t *in, uint64_t n, int follow_env, uint64_t *out, uint64_t *total) {
  std::vector<StreamDesc> sds(n);
  std::vector<BlocksJob> jobs(n);
  std::vector<FindCounts> fc(n);
  std::vector<uint32_t> alive(n);
  for (uint64_t j = 0; j < n; j++) {
    memset(&sds[j], 0, sizeof(StreamDesc));
    memset(&fc[j], 0, sizeof(FindCounts));
    sds[j].src_len = in[5 * j];
    jobs[j] = blocks_job((uint32_t)j, in[5 * j], 16384);
    fc[j].chain_ok = (uint32_t)in[5 * j + 1];
    fc[j].n_blocks = (uint32_t)in[5 * j + 2];
    fc[j].out_len = in[5 * j + 3];
    fc[j].n_intervals = (uint32_t)in[5 * j + 4];
    alive[j] = (uint32_t)j;
  }
  const TokenPlan p = blocks_token_plan(jobs, fc, alive, sds.data(), follow_env);
  memset(out, 0, 5 * n * sizeof(uint64_t));
  for (size_t k = 0; k < p.taken.size(); k++) {
    const BlocksJob &J = jobs[p.taken[k]];
    const uint64_t o[5] = {1, (uint64_t)J.follow, J.n, p.tok_at[k], J.out_len};
    memcpy(out + 5 * p.taken[k], o, sizeof o);
  }
  total[0] = p.call_out;
  total[1] = p.tok_bytes;
}

extern "C" int sim_resolve_rounds(int hops0, int hops1) { return resolve_rounds(hops0, hops1); }
extern "C" uint32_t sim_resolve_grid(int r, uint32_t out_grid) { return resolve_grid(r, out_grid); }

// The shares of n streams in the buffers they share.  waves[n] -> span_at[n] (bytes), chunks[n] -> sums_at[n] (bytes);
// total[2]: bytes of the span index, bytes of the Adler sums
extern "C" void sim_blocks_shares(const uint32_t *waves, const uint32_t *chunks, uint64_t n, uint64_t *span_at, uint64_t *sums_at,
                                  uint64_t *total) {
  std::vector<BlocksJob> jobs(n);
  std::vector<FindCounts> fc(n);
  std::vector<uint32_t> which(n);
  for (uint64_t j = 0; j < n; j++) {
    memset(&jobs[j], 0, sizeof(BlocksJob));
    memset(&fc[j], 0, sizeof(FindCounts));
    jobs[j].n = waves[j];
    fc[j].n_chunks = chunks[j];
    which[j] = (uint32_t)j;
  }
  std::vector<size_t> at;
  total[0] = blocks_span_slots(jobs, which, at);
  for (uint64_t j = 0; j < n; j++) span_at[j] = at[j];
  total[1] = blocks_adler_sums(fc, which, at);
  for (uint64_t j = 0; j < n; j++) sums_at[j] = at[j];
}
