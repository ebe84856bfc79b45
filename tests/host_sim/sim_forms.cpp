// The launch rules of zipc_amd/csrc/forms.h and the scratch layout of deflate_scratch.h behind a C view.
// TEST TOOLING ONLY: the very headers deflate.hip and api.hip compile, so that tests/test_host_sim.py can hold
// every threshold to rows written out by hand.
#include <string.h>

#include "../../zipc_amd/csrc/deflate_scratch.h"
#include "../../zipc_amd/csrc/forms.h"

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
