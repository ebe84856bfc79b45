// sim_size_blocks.cpp -- the HIP-free rules of sizing by blocks (zipc_amd/csrc/forms.h size_blocks_gate / size_blocks_pick,
// inflate_blocks.h size_chain_at / size_blocks_verdict / size_blocks_groups / size_head_scratch) behind a C interface, for
// tests/test_size_blocks_rules.py.  Built with g++ as a shared library; with -DSIZE_BLOCKS_MAIN as a stand-alone program
// that runs the same calls over a few shapes (what a host sanitizer build of the planning code runs).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../zipc_amd/csrc/inflate_blocks.h"

using namespace zd;

extern "C" {

uint64_t sim_blocks_min_src() { return BLOCKS_MIN_SRC; }
uint64_t sim_blocks_max_src() { return BLOCKS_MAX_SRC; }
uint64_t sim_blocks_max_streams() { return BLOCKS_MAX_STREAMS; }
uint64_t sim_size_scratch_budget() { return SIZE_BLOCKS_SCRATCH_BUDGET; }

static std::vector<StreamDesc> descs_of(uint64_t n, const uint64_t *src_len, const uint64_t *dst_off, const uint64_t *dst_cap,
                                        const uint32_t *flags) {
  std::vector<StreamDesc> sds(n);
  uint64_t off = 0;
  for (uint64_t i = 0; i < n; i++) {
    StreamDesc sd{};
    sd.src_off = off; sd.src_len = src_len[i];
    sd.dst_off = dst_off ? dst_off[i] : 0; sd.dst_cap = dst_cap ? dst_cap[i] : 0;
    sd.flags = flags ? flags[i] : 0;
    off += src_len[i] <= MAX_STREAM_LEN ? src_len[i] : 0;
    sds[i] = sd;
  }
  return sds;
}

int sim_size_gate(uint64_t src_len, uint64_t dst_off, uint64_t dst_cap, uint32_t flags) {
  StreamDesc sd{};
  sd.src_len = src_len; sd.dst_off = dst_off; sd.dst_cap = dst_cap; sd.flags = flags;
  return size_blocks_gate(sd) ? 1 : 0;
}

// picked[]: room for n entries; returns how many streams go by blocks
uint64_t sim_size_pick(uint64_t n, const uint64_t *src_len, const uint64_t *dst_off, const uint64_t *dst_cap, const uint32_t *flags,
                       uint32_t *picked) {
  const std::vector<StreamDesc> sds = descs_of(n, src_len, dst_off, dst_cap, flags);
  const std::vector<uint32_t> p = size_blocks_pick(sds.data(), n);
  for (size_t k = 0; k < p.size(); k++) picked[k] = p[k];
  return p.size();
}

// the groups of picked streams (all of src_len[] taken as picked): ends[] (room for n), returns their number; *worst: the
// largest group's scratch, as carve_blocks_scratch lays it out
uint64_t sim_size_groups(uint64_t n, const uint64_t *src_len, uint64_t explore_stride, uint64_t *ends, uint64_t *worst) {
  const std::vector<StreamDesc> sds = descs_of(n, src_len, nullptr, nullptr, nullptr);
  std::vector<uint32_t> picked(n);
  for (uint64_t i = 0; i < n; i++) picked[i] = (uint32_t)i;
  const std::vector<size_t> e = size_blocks_groups(sds.data(), picked, explore_stride);
  size_t begin = 0;
  *worst = 0;
  for (size_t g = 0; g < e.size(); g++) {
    std::vector<BlocksJob> jobs;
    for (size_t j = begin; j < e[g]; j++) jobs.push_back(blocks_job(picked[j], sds[picked[j]].src_len, explore_stride));
    FindCounts *c;
    BlocksJob *l;
    const uint64_t bytes = carve_blocks_scratch(0, jobs, c, l);
    if (bytes > *worst) *worst = bytes;
    ends[g] = e[g];
    begin = e[g];
  }
  return e.size();
}

// what the chain (bits[] ascending, out_pos[]) holds at (bit, out_pos): SizeChainAt
int sim_size_chain_at(uint32_t n_blocks, const uint64_t *bits, const uint32_t *out_pos, uint64_t bit, uint64_t pos) {
  std::vector<BlockStart> chain(n_blocks);
  for (uint32_t k = 0; k < n_blocks; k++) { chain[k].bit = bits[k]; chain[k].out_pos = out_pos[k]; chain[k].chunk0 = 0; }
  return size_chain_at(chain.data(), n_blocks, bit, pos);
}

// the verdict; returns sized, *out_len the size
uint32_t sim_size_verdict(uint32_t head_status, uint32_t head_final, uint64_t head_out, uint32_t chain_ok, int chain_at, uint64_t chain_out,
                          uint64_t *out_len) {
  const SizeVerdict v = size_blocks_verdict(head_status, head_final, head_out, chain_ok, chain_at, chain_out);
  *out_len = v.out_len;
  return v.sized;
}

// the layout of a group's head scratch: {heads, streams, span, bytes}
void sim_size_head_scratch(uint64_t nj, uint64_t *out4) {
  const SizeHeadScratch s = size_head_scratch(nj);
  out4[0] = s.heads; out4[1] = s.streams; out4[2] = s.span; out4[3] = s.bytes;
}

}  // extern "C"

#ifdef SIZE_BLOCKS_MAIN
int main() {
  int bad = 0;
  // a few long streams, the long ones among many short ones, thousands of equal ones
  for (uint64_t n : {1ull, 3ull, 500ull, 4096ull}) {
    std::vector<uint64_t> len(n, (uint64_t)1 << 20);
    if (n == 500) for (uint64_t i = 3; i < n; i++) len[i] = 3000 + i;
    std::vector<uint32_t> picked(n);
    const uint64_t k = sim_size_pick(n, len.data(), nullptr, nullptr, nullptr, picked.data());
    const uint64_t want = n == 4096 ? 0 : n == 500 ? 3 : n;
    if (k != want) { std::printf("pick %llu: %llu\n", (unsigned long long)n, (unsigned long long)k); bad++; }
    std::vector<uint64_t> ends(n);
    uint64_t worst = 0;
    const uint64_t g = sim_size_groups(n, len.data(), 32768, ends.data(), &worst);
    if (g == 0 || ends[g - 1] != n) { std::printf("groups %llu\n", (unsigned long long)n); bad++; }
  }
  const uint64_t bits[3] = {0, 100, 900};
  const uint32_t pos[3] = {0, 40000, 90000};
  if (sim_size_chain_at(3, bits, pos, 100, 40000) != SIZE_CHAIN_SAME || sim_size_chain_at(3, bits, pos, 100, 40001) != SIZE_CHAIN_OTHER_POS ||
      sim_size_chain_at(3, bits, pos, 101, 40000) != SIZE_CHAIN_NONE || sim_size_chain_at(0, bits, pos, 0, 0) != SIZE_CHAIN_NONE) {
    std::printf("chain_at\n");
    bad++;
  }
  std::printf(bad ? "FAILED\n" : "ok\n");
  return bad ? 1 : 0;
}
#endif
