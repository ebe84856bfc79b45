// inflate_blocks.h -- what inflate by a wave per block decides between its launches (inflate.hip BlocksRun::front, inflate_blocks_group), free
// of HIP like forms.h, which has the way into that path: the lengths of a stream's lists, the ONE layout of their scratch, what
// the host makes of every read-back of the counts, the plan of the token run.  tests/test_host_sim.py pins it row by row.
#pragma once

#include <type_traits>
#include <vector>

#include "forms.h"

namespace zd {

constexpr size_t INFLATE_SCRATCH_PER_STREAM = 64 * 18 * 2;  // the span decoder's index of one wave (inflate_span.h)

// one stream by a wave per block (inflate.hip has the description and the order of the launches)
struct BlockStart {
  uint64_t bit;       // of the block's header in the stream's input
  uint32_t out_pos;   // of its first byte in the stream's output (the token run)
  uint32_t chunk0;    // the chain: Adler-32 chunks of the blocks before
};
struct BlockEnd {
  uint32_t status, final_block;
  uint64_t end_bit;   // of the first bit behind the block (a stored block: behind its bytes)
  uint32_t out_len, pad;
};
struct BlockRec { uint64_t bit; BlockEnd e; };  // a block that was walked from its header's bit to its end (e.pad: its checkpoints)
// checkpoints of a block's dry run (inflate_span.h SpanCk): bit from the header's bit, output byte from the block's first
constexpr uint32_t BLOCK_CK_MAX = 31;
struct BlockCk { uint32_t n; uint32_t e[2 * BLOCK_CK_MAX]; uint32_t pad; };
struct ChainIv { uint32_t first, ck; };  // a chain block's first interval (the token run: a wave per interval), its BlockCk
constexpr int RESOLVE_ROUNDS = 12;  // (h hops a round: pointers of h^r copies after round r)
struct FindCounts {
  uint32_t n_first;   // offsets that passed the header test (may exceed the list: those are lost)
  uint32_t n_cand;    // candidates (likewise)
  uint32_t chain_ok;  // inflate_chain_kernel: 1 = the blocks chain up to a final one and fit
  uint32_t n_blocks;
  uint64_t out_len;
  uint32_t token_bad; // inflate_blocks_token_kernel: blocks that did not end as the dry run said
  uint32_t more[RESOLVE_ROUNDS];  // inflate_resolve_kernel: bytes round r left short of a literal
  uint32_t n_walked;  // inflate_chain_kernel: blocks of the chain that it had to walk itself
  uint32_t n_recs;    // blocks listed: the candidates' (inflate_blocks_dry_kernel), then the explorers' (may exceed the list)
  uint32_t n_chunks;  // inflate_chain_kernel: Adler-32 chunks of the chain's blocks (every block has its own grid, zd.ml:682-690)
  uint32_t n_intervals, pad2;  // inflate_chain_kernel: intervals of the chain's blocks (a block and its checkpoints)
  uint64_t miss_bit;  // inflate_chain_kernel without walking: where the chain could not go on (~0: nowhere)
};
// A stream of a call that goes by blocks: where its lists live and what this launch takes of it.  The kernels' grids
// have the call's streams as their second dimension (jobs[blockIdx.y]) and the longest stream's need as their first.
struct BlocksJob {
  uint32_t stream;           // its descriptor and result
  uint32_t first_cap, cand_cap, rec_cap, chain_cap;
  uint32_t n;                // this launch's waves of the stream: explorers, or intervals / blocks of the token run
  uint32_t n_blocks;         // blocks of its chain (the explore launch: how many of its n waves are explorers, the rest followers)
  uint32_t out_len;          // its output bytes
  int32_t follow, pad;
  FindCounts *counts;
  uint32_t *first, *cand;
  BlockRec *recs, *sorted;
  uint32_t *sorted_src;
  BlockStart *chain;
  BlockEnd *chain_end;
  ChainIv *chain_iv;
  BlockCk *cks;
  uint16_t *span;            // the span decoder's index, a slot per wave of the launch
  uint32_t *tok;             // a word per output byte, then the two lists of the resolve rounds
  uint32_t *sums;            // Adler-32: three words per chunk
};

// the job of stream `stream` of a call, its lists not yet anywhere.  explore_stride: bytes of input between two explorers
// (blocks without a findable header: one every explore_stride bytes at most, 4 blocks listed each on average)
inline uint32_t blocks_max_explorers(uint64_t src_len, uint64_t explore_stride) { return (uint32_t)(src_len / explore_stride + 1); }
inline BlocksJob blocks_job(uint32_t stream, uint64_t src_len, uint64_t explore_stride) {
  BlocksJob J{};
  J.stream = stream;
  J.first_cap = (uint32_t)(src_len / 8 + 4096);
  J.cand_cap = (uint32_t)(src_len / 512 + 64);
  if (J.cand_cap > BLOCKS_CAND_CAP) J.cand_cap = BLOCKS_CAND_CAP;
  uint64_t rec_cap64 = 2ull * J.cand_cap + 4ull * blocks_max_explorers(src_len, explore_stride);  // (candidates, the blocks behind them, the explorers')
  if (rec_cap64 > BLOCKS_REC_CAP) rec_cap64 = BLOCKS_REC_CAP;
  J.rec_cap = J.chain_cap = (uint32_t)rec_cap64;
  return J;
}

// ctx->blocks_scratch of a group: counts of every stream | the launches' job list | per stream: first | cand | recs | sorted |
// sorted_src | chain | chain_end | chain_iv | cks (listed blocks, then blocks the chain walked), each array on a 256-byte
// boundary.  Carves them from base, fills every job's pointers and returns the end: from 0, that is the size to allocate --
// ONE layout for the size and the pointers.
inline uintptr_t carve_blocks_scratch(uintptr_t base, std::vector<BlocksJob> &jobs, FindCounts *&counts, BlocksJob *&job_list) {
  uintptr_t q = base;
  auto take = [&q](auto *&p, size_t bytes) {
    p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(q);
    q += align_up(bytes, 256);
  };
  take(counts, jobs.size() * sizeof(FindCounts));
  take(job_list, jobs.size() * sizeof(BlocksJob));
  for (size_t j = 0; j < jobs.size(); j++) {
    BlocksJob &J = jobs[j];
    J.counts = counts + j;
    take(J.first, (size_t)J.first_cap * 4);
    take(J.cand, (size_t)J.cand_cap * 4);
    take(J.recs, (size_t)J.rec_cap * sizeof(BlockRec));
    take(J.sorted, (size_t)J.rec_cap * sizeof(BlockRec));
    take(J.sorted_src, (size_t)J.rec_cap * 4);
    take(J.chain, (size_t)J.chain_cap * sizeof(BlockStart));
    take(J.chain_end, (size_t)J.chain_cap * sizeof(BlockEnd));
    take(J.chain_iv, (size_t)J.chain_cap * sizeof(ChainIv));
    take(J.cks, ((size_t)J.rec_cap + J.chain_cap) * sizeof(BlockCk));
  }
  return q;
}

// ---- what the host makes of the counts, read-back by read-back
// (how many candidates there are: the host asks when the lists are long or many -- a wave each is launched -- and lets
// the kernels read it themselves for one stream of a few MiB: a round trip less)
inline bool blocks_read_candidates(size_t nj, uint32_t cand_cap_of_first) { return nj > 1 || cand_cap_of_first > 8192u; }
// after the find: a stream without a candidate, or with more than its list holds, is dropped
inline bool blocks_found(const FindCounts &c, const BlocksJob &J) { return c.n_cand != 0 && c.n_cand <= J.cand_cap; }
// after the first chain: lost = it came to a block nobody listed (explorers from there on, then the chain again)
enum BlocksChained : int { BLOCKS_DROPPED = 0, BLOCKS_KEPT = 1, BLOCKS_LOST = 2 };
inline BlocksChained blocks_chained(const FindCounts &c, const BlocksJob &J) {
  return !blocks_found(c, J) ? BLOCKS_DROPPED : !c.chain_ok && c.miss_bit != ~0ull ? BLOCKS_LOST : BLOCKS_KEPT;
}
// a lost stream's explore launch: J.n_blocks explorers, one every explore_stride bytes from the miss on, and behind them a
// wave per block listed so far (the block that follows it, inflate.hip): J.n waves
inline void blocks_explore_waves(const FindCounts &c, BlocksJob &J, uint64_t src_len, uint64_t explore_stride) {
  const uint64_t bits_left = src_len * 8u - c.miss_bit;
  uint64_t ne = (bits_left + explore_stride * 8u - 1) / (explore_stride * 8u);
  if (ne > blocks_max_explorers(src_len, explore_stride)) ne = blocks_max_explorers(src_len, explore_stride);
  J.n_blocks = (uint32_t)ne;
  J.n = (uint32_t)ne + (c.n_recs < J.rec_cap ? c.n_recs : J.rec_cap);
}
// into the token run: a chain of two blocks and more that produces something (one block: nothing to gain)
inline bool blocks_token_taken(const FindCounts &c) { return c.chain_ok && c.n_blocks >= 2 && c.out_len != 0; }
// after the gather: done, or left to the stream's one wave (which writes the output again)
inline bool blocks_done(const FindCounts &c, int rounds) { return c.token_bad == 0 && c.more[rounds - 1] == 0; }

// The shares of a launch's streams in a buffer they divide among them, every stream's behind those of the one before:
// at[k], where the units(j) units of `unit` bytes of stream j = which[k] begin, in bytes; returns the bytes of all of them
template <class Units> inline size_t blocks_shares(const std::vector<uint32_t> &which, size_t unit, Units units, std::vector<size_t> &at) {
  size_t n = 0;
  at.clear();
  for (uint32_t j : which) { at.push_back(n * unit); n += units(j); }
  return n * unit;
}
// ctx->inflate_scratch: the span decoder's index, a slot per wave of the launch (jobs[j].n of them)
inline size_t blocks_span_slots(const std::vector<BlocksJob> &jobs, const std::vector<uint32_t> &which, std::vector<size_t> &at) {
  return blocks_shares(which, INFLATE_SCRATCH_PER_STREAM, [&](uint32_t j) { return jobs[j].n; }, at);
}
// ctx->adler_sums: Adler-32 block by block, every block's bytes in chunks of their own, three words a chunk and a chunk to spare
inline size_t blocks_adler_sums(const std::vector<FindCounts> &fc, const std::vector<uint32_t> &which, std::vector<size_t> &at) {
  return blocks_shares(which, 12, [&](uint32_t j) { return fc[j].n_chunks; }, at) + 12;
}

// ---- sizing by blocks (inflate.hip inflate_size_blocks_group): find, dry, chain as above, no token run, and a HEAD
// Why the answer is exact.  The chain starts at bit 0 and only steps from a block's true end bit to a record that begins at
// exactly that bit; every record is a real dry decode from its bit with every check of the decoder except the distance
// against the output position; the chain applies the limit and MAX_STREAM_LEN to the running sum.  So chain_ok means: every
// block decodes, they end in a final block, the sizes add up to a length within the limit -- all but "no distance reaches
// before the output".  A distance is at most 32768, so that can only fail in a block whose first byte lies below 32768:
// the head, one wave from bit 0 and position 0 with the one-wave sizing kernel's checks (the true position), walks exactly
// those blocks.  It stops at the first block end where the position has reached 32768, or behind the final block.
// (A block that inflates past 32 bits of length is no wrapped BlockEnd::out_len: the dry run's and the head's room is
// MAX_STREAM_LEN < 2^32 bytes, beyond which both report ST_DST_TOO_SMALL / ST_SIZE_EXCEEDED, never ST_OK.)
// Whatever is not shown to be OK that way is left to the stream's one wave, which owns every message.
//
// what the chain holds at the head's end: no block that starts at that bit / one, at the head's output position / one, elsewhere
enum SizeChainAt : int { SIZE_CHAIN_NONE = 0, SIZE_CHAIN_SAME = 1, SIZE_CHAIN_OTHER_POS = 2 };
ZD_HD int size_chain_at(const BlockStart *chain, uint32_t n_blocks, uint64_t bit, uint64_t out_pos) {
  uint32_t lo = 0, hi = n_blocks;  // (the chain's blocks are in stream order: the first that starts at or behind `bit`)
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (chain[mid].bit < bit) lo = mid + 1u;
    else hi = mid;
  }
  if (lo >= n_blocks || chain[lo].bit != bit) return SIZE_CHAIN_NONE;
  return (uint64_t)chain[lo].out_pos == out_pos ? SIZE_CHAIN_SAME : SIZE_CHAIN_OTHER_POS;
}
// The verdict: sized by blocks, with this length, if and only if the head is OK and either saw the final block (its own
// position is the size) or the chain is chain_ok and holds a block that starts exactly at the head's end bit with exactly
// the head's output position (the two walks agree where they meet: that comparison is free)
struct SizeVerdict { uint32_t sized; uint64_t out_len; };
ZD_HD SizeVerdict size_blocks_verdict(uint32_t head_status, uint32_t head_final, uint64_t head_out, uint32_t chain_ok, int chain_at,
                                      uint64_t chain_out) {
  SizeVerdict v;
  v.sized = 0; v.out_len = 0;
  if (head_status != ST_OK) return v;
  if (head_final != 0u) { v.sized = 1; v.out_len = head_out; return v; }
  if (chain_ok != 0u && chain_at == SIZE_CHAIN_SAME) { v.sized = 1; v.out_len = chain_out; }
  return v;
}
// ctx->size_head of a group of nj streams: every head's BlockEnd | the streams' indices | the heads' span index slots
struct SizeHeadScratch { size_t heads, streams, span, bytes; };
inline SizeHeadScratch size_head_scratch(size_t nj) {
  SizeHeadScratch s;
  s.heads = 0;
  s.streams = align_up(nj * sizeof(BlockEnd), 256);
  s.span = s.streams + align_up(nj * sizeof(uint32_t), 256);
  s.bytes = s.span + nj * INFLATE_SCRATCH_PER_STREAM;
  return s;
}
// The picked streams in groups that go through the steps side by side: there is no tok[], so a group is bounded only by
// the lists of carve_blocks_scratch -- ends[g] is one past group g's last entry of picked
constexpr size_t SIZE_BLOCKS_SCRATCH_BUDGET = (size_t)1 << 30;
inline std::vector<size_t> size_blocks_groups(const StreamDesc *sds, const std::vector<uint32_t> &picked, uint64_t explore_stride) {
  std::vector<size_t> ends;
  size_t group_bytes = 0;
  for (size_t j = 0; j < picked.size(); j++) {
    std::vector<BlocksJob> one(1, blocks_job(picked[j], sds[picked[j]].src_len, explore_stride));
    FindCounts *c;
    BlocksJob *l;
    const size_t need = (size_t)carve_blocks_scratch(0, one, c, l);
    const size_t begin = ends.empty() ? 0 : ends.back();
    if (j > begin && group_bytes + need > SIZE_BLOCKS_SCRATCH_BUDGET) { ends.push_back(j); group_bytes = 0; }
    group_bytes += need;
  }
  if (!picked.empty()) ends.push_back(picked.size());
  return ends;
}

// ---- the token run
// follow: sources written down as what they are copies of -- inflate_span.h -- cost the token run 0.2-0.4 ms a block and a
// wave per block instead of one per interval, and save the resolve rounds of a long stream more: with 256 hops a
// round, 64 MiB of text 6.3-10.8 -> 5.7-6.5 ms, 16 MiB 2.7-4.4 <- 3.3-4.2.
// What counts is the output of the whole call, whose bytes the rounds look at side by side: 64 x 1 MiB of text
// 5.8 -> 5.0 ms, 8 x 8 MiB 5.3 -> 4.7; 16 x 1 MiB 2.5 <- 3.2, one MiB 1.4 <- 2.4 ...
// ... and nothing on data with few matches: 16 MiB of records that deflate to 0.85, resolve 0.13 ms either way.
// follow_env: Tuning::inflate_follow (0 / 1: never / always).
inline int32_t blocks_follow(size_t call_out, uint32_t out_len, uint64_t src_len, int follow_env) {
  return follow_env >= 0 ? follow_env : call_out >= ((size_t)32 << 20) && (uint64_t)out_len * 2u >= src_len * 3u;
}
// tok[], and two lists of bytes still to resolve: 12 bytes of ctx->tok_scratch per output byte
inline size_t blocks_tok_words(uint64_t out_len) { return ((size_t)out_len * 3 + 63) & ~(size_t)63; }
// The streams of `alive` that go into the token run (taken), their jobs' out_len, n_blocks, follow and n set; tok_at[k]:
// where the k-th of them has its tok[] in ctx->tok_scratch, in bytes; tok_bytes: what to allocate
struct TokenPlan { std::vector<uint32_t> taken; std::vector<size_t> tok_at; size_t call_out, tok_bytes; };
inline TokenPlan blocks_token_plan(std::vector<BlocksJob> &jobs, const std::vector<FindCounts> &fc, const std::vector<uint32_t> &alive,
                                   const StreamDesc *sds, int follow_env) {
  TokenPlan p;
  p.call_out = 0;
  for (uint32_t j : alive)
    if (fc[j].chain_ok && fc[j].n_blocks >= 2) p.call_out += fc[j].out_len;
  for (uint32_t j : alive) {
    if (!blocks_token_taken(fc[j])) continue;
    BlocksJob &J = jobs[j];
    J.out_len = (uint32_t)fc[j].out_len;
    J.n_blocks = fc[j].n_blocks;
    J.follow = blocks_follow(p.call_out, J.out_len, sds[J.stream].src_len, follow_env);
    // a wave per interval of a block (its checkpoints), or -- follow -- a wave per block
    J.n = J.follow ? J.n_blocks : fc[j].n_intervals;
    p.taken.push_back(j);
  }
  p.tok_bytes = blocks_shares(p.taken, 4, [&](uint32_t j) { return blocks_tok_words(jobs[j].out_len); }, p.tok_at);
  return p;
}
// (hops a thread follows in a round: 8 left most bytes of a text for the next round -- 16 MiB: three rounds over nearly
// everything, 3.4 ms; 64 and more let nearly every byte arrive in the first: 0.28 ms)
inline int resolve_rounds(int hops0, int hops1) { return hops0 >= 16 && hops1 >= 16 ? 6 : RESOLVE_ROUNDS; }  // (16^6 links: more than a stream has bytes)
// workgroups of resolve round r per stream; out_grid: a thread per output byte of the longest stream
inline unsigned resolve_grid(int r, unsigned out_grid) { return r == 0 || out_grid < 2048u ? out_grid : 2048u; }

}  // namespace zd
