// forms.h -- which kernels run for a call's shape, with which grids, segment sizes and scratch: free of HIP.
//
// Every rule the launch code follows between its ZD_LAUNCH lines is a pure function of plain numbers here (no context,
// no environment: the switches come in as a Tuning), so that the same code is compiled twice:
//   * into libzipc_hip.so (deflate.hip launch_deflate_group, inflate.hip launch_inflate: they compute the forms, then launch);
//   * into tests/host_sim/sim_forms.cpp with g++, where tests/test_host_sim.py pins both sides of every threshold.
// The constants the rules share with the kernels live here too.  DESIGN.md section 4.0 is a summary of this file.
#pragma once

#include <algorithm>
#include <vector>

#include "tuning.h"
#include "zd_common.h"

namespace zd {

// ---------------------------------------------------------------------------------
// deflate: the scratch
constexpr uint32_t POS_PAD = 256;            // scratch slack per stream, in positions
constexpr uint32_t MIN_BLOCK_SRC = 65277;    // a non-final block holds > 65534 - 258 source bytes

// streams with an out-of-range length are rejected by every kernel and take no scratch
ZD_HD uint64_t padded_positions(uint64_t src_len) {
  if (src_len > MAX_STREAM_LEN) src_len = 0;
  return ((src_len + 255) & ~255ull) + POS_PAD;
}
ZD_HD uint64_t max_blocks_of(uint64_t src_len) {
  if (src_len > MAX_STREAM_LEN) src_len = 0;
  return src_len / MIN_BLOCK_SRC + 2;
}

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// position slots and block slots of a group's scratch
inline void scratch_caps(size_t n, size_t total_src_len, uint64_t &P, uint64_t &Bk) {
  P = total_src_len + (uint64_t)(POS_PAD + 256) * n + 256;
  Bk = total_src_len / MIN_BLOCK_SRC + 2 * (uint64_t)n + 16;
}

// A batch of more than DEFLATE_GROUP_BYTES of source (8 GiB) goes through the pipeline in groups of
// consecutive streams, each group of at most that much, one after the other through the same
// scratch: 14 bytes of scratch per source byte of a GROUP (2-byte links, 8-byte match entries,
// 4-byte symbols), 112 GiB at most however large the batch.  Smaller groups were measured on C4
// (8192 x 1 MiB): 4 GiB groups deflate 9 % slower and 2 GiB groups 23 % slower than one group --
// lz_parse and deflate_emit are one wave per stream, and 2048 streams leave 2 waves per SIMD where
// 8192 leave 8 -- so the scratch is bounded, not halved.  ZIPC_HIP_DEFLATE_GROUP_BYTES overrides
// the size (tests run with groups of a few streams).
// streams per group, and the source bytes a group can hold at most
inline void deflate_grouping(size_t n, size_t max_src_len, size_t total_src_len, const Tuning &t, size_t &per_group, size_t &group_total) {
  per_group = n;
  group_total = total_src_len;
  if (total_src_len > t.deflate_group_bytes && max_src_len > 0 && n > 1) {
    per_group = t.deflate_group_bytes / max_src_len;
    per_group = per_group < 1 ? 1 : (per_group > n ? n : per_group);
    const unsigned __int128 bound = (unsigned __int128)per_group * max_src_len;
    group_total = bound < total_src_len ? (size_t)bound : total_src_len;
  }
}

// Into how many slices of consecutive streams a batch of n is cut (1: no side streams).  ZIPC_HIP_SLICES (or
// slices_override, zipc_hip_debug_set_slices: measurements that want every kernel alone on the device) overrides the
// default; a slice holds at least 2048 streams.
inline size_t batch_slices(size_t n_streams, const Tuning &t, long slices_override) {
  // Two slices by default (each of at least 2048 streams): since lz_chain is four waves per CU (round 4) the second
  // slice's chain links are made beside the first one's parse and blocks -- C2 deflate 13.25 -> 12.67 ms, the step
  // 16.97 -> 16.34; text the same either way; 3 / 4 / 6 slices lose 7 / 3 / 8 % (one box, tools/exp_wall.py).
  const long env = slices_override > 0 ? slices_override : t.slices, env_min = t.slice_min;
  size_t k = env > 0 ? (size_t)env : 2;
  if (k > 8) k = 8;
  const size_t least = env_min > 0 ? (size_t)env_min : 2048;
  while (k > 1 && n_streams / k < least) k--;
  return k;
}

// ---------------------------------------------------------------------------------
// deflate: constants the rules below share with the kernels of deflate.hip

// lz_chain_kernel: head holds positions mod 2^16; every 16384 positions entries older than 32768
// are replaced by a marker that decodes as "none" until the next sweep.
constexpr uint32_t SWEEP_PERIOD = 16384;
// (seg_positions: a multiple of the sweep period; 32 or 64 Ki while that leaves the chip workgroups to spare -- twice
// or half again the work for four times or twice the workgroups -- else 128 Ki)
constexpr uint32_t CHAIN_SEG_MIN = 2 * SWEEP_PERIOD, CHAIN_SEG_MAX = 8 * SWEEP_PERIOD;

constexpr uint32_t MATCH_TILE = 1024;  // lz_match_kernel: positions of a workgroup (MATCH_THREADS * MATCH_NP)
constexpr uint32_t MATCHW_TILE = 16384;
constexpr size_t MATCHW_GROUPS_PER_WG = 8;  // groups a workgroup takes one behind the other, at most (DeflateSliceForms::gpw)
constexpr size_t MATCHW_SMALL = 8192;  // streams up to this long keep the global-memory kernel
// A stream's FIRST tile has no window in front of it, so the LDS that holds a window and a tile holds three tiles' worth of
// the stream's start: tile 0 is 48 Ki positions, the others 16 Ki.  Every tile ends with its workgroup's waves running dry
// one after the other -- the pool is empty, a wave's last walks go on with few lanes, and the longest chain of the last
// positions sets how long: about 5 of a wave's 17 iterations of a 16 Ki tile on the benchmark's symbols (its lane use of
// 0.58 is mostly that) -- and a 64 KiB stream now has two such ends where it had four (round 5).
constexpr uint32_t MATCHW_TILE0 = MAX_MATCH_DIST + MATCHW_TILE;  // positions of a stream's first tile
// tiles of a stream of len bytes (len >= 4): a tile exists when its first position can start a match
ZD_HD uint64_t match_tiles_of(uint64_t len) {
  const uint64_t last = len - 4;  // the last position that can
  return last < MATCHW_TILE0 ? 1 : 2 + (last - MATCHW_TILE0) / MATCHW_TILE;
}

// positions per segment (ParseSegs::seg_positions): a multiple of the tile, far above the longest step (63 + 512);
// chosen per call -- the stitch takes a couple of microseconds per segment, one after the other, the waves of
// lz_parse_spec_kernel a third of a microsecond per tile, side by side
constexpr uint32_t PARSE_SEG_MIN = 4096;
constexpr uint32_t PARSE_SEG_SLACK = 576;  // symbols of a segment at most: one per position before its last step, and that step's
// lz_parse_meet_kernel: a segment's own small buffer (MEET_CAP symbols; more: left to the stitch)
constexpr uint32_t MEET_CAP = 2048;
constexpr uint32_t EMIT_PART = 8192;   // symbols a pack wave takes
constexpr uint32_t EMIT_PARTS = 8;     // parts of a block at most (65534 symbols: all literals)
static_assert(EMIT_PART * EMIT_PARTS >= (uint32_t)MAX_BLOCK_SRC_LEN, "a block's symbols fit its parts");

constexpr unsigned long long GRID_MAX = 0x7FFFFFFFull;  // workgroups of a launch at most

// ---------------------------------------------------------------------------------
// deflate: the forms of a group of n streams (the pipeline of launch_deflate_group), and of a slice of m of them
enum ChainKernel : int {
  CHAIN_XCHG = 0,           // lz_chain_xchg_kernel: a workgroup per stream, ordered LDS exchange
  CHAIN_XCHG_SEGMENTS = 1,  // lz_chain_xchg_segments_kernel: a workgroup per xseg positions of a stream
  CHAIN_PEEL = 2,           // lz_chain_kernel: a workgroup per stream that orders equal hashes itself
  CHAIN_PEEL_SEGMENTS = 3,  // lz_chain_segments_kernel: a workgroup per chain_seg positions of a stream
};

// the segment sizes deflate_forms below can give a chain form by segments: chain_seg 32, 64 or 128 Ki, xseg 96 Ki << k
// (zipc_hip_debug_chain_links_form launches a form by segments with no other size)
inline bool chain_seg_known(int chain, size_t seg_positions) {
  if (chain == CHAIN_PEEL_SEGMENTS) return seg_positions == CHAIN_SEG_MIN || seg_positions == 2 * CHAIN_SEG_MIN || seg_positions == CHAIN_SEG_MAX;
  if (chain != CHAIN_XCHG_SEGMENTS) return false;
  for (uint64_t x = (uint64_t)96 << 10; x <= MAX_STREAM_LEN; x *= 2)
    if (x == seg_positions) return true;
  return false;
}

struct DeflateForms {
  size_t n, max_src_len;
  bool grid_too_large;      // lz_match's grid does not fit: the call fails (hipErrorInvalidValue)
  int good_match, K;        // level_params
  size_t slices;            // the group goes out in this many slices on queues of their own (1: none)
  // lz_match
  size_t tps, cps;          // tiles of the longest stream: lz_match_window_kernel's, lz_match_kernel's
  size_t tpg, gps;          // consecutive tiles of a stream per workgroup, and such groups of the longest stream
  // parse and blocks by many waves
  bool segmented;           // lz_parse_spec .. gather and deflate_plan .. seal instead of lz_parse and deflate_emit
  bool segments_required;   // ZIPC_HIP_PARSE_SEGMENTS=1: a call that cannot have its parse scratch fails (hipErrorOutOfMemory)
  size_t segp, sps;         // positions per parse segment, segments of the longest stream
  size_t bps;               // block slots of the longest stream
  size_t n_slots, tiles, seg_syms;  // what the parse scratch is carved with (deflate.hip carve_parse_scratch)
  // lz_chain
  bool xchg_chain;          // by ordered LDS exchange
  size_t chain_seg, csegs;  // lz_chain_segments_kernel: positions per workgroup, workgroups of the longest stream
  size_t xseg, xsegs;       // lz_chain_xchg_segments_kernel: the same (0, 1: whole streams)
};

// segments_ok = false: the forms by a wave per stream whatever the shape -- what launch_deflate_group asks for when the
// device cannot give the parse scratch
inline DeflateForms deflate_forms(size_t n, size_t max_src_len, size_t total_src_len, int level, const Tuning &t, bool xchg_ok,
                                  long slices_override, bool segments_ok = true) {
  DeflateForms f{};
  f.n = n;
  f.max_src_len = max_src_len;
  level_params(level, f.good_match, f.K);
  f.slices = batch_slices(n, t, slices_override);
  f.tps = max_src_len >= 4 ? (size_t)match_tiles_of(max_src_len) : 1;
  f.cps = max_src_len ? (max_src_len + MATCH_TILE - 1) / MATCH_TILE : 1;
  f.grid_too_large = n * (max_src_len <= MATCHW_SMALL ? f.cps : f.tps) > GRID_MAX;
  // consecutive tiles of a stream per workgroup: as many as leave the grid >= 8192
  // workgroups (32 per CU: with 2048 a group of 2048 long streams had one workgroup per stream
  // and a long tail), so few long streams still spread over the chip
  // (ZIPC_HIP_MATCH_TILES_PER_GROUP, read once, overrides the rule: tuning and tests)
  f.tpg = t.match_tiles_per_group > 0 ? (size_t)t.match_tiles_per_group : n * f.tps / 8192;
  f.tpg = f.tpg < 1 ? 1 : (f.tpg > f.tps ? f.tps : f.tpg);
  f.gps = (f.tps + f.tpg - 1) / f.tpg;
  // Few long streams: lz_parse by a wave per segment (lz_parse_spec_kernel) and the blocks coded by a wave each
  // (deflate_plan_kernel); many streams fill the chip with a wave each.  ZIPC_HIP_PARSE_SEGMENTS=0 never, =1
  // whenever a stream has more than one segment (tests).
  const long segs_env = t.parse_segments;
  const long segp_env = t.parse_seg;  // positions per segment (tuning)
  // segment size: the stitch's serial time per stream is segments x ~0.25 us, the parallel part's a segment's tiles x ~0.3 us
  // (one stream alone, 4-bit symbols, whole deflate, ms at 4096 / 8192 / 16384 / 32768 / 65536 positions: 1 MiB 0.91 / 1.04 /
  // 1.09 / 1.38 / 1.94, 16 MiB 2.18 / 1.89 / 1.87 / 2.10 / 2.57 -- since lz_parse_meet_kernel the stitch's turn per
  // segment is a quarter of a microsecond)
  size_t segp = max_src_len <= ((size_t)4 << 20) ? 4096 : max_src_len <= ((size_t)32 << 20) ? 8192 : 16384;
  // (many long streams: as long as the call keeps 64 Ki waves, longer segments -- fewer seams to stitch and to gather across.
  // 8192 x 1 MiB, ms a step at 4096 / 8192 / 16 384 / 32 768 positions: 175.2 / 174.3 / 172.7 / 171.9, profiles/r06_c4_parse_segments.txt)
  while (segp < 32768 && n * ((max_src_len + 2 * segp - 1) / (2 * segp)) >= 65536) segp *= 2;
  if (segp_env >= (long)PARSE_SEG_MIN && segp_env % 64 == 0 && segp_env <= (1L << 20)) segp = (size_t)segp_env;
  f.segp = segp;
  const size_t sps = f.sps = (max_src_len + segp - 1) / segp;
  // (4096 x 1 MiB: 133 -> 124 ms; 64 KiB streams, 256 / 1024 / 2048 / 4096 / 16 384 of them:
  // 1.77 -> 0.73, 2.38 -> 1.67, 3.16 -> 2.85, 4.78 -> 5.11, 15.6 -> 17.4 ms; 8192 x 1 MiB, BASELINE's C4: the same either way
  // until round 6, then -- both parses a third shorter in instructions, the one wave per member still waiting for the LDS
  // 60 % of its cycles -- 182.1 -> 175.2 ms a step, profiles/r06_c4_parse_segments.txt)
  bool segmented = segs_env == 0 ? false : segs_env == 1 ? sps > 1
                   : (sps >= 8 && (n <= 2048 || (n <= 4096 && max_src_len >= ((size_t)512 << 10)) || (n <= 8192 && max_src_len >= ((size_t)1 << 20))));
  const size_t bps = f.bps = (size_t)max_blocks_of(max_src_len);  // block slots of the longest stream
  f.chain_seg = n * ((max_src_len + CHAIN_SEG_MIN - 1) / CHAIN_SEG_MIN) <= 512 ? CHAIN_SEG_MIN
                : n * ((max_src_len + 2 * CHAIN_SEG_MIN - 1) / (2 * CHAIN_SEG_MIN)) <= 1024 ? 2 * CHAIN_SEG_MIN : CHAIN_SEG_MAX;
  f.csegs = (max_src_len + f.chain_seg - 1) / f.chain_seg;  // lz_chain: workgroups of the longest stream
  // (grids of the segmented forms that do not fit only turn them off: the forms by a wave per stream take the call)
  if (segmented && (n * sps > GRID_MAX || n * bps * EMIT_PARTS > GRID_MAX)) segmented = false;
  f.segmented = segmented && segments_ok;
  f.segments_required = segs_env == 1;
  if (f.segmented) {
    uint64_t P, Bk;
    scratch_caps(n, total_src_len, P, Bk);
    f.n_slots = (size_t)(P / segp) + n + 1, f.tiles = (size_t)(P / 64) + 4;  // (ParseSegs::slot)
    f.seg_syms = segp + PARSE_SEG_SLACK;
  }
  // lz_chain: by ordered exchange where the context's probe passed (ZIPC_HIP_CHAIN=peel keeps the peel kernel: tests, A/B).
  // A wave per stream leaves most of the chip idle while there are fewer streams than CUs: a long stream is then cut into
  // segments of xseg positions, each warmed up with the 32 Ki positions before it (at most a third more work at 96 Ki).
  f.xchg_chain = xchg_ok;
  f.xseg = 0, f.xsegs = 1;
  if (f.xchg_chain && n < 1024 && max_src_len > ((size_t)192 << 10)) {
    f.xseg = (size_t)96 << 10;
    while (n * ((max_src_len + 2 * f.xseg - 1) / (2 * f.xseg)) >= 2048) f.xseg *= 2;  // twice the chip's CUs of waves is plenty
    f.xsegs = (max_src_len + f.xseg - 1) / f.xseg;
  }
  return f;
}

// The grids of one slice of m of the group's streams (m = n where the group goes out whole)
struct DeflateSliceForms {
  ChainKernel chain;
  size_t chain_grid;
  bool match_window;       // lz_match_window_kernel (else lz_match_kernel: streams of up to MATCHW_SMALL bytes)
  size_t match_grid, gpw;  // ... and the groups a workgroup of lz_match_window_kernel takes one behind the other
  size_t streams;          // a wave per stream: lz_parse, deflate_emit; lz_parse_stitch, deflate_counts, deflate_scan
  size_t segments;         // a wave per parse segment: lz_parse_spec, lz_parse_meet, lz_parse_gather
  size_t blocks;           // a wave per block: deflate_plan, deflate_codelen
  size_t ppb;              // parts per block of deflate_pack (1: no deflate_bits)
  size_t bits_grid, pack_grid, seal_grid;
};

inline DeflateSliceForms deflate_slice_forms(const DeflateForms &f, size_t m) {
  DeflateSliceForms s{};
  s.streams = m;
  if (f.xchg_chain) {  // one wave per stream (per segment of a long one while there are few): ordered LDS exchange
    const bool by_segments = m * f.xsegs > m && m * f.xsegs <= GRID_MAX;
    s.chain = by_segments ? CHAIN_XCHG_SEGMENTS : CHAIN_XCHG;
    s.chain_grid = by_segments ? m * f.xsegs : m;
  } else if (f.segmented && f.csegs > 1 && m <= 128) {  // (the run-up is a quarter more work: only while workgroups are what is missing)
    s.chain = CHAIN_PEEL_SEGMENTS;
    s.chain_grid = m * f.csegs;
  } else {
    s.chain = CHAIN_PEEL;
    s.chain_grid = m;
  }
  s.match_window = f.max_src_len > MATCHW_SMALL;  // short streams: a whole-CU window per tile would sit mostly idle
  if (!s.match_window) {
    s.match_grid = (m * f.cps + 7) / 8 * 8;
  } else {
    // groups a workgroup takes one behind the other: as many as leave 2048 workgroups and more, 8 at most (measured 1 / 2 / 4 / 8:
    // the benchmark's streams 4.70 / 4.60 / 4.50 / 4.50 ms, text 48.6 / 47.0 / 45.7 / 46.2, 1 MiB members of 3-bit symbols 31.9 / 32.2 / 32.7 / 30.6)
    size_t gpw = m * f.gps / 2048;
    gpw = gpw < 1 ? 1 : gpw > MATCHW_GROUPS_PER_WG ? MATCHW_GROUPS_PER_WG : gpw;
    // (... of groups that are short: a launch ends when its last workgroup does, and at `Best a group of text takes milliseconds --
    // 2048 streams: 8 workgroups of two groups a CU 76.8 ms, 16 of one 66.5.  Taking the groups from a counter instead of by
    // position in the grid evened that out -- 66.0 -- and cost 1 MiB members 13 % and the benchmark's streams 2-10 %; three
    // quarters of the groups in workgroups of several and the rest in workgroups of one: 73.0.  Both measured, neither kept.)
    if (f.K >= 1024) gpw = 1;
    s.gpw = gpw;
    const size_t wgs = (m * f.gps + gpw - 1) / gpw;
    s.match_grid = (wgs + 7) / 8 * 8;
  }
  if (f.segmented) {
    s.segments = m * f.sps;
    s.blocks = m * f.bps;
    // few blocks in the call: a coded block's symbols by a wave per EMIT_PART of them
    s.ppb = m * f.bps <= 2048 ? EMIT_PARTS : 1;
    s.bits_grid = s.ppb != 1 ? m * f.bps * EMIT_PARTS : 0;
    s.pack_grid = m * f.bps * s.ppb;
    s.seal_grid = (m * f.bps * s.ppb + 255) / 256;
  }
  return s;
}

// ---------------------------------------------------------------------------------
// inflate: streams of at least BLOCKS_MIN_SRC bytes by a wave per block (inflate.hip inflate_by_blocks; the rules between
// that path's launches: inflate_blocks.h)
constexpr size_t BLOCKS_MIN_SRC = 40u << 10, BLOCKS_MAX_SRC = 0x1FFFFFFFull;  // (bit offsets are 32-bit words here)
constexpr uint32_t BLOCKS_CAND_CAP = 65536, BLOCKS_REC_CAP = 262144;
// (a call whose descriptors are worth reading back: its longest stream alone is 4 ms of one wave.  Round 4 began with
// 1 MiB here and 96 KiB of input above: 64 x 512 KiB of text 8.5 -> 4.0 ms, 64 x 256 KiB 4.3 -> 2.6, one stream of
// 256 KiB 3.8 -> 1.3, of 128 KiB 2.0 -> 1.2; the block path's own floor is a good millisecond)
constexpr size_t BLOCKS_BATCH_MIN_DST = 256u << 10, BLOCKS_MAX_STREAMS = 1u << 20;
// tok[] and the two lists: 12 bytes of scratch per output byte.  Streams share a group while their capacities fit
// this much of it (a stream that needs more has a group to itself, and its scratch goes back afterwards)
constexpr size_t BLOCKS_TOK_BUDGET = (size_t)1 << 30;

// one long stream, or a call of long streams (an archive's big members): by blocks, side by side -- their one
// waves take 10-17 ms per MiB of the longest
inline bool inflate_blocks_gate(size_t n_streams, size_t max_dst_cap) {
  return max_dst_cap <= MAX_STREAM_LEN && n_streams <= BLOCKS_MAX_STREAMS &&
         max_dst_cap >= (n_streams == 1 ? BLOCKS_MIN_SRC : BLOCKS_BATCH_MIN_DST);
}

// a stream the block path takes at all
inline bool inflate_blocks_fits(const StreamDesc &sd) {
  if (sd.src_len < BLOCKS_MIN_SRC || sd.src_len > BLOCKS_MAX_SRC || sd.dst_cap < 8 || sd.dst_cap > MAX_STREAM_LEN) return false;
  // Runs (zeros, short periods: output beyond 64 x the input) are not for this path: a word of tok[] per byte of a
  // run costs more than the run (16 MiB of zeros as zlib codes them, 4 blocks: token run 10-11 ms, the one wave
  // 3.4-6.9), and where the reference's encoder has coded them with the fixed code, the explorers' walks never fall
  // into step with a bit stream that has a period (64 MiB: the chain walks nearly every block itself, 65 ms).
  return sd.dst_cap / 64 <= sd.src_len;
}
// every stream of a call that fits, in ascending order (zipc_hip_debug_inflate_tokens runs these: no cost rule)
inline std::vector<uint32_t> inflate_blocks_fit(const StreamDesc *sds, size_t n_streams) {
  std::vector<uint32_t> fit;
  for (size_t i = 0; i < n_streams; i++)
    if (inflate_blocks_fits(sds[i])) fit.push_back((uint32_t)i);
  return fit;
}

// which of a call's streams go by blocks, in ascending order
inline std::vector<uint32_t> inflate_blocks_pick(const StreamDesc *sds, size_t n_streams) {
  std::vector<uint32_t> fit = inflate_blocks_fit(sds, n_streams);
  // Which of them go by blocks: the one waves of a call run side by side, and a call of thousands of streams fills
  // the device with them -- its time is the longest stream's, about 15 ms per MiB of output -- while the block path
  // takes the streams' bytes one after the other, about 0.09 ms per MiB and 1 ms for a group's launches and
  // read-backs (64 x 1 MiB: 5.0 ms against 17; 4096 x 1 MiB: 370 ms against 16).  So the k longest streams go by
  // blocks, with the k that makes the sum of both parts smallest: all of a few long streams, the few long members
  // among an archive's many short ones, none of thousands of equal ones.
  constexpr double WAVE_MS_PER_MIB = 15.0, BLOCKS_MS_PER_MIB = 0.09, BLOCKS_MS_FIXED = 1.0, MIB = 1048576.0;
  std::sort(fit.begin(), fit.end(), [&](uint32_t x, uint32_t y) { return sds[x].dst_cap != sds[y].dst_cap ? sds[x].dst_cap > sds[y].dst_cap : x < y; });
  uint64_t longest_other = 0;  // (of the streams the block path does not take)
  {
    std::vector<uint8_t> in_fit(n_streams, 0);
    for (uint32_t i : fit) in_fit[i] = 1;
    for (size_t i = 0; i < n_streams; i++)
      if (!in_fit[i] && sds[i].dst_cap > longest_other) longest_other = sds[i].dst_cap;
  }
  size_t best_k = 0;
  double best_ms = 0, taken_mib = 0;
  for (size_t k = 0; k <= fit.size(); k++) {
    const uint64_t longest_left = k < fit.size() ? (sds[fit[k]].dst_cap > longest_other ? sds[fit[k]].dst_cap : longest_other) : longest_other;
    const bool any_left = k < n_streams;
    const double ms = (k ? BLOCKS_MS_FIXED + taken_mib * BLOCKS_MS_PER_MIB : 0.0) + (any_left ? (double)longest_left / MIB * WAVE_MS_PER_MIB : 0.0);
    if (k == 0 || ms < best_ms) { best_ms = ms; best_k = k; }
    if (k < fit.size()) taken_mib += (double)sds[fit[k]].dst_cap / MIB;
  }
  fit.resize(best_k);
  std::sort(fit.begin(), fit.end());
  return fit;
}

// The picked streams cut into groups that go through the steps side by side: ends[g] is one past group g's last entry of picked
inline std::vector<size_t> inflate_blocks_groups(const StreamDesc *sds, const std::vector<uint32_t> &picked) {
  std::vector<size_t> ends;
  size_t group_cap = 0;
  for (size_t j = 0; j < picked.size(); j++) {
    // (what a stream may produce: its capacity; the group's share of tok[] is sized by what the chains then say)
    const size_t may = (size_t)sds[picked[j]].dst_cap * 12;
    const size_t begin = ends.empty() ? 0 : ends.back();
    if (j > begin && group_cap + may > BLOCKS_TOK_BUDGET) { ends.push_back(j); group_cap = 0; }
    group_cap += may;
  }
  if (!picked.empty()) ends.push_back(picked.size());
  return ends;
}

// ---------------------------------------------------------------------------------
// sizing: streams of at least BLOCKS_MIN_SRC bytes by the block path's first half (inflate.hip launch_inflate_size_blocks: find,
// dry, chain -- and a head walk for the one check the dry runs leave out; the verdict's rule: inflate_blocks.h)
// A stream the path takes at all.  There is no destination, so no capacity to go by: the source's length alone (dst_off and
// dst_cap are not looked at, as in every sizing form).  A descriptor with a flag bit that is an argument error is the one
// wave's to report, like every other error.
inline bool size_blocks_gate(const StreamDesc &sd) {
  return (sd.flags & ~STREAM_HAS_LIMIT) == 0 && sd.src_len >= BLOCKS_MIN_SRC && sd.src_len <= BLOCKS_MAX_SRC;
}
// The model's constants, measured (tools/bench_inflate_size.py --blocks, profiles/inflate_size_blocks.json), in
// milliseconds per MiB of INPUT:
//   the one-wave sizing kernel walks a lone stream of text at 15.6 ms a MiB of input (1 -> 16 MiB of text at `Default:
//   6.95 -> 76.6 ms for 0.26 -> 4.73 MiB of input) and C2's 4-bit symbols at 13.2 - 13.4 (7.21 -> 115.9 ms for 0.54 -> 8.66
//   MiB); a call's one waves run side by side, so its time is the longest stream's (64 x 1 MiB of text: 4.35 ms, one
//   alone 6.9);
//   this path takes 0.80 ms for its launches and read-backs whatever it is given (the intercept of both pairs of points),
//   and then, for ONE stream, 0.43 ms a MiB of text (0.92 -> 2.83 ms: the explorers and the chain's walks of the oracle's
//   fixed blocks, a stream's own serial part) and 0.044 - 0.067 a MiB of C2's symbols (0.83 -> 1.38 ms: dynamic blocks,
//   found by their headers); streams side by side share everything but that serial part (8 -> 64 streams of 1 MiB of
//   text, 1.2 -> 8.7 MiB of input: 1.17 -> 1.54 ms, 0.049 a MiB, where their one waves take 4.4).
// So the path's cost is its fixed part, a serial part per MiB of the LONGEST stream it takes (text's 0.43 less the
// throughput part) and a throughput part per MiB of all it takes (0.067, the largest of the figures there are); the one
// waves are given C2's 13.2, the smallest -- of each pair the figure that favours the one waves, which need no read-back.
constexpr double SIZE_WAVE_MS_PER_MIB = 13.2, SIZE_BLOCKS_MS_FIXED = 0.8, SIZE_BLOCKS_SERIAL_MS_PER_MIB = 0.36, SIZE_BLOCKS_MS_PER_MIB = 0.067;
// which of a call's streams are sized by blocks, in ascending order: the model of inflate_blocks_pick over the sources --
// the k longest streams that pass the gate, with the k that makes (the block path's fixed cost and its cost per MiB of
// what it takes, the longest of them once more for its serial part) plus (the one-wave time of the longest stream left)
// smallest
inline std::vector<uint32_t> size_blocks_pick(const StreamDesc *sds, size_t n_streams) {
  std::vector<uint32_t> fit;
  if (n_streams > BLOCKS_MAX_STREAMS) return fit;
  uint64_t longest_other = 0;  // (of the streams the block path does not take; one above MAX_STREAM_LEN or with a stray flag bit is refused at once)
  for (size_t i = 0; i < n_streams; i++) {
    if (size_blocks_gate(sds[i])) fit.push_back((uint32_t)i);
    else if ((sds[i].flags & ~STREAM_HAS_LIMIT) == 0 && sds[i].src_len <= MAX_STREAM_LEN && sds[i].src_len > longest_other) longest_other = sds[i].src_len;
  }
  if (n_streams == 1) return fit;  // (one stream alone goes by blocks from BLOCKS_MIN_SRC on, as it does to be decoded: inflate_blocks_gate)
  constexpr double MIB = 1048576.0;
  std::sort(fit.begin(), fit.end(), [&](uint32_t x, uint32_t y) { return sds[x].src_len != sds[y].src_len ? sds[x].src_len > sds[y].src_len : x < y; });
  size_t best_k = 0;
  double best_ms = 0, taken_mib = 0;
  for (size_t k = 0; k <= fit.size(); k++) {
    const uint64_t longest_left = k < fit.size() && sds[fit[k]].src_len > longest_other ? sds[fit[k]].src_len : longest_other;
    const double serial_mib = k ? (double)sds[fit[0]].src_len / MIB : 0.0;  // (the longest stream taken: fit is in descending order)
    const double ms = (k ? SIZE_BLOCKS_MS_FIXED + serial_mib * SIZE_BLOCKS_SERIAL_MS_PER_MIB + taken_mib * SIZE_BLOCKS_MS_PER_MIB : 0.0) +
                      (double)longest_left / MIB * SIZE_WAVE_MS_PER_MIB;
    if (k == 0 || ms < best_ms) { best_ms = ms; best_k = k; }
    if (k < fit.size()) taken_mib += (double)sds[fit[k]].src_len / MIB;
  }
  fit.resize(best_k);
  std::sort(fit.begin(), fit.end());
  return fit;
}

// the batch kernel of a call's one waves: a few streams take the form that shares the tables of blocks with one and the
// same header (inflate.hip inflate_batch_few_kernel)
inline bool inflate_few_streams(size_t n_streams) { return n_streams <= 256; }

}  // namespace zd
