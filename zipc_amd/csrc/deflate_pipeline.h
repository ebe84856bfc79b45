// deflate_pipeline.h -- what the kernels of the deflate pipeline share (deflate.hip): the scratch
// (deflate_scratch.h), the constants the launch rules know too (forms.h) and the barrier that waits for LDS only.
#pragma once

#include "ctx.h"
#include "deflate_lane.h"
#include "deflate_scratch.h"
#include "wave_ops.h"

namespace zd {

constexpr uint32_t PARSE_PAD = 200;          // table entries behind the last position the parse may load (3 tiles of 64 + 3)
static_assert(PARSE_PAD <= POS_PAD, "inside the stream's scratch");

constexpr uint32_t MATCH_SNAP = 1u << 31;
// both answers of a position as the 64-bit word the parse works on (best of K | best of K/4 << 32) from the two tables
__device__ __forceinline__ uint64_t match_pair(const uint32_t *__restrict__ match, const uint32_t *__restrict__ snap, uint64_t i) {
  const uint32_t lo = match[i];
  const uint32_t hi = (lo & MATCH_SNAP) ? snap[i] : lo;
  return (uint64_t)(lo & ~MATCH_SNAP) | ((uint64_t)hi << 32);
}

// The threads of a workgroup that exchange data through LDS only wait for the LDS counter alone:
// __syncthreads() would also wait (vmcnt) for every global load and store the wave has in flight --
// source words requested ahead, the stores of results.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
}

}  // namespace zd
