// kernels.h -- the kernels, constants and structs that more than one translation unit needs: checksum.hip's (api.hip, deflate.hip).
// Every other unit keeps its kernels to itself, behind the launchers of ctx.h (launch_deflate, launch_inflate, launch_recode, launch_zlib_*).
#pragma once

#include "adler_chain.h"
#include "checksum_ranges.h"
#include "zd_common.h"

namespace zd {

// ---- checksum.hip
constexpr uint32_t CRC_PIECE_BYTES = 128;  // bytes per thread of crc32_segments_kernel
constexpr uint32_t CRC_SEG_BYTES = 32768;   // per workgroup (256 threads)
enum : int { RANGE_INFLATE_OUT = 0, RANGE_DEFLATE_SRC = 1, RANGE_SINGLE = 2 };
struct CrcConsts {
  uint32_t xpiece[8];
  uint32_t xseg;
  uint32_t xbyte[48];  // x^(8 * 2^k) mod P: x^(8n) is one multiply per set bit of n
};
// nibble tables (zd_common.h gf2_mul_nib) of the constant multipliers, in device memory
// owned by the context: xpiece[0..7], then xseg
constexpr int CRC_NIB_CONSTS = 9;
constexpr int CRC_NIB_XSEG = 8;
__global__ void crc32_segments_kernel(const uint8_t *__restrict__ base, int mode,
                                      const StreamDesc *__restrict__ descs,
                                      const StreamResult *__restrict__ results,
                                      uint64_t single_off, uint64_t single_len,
                                      uint32_t segs_per_range, const uint32_t *__restrict__ nib,
                                      uint32_t *__restrict__ partials);
__global__ void crc32_adler_segments_kernel(const uint8_t *__restrict__ p, uint64_t len, uint32_t n_segs,
                                            const uint32_t *__restrict__ nib, uint32_t *__restrict__ partials,
                                            uint2 *__restrict__ adler_sums, uint64_t n_chunks);
__global__ void crc32_finish_kernel(int mode, const StreamDesc *__restrict__ descs,
                                    StreamResult *__restrict__ results, uint64_t single_len,
                                    uint32_t segs_per_range, CrcConsts K, const uint32_t *__restrict__ nib,
                                    const uint32_t *__restrict__ partials,
                                    uint32_t *__restrict__ single_out);
__global__ void crc32_finish_streams_kernel(int mode, const StreamDesc *__restrict__ descs,
                                            StreamResult *__restrict__ results, uint32_t n_ranges,
                                            uint32_t segs_per_range, CrcConsts K,
                                            const uint32_t *__restrict__ partials);
__global__ void adler_chunks_kernel(const uint8_t *__restrict__ p, uint64_t n, uint64_t n_chunks,
                                    uint2 *__restrict__ sums);
// RFC 1950's Adler-32 from the chunk sums (one workgroup)
__global__ void adler_rfc_finish_kernel(const uint2 *__restrict__ sums, uint64_t n, uint64_t n_chunks,
                                        uint32_t *__restrict__ out);
// (ADLER_AMB_CAP records of 16 bytes, ADLER_MAX_RUNS: adler_chain.h)
// per-run arrays of the Adler chain (device scratch, n_runs entries each)
struct AdlerRuns {
  uint32_t n_runs;       // a multiple of 1024
  uint32_t *sum;         // S1 sum of the run, later its a sum (mod p)
  uint32_t *s1_before;   // s1 before the run
  uint32_t *s1_after;
  uint32_t *last_hi;     // branch of the run's last chunk, 0xFFFFFFFF for an empty run
  uint32_t *res_before;  // residue of s2 before the run
  uint32_t *amb_count;   // [1]
};
__global__ void adler_runs_s1_kernel(const uint2 *__restrict__ sums, uint64_t n_chunks, uint64_t per, AdlerRuns R);
__global__ void adler_scan_runs_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, uint32_t n_runs,
                                       uint32_t first);
__global__ void adler_runs_a_kernel(const uint2 *__restrict__ sums, uint64_t n, uint64_t n_chunks, uint64_t per,
                                    AdlerRuns R, uint32_t *__restrict__ amb, uint32_t amb_cap);
__global__ void adler_replay_kernel(const uint2 *__restrict__ sums, uint64_t n, uint64_t n_chunks, uint64_t per,
                                    AdlerRuns R, uint32_t *__restrict__ amb, uint32_t amb_cap,
                                    uint32_t *__restrict__ out);

// ---- the ragged pass over many ranges of one arena (zipc_hip_checksum_batch; every rule: checksum_ranges.h)
// what checksum_plan_kernel leaves in the context's scratch: the call-wide word and, per range, where its partials and
// its chunk sums begin
struct RangesPlan {
  RangesCall *call;
  uint64_t *chunk_base;
  uint32_t *seg_base;
};
__global__ void checksum_plan_kernel(const Range *__restrict__ ranges, uint32_t n_ranges, uint64_t arena_len, uint64_t total_len,
                                     RangesPlan P, RangeResult *__restrict__ results, uint2 *__restrict__ sums, uint64_t n_sums);
__global__ void crc32_ranges_kernel(const uint8_t *__restrict__ arena, const Range *__restrict__ ranges, uint32_t n_ranges, RangesPlan P,
                                    const uint32_t *__restrict__ nib, uint32_t *__restrict__ partials);
__global__ void crc32_adler_ranges_kernel(const uint8_t *__restrict__ arena, const Range *__restrict__ ranges, uint32_t n_ranges,
                                          RangesPlan P, const uint32_t *__restrict__ nib, uint32_t *__restrict__ partials,
                                          uint2 *__restrict__ sums);
__global__ void crc32_finish_ranges_kernel(const Range *__restrict__ ranges, uint32_t n_ranges, RangesPlan P, CrcConsts K,
                                           const uint32_t *__restrict__ partials, RangeResult *__restrict__ results);
__global__ void adler_finish_ranges_kernel(const Range *__restrict__ ranges, uint32_t n_ranges, RangesPlan P,
                                           const uint2 *__restrict__ sums, int rfc, RangeResult *__restrict__ results);

}  // namespace zd
