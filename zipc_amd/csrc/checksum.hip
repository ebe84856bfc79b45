// checksum.hip -- CRC-32 and Adler-32 kernels for gfx950.
//
// CRC-32 (Crc_32.string_update, src/zipc_deflate.ml:137-156): the reference's
// slice-by-4 table walk is a serial chain over the bytes.  Here a range is cut
// into 32 KiB segments (one 256-thread workgroup each) and every thread walks a
// 128-byte piece with the same 4x256 tables held in LDS; pieces and segments
// are merged with the CRC combination rule (zd_common.h: gf2_mul), the range
// being RIGHT-aligned on the piece grid so that all pieces have equal length
// (leading zero bytes do not change a raw CRC).  A segment goes through LDS on
// its way to the threads: it is read from memory as coalesced 16-byte units
// (every byte fetched once) and written so that piece t starts at 144 t -- 16
// bytes of padding per piece make the threads' 16-byte reads of their own
// pieces conflict free.  (Threads reading their pieces straight from memory,
// 64 lanes x 16 B at a 256 B stride, re-fetched every line several times: the
// lines in flight on a CU did not fit the caches.)  Chaining across the
// reference's per-block update calls is exact for CRC-32, so the fused forms
// (inflate_and_crc_32, crc_32_and_deflate) run this once over the whole
// produced / consumed range of each stream.
//
// Adler-32 (Adler_32.string_update, src/zipc_deflate.ml:175-198): one wave per
// 5552-byte chunk of the reference's chunk grid (FIRST chunk = len mod 5552)
// reduces (S1, S2); the chunk chain with the signed 32-bit remainder
// (src/zipc_deflate.ml:95,196) is then applied in order by the adler_runs / adler_scan /
// adler_replay kernels.
#include "kernels.h"
#include "wave_ops.h"

namespace zd {

constexpr uint32_t CRC_PIECE = CRC_PIECE_BYTES;      // bytes per thread
constexpr uint32_t CRC_THREADS = 256;
constexpr uint32_t CRC_SEG = CRC_PIECE * CRC_THREADS;  // 32 KiB per workgroup
constexpr uint32_t CRC_PIECE_STRIDE = CRC_PIECE + 16;  // of a piece in LDS
static_assert(CRC_SEG == CRC_SEG_BYTES, "kernels.h");

__device__ __forceinline__ void get_range(int mode, uint32_t i, const StreamDesc *descs,
                                          const StreamResult *results, uint64_t single_off,
                                          uint64_t single_len, uint64_t &off, uint64_t &len) {
  if (mode == RANGE_SINGLE) { off = single_off; len = single_len; return; }
  const StreamDesc d = descs[i];
  if (mode == RANGE_DEFLATE_SRC) { off = d.src_off; len = d.src_len; return; }
  const StreamResult r = results[i];
  off = d.dst_off;
  len = r.status == ST_OK ? r.out_len : 0;
}

// Crc_32.table (src/zipc_deflate.ml:114-133) built in LDS by the workgroup
__device__ __forceinline__ void build_crc_tables(uint32_t (*T)[256], int t) {
  uint32_t c = (uint32_t)t;
#pragma unroll
  for (int k = 0; k < 8; k++) c = (c & 1u) ? (CRC_POLY ^ (c >> 1)) : (c >> 1);
  T[0][t] = c;
  __syncthreads();
  uint32_t v = c;
#pragma unroll
  for (int k = 1; k < 4; k++) {
    v = (v >> 8) ^ T[0][v & 0xFF];
    T[k][t] = v;
  }
  __syncthreads();
}

// ADLER: the same pass also leaves the Adler-32 chunk sums of the range (RANGE_SINGLE only): the chunk grid
// (first chunk = len mod 5552, then 5552 each) and the right-aligned piece grid agree mod 16 -- 5552 = 16 * 347
// and both are congruent to len -- so a chunk boundary falls between two 16-byte units of a thread's piece,
// never inside one.  A thread sums its 8 units (S1 = sum b, S2 = sum (end - i) b, two dot products per word),
// splits them at the boundary if its piece holds one, and the wave adds what it has of at most three chunks
// to `adler_sums` (zeroed by the caller; integer adds: any order gives the same sums).
// The body: segment `seg` of the `nseg` of the range of `len` bytes at p (seg < nseg, uniform per workgroup); the
// segment's raw CRC goes to *partial.  Which range and segment a workgroup has, and where its partial lies, is its
// caller's: crc32_segment below for the rectangular grids, crc32_ranges_kernel for the ragged one.
template <bool ADLER>
__device__ __forceinline__ void crc32_segment_body(const uint8_t *__restrict__ p, uint64_t len, uint32_t seg, uint64_t nseg,
                                                   const uint32_t *__restrict__ nib, uint32_t *__restrict__ partial,
                                                   uint32_t *__restrict__ adler_sums, uint64_t n_chunks) {
  __shared__ uint32_t T[4][256];
  static_assert(8 * GF2_NIB_WORDS == 4 * CRC_THREADS, "one 16-byte load per thread");
  __shared__ __attribute__((aligned(16))) uint8_t stage[CRC_THREADS * CRC_PIECE_STRIDE];
  // xpiece[0..7] as nibble tables (4 KiB) and the waves' partials: in the staged segment's place once every thread has walked
  // its piece -- 40 KiB of LDS a workgroup, so that FOUR fit a CU (three with tables of their own: the table walk of one
  // workgroup hides behind the loads of the others, and C3 is the one kernel here that waits for memory)
  uint32_t *N = (uint32_t *)stage;
  uint32_t *wave_part = (uint32_t *)(stage + 8 * GF2_NIB_WORDS * 4);
  const int t = threadIdx.x;
  build_crc_tables(T, t);

  // right-aligned piece grid: `pad` virtual zero bytes in front of the range;
  // seg0 = range position of the segment's first byte (negative inside the pad)
  const uint64_t pad = nseg * CRC_SEG - len;
  const int64_t seg0 = (int64_t)((uint64_t)seg * CRC_SEG) - (int64_t)pad;
  constexpr int UNITS = CRC_SEG / 16 / CRC_THREADS;  // 16-byte units per thread
  u32x4 v[UNITS];
  if (len >= 16) {
    // unit u = i * 256 + t: consecutive threads, consecutive 16 bytes; all loads in flight together
#pragma unroll
    for (int i = 0; i < UNITS; i++) {
      const int64_t q = seg0 + (int64_t)((uint32_t)i * CRC_THREADS + (uint32_t)t) * 16;
      v[i] = load16_unaligned(p + (q > 0 ? q : 0));  // q + 16 <= len by construction
    }
#pragma unroll
    for (int i = 0; i < UNITS; i++) {
      const int64_t q = seg0 + (int64_t)((uint32_t)i * CRC_THREADS + (uint32_t)t) * 16;
      if (q < 0) {  // only in the first segment of a range: pad bytes are zero
        uint8_t b[16];
#pragma unroll
        for (int k = 0; k < 16; k++) b[k] = q + k >= 0 ? p[q + k] : (uint8_t)0;
        __builtin_memcpy(&v[i], b, 16);
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < UNITS; i++) {
      const int64_t q = seg0 + (int64_t)((uint32_t)i * CRC_THREADS + (uint32_t)t) * 16;
      uint8_t b[16];
#pragma unroll
      for (int k = 0; k < 16; k++) b[k] = (q + k >= 0 && q + k < (int64_t)len) ? p[q + k] : (uint8_t)0;
      __builtin_memcpy(&v[i], b, 16);
    }
  }
#pragma unroll
  for (int i = 0; i < UNITS; i++) {
    const uint32_t u = (uint32_t)i * CRC_THREADS + (uint32_t)t;
    *(u32x4 *)(stage + (u / (CRC_PIECE / 16)) * CRC_PIECE_STRIDE + (u % (CRC_PIECE / 16)) * 16) = v[i];
  }
  __syncthreads();
  // my piece (Crc_32.string_update's word loop, src/zipc_deflate.ml:141-150; leading
  // zero bytes leave c = 0)
  uint32_t c = 0;
  const u32x4 *mine = (const u32x4 *)(stage + (uint32_t)t * CRC_PIECE_STRIDE);
  // Adler: the chunk that holds the piece's first byte, and the unit at which the next chunk starts (8: none)
  uint32_t cut = 8, s1 = 0, s2 = 0, A1 = 0, A2 = 0;
  uint64_t kA = 0;
  int64_t to_end = 0;  // from the piece's start to the end of chunk kA: a positive multiple of 16
  if constexpr (ADLER) {
    const int64_t ps = seg0 + (int64_t)((uint32_t)t * CRC_PIECE);
    const uint64_t r = len % ADLER_CHUNK;
    const uint64_t pos0 = ps > 0 ? (uint64_t)ps : 0;
    uint64_t eA = r;
    if (pos0 >= r) { kA = (pos0 - r) / ADLER_CHUNK + 1; eA = r + kA * ADLER_CHUNK; }
    to_end = (int64_t)eA - ps;
    cut = to_end < (int64_t)CRC_PIECE ? (uint32_t)to_end / 16u : 8u;
  }
#pragma unroll
  for (int j = 0; j < (int)(CRC_PIECE / 16); j++) {
    const u32x4 w = mine[j];
    if constexpr (ADLER) {
      A1 = cut == (uint32_t)j ? s1 : A1;  // the sums of the units before the boundary
      A2 = cut == (uint32_t)j ? s2 : A2;
      uint32_t u1 = __builtin_amdgcn_udot4(w.x, 0x01010101u, 0u, false);
      u1 = __builtin_amdgcn_udot4(w.y, 0x01010101u, u1, false);
      u1 = __builtin_amdgcn_udot4(w.z, 0x01010101u, u1, false);
      u1 = __builtin_amdgcn_udot4(w.w, 0x01010101u, u1, false);
      uint32_t u2 = __builtin_amdgcn_udot4(w.x, 0x0D0E0F10u, 0u, false);  // byte i of the unit weighs 16 - i
      u2 = __builtin_amdgcn_udot4(w.y, 0x090A0B0Cu, u2, false);
      u2 = __builtin_amdgcn_udot4(w.z, 0x05060708u, u2, false);
      u2 = __builtin_amdgcn_udot4(w.w, 0x01020304u, u2, false);
      s2 += 16u * s1 + u2;
      s1 += u1;
    }
    uint32_t u = c ^ w.x;
    c = T[3][u & 0xFF] ^ T[2][(u >> 8) & 0xFF] ^ T[1][(u >> 16) & 0xFF] ^ T[0][u >> 24];
    u = c ^ w.y;
    c = T[3][u & 0xFF] ^ T[2][(u >> 8) & 0xFF] ^ T[1][(u >> 16) & 0xFF] ^ T[0][u >> 24];
    u = c ^ w.z;
    c = T[3][u & 0xFF] ^ T[2][(u >> 8) & 0xFF] ^ T[1][(u >> 16) & 0xFF] ^ T[0][u >> 24];
    u = c ^ w.w;
    c = T[3][u & 0xFF] ^ T[2][(u >> 8) & 0xFF] ^ T[1][(u >> 16) & 0xFF] ^ T[0][u >> 24];
  }
  // merge the 256 equal-length pieces: tree over lanes, then over waves.  The
  // multipliers are constants: nibble-table products (the bit-serial gf2_mul here was
  // two thirds of the kernel's instructions)
  const u32x4 nib_mine = ((const u32x4 *)nib)[t];  // (requested here, not beside the data: four more registers held through the walk spill others)
  __syncthreads();  // every piece has been read: the segment's place takes the tables
  ((u32x4 *)N)[t] = nib_mine;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const uint32_t other = __shfl_down(c, 1u << k, 64);
    c = gf2_mul_nib(c, N + k * GF2_NIB_WORDS) ^ other;  // only lanes with (t & ((2 << k) - 1)) == 0 are used further
  }
  if ((t & 63) == 0) wave_part[t >> 6] = c;
  __syncthreads();
  if (t == 0) {
    const uint32_t a = gf2_mul_nib(wave_part[0], N + 6 * GF2_NIB_WORDS) ^ wave_part[1];
    const uint32_t b = gf2_mul_nib(wave_part[2], N + 6 * GF2_NIB_WORDS) ^ wave_part[3];
    *partial = gf2_mul_nib(a, N + 7 * GF2_NIB_WORDS) ^ b;
  }
  if constexpr (ADLER) {
    if (cut == 8u) { A1 = s1; A2 = s2; }
    // what the piece adds to chunk kA (units before the boundary) and to chunk kA + 1 (the rest): S2 counts a
    // byte by its distance to the end of ITS CHUNK, the piece sums count it to the end of the part
    const uint32_t B1 = s1 - A1, B2 = s2 - A2 - (CRC_PIECE - 16u * cut) * A1;
    const uint32_t a2 = A2 + (cut == 8u ? (uint32_t)(to_end - (int64_t)CRC_PIECE) * A1 : 0u);
    const uint32_t b2 = B2 + ((uint32_t)to_end + ADLER_CHUNK - CRC_PIECE) * B1;  // (B1 = 0 when there is no boundary)
    // the wave's 8 KiB touch at most three chunks: three sums of each kind, lane 63 of a scan holds the total
    const uint64_t k0 = ((uint64_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(kA >> 32)) << 32) |
                        (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)kA);
    const uint32_t dk = (uint32_t)(kA - k0);
    uint32_t tot[6];
#pragma unroll
    for (uint32_t k = 0; k < 3; k++) {
      const uint32_t v1 = (dk == k ? A1 : 0u) + (dk + 1u == k ? B1 : 0u);
      const uint32_t v2 = (dk == k ? a2 : 0u) + (dk + 1u == k ? b2 : 0u);
      tot[2 * k] = (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_incl(v1), 63);
      tot[2 * k + 1] = (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_incl(v2), 63);
    }
    const uint32_t ln = (uint32_t)t & 63u;
    uint32_t mine_v = tot[0];
#pragma unroll
    for (uint32_t m = 1; m < 6; m++) mine_v = ln == m ? tot[m] : mine_v;
    const uint64_t kc = k0 + (ln >> 1);
    if (ln < 6u && kc < n_chunks && mine_v) atomicAdd(adler_sums + 2 * kc + (ln & 1u), mine_v);
  }
}

// workgroup -> (range, segment) of a rectangular grid: n_ranges x segs_per_range workgroups and as many partials
template <bool ADLER>
__device__ __forceinline__ void crc32_segment(
    const uint8_t *__restrict__ base, int mode, const StreamDesc *__restrict__ descs,
    const StreamResult *__restrict__ results, uint64_t single_off, uint64_t single_len,
    uint32_t segs_per_range, const uint32_t *__restrict__ nib, uint32_t *__restrict__ partials,
    uint32_t *__restrict__ adler_sums, uint64_t n_chunks) {
  const uint32_t range = blockIdx.x / segs_per_range;
  const uint32_t seg = blockIdx.x % segs_per_range;
  uint64_t off, len;
  get_range(mode, range, descs, results, single_off, single_len, off, len);
  const uint64_t nseg = (len + CRC_SEG - 1) / CRC_SEG;
  if (seg >= nseg) return;  // uniform per workgroup
  crc32_segment_body<ADLER>(base + off, len, seg, nseg, nib, partials + ((uint64_t)range * segs_per_range + seg), adler_sums, n_chunks);
}

__global__ __launch_bounds__(CRC_THREADS, 4) void crc32_segments_kernel(
    const uint8_t *__restrict__ base, int mode, const StreamDesc *__restrict__ descs,
    const StreamResult *__restrict__ results, uint64_t single_off, uint64_t single_len,
    uint32_t segs_per_range, const uint32_t *__restrict__ nib, uint32_t *__restrict__ partials) {
  crc32_segment<false>(base, mode, descs, results, single_off, single_len, segs_per_range, nib, partials, nullptr, 0);
}

// CRC-32 partials and Adler-32 chunk sums of ONE buffer in one pass over its bytes
__global__ __launch_bounds__(CRC_THREADS, 4) void crc32_adler_segments_kernel(
    const uint8_t *__restrict__ p, uint64_t len, uint32_t n_segs, const uint32_t *__restrict__ nib,
    uint32_t *__restrict__ partials, uint2 *__restrict__ adler_sums, uint64_t n_chunks) {
  crc32_segment<true>(p, RANGE_SINGLE, nullptr, nullptr, 0, len, n_segs, nib, partials, (uint32_t *)adler_sums, n_chunks);
}

// One workgroup per range: folds the segment partials (Horner runs per thread,
// then a tree), applies init/finish (src/zipc_deflate.ml:135-136) and stores
// the checksum.
// x^(8 * nbytes) mod P from the context's table of x^(8 * 2^k): one multiply per set
// bit of nbytes (gf2_xpow8n squares once per bit position on top of that)
__device__ __forceinline__ uint32_t xpow8n_tab(const CrcConsts &K, uint64_t nbytes) {
  uint32_t r = 0x80000000u;  // x^0
  for (int k = 0; k < 48 && nbytes; k++, nbytes >>= 1)
    if (nbytes & 1) r = gf2_mul(r, K.xbyte[k]);
  if (nbytes) {  // beyond 2^48 bytes: keep squaring
    uint32_t sq = gf2_mul(K.xbyte[47], K.xbyte[47]);
    while (nbytes) {
      if (nbytes & 1) r = gf2_mul(r, sq);
      sq = gf2_mul(sq, sq);
      nbytes >>= 1;
    }
  }
  return r;
}

// The finish of a batch of SHORT ranges (at most 16 segments each, the batch forms'
// streams): one range per thread.  (One workgroup per range left 255 threads waiting
// for thread 0's ~20 dependent gf2_mul: 0.19 ms for C2's 16 384 streams.)
__global__ __launch_bounds__(256) void crc32_finish_streams_kernel(
    int mode, const StreamDesc *__restrict__ descs, StreamResult *__restrict__ results, uint32_t n_ranges,
    uint32_t segs_per_range, CrcConsts K, const uint32_t *__restrict__ partials) {
  const uint32_t range = blockIdx.x * 256u + threadIdx.x;
  if (range >= n_ranges) return;
  uint64_t off, len;
  get_range(mode, range, descs, results, 0, 0, off, len);
  if (mode == RANGE_INFLATE_OUT && results[range].status != ST_OK) return;
  const uint64_t nseg = (len + CRC_SEG - 1) / CRC_SEG;
  if (nseg > segs_per_range) {  // longer than the caller declared (max_src_len / max_dst_cap): only part of it was summed
    results[range].status = ST_INVALID_ARG;
    results[range].checksum = 0;
    return;
  }
  const uint32_t *P = partials + (uint64_t)range * segs_per_range;
  uint32_t raw = 0;
  for (uint32_t j = 0; j < (uint32_t)nseg; j++) raw = gf2_mul(raw, K.xseg) ^ P[j];
  const uint32_t state = crc_state_advance(0xFFFFFFFFu, raw, xpow8n_tab(K, len));
  results[range].checksum = state ^ 0xFFFFFFFFu;
}

// (NT = blockDim.x threads, a power of two up to 1024: the launch takes 1024 for ranges of many segments -- C3's 131 072
// partials as 256 Horner runs of 512 dependent steps took 0.118 ms, a tenth of the pass over the 4 GiB themselves)
__global__ __launch_bounds__(1024) void crc32_finish_kernel(
    int mode, const StreamDesc *__restrict__ descs, StreamResult *__restrict__ results,
    uint64_t single_len, uint32_t segs_per_range, CrcConsts K, const uint32_t *__restrict__ nib,
    const uint32_t *__restrict__ partials, uint32_t *__restrict__ single_out) {
  __shared__ uint32_t sh[1024];
  const uint32_t NT = blockDim.x;
  __shared__ uint32_t NS[GF2_NIB_WORDS];  // xseg as a nibble table
  const int t = threadIdx.x;
  const uint32_t range = blockIdx.x;
  uint64_t off, len;
  get_range(mode, range, descs, results, 0, single_len, off, len);
  if (mode == RANGE_INFLATE_OUT && results[range].status != ST_OK) return;
  const uint64_t nseg = (len + CRC_SEG - 1) / CRC_SEG;
  if (nseg > segs_per_range) {  // see crc32_finish_streams_kernel (uniform per workgroup)
    if (t == 0 && mode != RANGE_SINGLE) { results[range].status = ST_INVALID_ARG; results[range].checksum = 0; }
    return;
  }
  const uint32_t *P = partials + (uint64_t)range * segs_per_range;
  uint32_t raw = 0;
  if (nseg <= 1) {
    raw = nseg ? P[0] : 0;
  } else if (crc_finish_by_one_thread(nseg)) {  // short ranges (the batch forms' streams): Horner by the one thread that stores
    if (t == 0)
      for (uint32_t j = 0; j < (uint32_t)nseg; j++) raw = gf2_mul(raw, K.xseg) ^ P[j];
  } else {
    // right-aligned grid of R rows of NT partials: thread t takes column t -- consecutive threads, consecutive words of every row
    // (a run of consecutive partials per thread read a cache line per thread and step: C3's finish took 0.11 ms, a tenth
    // of the pass over the 4 GiB themselves) -- so its Horner step is a shift by a whole ROW, x^(8 * segment * NT), whose
    // nibble table the workgroup makes first; the tree then shifts by a segment, two, four ...
    const uint64_t R = crc_finish_rows(nseg, NT);
    const uint64_t padp = crc_finish_padp(nseg, NT);  // (the index rules: adler_chain.h)
    const uint32_t xrow = xpow8n_tab(K, (uint64_t)CRC_SEG * NT);
    if (t < GF2_NIB_WORDS) NS[t] = gf2_mul(((uint32_t)t & 15u) << (4 * (t >> 4)), xrow);  // (gf2_nib_table's entries, one per thread)
    __syncthreads();
    uint32_t c = 0;
    static_assert(CRC_FINISH_ROWS_AT_ONCE == 8, "adler_chain.h");
    for (uint64_t j0 = 0; j0 < R; j0 += 8) {  // eight rows' words requested together (clamped index, value selected afterwards: one
      uint32_t v[8];                          // load at a time behind a branch cost a memory round trip per row)
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const int64_t idx = crc_finish_index(j0 + (uint64_t)u, NT, (uint32_t)t, padp);
        const uint32_t w = P[crc_finish_load_index(idx, j0 + (uint64_t)u, R)];
        v[u] = idx >= 0 ? w : 0u;
      }
#pragma unroll
      for (int u = 0; u < 8; u++)
        if (j0 + (uint64_t)u < R) c = gf2_mul_nib(c, NS) ^ v[u];
    }
    sh[t] = c;
    __syncthreads();
    uint32_t xr = K.xseg;  // shift of one segment
    for (int s = 1; s < (int)NT; s <<= 1) {
      if ((t & (2 * s - 1)) == 0) sh[t] = gf2_mul(sh[t], xr) ^ sh[t + s];
      xr = gf2_mul(xr, xr);
      __syncthreads();
    }
    raw = sh[0];
  }
  if (t == 0) {
    const uint32_t state = crc_state_advance(0xFFFFFFFFu, raw, xpow8n_tab(K, len));
    const uint32_t crc = state ^ 0xFFFFFFFFu;
    if (mode == RANGE_SINGLE) single_out[0] = crc;
    else results[range].checksum = crc;
  }
}

// ---- Adler-32 over one buffer ---------------------------------------------------

// chunk k of the reference's grid for a buffer of n bytes: chunk 0 is
// [0, n mod 5552) (possibly empty), chunk k >= 1 is 5552 bytes
__global__ __launch_bounds__(256) void adler_chunks_kernel(const uint8_t *__restrict__ p, uint64_t n,
                                                           uint64_t n_chunks,
                                                           uint2 *__restrict__ sums) {
  const int lane = threadIdx.x & 63;
  const uint64_t chunk = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (chunk >= n_chunks) return;
  const uint64_t r = n % ADLER_CHUNK;
  const uint64_t start = chunk == 0 ? 0 : r + (chunk - 1) * ADLER_CHUNK;
  const uint32_t len = chunk == 0 ? (uint32_t)r : ADLER_CHUNK;
  uint32_t S1, S2;
  wave_adler_chunk_sums(p + start, len, lane, S1, S2);
  if (lane == 0) sums[chunk] = make_uint2(S1, S2);
}

// RFC 1950's Adler-32 of the buffer from its chunk sums: with the unsigned remainder the chunk
// steps are an affine map mod 65521 in (s1, s2), so chunks combine in any grouping: every thread
// folds a run of chunks starting from (0, 0), then the runs are chained by one thread
// (s1' = s1 + A1, s2' = s2 + bytes_of_run * s1 + A2 for a run that maps (0, 0) to (A1, A2)).
__global__ __launch_bounds__(1024) void adler_rfc_finish_kernel(const uint2 *__restrict__ sums, uint64_t n,
                                                                uint64_t n_chunks, uint32_t *__restrict__ out) {
  static_assert(ADLER_RFC_THREADS == 1024, "adler_chain.h");
  __shared__ uint32_t a1[1024], a2[1024];
  __shared__ uint64_t nb[1024];
  const uint32_t t = threadIdx.x;
  uint64_t lo, hi;
  adler_run_bounds(t, adler_rfc_per(n_chunks), n_chunks, lo, hi);
  uint32_t s1, s2;
  uint64_t bytes;
  adler_rfc_fold_run(sums, lo, hi, (uint32_t)(n % ADLER_CHUNK), s1, s2, bytes);
  a1[t] = s1; a2[t] = s2; nb[t] = bytes;
  __syncthreads();
  if (t == 0) out[0] = adler_rfc_chain(a1, a2, nb, 1024);
}

// The chunk chain: its arithmetic is adler_chain.h (HIP-free, pinned in tests/host_sim); here are its launches.
constexpr uint32_t CHAIN_THREADS_A = 1024;

__device__ __forceinline__ uint32_t block_excl_scan_mod(uint32_t v, uint32_t *sh, int t) {
  // exclusive scan of per-thread values (each < 65521) over the 1024 threads, mod p
  sh[t] = v;
  __syncthreads();
  for (int o = 1; o < (int)CHAIN_THREADS_A; o <<= 1) {
    const uint32_t u = t >= o ? sh[t - o] : 0;
    __syncthreads();
    sh[t] = addmod(sh[t], u);
    __syncthreads();
  }
  const uint32_t incl = sh[t];
  __syncthreads();
  return incl >= v ? incl - v : incl + ADLER_BASE - v;
}

// The chain runs as five small launches over R runs of `per` consecutive chunks
// (R a multiple of 1024, up to 64 Ki: a thread per run, hundreds of workgroups):
//   adler_runs_s1    sum of S1 per run
//   adler_scan_runs  exclusive scan (mod p) of the run sums by one workgroup -> s1 before each run
//   adler_runs_a     a_k summed per run from that s1; ambiguous chunks recorded
//   adler_scan_runs  scan of the a sums -> residue of s2 before each run
//   adler_replay     one thread: ambiguous chunks replayed in order, final value
// AdlerRuns: the per-run arrays in device scratch.
__global__ __launch_bounds__(256) void adler_runs_s1_kernel(const uint2 *__restrict__ sums, uint64_t n_chunks,
                                                            uint64_t per, AdlerRuns R) {
  const uint64_t run = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (run >= R.n_runs) return;
  uint64_t lo, hi;
  adler_run_bounds(run, per, n_chunks, lo, hi);
  uint64_t acc = 0;
  for (uint64_t k = lo; k < hi; k++) acc += sums[k].x;
  R.sum[run] = (uint32_t)(acc % ADLER_BASE);
}

// out[run] = (first + exclusive prefix of in[0 .. run)) mod p; the inputs are < p.  A thread owns `each`
// consecutive runs (1, 2, 4 .. 64 of them: 16-byte loads from 4 on) and everything is 32-bit: a run of 64
// values sums below 2^22, and a sum of two residues needs one conditional subtraction.
__global__ __launch_bounds__(CHAIN_THREADS_A) void adler_scan_runs_kernel(const uint32_t *__restrict__ in,
                                                                          uint32_t *__restrict__ out,
                                                                          uint32_t n_runs, uint32_t first) {
  __shared__ uint32_t sh[CHAIN_THREADS_A];
  const int t = threadIdx.x;
  const uint32_t each = n_runs / CHAIN_THREADS_A;  // n_runs is 1024 times a power of two
  const uint32_t *mine = in + (uint32_t)t * each;
  uint32_t *mine_out = out + (uint32_t)t * each;
  uint32_t acc = 0;
  if (each >= 4) {
    for (uint32_t j = 0; j < each; j += 4) {
      const u32x4 v = *(const u32x4 *)(mine + j);
      acc += v.x + v.y + v.z + v.w;
    }
  } else {
    for (uint32_t j = 0; j < each; j++) acc += mine[j];
  }
  uint32_t pre = addmod(first % ADLER_BASE, block_excl_scan_mod(acc % ADLER_BASE, sh, t));
  if (each >= 4) {
    for (uint32_t j = 0; j < each; j += 4) {
      const u32x4 v = *(const u32x4 *)(mine + j);
      u32x4 o;
      o.x = pre; pre = addmod(pre, v.x);
      o.y = pre; pre = addmod(pre, v.y);
      o.z = pre; pre = addmod(pre, v.z);
      o.w = pre; pre = addmod(pre, v.w);
      *(u32x4 *)(mine_out + j) = o;
    }
  } else {
    for (uint32_t j = 0; j < each; j++) {
      const uint32_t v = mine[j];
      mine_out[j] = pre;
      pre = addmod(pre, v);
    }
  }
}

__global__ __launch_bounds__(256) void adler_runs_a_kernel(const uint2 *__restrict__ sums, uint64_t n,
                                                           uint64_t n_chunks, uint64_t per, AdlerRuns R,
                                                           uint32_t *__restrict__ amb_raw, uint32_t amb_cap) {
  AmbRecord *amb = (AmbRecord *)amb_raw;
  const uint64_t run = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (run >= R.n_runs) return;
  const uint32_t r = (uint32_t)(n % ADLER_CHUNK);
  uint64_t lo, hi;
  adler_run_bounds(run, per, n_chunks, lo, hi);
  uint64_t s1 = R.s1_before[run], a_acc = 0;
  uint32_t last_hi = 0xFFFFFFFFu;  // branch of the previous chunk (unknown for the first of the run)
  for (uint64_t k = lo; k < hi; k++) {
    const uint2 sm = sums[k];
    AmbRecord rec;
    if (adler_runs_a_step(k, adler_chunk_len(k, r), sm.x, sm.y, s1, a_acc, last_hi, rec)) {
      const uint32_t slot = atomicAdd(R.amb_count, 1u);
      if (slot < amb_cap) amb[slot] = rec;
    }
  }
  R.sum[run] = (uint32_t)a_acc;       // the run's a sum (the S1 sums are no longer needed)
  R.last_hi[run] = last_hi;
  R.s1_after[run] = (uint32_t)s1;
}

__global__ __launch_bounds__(CHAIN_THREADS_A) void adler_replay_kernel(const uint2 *__restrict__ sums, uint64_t n,
                                                                       uint64_t n_chunks, uint64_t per, AdlerRuns R,
                                                                       uint32_t *__restrict__ amb_raw,
                                                                       uint32_t amb_cap, uint32_t *__restrict__ out) {
  // everything the serial replay reads is gathered into LDS by the whole
  // workgroup first: one thread walking global memory pays a full memory latency
  // per access
  // -- and everything that does not depend on the chunks before a record is worked out by the thread that
  // ranks it: the one thread's loop is a handful of 32-bit operations per record.
  __shared__ uint32_t keys[REPLAY_MAX];
  __shared__ uint32_t r_k[REPLAY_MAX];     // sorted by chunk index: the chunk,
  __shared__ uint32_t r_res[REPLAY_MAX];   // the predicted residue of s2 before it,
  __shared__ uint32_t r_C[REPLAY_MAX];     // C = n * s1 + S2 (< 2^32),
  __shared__ uint32_t r_pc[REPLAY_MAX];    // what the prediction adds for the chunk: (C - 225 * hi) mod p,
  __shared__ uint8_t r_prev[REPLAY_MAX];   // the branch of the chunk before it as C alone decides it
  const AmbRecord *amb = (const AmbRecord *)amb_raw;
  const int t = threadIdx.x;
  const uint32_t r = (uint32_t)(n % ADLER_CHUNK);
  const uint32_t *run_res = R.res_before, *run_a = R.sum, *run_last_hi = R.last_hi;
  const uint32_t n_amb = R.amb_count[0];
  if (adler_replay_falls_back(n_amb, amb_cap, REPLAY_MAX)) {
    // adversarial input: more ambiguous chunks than worth sorting -- plain walk
    if (t != 0) return;
    out[0] = adler_plain_walk(sums, n_chunks, r);
    return;
  }
  for (uint32_t i = (uint32_t)t; i < n_amb; i += CHAIN_THREADS_A) keys[i] = amb[i].k;
  __syncthreads();
  for (uint32_t i = (uint32_t)t; i < n_amb; i += CHAIN_THREADS_A) {  // rank sort (chunk indices are distinct)
    const AmbRecord rec = amb[i];
    uint32_t rank = 0;
    for (uint32_t j = 0; j < n_amb; j++) rank += keys[j] < rec.k ? 1u : 0u;
    const ReplayRecord p = adler_replay_prepare(rec, r, sums[rec.k].y, per, run_res, run_last_hi);
    r_k[rank] = p.k;
    r_res[rank] = p.res;
    r_C[rank] = p.C;
    r_pc[rank] = p.pc;
    r_prev[rank] = p.prev;
  }
  __syncthreads();
  if (t != 0) return;
  // ---- replay of the ambiguous chunks, in order, by one thread
  ReplayState st;
  for (uint32_t i = 0; i < n_amb; i++) adler_replay_step(st, r_k[i], r_res[i], r_C[i], r_pc[i], r_prev[i] != 0);
  out[0] = adler_replay_final(st, n_chunks, per, run_res, run_a, run_last_hi, R.s1_after);
}

// ---- many ranges of one arena, ragged (zipc_hip_checksum_batch) -----------------------------------------------------
// The rectangular grid above is n_ranges x segments(longest range): ten thousand short ranges beside one long one are
// almost only empty workgroups.  Here a plan first gives every range a run of the partials and of the chunk sums as long
// as IT needs (two exclusive scans), and the segment pass is one workgroup per segment that exists: the grid is the
// bound total_len / 32 KiB + n_ranges, and a workgroup finds its range by bisection of the bases.  Every index, bound and
// verdict below is checksum_ranges.h's; tests/checksum_ranges_sim runs the same functions as loops on the host.
static_assert(RANGES_SEG_BYTES == CRC_SEG, "checksum_ranges.h");
static_assert(RANGES_FINISH_LANES == 64, "a wave per range");

// One workgroup: tiles of RANGES_PLAN_TILE ranges, a range per thread, an inclusive scan of the three counts in LDS and
// a carry from tile to tile.  Then the call-wide word, and every result's first state: the verdict (or INVALID_ARG for
// all of a bad call) and no checksum.  It also zeroes the call's n_sums pairs of chunk sums (none where no Adler-32 is
// asked for): the segment pass adds into them, and a kernel in front of it in the queue is an order the pass can rely on.
__global__ __launch_bounds__(RANGES_PLAN_TILE) void checksum_plan_kernel(const Range *__restrict__ ranges, uint32_t n_ranges,
                                                                         uint64_t arena_len, uint64_t total_len, RangesPlan P,
                                                                         RangeResult *__restrict__ results, uint2 *__restrict__ sums,
                                                                         uint64_t n_sums) {
  __shared__ RangeCounts sh[RANGES_PLAN_TILE];
  const uint32_t t = threadIdx.x;
  for (uint64_t k = t; k < n_sums; k += RANGES_PLAN_TILE) sums[k] = make_uint2(0u, 0u);
  RangeCounts carry{0, 0, 0};
  for (uint64_t t0 = 0; t0 < n_ranges; t0 += RANGES_PLAN_TILE) {  // (uniform: every thread takes every tile)
    const uint64_t i = t0 + t;
    RangeCounts mine{0, 0, 0};
    uint32_t verdict = ST_OK;
    if (i < n_ranges) {
      const Range r = ranges[i];
      mine = range_counts(r, arena_len);
      verdict = range_verdict(r, arena_len);
    }
    sh[t] = mine;
    __syncthreads();
    for (uint32_t o = 1; o < RANGES_PLAN_TILE; o <<= 1) {
      RangeCounts u{0, 0, 0};
      if (t >= o) u = sh[t - o];
      __syncthreads();
      if (t >= o) sh[t] = ranges_counts_add(u, sh[t]);
      __syncthreads();
    }
    const RangeCounts before = t ? ranges_counts_add(carry, sh[t - 1]) : carry;
    if (i < n_ranges) {
      P.seg_base[i] = ranges_seg_base(before);
      P.chunk_base[i] = ranges_chunk_base(before);
      results[i].status = verdict;
    }
    carry = ranges_counts_add(carry, sh[RANGES_PLAN_TILE - 1]);
    __syncthreads();  // (the next tile overwrites sh)
  }
  const RangesCall call = ranges_call_word(carry, total_len);
  if (t == 0) *P.call = call;
  for (uint64_t i = t; i < n_ranges; i += RANGES_PLAN_TILE) {  // (i = t0 + t: the thread that wrote the verdict reads it)
    RangeResult r;
    r.status = ranges_status(call, results[i].status);
    r.crc32 = r.adler32 = r.reserved = 0;
    results[i] = r;
  }
}

// workgroup -> (range, segment) of the ragged grid.  ADLER: the chunk sums go to the range's own run of `sums`; each
// range has its own chunk grid (first chunk = len mod 5552), and crc32_segment_body's argument that a chunk boundary
// falls between two 16-byte units holds per range: both grids are congruent to THAT range's len.
template <bool ADLER>
__device__ __forceinline__ void crc32_ranges(const uint8_t *__restrict__ arena, const Range *__restrict__ ranges, uint32_t n_ranges,
                                             const RangesPlan &P, const uint32_t *__restrict__ nib, uint32_t *__restrict__ partials,
                                             uint2 *__restrict__ sums) {
  const RangesCall call = *P.call;
  const uint32_t w = blockIdx.x;
  if (ranges_wg_idle(call, w)) return;  // (uniform per workgroup, like every return here)
  const RangeWork k = ranges_work(P.seg_base, P.chunk_base, n_ranges, w);
  if (k.range >= n_ranges) return;  // (never: w < total_segs)
  const Range r = ranges[k.range];
  const uint64_t nseg = range_segs(r.len);
  if (k.seg >= nseg) return;  // (never: the range found is the one whose run of partials holds w)
  crc32_segment_body<ADLER>(arena + r.off, r.len, k.seg, nseg, nib, partials + k.slot, ADLER ? (uint32_t *)(sums + k.chunk_at) : nullptr,
                            adler_n_chunks(r.len));
}
__global__ __launch_bounds__(CRC_THREADS, 4) void crc32_ranges_kernel(const uint8_t *__restrict__ arena, const Range *__restrict__ ranges,
                                                                      uint32_t n_ranges, RangesPlan P, const uint32_t *__restrict__ nib,
                                                                      uint32_t *__restrict__ partials) {
  crc32_ranges<false>(arena, ranges, n_ranges, P, nib, partials, nullptr);
}
__global__ __launch_bounds__(CRC_THREADS, 4) void crc32_adler_ranges_kernel(const uint8_t *__restrict__ arena,
                                                                            const Range *__restrict__ ranges, uint32_t n_ranges,
                                                                            RangesPlan P, const uint32_t *__restrict__ nib,
                                                                            uint32_t *__restrict__ partials, uint2 *__restrict__ sums) {
  crc32_ranges<true>(arena, ranges, n_ranges, P, nib, partials, sums);
}

// A wave per range (the batch is ragged: a workgroup of 1024 per short range would idle, a thread per long range would
// walk thousands of partials alone): up to 16 partials by lane 0, more by a column per lane and a tree over the lanes.
__global__ __launch_bounds__(256) void crc32_finish_ranges_kernel(const Range *__restrict__ ranges, uint32_t n_ranges, RangesPlan P,
                                                                  CrcConsts K, const uint32_t *__restrict__ partials,
                                                                  RangeResult *__restrict__ results) {
  const uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63u;
  if (i >= n_ranges || P.call->bad != 0 || results[i].status != ST_OK) return;  // (uniform per wave)
  const uint64_t len = ranges[i].len, nseg = range_segs(len), base = P.seg_base[i];
  uint32_t raw;
  if (ranges_crc_by_one_lane(nseg)) {
    if (lane != 0) return;
    raw = ranges_crc_horner(partials, base, nseg, K.xseg);
  } else {
    uint32_t c = ranges_crc_column(partials, base, nseg, lane, xpow8n_tab(K, (uint64_t)CRC_SEG * RANGES_FINISH_LANES));
    uint32_t xr = K.xseg;  // shift of one segment
    for (uint32_t s = 1; s < RANGES_FINISH_LANES; s <<= 1) {
      const uint32_t other = __shfl_down(c, s, 64);
      c = ranges_crc_tree_step(c, other, xr);  // only lanes with (lane & (2 s - 1)) == 0 are used further
      xr = gf2_mul(xr, xr);
    }
    if (lane != 0) return;
    raw = c;
  }
  results[i].crc32 = ranges_crc_value(raw, xpow8n_tab(K, len));
}

// A lane per range: the walk over the range's chunk sums, serial per range (a long range's chunks by run, scan and
// replay as zipc_hip_checksum_device chains them are not built for the batch).
__global__ __launch_bounds__(256) void adler_finish_ranges_kernel(const Range *__restrict__ ranges, uint32_t n_ranges, RangesPlan P,
                                                                  const uint2 *__restrict__ sums, int rfc,
                                                                  RangeResult *__restrict__ results) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_ranges || P.call->bad != 0 || results[i].status != ST_OK) return;
  results[i].adler32 = ranges_adler_walk(sums, P.chunk_base[i], ranges[i].len, rfc != 0);
}

}  // namespace zd
