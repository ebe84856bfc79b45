// sim_ranges.cpp -- host model of the ragged checksum pass (zipc_hip_checksum_batch): the launches of checksum.hip as loops.
//
// Everything a kernel of that pass decides -- verdicts, counts, bases, grid bounds, the workgroup's range, the finishes'
// indices -- is zipc_amd/csrc/checksum_ranges.h, compiled here with g++.  What the model adds is what a kernel does
// between those decisions, in its plainest form: a byte-wise CRC-32 of the segment's bytes and byte sums per chunk stand
// in for the LDS walk.  Every array is reached through a wrapper that checks the index against the size the CALL gives
// that array (segs_bound partials, chunks_bound pairs of sums, n entries of the plan) before it is used: an index that
// leaves is counted, never followed, so a mutant of the header cannot harm the process that runs it.
// tests/test_checksum_ranges_rules.py loads this as a library; audit_main.cpp includes it and aborts on any violation.
#include <stdint.h>
#include <string.h>

#include <vector>

#ifndef RANGES_HEADER
#define RANGES_HEADER "../../zipc_amd/csrc/checksum_ranges.h"
#endif
#include RANGES_HEADER

using namespace zd;

namespace sim {

struct Audit {
  uint64_t violations = 0;
  uint64_t one_lane = 0, columns = 0, max_rows = 0, tiles = 0, loads = 0;
};

template <class T>
struct Checked {
  std::vector<T> v;
  Audit *a;
  mutable T sink{};
  Checked(size_t n, Audit *a_) : v(n), a(a_) {}
  T &operator[](uint64_t i) {
    if (i >= v.size()) { a->violations++; sink = T{}; return sink; }
    return v[i];
  }
  const T &operator[](uint64_t i) const {
    if (i >= v.size()) { a->violations++; sink = T{}; return sink; }
    return v[i];
  }
};

struct Sums { uint32_t x, y; };

static uint32_t crc_table[256];
static void crc_init() {
  if (crc_table[1]) return;
  for (uint32_t i = 0; i < 256; i++) {
    uint32_t c = i;
    for (int k = 0; k < 8; k++) c = (c & 1u) ? (CRC_POLY ^ (c >> 1)) : (c >> 1);
    crc_table[i] = c;
  }
}
// raw CRC (init 0, no final xor) of bytes [lo, hi)
static uint32_t crc_raw(const uint8_t *p, uint64_t lo, uint64_t hi) {
  uint32_t c = 0;
  for (uint64_t i = lo; i < hi; i++) c = crc_table[(c ^ p[i]) & 0xFF] ^ (c >> 8);
  return c;
}

// the CRC-32 itself (init and final xor), for audit_main.cpp
static uint32_t crc_raw_init(const uint8_t *p, uint64_t n) {
  crc_init();
  uint32_t c = 0xFFFFFFFFu;
  for (uint64_t i = 0; i < n; i++) c = crc_table[(c ^ p[i]) & 0xFF] ^ (c >> 8);
  return c ^ 0xFFFFFFFFu;
}

// One call.  stats: [0] true segments, [1] true chunks, [2] segs_bound, [3] chunks_bound, [4] bad call, [5] violations,
// [6] ranges finished by one lane, [7] by columns, [8] the most rows of a column, [9] tiles of the plan's scan,
// [10] bytes the segment pass loaded, [11] workgroups that found work.  Returns the violations.
static uint64_t run(const uint8_t *arena, uint64_t arena_len, const Range *ranges, uint32_t n, uint64_t total_len, int want_crc,
                    int want_adler, int rfc, RangeResult *results, uint64_t *stats) {
  crc_init();
  Audit au;
  const uint64_t segs_bound = ranges_segs_bound(total_len, n), chunks_bound = ranges_chunks_bound(total_len, n);
  Checked<uint32_t> seg_base(n, &au), partials(segs_bound, &au);
  Checked<uint64_t> chunk_base(n, &au);
  Checked<Sums> sums(chunks_bound, &au);  // (zeroed: checksum_plan's first loop)
  Checked<RangeResult> res(n, &au);

  // ---- checksum_plan: one workgroup, tiles of RANGES_PLAN_TILE ranges, a carry from tile to tile
  RangeCounts carry{0, 0, 0};
  for (uint64_t t0 = 0; t0 < n; t0 += RANGES_PLAN_TILE) {
    au.tiles++;
    RangeCounts run_sum = carry;
    for (uint64_t t = 0; t < RANGES_PLAN_TILE && t0 + t < n; t++) {  // (the tile's exclusive scan, thread by thread)
      const uint64_t i = t0 + t;
      seg_base[i] = ranges_seg_base(run_sum);
      chunk_base[i] = ranges_chunk_base(run_sum);
      res[i].status = range_verdict(ranges[i], arena_len);
      run_sum = ranges_counts_add(run_sum, range_counts(ranges[i], arena_len));
    }
    carry = run_sum;
  }
  const RangesCall call = ranges_call_word(carry, total_len);
  for (uint64_t i = 0; i < n; i++) {
    RangeResult r{ranges_status(call, res[i].status), 0, 0, 0};
    res[i] = r;
  }

  // ---- crc32_ranges: segs_bound workgroups
  uint64_t worked = 0;
  for (uint64_t w = 0; w < segs_bound; w++) {
    if (ranges_wg_idle(call, w)) continue;
    const RangeWork k = ranges_work(seg_base, chunk_base, n, (uint32_t)w);
    if (k.range >= n) { au.violations++; continue; }  // the search left [0, n)
    const Range r = ranges[k.range];
    if (res[k.range].status != ST_OK) { au.violations++; continue; }  // a bad range's bytes are never read
    if (k.seg >= range_segs(r.len)) { au.violations++; continue; }
    uint64_t lo, hi;
    ranges_seg_interval(r.len, k.seg, lo, hi);
    if (!(lo < hi && hi <= r.len && hi - lo <= RANGES_SEG_BYTES) || r.off + hi > arena_len) { au.violations++; continue; }
    worked++;
    au.loads += hi - lo;
    partials[k.slot] = crc_raw(arena + r.off, lo, hi);
    if (want_adler) {
      const uint64_t n_chunks = adler_n_chunks(r.len);
      for (uint64_t pos = lo; pos < hi;) {  // chunk by chunk of the range's own grid
        uint64_t end;
        const uint64_t c = ranges_chunk_of(r.len, pos, end);
        if (c >= n_chunks || end <= pos) { au.violations++; break; }
        Sums &s = sums[k.chunk_at + c];
        for (; pos < hi && pos < end; pos++) {
          const uint32_t b = arena[r.off + pos];
          s.x += b;
          s.y += (uint32_t)(end - pos) * b;
        }
      }
    }
  }

  // ---- crc32_finish_ranges: a wave per range
  if (want_crc && !call.bad) {
    const uint32_t xseg = gf2_xpow8n(RANGES_SEG_BYTES), xrow = gf2_xpow8n((uint64_t)RANGES_SEG_BYTES * RANGES_FINISH_LANES);
    for (uint64_t i = 0; i < n; i++) {
      if (res[i].status != ST_OK) continue;
      const uint64_t len = ranges[i].len, nseg = range_segs(len), base = seg_base[i];
      uint32_t raw;
      if (ranges_crc_by_one_lane(nseg)) {
        au.one_lane++;
        raw = ranges_crc_horner(partials, base, nseg, xseg);
      } else {
        au.columns++;
        const uint64_t R = crc_finish_rows(nseg, RANGES_FINISH_LANES);
        au.max_rows = R > au.max_rows ? R : au.max_rows;
        uint32_t c[RANGES_FINISH_LANES];
        for (uint32_t t = 0; t < RANGES_FINISH_LANES; t++) c[t] = ranges_crc_column(partials, base, nseg, t, xrow);
        uint32_t xr = xseg;
        for (uint32_t s = 1; s < RANGES_FINISH_LANES; s <<= 1) {
          for (uint32_t t = 0; t + s < RANGES_FINISH_LANES; t += 2 * s) c[t] = ranges_crc_tree_step(c[t], c[t + s], xr);
          xr = gf2_mul(xr, xr);
        }
        raw = c[0];
      }
      res[i].crc32 = ranges_crc_value(raw, gf2_xpow8n(len));
    }
  }
  // ---- adler_finish_ranges: a lane per range
  if (want_adler && !call.bad)
    for (uint64_t i = 0; i < n; i++) {
      if (res[i].status != ST_OK) continue;
      res[i].adler32 = ranges_adler_walk(sums, chunk_base[i], ranges[i].len, rfc != 0);
    }

  for (uint64_t i = 0; i < n; i++) results[i] = res[i];
  if (!call.bad && (carry.segs > segs_bound || carry.chunks > chunks_bound)) au.violations++;
  stats[0] = carry.segs; stats[1] = carry.chunks; stats[2] = segs_bound; stats[3] = chunks_bound; stats[4] = call.bad;
  stats[5] = au.violations; stats[6] = au.one_lane; stats[7] = au.columns; stats[8] = au.max_rows; stats[9] = au.tiles;
  stats[10] = au.loads; stats[11] = worked;
  return au.violations;
}

}  // namespace sim

extern "C" {
uint64_t sim_ranges_run(const uint8_t *arena, uint64_t arena_len, const Range *ranges, uint32_t n, uint64_t total_len, int want_crc,
                        int want_adler, int rfc, RangeResult *results, uint64_t *stats) {
  return sim::run(arena, arena_len, ranges, n, total_len, want_crc, want_adler, rfc, results, stats);
}
uint32_t sim_ranges_plan_tile() { return RANGES_PLAN_TILE; }
uint32_t sim_ranges_horner_max() { return CRC_FINISH_HORNER_MAX; }
uint32_t sim_ranges_finish_lanes() { return RANGES_FINISH_LANES; }
uint32_t sim_range_verdict(uint64_t off, uint64_t len, uint64_t arena_len) { return range_verdict(Range{off, len}, arena_len); }
}
