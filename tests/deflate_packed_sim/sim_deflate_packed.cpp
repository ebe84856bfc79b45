// sim_deflate_packed.cpp -- host model of the packed encode forms (zipc_hip_deflate_packed_batch): the four kernels of
// zipc_amd/csrc/deflate_packed.hip as plain loops over real host byte arrays.
//
// Everything those kernels decide -- the declared-size verdict, the slots, the descriptors deflate runs with, which streams
// take room and fit, the verdicts, `need`, the segment bases, a workgroup's stream and segment, the head, body and tail of a
// segment, the results -- is zipc_amd/csrc/deflate_packed.h, compiled here with g++.  What the model adds is the kernels'
// shape: tiles of DPACKED_TILE streams, waves of DPACKED_WAVE lanes with an inclusive scan each, the waves' totals summed
// behind them, bases carried from tile to tile; the copy per (workgroup, thread) over every workgroup of the grid bound,
// a thread's loads of a round before its stores.  A stub stands in for the codec: the caller says what deflate would report
// of every stream IF it runs, the stub fills that stream's slot with bytes that depend on the stream and the position, and
// a "no stream" descriptor gets what deflate says of one (ST_DST_TOO_SMALL, no bytes).  Every array is reached through a
// wrapper that checks the index before it is used: an index that leaves is counted, never followed.  The destination is
// written through a recorder that keeps, per byte, how often it was written and by which workgroup.
// tests/test_deflate_packed_rules.py loads this as a library; audit_main.cpp includes it.
#include <stdint.h>
#include <string.h>

#include <type_traits>
#include <vector>

#ifndef DPACKED_HEADER
#define DPACKED_HEADER "../../zipc_amd/csrc/deflate_packed.h"
#endif
#include DPACKED_HEADER

using namespace zd;

namespace sim {

template <class T>
struct Checked {
  T *p;
  uint64_t n;
  uint64_t *violations;
  typename std::remove_const<T>::type sink{};
  Checked(T *p_, uint64_t n_, uint64_t *v) : p(p_), n(n_), violations(v) {}
  T &operator[](uint64_t i) {
    if (i >= n) { ++*violations; sink = {}; return sink; }
    return p[i];
  }
  // (ranges_find reads through a const reference)
  const T &operator[](uint64_t i) const {
    if (i >= n) { ++*violations; return sink; }
    return p[i];
  }
};

// the byte the stub's deflate leaves at position j of stream i's output
inline uint8_t staged_byte(uint64_t i, uint64_t j) { return (uint8_t)(i * 167 + j * 13 + (j >> 8) + 1); }

}  // namespace sim

extern "C" {

uint32_t sim_dpacked_tile() { return DPACKED_TILE; }
uint32_t sim_dpacked_wave() { return DPACKED_WAVE; }
uint32_t sim_dpacked_seg_bytes() { return DPACKED_SEG_BYTES; }
uint64_t sim_dpacked_slot_align() { return DPACKED_SLOT_ALIGN; }
uint32_t sim_dpacked_call_status(int dst_null, uint64_t dst_arena_len, uint64_t n, uint64_t max_src_len, uint64_t total_src_len, int level,
                                 int crc_op, uint64_t align, int zlib) {
  return dpacked_call_status(dst_null != 0, dst_arena_len, n, max_src_len, total_src_len, level, crc_op, align, zlib != 0);
}
uint64_t sim_dpacked_slot_bytes(uint64_t src_len, int zlib) { return dpacked_slot_bytes(src_len, zlib != 0); }
uint64_t sim_dpacked_arena_bound(uint64_t n, uint64_t total_src_len, uint64_t align, int zlib) { return dpacked_arena_bound(n, total_src_len, align, zlib != 0); }
uint64_t sim_dpacked_staging_bound(uint64_t n, uint64_t total_src_len, int zlib) { return dpacked_staging_bound(n, total_src_len, zlib != 0); }
uint64_t sim_dpacked_copy_grid(uint64_t n, uint64_t total_src_len, int zlib) { return dpacked_copy_grid(n, total_src_len, zlib != 0); }
uint8_t sim_dpacked_staged_byte(uint64_t i, uint64_t j) { return sim::staged_byte(i, j); }

// One call over n streams.  descs: the caller's descriptors; would: what deflate reports of stream i if it runs (out_len
// at most its slot).  base_mis: the destination arena's address modulo 16.  dst: dst_alloc >= dst_arena_len bytes, the
// arena and guard bytes behind it; written[dst_alloc]: per byte, how often it was written; owner[dst_alloc]: the workgroup
// that wrote it last, plus one.  Out: inner (the descriptors deflate ran with), stage_status, verdicts, seg_base, results,
// need[0].  stats: [0] violations, [1] vector stores off a 16-byte boundary, [2] bytes written more than once, [3] the
// segments, [4] the call's bad flag, [5] streams that reached deflate, [6] the copy's grid, [7] the end of the last slot,
// [8] vector stores, [9] byte stores, [10] the stage's tiles, [11] workgroups that found work.  Returns the violations.
uint64_t sim_dpacked_run(const StreamDesc *descs_, const StreamResult *would_, uint32_t n, uint64_t max_src_len, uint64_t total_src_len, int zlib_,
                         int crc_op, uint64_t align, uint64_t dst_arena_len, uint32_t base_mis, uint8_t *dst_, uint64_t dst_alloc,
                         uint8_t *written_, uint32_t *owner_, StreamDesc *inner_, uint32_t *stage_status_, PackedVerdict *verdicts_,
                         uint32_t *seg_base_, PackedResult *results_, uint64_t *need_out, uint64_t *stats) {
  const bool zlib = zlib_ != 0;
  uint64_t violations = 0, misaligned = 0, twice = 0, reached = 0, tiles = 0, slots_end = 0, vec_stores = 0, byte_stores = 0, busy = 0;
  sim::Checked<const StreamDesc> descs(descs_, n, &violations);
  sim::Checked<const StreamResult> would(would_, n, &violations);
  sim::Checked<StreamDesc> inner(inner_, n, &violations);
  sim::Checked<uint32_t> stage_status(stage_status_, n, &violations), seg_base(seg_base_, n, &violations);
  sim::Checked<PackedVerdict> verdicts(verdicts_, n, &violations);
  sim::Checked<PackedResult> results(results_, n, &violations);
  sim::Checked<uint8_t> dst(dst_, dst_alloc, &violations), written(written_, dst_alloc, &violations);
  sim::Checked<uint32_t> owner(owner_, dst_alloc, &violations);
  constexpr uint32_t WAVES = DPACKED_TILE / DPACKED_WAVE;
  // the launcher's scratch, from the declared numbers alone (deflate_packed.hip dpacked_reserve)
  const uint64_t staging_len = dpacked_staging_bound(n, total_src_len, zlib) + DPACKED_UNIT;
  std::vector<uint8_t> staging_v(staging_len, 0xA5);
  std::vector<StreamResult> staged_v(n ? n : 1);
  sim::Checked<uint8_t> staging(staging_v.data(), staging_len, &violations);
  sim::Checked<StreamResult> staged(staged_v.data(), n, &violations);
  DpackedCall call{};

  // ---- dpacked_stage_kernel: the declared sizes (a thread's streams, a wave's sum, the waves' sums) ...
  {
    uint64_t wave_total[WAVES] = {};
    uint32_t wave_over[WAVES] = {};
    for (uint32_t t = 0; t < DPACKED_TILE; t++) {
      uint64_t mine = 0;
      uint32_t over = 0;
      for (uint64_t i = t; i < n; i += DPACKED_TILE) {
        const uint64_t l = descs[i].src_len;
        mine = packed_add(mine, dpacked_declared_len(l));
        over |= dpacked_over_max(l, max_src_len) ? 1u : 0u;
      }
      wave_total[t / DPACKED_WAVE] = packed_add(wave_total[t / DPACKED_WAVE], mine);
      wave_over[t / DPACKED_WAVE] |= over;
    }
    uint64_t sum_len = 0;
    uint32_t any_over = 0;
    for (uint32_t k = 0; k < WAVES; k++) { sum_len = packed_add(sum_len, wave_total[k]); any_over |= wave_over[k]; }
    call.bad = dpacked_declared_bad(any_over != 0, sum_len, total_src_len);
  }
  // ... then the slots
  {
    uint64_t base = 0;
    std::vector<uint64_t> room(DPACKED_TILE), incl(DPACKED_TILE);
    for (uint64_t t0 = 0; t0 < n; t0 += DPACKED_TILE) {
      tiles++;
      uint64_t wave_total[WAVES];
      for (uint32_t t = 0; t < DPACKED_TILE; t++) room[t] = t0 + t < n ? dpacked_slot_room(descs[t0 + t].src_len, zlib) : 0;
      for (uint32_t w = 0; w < WAVES; w++) {  // a wave's two inclusive scans
        uint32_t lo = 0, hi = 0;
        for (uint32_t lane = 0; lane < DPACKED_WAVE; lane++) {
          const uint32_t t = w * DPACKED_WAVE + lane;
          lo += packed_scan_lo(room[t]);
          hi += packed_scan_hi(room[t]);
          incl[t] = packed_scan_join(lo, hi);
        }
        wave_total[w] = incl[w * DPACKED_WAVE + DPACKED_WAVE - 1];
      }
      uint64_t tile_total = 0;
      for (uint32_t w = 0; w < WAVES; w++) tile_total = packed_add(tile_total, wave_total[w]);
      for (uint32_t t = 0; t < DPACKED_TILE; t++) {
        const uint64_t i = t0 + t;
        if (i >= n) continue;
        uint64_t before = 0;
        for (uint32_t k = 0; k < t / DPACKED_WAVE; k++) before = packed_add(before, wave_total[k]);
        const uint64_t off = packed_add(packed_add(base, before), incl[t] - room[t]);
        const uint32_t st = dpacked_stage_status(call.bad, descs[i].src_len);
        stage_status[i] = st;
        inner[i] = dpacked_inner_desc(descs[i], st, off, zlib);
      }
      base = packed_tile_base(base, tile_total);
    }
  }

  // ---- deflate (the stub): a stream that runs fills its slot -- which must begin on a slot boundary, behind the slot in
  // front of it and inside the staging arena -- with its bytes
  for (uint64_t i = 0; i < n; i++) {
    const StreamDesc in = inner[i];
    const bool no_stream = in.src_len == 0 && in.dst_cap == 0 && in.flags == 0;
    StreamResult r = StreamResult{ST_DST_TOO_SMALL, 0, 0};
    if (!no_stream) {
      reached++;
      r = would[i];
      if (in.dst_off % DPACKED_SLOT_ALIGN != 0) violations++;
      if (in.dst_off < slots_end) violations++;
      if (in.dst_off + in.dst_cap > dpacked_staging_bound(n, total_src_len, zlib)) violations++;
      if (r.out_len > in.dst_cap) violations++;
      slots_end = in.dst_off + in.dst_cap;
      if (r.status == ST_OK)
        for (uint64_t j = 0; j < r.out_len; j++) staging[in.dst_off + j] = sim::staged_byte(i, j);
    }
    staged[i] = r;
  }

  // ---- dpacked_layout_kernel
  {
    uint64_t base = 0, need = 0;
    uint32_t segs_carried = 0;
    std::vector<uint32_t> st(DPACKED_TILE), segs(DPACKED_TILE), segs_incl(DPACKED_TILE);
    std::vector<StreamResult> s(DPACKED_TILE);
    std::vector<uint64_t> room(DPACKED_TILE), incl(DPACKED_TILE);
    std::vector<PackedVerdict> v(DPACKED_TILE);
    for (uint64_t t0 = 0; t0 < n; t0 += DPACKED_TILE) {
      uint64_t wave_total[WAVES], wave_end[WAVES];
      uint32_t wave_segs[WAVES];
      for (uint32_t t = 0; t < DPACKED_TILE; t++) {
        const uint64_t i = t0 + t;
        st[t] = ST_INVALID_ARG;
        s[t] = StreamResult{ST_INVALID_ARG, 0, 0};  // (past the end: no room)
        if (i < n) { st[t] = stage_status[i]; s[t] = staged[i]; }
        room[t] = dpacked_room(st[t], s[t], align);
      }
      for (uint32_t w = 0; w < WAVES; w++) {
        uint32_t lo = 0, hi = 0;
        for (uint32_t lane = 0; lane < DPACKED_WAVE; lane++) {
          const uint32_t t = w * DPACKED_WAVE + lane;
          lo += packed_scan_lo(room[t]);
          hi += packed_scan_hi(room[t]);
          incl[t] = packed_scan_join(lo, hi);
        }
        wave_total[w] = incl[w * DPACKED_WAVE + DPACKED_WAVE - 1];
      }
      uint64_t tile_total = 0;
      for (uint32_t w = 0; w < WAVES; w++) tile_total = packed_add(tile_total, wave_total[w]);
      for (uint32_t w = 0; w < WAVES; w++) {
        uint64_t before = 0;
        for (uint32_t k = 0; k < w; k++) before = packed_add(before, wave_total[k]);
        uint64_t end = 0;
        uint32_t run = 0;
        for (uint32_t lane = 0; lane < DPACKED_WAVE; lane++) {
          const uint32_t t = w * DPACKED_WAVE + lane;
          const uint64_t off = packed_add(packed_add(base, before), incl[t] - room[t]);
          v[t] = dpacked_verdict(st[t], s[t], off, dst_arena_len);
          if (t0 + t < n) verdicts[t0 + t] = v[t];
          segs[t] = (uint32_t)dpacked_copy_segs(v[t], s[t].out_len);
          run += segs[t];
          segs_incl[t] = run;
          end = packed_need_join(end, dpacked_end(v[t], s[t].out_len));
        }
        wave_segs[w] = run;
        wave_end[w] = end;
      }
      uint32_t segs_total = 0;
      for (uint32_t w = 0; w < WAVES; w++) {
        for (uint32_t lane = 0; lane < DPACKED_WAVE; lane++) {
          const uint32_t t = w * DPACKED_WAVE + lane;
          if (t0 + t < n) seg_base[t0 + t] = segs_carried + segs_total + (segs_incl[t] - segs[t]);
        }
        segs_total += wave_segs[w];
        need = packed_need_join(need, wave_end[w]);
      }
      segs_carried += segs_total;
      base = packed_tile_base(base, tile_total);
    }
    call.need = need;
    call.total_segs = segs_carried;
    if (need_out) need_out[0] = need;
  }

  // ---- dpacked_copy_kernel, every workgroup of the grid bound, thread by thread
  const uint64_t grid = dpacked_copy_grid(n, total_src_len, zlib);
  if (call.total_segs > grid) violations++;
  for (uint64_t w = 0; w < grid; w++) {
    if (dpacked_wg_idle(call, w)) continue;
    busy++;
    const DpackedWork k = dpacked_work(seg_base, n, (uint32_t)w);
    const uint64_t len = staged[k.stream].out_len;
    const uint64_t d0 = verdicts[k.stream].dst_off;
    if (k.seg >= dpacked_segs(len)) { violations++; continue; }
    const DpackedSpan sp = dpacked_span(len, k.seg, (uint64_t)base_mis + d0);
    const uint64_t s0 = inner[k.stream].dst_off + sp.lo;
    const uint64_t d = d0 + sp.lo;
    auto put = [&](uint64_t at, uint8_t b) {
      dst[at] = b;
      if (written[at]) twice++;
      if (written[at] < 255) written[at]++;
      owner[at] = (uint32_t)w + 1;
    };
    for (uint32_t t = 0; t < DPACKED_COPY_THREADS; t++) {
      const uint32_t rounds = dpacked_rounds(sp.units);
      for (uint32_t r = 0; r < rounds; r++) {
        uint8_t v[DPACKED_IN_FLIGHT][DPACKED_UNIT];
        for (uint32_t j = 0; j < DPACKED_IN_FLIGHT; j++) {
          const uint32_t u = dpacked_unit_of(r, j, t);
          if (u < sp.units)
            for (uint32_t b = 0; b < DPACKED_UNIT; b++) v[j][b] = staging[s0 + dpacked_unit_at(sp, u) + b];
        }
        for (uint32_t j = 0; j < DPACKED_IN_FLIGHT; j++) {
          const uint32_t u = dpacked_unit_of(r, j, t);
          if (u >= sp.units) continue;
          const uint64_t at = d + dpacked_unit_at(sp, u);
          if ((base_mis + at) % DPACKED_UNIT != 0) misaligned++;
          vec_stores++;
          for (uint32_t b = 0; b < DPACKED_UNIT; b++) put(at + b, v[j][b]);
        }
      }
      if (t < sp.head) { put(d + t, staging[s0 + t]); byte_stores++; }
      if (t < sp.tail) { put(d + dpacked_tail_at(sp) + t, staging[s0 + dpacked_tail_at(sp) + t]); byte_stores++; }
    }
  }

  // ---- dpacked_close_kernel
  for (uint64_t i = 0; i < n; i++) results[i] = dpacked_close(verdicts[i], stage_status[i], staged[i], crc_op);

  stats[0] = violations; stats[1] = misaligned; stats[2] = twice; stats[3] = call.total_segs; stats[4] = call.bad; stats[5] = reached;
  stats[6] = grid; stats[7] = slots_end; stats[8] = vec_stores; stats[9] = byte_stores; stats[10] = tiles; stats[11] = busy;
  return violations;
}

}  // extern "C"
