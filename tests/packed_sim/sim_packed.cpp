// sim_packed.cpp -- host model of the packed decode forms' layout and close (zipc_hip_inflate_packed_batch): the two kernels
// of zipc_amd/csrc/packed.hip as plain loops.
//
// Everything those kernels decide -- which streams take room, the rooms, the scan's halves and their join, the base a
// tile begins at, the verdicts, the descriptors inflate runs with, `need`, the results -- is zipc_amd/csrc/packed_layout.h,
// compiled here with g++.  What the model adds is the kernel's shape: tiles of PACKED_TILE streams, waves of PACKED_WAVE
// lanes with an inclusive scan each, the waves' totals summed behind them, a base carried from tile to tile.  A stub stands
// in for the codec: the caller says what inflate would report of every stream IF it reaches it, and a "no stream"
// descriptor gets what inflate says of one (ST_CORRUPTED, no bytes).  Every array is reached through a wrapper that checks
// the index before it is used: an index that leaves is counted, never followed.  tests/test_packed_rules.py loads this as a
// library.
#include <stdint.h>

#include <type_traits>
#include <vector>

#ifndef PACKED_HEADER
#define PACKED_HEADER "../../zipc_amd/csrc/packed_layout.h"
#endif
#include PACKED_HEADER

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
};

}  // namespace sim

extern "C" {

uint32_t sim_packed_tile() { return PACKED_TILE; }
uint32_t sim_packed_wave() { return PACKED_WAVE; }
uint32_t sim_packed_call_status(int dst_null, uint64_t dst_arena_len, uint64_t n, uint64_t max_out_len, uint64_t align, int crc_op) {
  return packed_call_status(dst_null != 0, dst_arena_len, n, max_out_len, align, crc_op);
}
int sim_packed_size_form(uint64_t max_out_len) { return packed_size_form(max_out_len); }

// One call over n streams.  descs, sized: the caller's descriptors and what the sizing pass said; would_decode: what
// inflate reports of stream i if it reaches it.  Out: verdicts, inner (the descriptors inflate ran with), results, need[0].
// stats: [0] violations, [1] tiles, [2] streams that reached inflate.  Returns the violations.
uint64_t sim_packed_run(const StreamDesc *descs_, const StreamResult *sized_, const StreamResult *would_decode_, uint32_t n, uint64_t max_out_len,
                        uint64_t align, uint64_t dst_arena_len, PackedVerdict *verdicts_, StreamDesc *inner_, PackedResult *results_,
                        uint64_t *need_out, uint64_t *stats) {
  uint64_t violations = 0, tiles = 0, reached = 0;
  sim::Checked<const StreamDesc> descs(descs_, n, &violations);
  sim::Checked<const StreamResult> sized(sized_, n, &violations), would_decode(would_decode_, n, &violations);
  sim::Checked<PackedVerdict> verdicts(verdicts_, n, &violations);
  sim::Checked<StreamDesc> inner(inner_, n, &violations);
  sim::Checked<PackedResult> results(results_, n, &violations);
  constexpr uint32_t WAVES = PACKED_TILE / PACKED_WAVE;

  // ---- packed_layout_kernel
  uint64_t base = 0, need = 0;
  std::vector<StreamResult> s(PACKED_TILE);
  std::vector<uint64_t> room(PACKED_TILE), incl(PACKED_TILE), off(PACKED_TILE);
  for (uint64_t t0 = 0; t0 < n; t0 += PACKED_TILE) {
    tiles++;
    uint64_t wave_total[WAVES], wave_end[WAVES];
    for (uint32_t t = 0; t < PACKED_TILE; t++) {
      const uint64_t i = t0 + t;
      s[t] = StreamResult{ST_CORRUPTED, 0, 0};  // (past the end: no room)
      if (i < n) s[t] = sized[i];
      room[t] = packed_room(s[t], max_out_len, align);
    }
    for (uint32_t w = 0; w < WAVES; w++) {  // a wave's two inclusive scans
      uint32_t lo = 0, hi = 0;
      for (uint32_t lane = 0; lane < PACKED_WAVE; lane++) {
        const uint32_t t = w * PACKED_WAVE + lane;
        lo += packed_scan_lo(room[t]);
        hi += packed_scan_hi(room[t]);
        incl[t] = packed_scan_join(lo, hi);
      }
      wave_total[w] = incl[w * PACKED_WAVE + PACKED_WAVE - 1];
    }
    uint64_t tile_total = 0;
    for (uint32_t w = 0; w < WAVES; w++) tile_total = packed_add(tile_total, wave_total[w]);
    for (uint32_t w = 0; w < WAVES; w++) {
      uint64_t before = 0;
      for (uint32_t k = 0; k < w; k++) before = packed_add(before, wave_total[k]);
      uint64_t end = 0;
      for (uint32_t lane = 0; lane < PACKED_WAVE; lane++) {
        const uint32_t t = w * PACKED_WAVE + lane;
        const uint64_t i = t0 + t;
        off[t] = packed_add(packed_add(base, before), incl[t] - room[t]);
        const PackedVerdict v = packed_verdict(s[t], off[t], max_out_len, dst_arena_len);
        if (i < n) {
          verdicts[i] = v;
          inner[i] = packed_inner_desc(descs[i], v, s[t].out_len);
        }
        end = packed_need_join(end, packed_end(v.roomed != 0, off[t], s[t].out_len));
      }
      wave_end[w] = end;
    }
    for (uint32_t w = 0; w < WAVES; w++) need = packed_need_join(need, wave_end[w]);
    base = packed_tile_base(base, tile_total);
  }
  if (need_out) need_out[0] = need;

  // ---- inflate (the stub), then packed_close_kernel
  for (uint64_t i = 0; i < n; i++) {
    const StreamDesc in = inner[i];
    const bool no_stream = in.src_len == 0 && in.dst_cap == 0 && in.flags == 0;
    StreamResult d = StreamResult{ST_CORRUPTED, 0, 0};
    if (!no_stream) {
      d = would_decode[i];
      reached++;
      if (in.dst_off + in.dst_cap > dst_arena_len || in.dst_off + in.dst_cap < in.dst_off) violations++;  // inflate may write [dst_off, dst_off + dst_cap)
    }
    results[i] = packed_close(verdicts[i], d);
  }
  stats[0] = violations;
  stats[1] = tiles;
  stats[2] = reached;
  return violations;
}

}  // extern "C"
