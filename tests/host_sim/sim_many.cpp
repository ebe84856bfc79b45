// sim_many.cpp -- zipc_amd/csrc/host_pipeline.h's plan of a many-stream call (many_slot, many_chunks, plan_many) as plain
// numbers, for tests/test_many_plan.py to hold against rows written out by hand.  TEST TOOLING ONLY: the very header
// many.hip compiles; nothing here decides anything.
#include "../../zipc_amd/csrc/host_pipeline.h"

using namespace zd_host;

extern "C" {

uint64_t sim_many_slot(uint64_t len) { return many_slot(len); }
uint64_t sim_many_chunks(long setting, uint64_t staged_bytes) { return many_chunks(setting, staged_bytes); }

// limit, mid_cap, expect_crc32: null, or n entries.  scalars[11]: src_arena_end, dst_arena_end, max_src, max_cap, max_mid,
// K, n_max, total_max, mid_arena, mid_total_max, ahead.  src_off, dst_off: n entries; cut: K + 1 (room for 65).  recode
// (op 2): rdescs 9 per stream (a zipc_hip_recode_desc's fields in order), inflate_descs 7 per stream (a stream
// descriptor's).  Returns K.
uint64_t sim_many_plan(int op, uint64_t n, const uint64_t *src_len, const uint64_t *dst_cap, const uint64_t *limit, const uint64_t *mid_cap,
                       const uint32_t *expect_crc32, long chunks, long chunk_min, uint64_t *scalars, uint64_t *src_off, uint64_t *dst_off,
                       uint64_t *cut, uint64_t *rdescs, uint64_t *inflate_descs) {
  static_assert(sizeof(size_t) == sizeof(uint64_t), "the arrays are handed on as they are");
  const ManyPlan p = plan_many((ManyOp)op, n, (const size_t *)src_len, (const size_t *)dst_cap, (const size_t *)limit, (const size_t *)mid_cap,
                               expect_crc32, chunks, chunk_min);
  const uint64_t s[11] = {p.src_arena_end, p.dst_arena_end, p.max_src, p.max_cap, p.max_mid, p.K(), p.n_max, p.total_max, p.mid_arena,
                          p.mid_total_max, p.ahead};
  for (int k = 0; k < 11; k++) scalars[k] = s[k];
  for (size_t i = 0; i < n; i++) { src_off[i] = p.descs[i].src_off; dst_off[i] = p.descs[i].dst_off; }
  for (size_t g = 0; g <= p.K(); g++) cut[g] = p.cut[g];
  for (size_t i = 0; i < p.rdescs.size(); i++) {
    const zd::RecodeDesc &r = p.rdescs[i];
    const zd::StreamDesc &d = p.inflate_descs[i];
    const uint64_t a[9] = {r.src_off, r.src_len, r.mid_off, r.mid_cap, r.dst_off, r.dst_cap, r.limit, r.flags, r.expect_crc32};
    const uint64_t b[7] = {d.src_off, d.src_len, d.dst_off, d.dst_cap, d.limit, d.flags, d.reserved};
    for (int k = 0; k < 9; k++) rdescs[9 * i + k] = a[k];
    for (int k = 0; k < 7; k++) inflate_descs[7 * i + k] = b[k];
  }
  return p.K();
}

}  // extern "C"
