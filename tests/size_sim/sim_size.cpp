// sim_size.cpp -- the sizing mode of the one inflate decoder (IM_SIZE: zipc_amd/csrc/inflate_lane.h, inflate_span.h)
// compiled with g++ and driven on the CPU, for tests/test_inflate_size_sim.py: a stream's status and decompressed size
// from a walk over the whole stream that stores nothing.  The driver is sim_inflate_token's (tests/host_sim/sim_inflate.cpp)
// with every byte left out: the plain step with no writer and nothing queued, the span decoder on the emulated wave
// (wave_emu.h) in its IM_SIZE form, a match or a stored block handed to the wave moves the position and copies nothing.
// Also zlib_container.h's close rule of zipc_hip_zlib_size_batch.  Test tooling only.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../zipc_amd/csrc/inflate_lane.h"
#include "../../zipc_amd/csrc/inflate_span.h"
#include "../../zipc_amd/csrc/zlib_container.h"

using namespace zd;

// ring refill as inflate.hip does it (one stream): words past the end are zero
static void refill(InflateLane &d, const LaneLds &L, const uint8_t *src) {
  if (d.phase == PH_DONE) return;
  const uint32_t lim = d.in_word + (uint32_t)RING_WORDS;
  uint32_t end = d.ring_wr + 64u < lim ? d.ring_wr + 64u : lim;
  for (uint32_t w = d.ring_wr; w < end; w++) {
    uint32_t v = 0;
    for (uint32_t b = 0; b < 4 && (uint64_t)w * 4 + b < d.src_len; b++) v |= (uint32_t)src[(uint64_t)w * 4 + b] << (8 * b);
    L.ring_put(w, v);
  }
  d.ring_wr = end;
}

// the span step on the emulated wave: every lane runs span_decode<IM_SIZE> on its own copy of the (wave-uniform) state
struct SpanCall {
  InflateLane d[64];
  int ret[64];
  const LaneLds *L;
  const uint8_t *src;
  uint8_t *dst;
};
static void span_lane(int lane, void *arg) {
  SpanCall &c = *(SpanCall *)arg;
  static uint16_t idx[SPAN_IDX_ENTRIES];  // the kernel's per-stream slot of global scratch
  c.ret[lane] = span_decode<IM_SIZE>(c.d[lane], *c.L, c.src, c.dst, idx, nullptr, nullptr, 0xFFFFFFFFu, nullptr, lane);
}
extern "C" { uint64_t sim_size_spans[2]; }  // spans that ran, output bytes they counted
static int span_model(InflateLane &d, const LaneLds &L, const uint8_t *src, uint8_t *dst, bool descending) {
  static wv::Emu emu;
  static SpanCall c;
  emu.descending = descending;
  for (int i = 0; i < 64; i++) c.d[i] = d;
  c.L = &L; c.src = src; c.dst = dst;
  emu.run(span_lane, &c);
  for (int i = 1; i < 64; i++) {
    if (c.ret[i] != c.ret[0] || memcmp(&c.d[i], &c.d[0], sizeof(InflateLane)) != 0) {
      fprintf(stderr, "sim_size: lane %d disagrees with lane 0\n", i);
      abort();
    }
  }
  if (c.ret[0] != SPAN_NONE) {
    sim_size_spans[0]++;
    sim_size_spans[1] += c.d[0].out_pos - d.out_pos;
  }
  d = c.d[0];
  return c.ret[0];
}

// span: 0 the plain step alone, 1 the span decoder with lanes resumed in ascending order, 2 in descending order
// budget: decode turns between two refills of the input ring (the kernel's round)
// dst: the sim's "destination arena" -- nothing may be stored there; dst_off / dst_cap: the descriptor's, to be ignored
extern "C" int sim_size(const uint8_t *src, uint64_t src_len, uint8_t *dst, uint64_t dst_off, uint64_t dst_cap, int has_limit,
                        uint64_t limit, uint32_t flags_extra, int span, int budget, uint64_t *out_len) {
  static __attribute__((aligned(16))) uint8_t block[LDS_BYTES_PER_LANE];
  LaneLds L;
  L.at(block);
  StreamDesc s;
  memset(&s, 0, sizeof s);
  s.src_len = src_len; s.dst_off = dst_off; s.dst_cap = dst_cap;
  s.limit = limit; s.flags = (has_limit ? STREAM_HAS_LIMIT : 0) | flags_extra;
  *out_len = 0;
  if ((s.flags & ~STREAM_HAS_LIMIT) != 0) return (int)ST_INVALID_ARG;  // (inflate.hip inflate_skips_stream, for a caller's descriptor)
  Arenas A;
  A.src = src; A.dst = dst;
  InflateLane d;
  lane_init_size(d, s);
  refill(d, L, src);
  for (;;) {
    for (int turn = 0; turn < budget; turn++) {
      if (d.phase == PH_HEADER || d.phase == PH_HDR_LENGTHS || d.phase == PH_HDR_CODELEN) {
        if (!lane_header_step(d, L, src)) break;
        if (d.phase == PH_TABLES) lane_finish_tables(d, L);
        if (d.phase == PH_SYMBOLS && !d.fixed_lazy)
          for (int lane = 0; lane < 64; lane++) build_wide_tables(d, L, lane);
      } else if (d.phase == PH_TABLES) {
        lane_finish_tables(d, L);
        if (d.phase == PH_SYMBOLS)
          for (int lane = 0; lane < 64; lane++) build_wide_tables(d, L, lane);
      } else if (d.phase == PH_SYMBOLS && d.fixed_lazy) {
        const int rr = lane_one_symbol_fixed(d, L, A, false, false);
        if (rr == SYM_EOB) { d.fixed_lazy = 0; lane_end_of_block(d, false); }
        else if (rr == SYM_STOP) {
          if (d.phase != PH_REQ_MATCH) break;
          lane_after_match(d);
        }
        if (d.phase == PH_SYMBOLS && d.fixed_lazy && --d.fixed_lazy == 0) d.phase = PH_TABLES;
      } else if (d.phase == PH_SYMBOLS) {
        if (span && !d.span_off && d.in_word >= d.span_retry_word) {
          const uint32_t out_before = d.out_pos;
          const int sr = span_model(d, L, src, dst, span == 2);
          if (sr != SPAN_NONE) {
            span_after(d, sr, d.out_pos != out_before);
            break;
          }
          d.span_off = 1;
        }
        const int rr = lane_one_symbol(d, L, A, false, false);
        if (rr == SYM_EOB) lane_end_of_block(d, false);
        else if (rr == SYM_STOP) {
          if (d.phase != PH_REQ_MATCH) break;
          lane_after_match(d);
        }
      } else {
        break;
      }
    }
    if (d.phase == PH_REQ_COPY) lane_after_copy(d, false);
    if (d.phase == PH_DONE) break;
    refill(d, L, src);
  }
  *out_len = d.status == ST_OK ? d.out_pos : 0;
  return (int)d.status;
}

// zlib_container.h zlib_close_size: out = {status, checksum, out_len}
extern "C" void sim_zlib_close_size(unsigned pre, unsigned status, unsigned checksum, unsigned long long out_len, unsigned long long *out) {
  const StreamResult r = zlib_close_size(pre, StreamResult{status, checksum, out_len});
  out[0] = r.status; out[1] = r.checksum; out[2] = r.out_len;
}
extern "C" unsigned sim_zlib_open_status(unsigned long long len, unsigned cmf, unsigned flg) { return zlib_open_status(len, cmf, flg); }
