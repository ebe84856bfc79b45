// sim_prefix.cpp -- the prefix form of the one inflate decoder (zipc_hip_inflate_prefix_batch: inflate_lane.h's plain step with
// `prefix` set, inflate_span.h, the rule of inflate_prefix.h) compiled with g++ and driven on the CPU, for
// tests/test_inflate_prefix_rules.py: the first dst_cap bytes of a stream, with real stores into the room it is given.  The
// driver is sim_size's (tests/size_sim/sim_size.cpp) with the bytes put back: the plain step with its writer and its queue
// of deferred copies, the span decoder on the emulated wave (wave_emu.h) in its IM_REAL form, and the services in the
// kernel's order -- the queued copies filled, then the match or the stored block that was asked for.  A symbol that was
// cut (status ST_PREFIX_CUT) is never served in line: it waits for the services like in inflate.hip's PREFIX wave.
// wave_copy_match and wave_copy have no host model: the part of a cut match that fits is copied serially from where
// inflate_prefix.h says it starts, a stored block's by memcpy; tests/test_gpu_inflate_prefix.py is those routines' coverage.
// Also zlib_container.h's close rule of zipc_hip_zlib_decompress_prefix_batch.  Test tooling only.
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

// the span step on the emulated wave: every lane runs span_decode<IM_REAL> on its own copy of the (wave-uniform) state
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
  c.ret[lane] = span_decode<IM_REAL>(c.d[lane], *c.L, c.src, c.dst, idx, nullptr, nullptr, 0xFFFFFFFFu, nullptr, lane);
}
extern "C" { uint64_t sim_prefix_spans[2]; }  // spans that ran, output bytes they stored
static int span_model(InflateLane &d, const LaneLds &L, const uint8_t *src, uint8_t *dst, bool descending) {
  static wv::Emu emu;
  static SpanCall c;
  emu.descending = descending;
  for (int i = 0; i < 64; i++) c.d[i] = d;
  c.L = &L; c.src = src; c.dst = dst;
  emu.run(span_lane, &c);
  for (int i = 1; i < 64; i++) {
    if (c.ret[i] != c.ret[0] || memcmp(&c.d[i], &c.d[0], sizeof(InflateLane)) != 0) {
      fprintf(stderr, "sim_prefix: lane %d disagrees with lane 0\n", i);
      abort();
    }
  }
  if (c.ret[0] != SPAN_NONE) {
    sim_prefix_spans[0]++;
    sim_prefix_spans[1] += c.d[0].out_pos - d.out_pos;
  }
  d = c.d[0];
  return c.ret[0];
}

// span: 0 the plain step alone, 1 the span decoder with lanes resumed in ascending order, 2 in descending order
// budget: decode turns between two refills of the input ring (the kernel's round)
// dst: the stream's room, dst_cap bytes -- nothing is stored or loaded outside it
// out: {status, ended, out_len}, the record of inflate_prefix.h
extern "C" void sim_prefix(const uint8_t *src, uint64_t src_len, uint8_t *dst, uint64_t dst_cap, int has_limit, uint64_t limit,
                           uint32_t flags_extra, int span, int budget, uint64_t *out) {
  static __attribute__((aligned(16))) uint8_t block[LDS_BYTES_PER_LANE];
  LaneLds L;
  L.at(block);
  StreamDesc s;
  memset(&s, 0, sizeof s);
  s.src_len = src_len; s.dst_off = 0; s.dst_cap = dst_cap;
  s.limit = limit; s.flags = (has_limit ? STREAM_HAS_LIMIT : 0) | flags_extra;
  out[0] = ST_INVALID_ARG; out[1] = 0; out[2] = 0;
  if ((s.flags & ~STREAM_HAS_LIMIT) != 0) return;  // (inflate.hip inflate_skips_stream, for a caller's descriptor)
  Arenas A;
  A.src = src; A.dst = dst;
  InflateLane d;
  lane_init(d, s);
  refill(d, L, src);
  for (;;) {
    for (int turn = 0; turn < budget; turn++) {
      if (d.phase == PH_HEADER || d.phase == PH_HDR_LENGTHS || d.phase == PH_HDR_CODELEN) {
        if (!lane_header_step(d, L, src, true)) break;
        if (d.phase == PH_TABLES) lane_finish_tables(d, L);
        if (d.phase == PH_SYMBOLS && !d.fixed_lazy)
          for (int lane = 0; lane < 64; lane++) build_wide_tables(d, L, lane);
      } else if (d.phase == PH_TABLES) {
        lane_finish_tables(d, L);
        if (d.phase == PH_SYMBOLS)
          for (int lane = 0; lane < 64; lane++) build_wide_tables(d, L, lane);
      } else if (d.phase == PH_SYMBOLS && d.fixed_lazy) {
        const int rr = lane_one_symbol_fixed(d, L, A, true, true, true);
        if (rr == SYM_EOB) { d.fixed_lazy = 0; lane_end_of_block(d, false); }
        else if (rr == SYM_STOP) {
          if (d.phase == PH_REQ_MATCH && d.q_count == 0 && d.status == ST_OK) {  // as inflate.hip: copied on the spot
            lane_copy_match(dst, d.out_pos, d.req_dist, d.req_len, d.hard_cap);
            lane_after_match(d);
          } else break;
        }
        if (d.phase == PH_SYMBOLS && d.fixed_lazy && --d.fixed_lazy == 0) d.phase = PH_TABLES;
      } else if (d.phase == PH_SYMBOLS) {
        if (span && !d.span_off && d.in_word >= d.span_retry_word) {
          if (d.q_count) break;  // queued copies first: the span reads its match sources from memory
          const uint32_t out_before = d.out_pos;
          const int sr = span_model(d, L, src, dst, span == 2);
          if (sr != SPAN_NONE) {
            span_after(d, sr, d.out_pos != out_before);
            break;
          }
          d.span_off = 1;
        }
        const int rr = lane_one_symbol(d, L, A, true, true, true);
        if (rr == SYM_EOB) lane_end_of_block(d, false);
        else if (rr == SYM_STOP) {
          if (d.phase == PH_REQ_MATCH && d.q_count == 0 && d.status == ST_OK) {
            lane_copy_match(dst, d.out_pos, d.req_dist, d.req_len, d.hard_cap);
            lane_after_match(d);
          } else break;
        }
      } else {
        break;
      }
    }
    // services, in the kernel's order: the queued copies first, whatever asked for the service
    for (uint32_t k = 0; k < d.q_count; k++) {
      DeferredCopy c;
      deferred_load(c, dst, d.hole_min, L.queue((int)k));
      deferred_store(c, dst);
    }
    d.q_count = 0;
    d.hole_min = 0xFFFFFFFFu;
    if (d.phase == PH_REQ_MATCH) {
      if (d.status == ST_PREFIX_CUT)
        for (uint32_t i = 0; i < d.req_len; i++) dst[d.out_pos + i] = dst[d.req_src + i];  // (serially: the periodic copy, cut short)
      else lane_copy_match(dst, d.out_pos, d.req_dist, d.req_len, d.hard_cap);
      lane_after_match(d);
    } else if (d.phase == PH_REQ_COPY) {
      memcpy(dst + d.out_pos, src + d.req_src, d.req_len);
      lane_after_copy(d, false);
    }
    if (d.status == ST_PREFIX_CUT) d.phase = PH_DONE;
    if (d.phase == PH_DONE) break;
    refill(d, L, src);
  }
  const PrefixResult r = prefix_result(d.status, d.out_pos, d.cap_min);
  out[0] = r.status; out[1] = r.ended; out[2] = r.out_len;
}

// zlib_container.h zlib_close_prefix: out = {status, ended, out_len}
extern "C" void sim_zlib_close_prefix(unsigned pre, unsigned expect, unsigned adler, unsigned status, unsigned ended, unsigned long long out_len,
                                      unsigned long long *out) {
  const PrefixResult r = zlib_close_prefix(pre, expect, adler, PrefixResult{status, ended, out_len});
  out[0] = r.status; out[1] = r.ended; out[2] = r.out_len;
}
