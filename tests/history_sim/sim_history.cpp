// sim_history.cpp -- the history forms of the one inflate decoder (zipc_hip_inflate_history_batch, _prefix_history_batch,
// _size_history_batch: inflate_lane.h's plain step, inflate_span.h, started through inflate_history.h) compiled with g++ and
// driven on the CPU, for tests/test_inflate_history_rules.py.  The driver is sim_prefix's (tests/prefix_sim/sim_prefix.cpp)
// with the kernels' start and result store around it: the record's verdict, the descriptor's flags, lane_init on the
// caller's values, history_start, the wave's loop, and the unbias of inflate_history.h.  Three modes as in inflate.hip:
// the all-or-nothing form with real stores (and RFC 1950's Adler-32 of the stream's own output, block by block from
// blk_out_start as the wave sums it), the prefix form, and the sizing form, which is handed no destination at all.
// Also zlib_container.h's open, seed and close rules of the dictionary forms.  Test tooling only.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../zipc_amd/csrc/inflate_history.h"
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

// the span step on the emulated wave: every lane runs span_decode on its own copy of the (wave-uniform) state
struct SpanCall {
  InflateLane d[64];
  int ret[64];
  const LaneLds *L;
  const uint8_t *src;
  uint8_t *dst;
  bool size;
};
static void span_lane(int lane, void *arg) {
  SpanCall &c = *(SpanCall *)arg;
  static uint16_t idx[SPAN_IDX_ENTRIES];  // the kernel's per-stream slot of global scratch
  c.ret[lane] = c.size ? span_decode<IM_SIZE>(c.d[lane], *c.L, c.src, c.dst, idx, nullptr, nullptr, 0xFFFFFFFFu, nullptr, lane)
                       : span_decode<IM_REAL>(c.d[lane], *c.L, c.src, c.dst, idx, nullptr, nullptr, 0xFFFFFFFFu, nullptr, lane);
}
extern "C" { uint64_t sim_history_spans[2]; }  // spans that ran, output bytes they stored or counted
static int span_model(InflateLane &d, const LaneLds &L, const uint8_t *src, uint8_t *dst, bool size, bool descending) {
  static wv::Emu emu;
  static SpanCall c;
  emu.descending = descending;
  for (int i = 0; i < 64; i++) c.d[i] = d;
  c.L = &L; c.src = src; c.dst = dst; c.size = size;
  emu.run(span_lane, &c);
  for (int i = 1; i < 64; i++) {
    if (c.ret[i] != c.ret[0] || memcmp(&c.d[i], &c.d[0], sizeof(InflateLane)) != 0) {
      fprintf(stderr, "sim_history: lane %d disagrees with lane 0\n", i);
      abort();
    }
  }
  if (c.ret[0] != SPAN_NONE) {
    sim_history_spans[0]++;
    sim_history_spans[1] += c.d[0].out_pos - d.out_pos;
  }
  d = c.d[0];
  return c.ret[0];
}

// RFC 1950's Adler-32 over n more bytes (the wave's wave_adler_update, serially)
static uint32_t adler_rfc_update(uint32_t adler, const uint8_t *p, uint32_t n) {
  uint32_t s1, s2;
  adler_unpack(adler, s1, s2);
  for (uint32_t i = 0; i < n; i++) {
    s1 = (s1 + p[i]) % ADLER_BASE;
    s2 = (s2 + s1) % ADLER_BASE;
  }
  return adler_pack(s1, s2);
}

enum { SIM_REAL = 0, SIM_PREFIX = 1, SIM_SIZE = 2 };

// mode: SIM_REAL / SIM_PREFIX / SIM_SIZE; span: 0 the plain step alone, 1 the span decoder with lanes resumed in ascending
// order, 2 in descending order; budget: decode turns between two refills of the input ring (the kernel's round)
// arena, dst_off: the destination arena and the caller's offset into it (SIM_SIZE: arena is never touched -- pass null);
// hist_len, start_bit: the record; adler: 1 -- the all-or-nothing form sums RFC 1950's Adler-32 of its output
// out: {status, checksum (SIM_PREFIX: ended), out_len}
extern "C" void sim_history(const uint8_t *src, uint64_t src_len, uint32_t hist_len, uint32_t start_bit, uint8_t *arena, uint64_t dst_off,
                            uint64_t dst_cap, int has_limit, uint64_t limit, uint32_t flags_extra, int mode, int adler, int span, int budget,
                            uint64_t *out) {
  static __attribute__((aligned(16))) uint8_t block[LDS_BYTES_PER_LANE];
  LaneLds L;
  L.at(block);
  const bool size = mode == SIM_SIZE, prefix = mode == SIM_PREFIX, crc_adler = mode == SIM_REAL && adler != 0;
  StreamDesc s;
  memset(&s, 0, sizeof s);
  s.src_len = src_len; s.dst_off = dst_off; s.dst_cap = dst_cap;
  s.limit = limit; s.flags = (has_limit ? STREAM_HAS_LIMIT : 0) | flags_extra;
  out[0] = ST_INVALID_ARG; out[1] = 0; out[2] = 0;
  if (history_record_status(hist_len, start_bit, size ? 0 : dst_off, !size) != ST_OK) return;  // (inflate.hip history_skips_stream)
  if ((s.flags & ~STREAM_HAS_LIMIT) != 0) return;                                               // (inflate.hip inflate_skips_stream)
  Arenas A;
  A.src = src; A.dst = arena;
  InflateLane d;
  if (size) lane_init_size(d, s);
  else lane_init(d, s);
  if (d.status == ST_OK) history_start(d, hist_len, start_bit, !size);
  uint8_t *dst = size ? nullptr : arena + d.dst_off;
  const bool writer = !size, may_queue = !size;
  refill(d, L, src);
  for (;;) {
    for (int turn = 0; turn < budget; turn++) {
      if (d.phase == PH_HEADER || d.phase == PH_HDR_LENGTHS || d.phase == PH_HDR_CODELEN) {
        if (!lane_header_step(d, L, src, prefix)) break;
        if (d.phase == PH_TABLES) lane_finish_tables(d, L);
        if (d.phase == PH_SYMBOLS && !d.fixed_lazy)
          for (int lane = 0; lane < 64; lane++) build_wide_tables(d, L, lane);
      } else if (d.phase == PH_TABLES) {
        lane_finish_tables(d, L);
        if (d.phase == PH_SYMBOLS)
          for (int lane = 0; lane < 64; lane++) build_wide_tables(d, L, lane);
      } else if (d.phase == PH_SYMBOLS && d.fixed_lazy) {
        const int rr = lane_one_symbol_fixed(d, L, A, writer, may_queue, prefix);
        if (rr == SYM_EOB) { d.fixed_lazy = 0; lane_end_of_block(d, crc_adler); }
        else if (rr == SYM_STOP) {
          if (d.phase == PH_REQ_MATCH && d.q_count == 0 && d.status == ST_OK) {  // as inflate.hip: copied on the spot
            if (!size) lane_copy_match(dst, d.out_pos, d.req_dist, d.req_len, d.hard_cap);
            lane_after_match(d);
          } else break;
        }
        if (d.phase == PH_SYMBOLS && d.fixed_lazy && --d.fixed_lazy == 0) d.phase = PH_TABLES;
      } else if (d.phase == PH_SYMBOLS) {
        if (span && !d.span_off && d.in_word >= d.span_retry_word) {
          if (d.q_count) break;  // queued copies first: the span reads its match sources from memory
          const uint32_t out_before = d.out_pos;
          const int sr = span_model(d, L, src, dst, size, span == 2);
          if (sr != SPAN_NONE) {
            span_after(d, sr, d.out_pos != out_before);
            break;
          }
          d.span_off = 1;
        }
        const int rr = lane_one_symbol(d, L, A, writer, may_queue, prefix);
        if (rr == SYM_EOB) lane_end_of_block(d, crc_adler);
        else if (rr == SYM_STOP) {
          if (d.phase == PH_REQ_MATCH && d.q_count == 0 && d.status == ST_OK) {
            if (!size) lane_copy_match(dst, d.out_pos, d.req_dist, d.req_len, d.hard_cap);
            lane_after_match(d);
          } else break;
        }
      } else {
        break;
      }
    }
    // services, in the kernel's order: the queued copies first, whatever asked for the service
    for (uint32_t k = 0; !size && k < d.q_count; k++) {
      DeferredCopy c;
      deferred_load(c, dst, d.hole_min, L.queue((int)k));
      deferred_store(c, dst);
    }
    d.q_count = 0;
    d.hole_min = 0xFFFFFFFFu;
    if (d.phase == PH_REQ_MATCH) {
      if (size) {}
      else if (d.status == ST_PREFIX_CUT)
        for (uint32_t i = 0; i < d.req_len; i++) dst[d.out_pos + i] = dst[d.req_src + i];  // (serially: the periodic copy, cut short)
      else lane_copy_match(dst, d.out_pos, d.req_dist, d.req_len, d.hard_cap);
      lane_after_match(d);
    } else if (d.phase == PH_REQ_COPY) {
      if (!size) memcpy(dst + d.out_pos, src + d.req_src, d.req_len);
      lane_after_copy(d, crc_adler);
    }
    if (d.status == ST_PREFIX_CUT) d.phase = PH_DONE;
    if (d.phase == PH_REQ_ADLER) {
      d.adler = adler_rfc_update(d.adler, dst + d.blk_out_start, d.out_pos - d.blk_out_start);
      lane_after_adler(d);
    }
    if (d.phase == PH_DONE) break;
    refill(d, L, src);
  }
  if (prefix) {
    const PrefixResult r = history_prefix_result(d.status, d.out_pos, d.cap_min, hist_len);
    out[0] = r.status; out[1] = r.ended; out[2] = r.out_len;
  } else {
    const StreamResult r = history_result(d.status, crc_adler ? d.adler : 0u, d.out_pos, hist_len);
    out[0] = r.status; out[1] = r.checksum; out[2] = r.out_len;
  }
}

// ---- the dictionary forms' container rules (zlib_container.h), as the open kernel and the launch put them together
// RFC 1950's Adler-32 of the dictionary, whatever flavour the context compares outputs in: by chunks of 5552 bytes with
// zd_common.h's chunk step, the checksum kernels' arithmetic
extern "C" unsigned sim_dict_adler(const uint8_t *dict, unsigned long long len) {
  uint32_t s1 = 1, s2 = 0;
  for (uint64_t at = 0; at < len; at += 5552) {
    const uint32_t n = len - at < 5552 ? (uint32_t)(len - at) : 5552u;
    uint32_t S1 = 0, S2 = 0;
    for (uint32_t i = 0; i < n; i++) { S1 += dict[at + i]; S2 += (n - i) * dict[at + i]; }
    adler_chunk_step(s1, s2, n, S1, S2, true);
  }
  return adler_pack(s1, s2);
}
// the open of one stream -> out = {status, expect (ST_ZLIB_DICT: the DICTID), body_off, body_len, hist_len}
extern "C" void sim_zlib_open_dict(const uint8_t *stream, unsigned long long len, const uint8_t *dict, unsigned long long dict_len,
                                   unsigned long long *out) {
  uint32_t cmf = 0, flg = 0, dictid = 0;
  if (len >= ZLIB_MIN_LEN) { cmf = stream[0]; flg = stream[1]; dictid = zlib_dictid(stream + 2); }
  const ZlibDictOpen o = zlib_open_dict(len, cmf, flg, dictid, dict_len, dict_len ? sim_dict_adler(dict, dict_len) : 0u);
  out[0] = o.status;
  out[1] = o.status == ST_OK ? zlib_expect(stream + len - 4) : o.dictid;
  out[2] = o.body_off; out[3] = o.body_len; out[4] = o.hist_len;
}
extern "C" int sim_zlib_dict_seeds(unsigned pre, unsigned hist_len, unsigned long long dst_off) { return zlib_dict_seeds(pre, hist_len, dst_off) ? 1 : 0; }
// the closes -> out = {status, checksum, out_len}
extern "C" void sim_zlib_close_dict(unsigned pre, unsigned expect, unsigned status, unsigned checksum, unsigned long long out_len, int size,
                                    unsigned long long *out) {
  const StreamResult r = zlib_close_dict(pre, expect, StreamResult{status, checksum, out_len}, size != 0);
  out[0] = r.status; out[1] = r.checksum; out[2] = r.out_len;
}
