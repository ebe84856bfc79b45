// sim_extent.cpp -- the extent forms of the one inflate decoder on the CPU (zipc_hip_inflate_extent_batch and its five
// siblings): inflate_lane.h's plain lane step run serially over one stream, to the ExtentResult that inflate_extent.h and
// zlib_container.h make of what the step ended with -- compiled with g++ for tests/test_inflate_extent_rules.py.  The
// driver is sim_prefix's (tests/prefix_sim/sim_prefix.cpp) without the span decoder and without a cut: the plain step with
// its writer and its queue of deferred copies, and the services in the kernel's order.  The sizing forms run the step as
// inflate_size_kernel does (lane_init_size, no writer, no queue, nothing stored: dst may be null).
// The zlib forms: zlib_open_status and the body's range as zlib.hip's open kernel applies them, then zlib_close_extent.
// The Adler-32 of the output is not this model's subject (tests/test_adler_chain_sim.py): the caller hands it in.
// Nothing is read outside [src, src + src_len) or written outside [dst, dst + dst_cap).  Test tooling only.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../zipc_amd/csrc/inflate_lane.h"
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

// one raw stream at src: the record extent_result makes of the status, `adler` (0 for a form without one), the length and
// the bit the step stands at.  size: the sizing form.  budget: decode turns between two refills of the input ring.
static ExtentResult raw_extent(const uint8_t *src, uint64_t src_len, uint8_t *dst, uint64_t dst_cap, int has_limit, uint64_t limit,
                               uint32_t flags_extra, bool size, uint32_t adler, int budget) {
  static __attribute__((aligned(16))) uint8_t block[LDS_BYTES_PER_LANE];
  LaneLds L;
  L.at(block);
  StreamDesc s;
  memset(&s, 0, sizeof s);
  s.src_len = src_len; s.dst_off = 0; s.dst_cap = dst_cap;
  s.limit = limit; s.flags = (has_limit ? STREAM_HAS_LIMIT : 0) | flags_extra;
  if ((s.flags & ~STREAM_HAS_LIMIT) != 0) return extent_result(ST_INVALID_ARG, 0, 0, 0);  // (inflate.hip inflate_skips_stream)
  Arenas A;
  A.src = src; A.dst = size ? nullptr : dst;
  InflateLane d;
  if (size) lane_init_size(d, s);
  else lane_init(d, s);
  const bool writer = !size, may_queue = !size;
  refill(d, L, src);
  for (;;) {
    for (int turn = 0; turn < budget; turn++) {
      if (d.phase == PH_HEADER || d.phase == PH_HDR_LENGTHS || d.phase == PH_HDR_CODELEN) {
        if (!lane_header_step(d, L, src)) break;
        if (d.phase == PH_TABLES) lane_finish_tables(d, L);
      } else if (d.phase == PH_TABLES) {
        lane_finish_tables(d, L);
      } else if (d.phase == PH_SYMBOLS && d.fixed_lazy) {
        const int rr = lane_one_symbol_fixed(d, L, A, writer, may_queue);
        if (rr == SYM_EOB) { d.fixed_lazy = 0; lane_end_of_block(d, false); }
        else if (rr == SYM_STOP) {
          if (d.phase == PH_REQ_MATCH && d.q_count == 0) {  // as inflate.hip: copied on the spot
            if (!size) lane_copy_match(dst, d.out_pos, d.req_dist, d.req_len, d.hard_cap);
            lane_after_match(d);
          } else break;
        }
        if (d.phase == PH_SYMBOLS && d.fixed_lazy && --d.fixed_lazy == 0) d.phase = PH_TABLES;
      } else if (d.phase == PH_SYMBOLS) {
        const int rr = lane_one_symbol(d, L, A, writer, may_queue);
        if (rr == SYM_EOB) lane_end_of_block(d, false);
        else if (rr == SYM_STOP) {
          if (d.phase == PH_REQ_MATCH && d.q_count == 0) {
            if (!size) lane_copy_match(dst, d.out_pos, d.req_dist, d.req_len, d.hard_cap);
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
      if (!size) lane_copy_match(dst, d.out_pos, d.req_dist, d.req_len, d.hard_cap);
      lane_after_match(d);
    } else if (d.phase == PH_REQ_COPY) {
      if (!size && d.req_len) memcpy(dst + d.out_pos, src + d.req_src, d.req_len);
      lane_after_copy(d, false);
    }
    if (d.phase == PH_DONE) break;
    refill(d, L, src);
  }
  return extent_result(d.status, adler, d.out_pos, (uint64_t)d.in_word * 32u + d.boff);  // (BlockEnd::end_bit, inflate.hip inflate_wave)
}

// form: 0 raw decode, 1 raw size, 2 zlib decode, 3 zlib size.  adler: the Adler-32 of the bytes the stream inflates to (the
// decode forms report it for an OK stream; 0 for a raw form without a checksum).  out: the five fields of the record.
extern "C" void sim_extent(const uint8_t *src, uint64_t src_len, uint8_t *dst, uint64_t dst_cap, int has_limit, uint64_t limit,
                           uint32_t flags_extra, int form, uint32_t adler, int budget, uint64_t *out) {
  const bool size = (form & 1) != 0, zlib = form >= 2;
  ExtentResult r;
  if (!zlib) {
    r = raw_extent(src, src_len, dst, dst_cap, has_limit, limit, flags_extra, size, size ? 0u : adler, budget);
  } else if (flags_extra != 0) {
    r = extent_result(ST_INVALID_ARG, 0, 0, 0);  // (zlib.hip zlib_open_kernel)
  } else {
    const bool whole = src_len >= ZLIB_MIN_LEN;  // (the reference looks at the length first: nothing is read of a shorter one)
    const uint32_t pre = zlib_open_status(src_len, whole ? src[0] : 0, whole ? src[1] : 0);
    ExtentResult inner = extent_result(ST_CORRUPTED, 0, 0, 0);  // (zlib_no_stream: inflate of nothing)
    if (pre == ST_OK)
      inner = raw_extent(src + zlib_body_off(0), zlib_body_len(src_len), dst, dst_cap, has_limit, limit, 0, size, size ? 0u : adler, budget);
    r = zlib_close_extent(pre, src_len, src, inner, !size);
  }
  out[0] = r.status; out[1] = r.checksum; out[2] = r.out_len; out[3] = r.src_used; out[4] = r.reserved;
}

// inflate_extent.h, as tables
extern "C" unsigned long long sim_extent_bytes(unsigned long long end_bit) { return extent_bytes(end_bit); }
extern "C" void sim_extent_with_crc(unsigned status, unsigned checksum, unsigned long long out_len, unsigned long long src_used,
                                    unsigned pass_status, unsigned crc, unsigned long long *out) {
  const ExtentResult r = extent_with_crc(ExtentResult{status, checksum, out_len, src_used, 0}, pass_status, crc);
  out[0] = r.status; out[1] = r.checksum; out[2] = r.out_len; out[3] = r.src_used; out[4] = r.reserved;
}
extern "C" unsigned long long sim_size_blocks_end_bit(unsigned head_final, unsigned long long head_end, unsigned long long chain_end) {
  return size_blocks_end_bit(head_final, head_end, chain_end);
}
