// recode_rules.h -- what joins inflate, the CRC-32 check and deflate when a batch is recoded on the device
// (zipc_hip_recode_batch / zipc_hip_recode_many): free of HIP.
//
// A recode is inflate_and_crc_32, Crc_32.check and deflate of one member (test/test.ml:58-74 redeflate_recode,
// test/zipc_tool.ml:437-545), and the decompressed bytes are the one thing no caller of it wants back.  The codec's
// kernels are not touched: three small steps stand before, between and behind them, and they are pure functions of
// plain numbers, so the same code is compiled three times:
//   * into recode.hip's kernels (a lane per stream opens, links and closes on the device; nothing is read back);
//   * into the host form's plan (host_pipeline.h plan_many: zipc_hip_recode_many hands inflate the descriptors it already knows);
//   * into tests/recode_sim/sim_recode.cpp with g++, where tests/test_recode_rules.py checks a table of every rule.
#pragma once

#include "zlib_container.h"  // (ST_CHECKSUM: the statuses the codec itself never gives)

namespace zd {

// include/zipc_hip.h: zipc_hip_recode_desc / zipc_hip_recode_result
constexpr uint32_t STREAM_EXPECT_CRC32 = 2u;
struct RecodeDesc {
  uint64_t src_off, src_len, mid_off, mid_cap, dst_off, dst_cap, limit;
  uint32_t flags, expect_crc32;
};
struct RecodeResult {
  uint32_t status, checksum;
  uint64_t out_len, mid_len;
  uint32_t stage, reserved;
};
enum : uint32_t { RECODE_STAGE_NONE = 0, RECODE_STAGE_INFLATE = 1, RECODE_STAGE_CRC = 2, RECODE_STAGE_DEFLATE = 3 };

// What is known of a stream between the steps (the context's scratch holds one per stream): the status and stage it
// stopped at, or ST_OK / RECODE_STAGE_NONE while it goes on; from the link on, the CRC-32 and the length of what it
// inflated to.
struct RecodeVerdict {
  uint32_t status, stage, checksum, reserved;
  uint64_t mid_len;
};

// A stream the codec is not to touch: nothing to read, no room to write (zlib.hip zlib_no_stream).  Inflate reports a
// corrupted stream for it, deflate a destination too small, neither stores a byte; the verdict stands in their place.
ZD_HD StreamDesc recode_no_stream(uint64_t src_off, uint64_t dst_off) {
  StreamDesc in;
  in.src_off = src_off; in.src_len = 0; in.dst_off = dst_off; in.dst_cap = 0; in.limit = 0;
  in.flags = 0; in.reserved = 0;
  return in;
}

// ---- open: the descriptor inflate runs with -- the stream into its room in the middle arena, ?decompressed_size as
// the caller gave it -- or the refusal: a flag bit nobody knows, room beyond what the call declared (the CRC-32 pass and
// deflate's grids are sized by max_mid_cap).
ZD_HD RecodeVerdict recode_open(const RecodeDesc &rd, uint64_t max_mid_cap, StreamDesc *inflate_desc) {
  RecodeVerdict v;
  v.status = ST_OK; v.stage = RECODE_STAGE_NONE; v.checksum = 0; v.reserved = 0; v.mid_len = 0;
  if ((rd.flags & ~(STREAM_HAS_LIMIT | STREAM_EXPECT_CRC32)) != 0) v.status = ST_INVALID_ARG;
  else if (rd.mid_cap > max_mid_cap) v.status = ST_INVALID_ARG;
  if (v.status != ST_OK) { *inflate_desc = recode_no_stream(rd.src_off, rd.mid_off); return v; }
  StreamDesc in;
  in.src_off = rd.src_off; in.src_len = rd.src_len; in.dst_off = rd.mid_off; in.dst_cap = rd.mid_cap; in.limit = rd.limit;
  in.flags = rd.flags & STREAM_HAS_LIMIT; in.reserved = 0;
  *inflate_desc = in;
  return v;
}

// ---- link: inflate and its CRC-32 pass are through.  A stream that was refused keeps its refusal; one that did not
// inflate stops with inflate's status; one whose CRC-32 is not the expected one stops with the value found
// (Crc_32.check, zd.ml:103-107).  Every other one goes on: deflate reads what inflate wrote, as long as inflate said it
// is, and writes the caller's destination slot.
ZD_HD RecodeVerdict recode_link(const RecodeDesc &rd, RecodeVerdict opened, StreamResult inflated, StreamDesc *deflate_desc) {
  RecodeVerdict v = opened;
  if (v.status == ST_OK) {
    if (inflated.status != ST_OK) {
      v.status = inflated.status; v.stage = RECODE_STAGE_INFLATE;
    } else {
      v.checksum = inflated.checksum; v.mid_len = inflated.out_len;
      if ((rd.flags & STREAM_EXPECT_CRC32) != 0 && inflated.checksum != rd.expect_crc32) { v.status = ST_CHECKSUM; v.stage = RECODE_STAGE_CRC; }
    }
  }
  if (v.status != ST_OK) { *deflate_desc = recode_no_stream(rd.mid_off, rd.dst_off); return v; }
  StreamDesc in;
  in.src_off = rd.mid_off; in.src_len = v.mid_len; in.dst_off = rd.dst_off; in.dst_cap = rd.dst_cap; in.limit = 0;
  in.flags = 0; in.reserved = 0;
  *deflate_desc = in;
  return v;
}

// ---- close: the public result.  Deflate's word counts only for a stream that got as far as deflate (the others ran as
// "no stream"): its status at stage 3 -- a destination too small, or the batch-wide refusal of the declared sizes --
// or the recoded length.
ZD_HD RecodeResult recode_close(RecodeVerdict v, StreamResult deflated) {
  RecodeResult r;
  r.status = v.status; r.checksum = v.checksum; r.out_len = 0; r.mid_len = v.mid_len; r.stage = v.stage; r.reserved = 0;
  if (v.status == ST_OK) {
    if (deflated.status != ST_OK) { r.status = deflated.status; r.stage = RECODE_STAGE_DEFLATE; }
    else r.out_len = deflated.out_len;
  }
  return r;
}
// ... and as the many-stream pipeline reads it (status, checksum, length of what is to come back)
ZD_HD StreamResult recode_plain_result(const RecodeResult &r) {
  StreamResult s;
  s.status = r.status; s.checksum = r.checksum; s.out_len = r.out_len;
  return s;
}

}  // namespace zd
