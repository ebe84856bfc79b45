// audit_main.cpp -- the host model of the packed encode forms (sim_deflate_packed.cpp) as a stand-alone program, meant to be
// built with -fsanitize=address,undefined: the seams of tests/deflate_packed_cases.py restated in their smallest form and a
// few thousand random ragged batches, each run as the launches would run it.  The program aborts when an index leaves its
// array, a vector store is off its boundary, a destination byte is written twice or outside a fitting stream, or a result,
// `need` or a byte of the arena differs from the serial restatement of the rule below.
// tests/test_deflate_packed_rules.py compiles and runs it; it is never loaded into another process.
#include <stdio.h>
#include <stdlib.h>

#include "sim_deflate_packed.cpp"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return rng_state;
}

static uint64_t batches = 0;
static const uint64_t GUARD = 4096;
static const uint8_t POISON = 0xEE;

#define AUDIT_FAIL(...) do { fprintf(stderr, "audit: batch %llu: ", (unsigned long long)batches); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); abort(); } while (0)

static uint64_t plain_bound(uint64_t len, bool zlib) { return len + 6 * (len / 65534 + 1) + 8 + (zlib ? 6 : 0); }

// src_len and what deflate would say of every stream; the call as declared
static void check(const std::vector<uint64_t> &src_len, const std::vector<StreamResult> &would, uint64_t max_src_len, uint64_t total_src_len, bool zlib,
                  int crc_op, uint64_t align, uint64_t arena, uint32_t base_mis) {
  batches++;
  const uint32_t n = (uint32_t)src_len.size();
  std::vector<StreamDesc> descs(n + 1);
  for (uint32_t i = 0; i < n; i++) { descs[i] = StreamDesc{i * 100ull, src_len[i], 0xDEAD, 0xBEEF, 0, i & 1u, 0}; }
  const uint64_t alloc = arena + GUARD;
  std::vector<uint8_t> dst(alloc, POISON), written(alloc, 0);
  std::vector<uint32_t> owner(alloc, 0), stage(n + 1), seg_base(n + 1);
  std::vector<StreamDesc> inner(n + 1);
  std::vector<PackedVerdict> verdicts(n + 1);
  std::vector<PackedResult> results(n + 1);
  uint64_t need = ~0ull, stats[12];
  sim_dpacked_run(descs.data(), would.data(), n, max_src_len, total_src_len, zlib, crc_op, align, arena, base_mis, dst.data(), alloc, written.data(),
                  owner.data(), inner.data(), stage.data(), verdicts.data(), seg_base.data(), results.data(), &need, stats);
  if (stats[0] || stats[1] || stats[2]) AUDIT_FAIL("%llu violations, %llu vector stores off their boundary, %llu bytes written twice",
                                                   (unsigned long long)stats[0], (unsigned long long)stats[1], (unsigned long long)stats[2]);
  // ---- the rule, serially
  uint64_t sum = 0;
  bool bad = false;
  for (uint32_t i = 0; i < n; i++)
    if (src_len[i] <= MAX_STREAM_LEN) { sum += src_len[i]; bad |= src_len[i] > max_src_len; }
  bad |= sum > total_src_len;
  if ((stats[4] != 0) != bad) AUDIT_FAIL("bad-call flag %llu", (unsigned long long)stats[4]);
  std::vector<uint8_t> want_dst(alloc, POISON), want_written(alloc, 0);
  uint64_t off = 0, want_need = 0, slot = 0;
  for (uint32_t i = 0; i < n; i++) {
    PackedResult w{ST_INVALID_ARG, 0, 0, 0, 0};
    if (!bad && src_len[i] <= MAX_STREAM_LEN) {
      if (inner[i].dst_off != slot || inner[i].dst_cap != plain_bound(src_len[i], zlib) || inner[i].src_len != src_len[i])
        AUDIT_FAIL("stream %u: slot {%llu, %llu}, want {%llu, %llu}", i, (unsigned long long)inner[i].dst_off, (unsigned long long)inner[i].dst_cap,
                   (unsigned long long)slot, (unsigned long long)plain_bound(src_len[i], zlib));
      slot += (plain_bound(src_len[i], zlib) + 15) / 16 * 16;
      const StreamResult s = would[i];
      if (s.status != ST_OK) w = PackedResult{s.status, s.checksum, 0, 0, 0};
      else {
        if (off + s.out_len <= arena) {
          w = PackedResult{ST_OK, s.checksum, s.out_len, off, 0};
          for (uint64_t j = 0; j < s.out_len; j++) { want_dst[off + j] = sim::staged_byte(i, j); want_written[off + j] = 1; }
        } else w = PackedResult{ST_DST_TOO_SMALL, crc_op == 1 ? s.checksum : 0u, 0, off, 0};
        want_need = off + s.out_len;
        off += (s.out_len + align - 1) / align * align;
      }
    } else if (inner[i].src_len != 0 || inner[i].dst_cap != 0) AUDIT_FAIL("stream %u reached deflate", i);
    const PackedResult r = results[i];
    if (r.status != w.status || r.checksum != w.checksum || r.out_len != w.out_len || r.dst_off != w.dst_off || r.reserved != 0)
      AUDIT_FAIL("stream %u: got %u %08x %llu @%llu, want %u %08x %llu @%llu", i, r.status, r.checksum, (unsigned long long)r.out_len,
                 (unsigned long long)r.dst_off, w.status, w.checksum, (unsigned long long)w.out_len, (unsigned long long)w.dst_off);
  }
  if (need != want_need) AUDIT_FAIL("need %llu, want %llu", (unsigned long long)need, (unsigned long long)want_need);
  if (want_need > dpacked_arena_bound(n, total_src_len, align, zlib) && !bad) AUDIT_FAIL("need %llu above the bound", (unsigned long long)want_need);
  if (dst != want_dst) AUDIT_FAIL("a byte of the arena or of its guard differs");
  if (written != want_written) AUDIT_FAIL("a byte was written outside a fitting stream, or one of a fitting stream was not");
}

// n streams; how: what the sources and outputs look like
static void make(uint32_t n, int how, bool zlib, std::vector<uint64_t> &src_len, std::vector<StreamResult> &would) {
  src_len.clear();
  would.clear();
  for (uint32_t i = 0; i < n; i++) {
    const uint64_t pick = rnd() % 100;
    uint64_t l = pick < 70 ? rnd() % 200 : pick < 95 ? rnd() % 5000 : rnd() % (3 * DPACKED_SEG_BYTES + 100);
    if (how == 1) l = rnd() % 40;
    if (how == 2 && i == n / 2) l = 5 * DPACKED_SEG_BYTES + rnd() % 1000;
    if (how == 3 && rnd() % 16 == 0) l = MAX_STREAM_LEN + 1 + rnd() % 1000;
    src_len.push_back(l);
    const uint64_t cap = l <= MAX_STREAM_LEN ? plain_bound(l, zlib) : 100;
    const uint64_t kind = rnd() % 20;
    StreamResult s{ST_OK, (uint32_t)rnd(), kind < 10 ? cap - rnd() % 15 : 2 + (zlib ? 6 : 0) + rnd() % (cap - 8)};
    if (kind == 19) s = StreamResult{rnd() % 2 ? (uint32_t)ST_DST_TOO_SMALL : (uint32_t)ST_HIP, (uint32_t)rnd(), 0};
    would.push_back(s);
  }
}

static uint64_t need_of(const std::vector<uint64_t> &src_len, const std::vector<StreamResult> &would, uint64_t align) {
  uint64_t off = 0, need = 0;
  for (size_t i = 0; i < src_len.size(); i++)
    if (src_len[i] <= MAX_STREAM_LEN && would[i].status == ST_OK) { need = off + would[i].out_len; off += (would[i].out_len + align - 1) / align * align; }
  return need;
}

int main() {
  const uint64_t aligns[] = {1, 2, 16, 4096};
  std::vector<uint64_t> src_len;
  std::vector<StreamResult> would;
  // ---- the named output lengths, every residue of dst_off modulo 16 at align 1, at every address of the arena modulo 16
  {
    const uint64_t S = DPACKED_SEG_BYTES;
    std::vector<uint64_t> outs = {5, 15, 16, 17, 31, 33};
    for (int k = 0; k < 16; k++) outs.push_back(17);
    for (uint64_t o : {S - 1, S, S + 1, 2 * S + 5, 3 * S, (uint64_t)7}) outs.push_back(o);
    for (uint64_t o : outs) { src_len.push_back(o - 5 < 65535 ? o - 5 : o - 10); would.push_back(StreamResult{ST_OK, (uint32_t)o, o}); }
    uint64_t mx = 0, total = 0;
    for (uint64_t l : src_len) { mx = l > mx ? l : mx; total += l; }
    for (uint64_t align : aligns) {
      const uint64_t need = need_of(src_len, would, align);
      for (uint32_t mis = 0; mis < 16; mis++)
        for (uint64_t arena : {need, need - 1, (uint64_t)0, need / 2, (uint64_t)46, dpacked_arena_bound(src_len.size(), total, align, false)})
          check(src_len, would, mx, total, false, (int)(mis % 4), align, arena, mis);
      check(src_len, would, mx - 1, total, false, 1, align, need, 3);
      check(src_len, would, mx, total - 1, false, 1, align, need, 3);
    }
  }
  // ---- n on both sides of a wave, of the tile and of twice it
  for (uint32_t n : {1u, 63u, 64u, 65u, DPACKED_TILE - 1, DPACKED_TILE, DPACKED_TILE + 1, 2 * DPACKED_TILE, 2 * DPACKED_TILE + 1}) {
    make(n, 1, false, src_len, would);
    uint64_t total = 0;
    for (uint64_t l : src_len) total += l;
    for (uint64_t align : aligns) {
      const uint64_t need = need_of(src_len, would, align);
      for (uint64_t arena : {need, need ? need - 1 : 0, need / 3}) check(src_len, would, 40, total, false, 2, align, arena, (uint32_t)(rnd() % 16));
    }
  }
  // ---- random ragged batches: most streams short, some of several segments, some refused by deflate, some beyond the
  // format's range; the declared sizes exact, generous or short; the arena need, short of it, far too small or the bound
  for (int b = 0; b < 3000; b++) {
    const bool many = b % 60 == 0;
    const bool zlib = b % 3 == 0;
    const uint32_t n = 1 + (uint32_t)(rnd() % (many ? 2500 : 40));
    make(n, many ? 1 : b % 5 == 1 ? 2 : b % 5 == 2 ? 3 : 0, zlib, src_len, would);
    uint64_t mx = 0, total = 0;
    for (uint64_t l : src_len)
      if (l <= MAX_STREAM_LEN) { mx = l > mx ? l : mx; total += l; }
    const uint64_t align = b % 7 == 0 ? 1ull << (rnd() % 13) : aligns[rnd() % 4];
    const uint64_t need = need_of(src_len, would, align);
    const int how = b % 6;
    const uint64_t arena = how == 0 ? need : how == 1 ? (need ? need - 1 : 0) : how == 2 ? rnd() % (need + 1) : how == 3 ? 0
                                       : dpacked_arena_bound(n, total, align, zlib) + rnd() % 100;
    uint64_t dmx = mx, dtotal = total;
    if (b % 11 == 0 && mx > 0) dmx = mx - 1 - rnd() % mx;
    else if (b % 13 == 0 && total > 0) dtotal = total - 1 - rnd() % total;
    else if (b % 4 == 0) { dmx = mx + rnd() % 1000; dtotal = total + rnd() % 100000; }
    check(src_len, would, dmx, dtotal, zlib, (int)(rnd() % 4), align, arena, (uint32_t)(rnd() % 16));
  }
  printf("audit: %llu batches, no index left its array\n", (unsigned long long)batches);
  return 0;
}
