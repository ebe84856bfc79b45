// audit_main.cpp -- the host model of the ragged checksum pass (sim_ranges.cpp) as a stand-alone program, meant to be
// built with -fsanitize=address,undefined: the seams of tests/checksum_batch_cases.py restated in their smallest form and a
// few thousand random ragged batches, each run as the launches would run it.  The program aborts when a load leaves its
// range, a slot reaches past segs_bound / chunks_bound, the search leaves [0, n), or a checksum differs from a plain
// byte-wise one.  tests/test_checksum_ranges_rules.py compiles and runs it; it is never loaded into another process.
#include <stdio.h>
#include <stdlib.h>

#include "sim_ranges.cpp"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return rng_state;
}

static uint32_t plain_crc(const uint8_t *p, uint64_t n) { return sim::crc_raw_init(p, n); }
// the reference's Adler-32 byte by byte in its chunks (zd.ml:175-198), or RFC 1950's
static uint32_t plain_adler(const uint8_t *p, uint64_t n, bool rfc) {
  int32_t s1 = 1, s2 = 0;  // (RFC 1950: the same sums with the unsigned remainder, which no chunking changes)
  uint64_t at = 0, len = n % ADLER_CHUNK;
  while (at < n || len) {
    uint32_t u1 = (uint32_t)s1, u2 = (uint32_t)s2;
    for (uint64_t i = 0; i < len; i++) { u1 += p[at + i]; u2 += u1; }
    s1 = rfc ? (int32_t)(u1 % ADLER_BASE) : (int32_t)u1 % (int32_t)ADLER_BASE;
    s2 = rfc ? (int32_t)(u2 % ADLER_BASE) : (int32_t)u2 % (int32_t)ADLER_BASE;
    at += len;
    if (at >= n) break;
    len = ADLER_CHUNK;
  }
  return ((uint32_t)s2 << 16) + (uint32_t)s1;
}

static uint64_t batches = 0;

static void check(const std::vector<uint8_t> &arena, const std::vector<Range> &ranges, uint64_t total_len, bool rfc, bool expect_bad) {
  std::vector<RangeResult> res(ranges.size() + 1);
  uint64_t stats[12];
  const uint64_t v = sim_ranges_run(arena.data(), arena.size(), ranges.data(), (uint32_t)ranges.size(), total_len, 1, 1, rfc, res.data(), stats);
  batches++;
  if (v) { fprintf(stderr, "audit: %llu violations in batch %llu\n", (unsigned long long)v, (unsigned long long)batches); abort(); }
  if ((stats[4] != 0) != expect_bad) { fprintf(stderr, "audit: bad-call flag %llu in batch %llu\n", (unsigned long long)stats[4], (unsigned long long)batches); abort(); }
  for (size_t i = 0; i < ranges.size(); i++) {
    const Range r = ranges[i];
    const bool ok = r.off + r.len >= r.off && r.off + r.len <= arena.size();
    uint32_t st = ok ? 0 : 18, crc = 0, adler = 0;
    if (expect_bad) st = 18;
    else if (ok) { crc = plain_crc(arena.data() + r.off, r.len); adler = plain_adler(arena.data() + r.off, r.len, rfc); }
    if (res[i].status != st || res[i].crc32 != crc || res[i].adler32 != adler) {
      fprintf(stderr, "audit: batch %llu range %zu {%llu, %llu}: got %u %08x %08x, want %u %08x %08x\n", (unsigned long long)batches, i,
              (unsigned long long)r.off, (unsigned long long)r.len, res[i].status, res[i].crc32, res[i].adler32, st, crc, adler);
      abort();
    }
  }
}

static uint64_t ok_sum(const std::vector<uint8_t> &arena, const std::vector<Range> &ranges) {
  uint64_t s = 0;
  for (const Range &r : ranges)
    if (r.off + r.len >= r.off && r.off + r.len <= arena.size()) s += r.len;
  return s;
}

static std::vector<uint8_t> fill(size_t n, int kind) {
  std::vector<uint8_t> a(n);
  for (size_t i = 0; i < n; i++) a[i] = kind == 0 ? (uint8_t)(rnd() >> 24) : kind == 1 ? 0xFF : 0;
  return a;
}

int main() {
  const uint64_t S = RANGES_SEG_BYTES;
  // ---- the named lengths, at offsets 3 and 21, in the three fills
  const uint64_t lengths[] = {0, 1, 15, 16, 17, 5551, 5552, 5553, 32767, 32768, 32769, 16 * S - 1, 16 * S, 16 * S + 1, 64 * S, 64 * S + 1};
  for (int kind = 0; kind < 3; kind++) {
    std::vector<Range> ranges;
    uint64_t at = 0;
    for (size_t k = 0; k < sizeof lengths / sizeof *lengths; k++) {
      at = (at + 31) / 32 * 32 + (k % 2 ? 21 : 3);
      ranges.push_back(Range{at, lengths[k]});
      at += lengths[k] + 5;
    }
    const std::vector<uint8_t> arena = fill(at + 7, kind);
    check(arena, ranges, ok_sum(arena, ranges), kind == 2, false);
    check(arena, ranges, ok_sum(arena, ranges), kind != 2, false);
  }
  // ---- n on both sides of the plan's tile and of twice it; one long range among short ones
  const std::vector<uint8_t> arena = fill((9 << 20) + 12345, 0);
  for (uint32_t n : {1u, RANGES_PLAN_TILE - 1, RANGES_PLAN_TILE, RANGES_PLAN_TILE + 1, 2 * RANGES_PLAN_TILE - 1, 2 * RANGES_PLAN_TILE, 2 * RANGES_PLAN_TILE + 1}) {
    std::vector<Range> ranges;
    for (uint32_t i = 0; i < n; i++) ranges.push_back(Range{rnd() % 100000, rnd() % 301});
    check(arena, ranges, ok_sum(arena, ranges), false, false);
  }
  for (int where = 0; where < 3; where++) {
    std::vector<Range> ranges;
    for (uint32_t i = 0; i < 300; i++) ranges.push_back(Range{rnd() % 100000, 1 + rnd() % 3000});
    ranges.insert(ranges.begin() + (where == 0 ? 0 : where == 1 ? 150 : 300), Range{21, (8 << 20) + 4321});
    check(arena, ranges, ok_sum(arena, ranges), false, false);
  }
  // ---- the verdicts: twice the same, overlapping, empty between full, past the arena by a byte, an overflowing end,
  // exactly at the end; the declared total exact, generous, and one too small
  {
    const uint64_t A = arena.size();
    const std::vector<Range> ranges = {{3, 40000}, {3, 40000}, {21, 70000}, {30021, 33000}, {50, 0}, {A - 7000, 7000}, {A, 0}, {A - 6999, 7000},
                                       {77, 5553}, {~0ull - 9, 11}, {0, 0}, {A - 1, 1}, {A + 1, 0}};
    const uint64_t sum = ok_sum(arena, ranges);
    check(arena, ranges, sum, false, false);
    check(arena, ranges, sum + 100000, false, false);
    check(arena, ranges, sum - 1, false, true);
    check(arena, ranges, 0, false, true);
  }
  // ---- random ragged batches: most ranges short, some long, some bad; a declared total that is exact, generous or short
  for (int b = 0; b < 2000; b++) {
    const bool many = b % 50 == 0;  // (thousands of ranges: short ones only, with a single long one among them)
    const uint32_t n = 1 + (uint32_t)(rnd() % (many ? 2500 : 40));
    std::vector<Range> ranges;
    for (uint32_t i = 0; i < n; i++) {
      const uint64_t pick = many ? (i == n / 2 ? 90 : rnd() % 60) : rnd() % 100;
      uint64_t len = pick < 60 ? rnd() % 3000 : pick < 90 ? rnd() % (3 * S) : pick < 91 ? rnd() % (70 * S) : 0;
      uint64_t off = rnd() % (arena.size() - len);
      if (b % 7 == 0 && rnd() % 10 == 0) off = arena.size() - len + rnd() % 3;  // ending at, or just past, the arena
      if (b % 11 == 0 && rnd() % 20 == 0) { off = ~0ull - rnd() % 100; len = 1 + rnd() % 200; }
      ranges.push_back(Range{off, len});
    }
    const uint64_t sum = ok_sum(arena, ranges);
    const int how = b % 5;
    if (how == 4 && sum > 0) check(arena, ranges, sum - 1 - rnd() % sum, b & 1, true);
    else check(arena, ranges, how == 3 ? sum + rnd() % 200000 : sum, b & 1, false);
  }
  printf("audit: %llu batches, no index left its array\n", (unsigned long long)batches);
  return 0;
}
