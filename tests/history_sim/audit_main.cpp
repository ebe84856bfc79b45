// audit_main.cpp -- the host model of the history forms (sim_history.cpp) as a stand-alone program, meant to be built with
// -fsanitize=address,undefined: every case of the file it is given runs in all four forms of the model and its three
// modes, its [history | room] a heap block of EXACTLY hist_len + dst_cap bytes and its source one of exactly src_len, so a
// load in front of the history, a store behind the room or a read past the input trips the sanitizer (the sizing mode
// is handed no block at all).  The program aborts when a result or a byte of a room differs from what the file says, or
// when a byte of the history has changed.  tests/test_inflate_history_rules.py writes the file, compiles the program and
// runs it; it is never loaded into another process.
//
// The file, little-endian words: n, then per case src_len, hist_len, start_bit, dst_cap, has_limit, limit, then for each of
// the modes history, prefix, size: status, checksum (prefix: ended), out_len, with_bytes; then the source, the history,
// plain_len and the plain bytes (a mode with_bytes: its room begins with the first out_len of them).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "sim_history.cpp"

static const struct { const char *name; int span, budget; } FORMS[] = {{"plain-512", 0, 512}, {"plain-7", 0, 7}, {"span-a", 1, 24}, {"span-d", 2, 24}};
static const char *MODE_NAMES[] = {"history", "prefix", "size"};

#define AUDIT_FAIL(...) do { fprintf(stderr, "audit: case %u, %s, %s: ", i, MODE_NAMES[mode], f.name); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); abort(); } while (0)

static uint32_t word(FILE *fp) {
  uint8_t b[4];
  if (fread(b, 1, 4, fp) != 4) { fprintf(stderr, "audit: the file ends early\n"); abort(); }
  return b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
}
static void bytes(FILE *fp, uint8_t *into, size_t n) {
  if (n && fread(into, 1, n, fp) != n) { fprintf(stderr, "audit: the file ends early\n"); abort(); }
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s cases\n", argv[0]); return 2; }
  FILE *fp = fopen(argv[1], "rb");
  if (!fp) { perror(argv[1]); return 2; }
  const uint32_t n = word(fp);
  uint64_t runs = 0;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t src_len = word(fp), hist_len = word(fp), start_bit = word(fp), dst_cap = word(fp), has_limit = word(fp), limit = word(fp);
    uint32_t want[3][4];
    for (auto &w : want)
      for (uint32_t &x : w) x = word(fp);
    uint8_t *src = (uint8_t *)malloc(src_len);
    std::vector<uint8_t> hist(hist_len);
    bytes(fp, src, src_len);
    bytes(fp, hist.data(), hist_len);
    std::vector<uint8_t> plain(word(fp));
    bytes(fp, plain.data(), plain.size());
    for (int mode = 0; mode < 3; mode++) {
      for (const auto &f : FORMS) {
        uint8_t *block = mode == SIM_SIZE ? nullptr : (uint8_t *)malloc((size_t)hist_len + dst_cap);
        if (block && hist_len + dst_cap) {
          memset(block, 0xA5, (size_t)hist_len + dst_cap);
          if (hist_len) memcpy(block, hist.data(), hist_len);
        }
        uint64_t out[3] = {0xEE, 0xEE, 0xEE};
        sim_history(src, src_len, hist_len, start_bit, block, hist_len, dst_cap, (int)has_limit, limit, 0, mode, 1, f.span, f.budget, out);
        const uint32_t *w = want[mode];
        if (out[0] != w[0] || out[1] != w[1] || out[2] != w[2])
          AUDIT_FAIL("{%llu, %llu, %llu}, not {%u, %u, %u}", (unsigned long long)out[0], (unsigned long long)out[1], (unsigned long long)out[2], w[0], w[1], w[2]);
        if (block) {
          if (w[2] > dst_cap) AUDIT_FAIL("out_len %u in a room of %u", w[2], dst_cap);
          if (hist_len && memcmp(block, hist.data(), hist_len) != 0) AUDIT_FAIL("the history has changed");
          if (w[3] && w[2] && (w[2] > plain.size() || memcmp(block + hist_len, plain.data(), w[2]) != 0)) AUDIT_FAIL("a byte of the first %u differs", w[2]);
        }
        free(block);
        runs++;
      }
    }
    free(src);
  }
  fclose(fp);
  printf("audit: %u cases, %llu runs in 4 forms and 3 modes, nothing outside a block\n", n, (unsigned long long)runs);
  return 0;
}
