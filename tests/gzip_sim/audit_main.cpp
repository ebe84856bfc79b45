// audit_main.cpp -- the host model of the gzip forms (sim_gzip.cpp) as a stand-alone program, meant to be built with
// -fsanitize=address,undefined: every case of the file it is given runs at two budgets of turns, its source a heap block of
// EXACTLY src_len bytes and its room one of exactly dst_cap, so a load behind the declared source -- a header field's, the
// search for a name's zero, the trailer's, the input ring's last word -- or a store outside the room trips the sanitizer.
// The program aborts when a record differs from what the file says.  tests/test_gzip_rules.py writes the file, compiles
// the program and runs it; it is never loaded into another process.
//
// The file, little-endian words: n, then per case src_len, dst_cap, has_limit, limit, flags, form, crc, and the record
// expected -- status, checksum, out_len, src_used, hdr_len, flg -- and the source.
#include <stdio.h>
#include <stdlib.h>

#include "sim_gzip.cpp"

static const int BUDGETS[] = {512, 7};

#define AUDIT_FAIL(...) do { fprintf(stderr, "audit: case %u, budget %d: ", i, budget); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); abort(); } while (0)

static uint32_t word(FILE *fp) {
  uint8_t b[4];
  if (fread(b, 1, 4, fp) != 4) { fprintf(stderr, "audit: the file ends early\n"); abort(); }
  return b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s cases\n", argv[0]); return 2; }
  FILE *fp = fopen(argv[1], "rb");
  if (!fp) { perror(argv[1]); return 2; }
  const uint32_t n = word(fp);
  uint64_t n_ok = 0;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t src_len = word(fp), dst_cap = word(fp), has_limit = word(fp), limit = word(fp), flags = word(fp), form = word(fp);
    const uint32_t crc = word(fp);
    uint64_t want[6];
    for (uint64_t &w : want) w = word(fp);
    uint8_t *src = (uint8_t *)malloc(src_len);
    if (src_len && fread(src, 1, src_len, fp) != src_len) { fprintf(stderr, "audit: the file ends early\n"); abort(); }
    for (const int budget : BUDGETS) {
      uint8_t *room = (uint8_t *)malloc(dst_cap);
      uint64_t out[6] = {0xEE, 0xEE, 0xEE, 0xEE, 0xEE, 0xEE};
      sim_gzip(src, src_len, form ? nullptr : room, dst_cap, (int)has_limit, limit, flags, (int)form, crc, budget, out);
      for (int k = 0; k < 6; k++)
        if (out[k] != want[k]) AUDIT_FAIL("field %d is %llu, not %llu", k, (unsigned long long)out[k], (unsigned long long)want[k]);
      if (out[3] > src_len) AUDIT_FAIL("src_used %llu of %u declared bytes", (unsigned long long)out[3], src_len);
      free(room);
    }
    n_ok += want[0] == 0;
    free(src);
  }
  fclose(fp);
  printf("audit: %u cases at 2 budgets, %llu of them OK, nothing outside a source or a room\n", n, (unsigned long long)n_ok);
  return 0;
}
