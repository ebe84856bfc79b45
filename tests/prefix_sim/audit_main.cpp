// audit_main.cpp -- the host model of the prefix form (sim_prefix.cpp) as a stand-alone program, meant to be built with
// -fsanitize=address,undefined: every case of the file it is given runs in all four forms of the model, its room a heap
// block of EXACTLY dst_cap bytes and its source one of exactly src_len, so a store (or a load) behind the cut, in front of
// the room or past the input trips the sanitizer.  The program aborts when a record or a byte of a room differs from what
// the file says.  tests/test_inflate_prefix_rules.py writes the file, compiles the program and runs it; it is never
// loaded into another process.
//
// The file, little-endian words: n, then per case src_len, dst_cap, has_limit, limit, status, ended, out_len, with_bytes,
// the source, and with_bytes ? out_len bytes the room must begin with : nothing.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "sim_prefix.cpp"

static const struct { const char *name; int span, budget; } FORMS[] = {{"plain-512", 0, 512}, {"plain-7", 0, 7}, {"span-a", 1, 24}, {"span-d", 2, 24}};

#define AUDIT_FAIL(...) do { fprintf(stderr, "audit: case %u, %s: ", i, f.name); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); abort(); } while (0)

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
  uint64_t cuts = 0;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t src_len = word(fp), dst_cap = word(fp), has_limit = word(fp), limit = word(fp);
    const uint32_t status = word(fp), ended = word(fp), out_len = word(fp), with_bytes = word(fp);
    uint8_t *src = (uint8_t *)malloc(src_len);
    std::vector<uint8_t> want(with_bytes ? out_len : 0);
    if ((src_len && fread(src, 1, src_len, fp) != src_len) || (!want.empty() && fread(want.data(), 1, want.size(), fp) != want.size())) { fprintf(stderr, "audit: the file ends early\n"); abort(); }
    for (const auto &f : FORMS) {
      uint8_t *room = (uint8_t *)malloc(dst_cap);
      if (dst_cap) memset(room, 0xA5, dst_cap);
      uint64_t out[3] = {0xEE, 0xEE, 0xEE};
      sim_prefix(src, src_len, room, dst_cap, (int)has_limit, limit, 0, f.span, f.budget, out);
      if (out[0] != status || out[1] != ended || out[2] != out_len)
        AUDIT_FAIL("{%llu, %llu, %llu}, not {%u, %u, %u}", (unsigned long long)out[0], (unsigned long long)out[1], (unsigned long long)out[2], status,
                   ended, out_len);
      if (out_len > dst_cap) AUDIT_FAIL("out_len %u in a room of %u", out_len, dst_cap);
      if (with_bytes && out_len && memcmp(room, want.data(), out_len) != 0) AUDIT_FAIL("a byte of the first %u differs", out_len);
      free(room);
    }
    cuts += status == 0 && !ended;
    free(src);
  }
  fclose(fp);
  printf("audit: %u cases in 4 forms, %llu of them cut, nothing outside a room\n", n, (unsigned long long)cuts);
  return 0;
}
