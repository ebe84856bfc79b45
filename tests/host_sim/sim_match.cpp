// A plain serial reading of the reference's match finder (Lz77.hash4, insert_hash and find_backref,
// zipc_deflate.ml:1145-1201) on the source bytes alone.  TEST TOOLING ONLY: the second opinion every record of lz_match
// is held to (tests/test_match_rules.py, tests/test_gpu_match_records.py).
//
// It shares nothing with the kernels: its own hash, its own head / prev tables of absolute positions, a compare byte by
// byte.  Nothing of zipc_amd/csrc is included above the line further down; what comes below it is only the export of
// deflate_lane.h's lz_match_position for the cross-check of the two.
//
// find_backref is a function of the pending match length; like lz_match_position this reading returns what does not
// depend on it: per position the best of the first K chain candidates and the best of the first Kq (the parse reads the
// second one where the pending match is at least good_match long), each as the longest common prefix above 3, the nearest
// candidate on ties, packed dist << 9 | len, 0 for none.  The reference's running threshold starts at the pending length
// instead of 3; comparing afterwards selects the same candidate (a maximum does not depend on where the threshold began).
//
// tests/test_match_rules.py patches single lines of sim_match_reference (its MUTANTS table): keep the statements it names
// on lines of their own.
#include <stdint.h>
#include <vector>

static const uint32_t REF_NO_POS = 0xFFFFFFFFu;  // lz77_no_pos

static uint32_t ref_hash4(const uint8_t *s, uint32_t i) {  // zd.ml:1145-1148: 15 bits of the little-endian word times a constant
  const uint32_t v = (uint32_t)s[i] | ((uint32_t)s[i + 1] << 8) | ((uint32_t)s[i + 2] << 16) | ((uint32_t)s[i + 3] << 24);
  return (uint32_t)(v * 0x9E3779B1u) >> (32 - 15);
}
extern "C" uint32_t sim_match_hash4(const uint8_t *four) { return ref_hash4(four, 0); }

// best[p], first[p] for p = 0 .. len - 4 (nothing is written for a stream of fewer than 4 bytes)
extern "C" void sim_match_reference(const uint8_t *src, uint32_t len, int K, int Kq, uint32_t *best, uint32_t *first) {
  if (len < 4) return;
  std::vector<uint32_t> head(1u << 15, REF_NO_POS), prev(len, REF_NO_POS);
  for (uint32_t p = 0; p + 4 <= len; p++) {  // Lz77.compress inserts every position up to max_pos, visited or skipped (zd.ml:1223, 1230)
    const uint32_t h = ref_hash4(src, p);
    uint32_t cap = 258;                   // max_match_len
    if (cap > len - p) cap = len - p;     // zd.ml:1220
    uint32_t best_len = 3, best_rec = 0, first_rec = 0;  // zd.ml:1178: at least min_match_len
    bool have_first = false;
    int steps = 0;
    uint32_t i = head[h];
    while (i != REF_NO_POS && steps != K && p - i <= 32768) {  // zd.ml:1187
      uint32_t l = 0;
      while (l < cap && src[i + l] == src[p + l]) l++;
      steps++;  // a candidate counts whether or not it shares four bytes (zd.ml:1192)
      if (l > best_len) { best_len = l; best_rec = ((p - i) << 9) | l; }  // strictly longer: the nearest wins a tie (zd.ml:1166-1174)
      if (steps == Kq) { first_rec = best_rec; have_first = true; }
      if (l == cap) break;  // zd.ml:1194
      i = prev[i];
    }
    if (!have_first) first_rec = best_rec;  // the chain ended before Kq candidates
    best[p] = best_rec;
    first[p] = first_rec;
    prev[p] = head[h];  // insert_hash zd.ml:1150-1152 (prev by absolute position: the reference's table mod 32768 holds
    head[h] = p;        // the same entry for every position the window test lets a walk reach)
  }
}

// The lazy parse (Lz77.compress zd.ml:1203-1244) over such records, for what it READS: read[p] = 0 where the parse never
// comes, 1 where it reads best[p], 2 where it reads first[p] (a pending match of good_match or more, zd.ml:1184), 3 where
// it comes and reads neither (the pending match already is as long as a match can be there, zd.ml:1181).
extern "C" void sim_match_parse_reads(uint32_t len, int good_match, const uint32_t *best, const uint32_t *first, uint8_t *read) {
  if (len < 4) return;
  const uint32_t max_pos = len - 4;
  uint32_t i = 0, pl = 0;
  while (i <= max_pos) {
    uint32_t cap = 258;
    if (cap > len - i) cap = len - i;
    const uint32_t thr = pl ? pl : 3;
    uint32_t ml = 0;
    if (thr >= cap) read[i] = 3;
    else {
      const bool quarter = pl >= (uint32_t)good_match;
      read[i] = quarter ? 2 : 1;
      const uint32_t r = quarter ? first[i] : best[i];
      if ((r & 511u) > thr) ml = r & 511u;
    }
    if (pl != 0 && pl > ml) { i = i - 1 + pl; pl = 0; }  // the pending match is written; the parse goes on behind it
    else if (ml == 0) { i++; pl = 0; }
    else { i++; pl = ml; }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Below this line only: the kernels' serial statement of the same thing, deflate_lane.h lz_match_position, over links as
// sim_chain.cpp's sim_chain_serial makes them -- sim_deflate proves that ITS records give the oracle's bytes, so the
// reference above is anchored by being equal to it at every position.
#include "../../zipc_amd/csrc/deflate_lane.h"

extern "C" void sim_match_lane_position(const uint8_t *src, uint32_t len, const uint16_t *links, int K, int Kq, uint32_t *best,
                                        uint32_t *first) {
  if (len < 4) return;
  for (uint32_t p = 0; p + 4 <= len; p++) {
    const uint64_t r = zd::lz_match_position(src, len, p, links, K, Kq);
    best[p] = (uint32_t)r;
    first[p] = (uint32_t)(r >> 32);
  }
}
