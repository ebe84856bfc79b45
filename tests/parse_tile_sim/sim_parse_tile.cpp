// zipc_amd/csrc/parse_tile.h behind a C view.  TEST TOOLING ONLY: the very predicate lz_parse_wave (deflate.hip) chooses a
// tile's form by, so that tests/test_parse_tile_form.py can enumerate it.
#include "parse_tile.h"

extern "C" int sim_parse_tile_interior(uint32_t B, uint32_t len, uint32_t blk_start, int cuts) {
  return zd::parse_tile_interior(B, len, blk_start, cuts != 0) ? 1 : 0;
}

// out[t]: the form of the tile at 64 t, for every tile of a stream of len bytes (at least one: the wave of an empty stream has none)
extern "C" void sim_parse_tile_forms(uint32_t len, uint32_t blk_start, int cuts, uint8_t *out) {
  for (uint32_t B = 0; B < len; B += 64u) out[B / 64u] = (uint8_t)sim_parse_tile_interior(B, len, blk_start, cuts);
}

extern "C" uint32_t sim_parse_interior_end(uint32_t len, uint32_t blk_start, int cuts) {
  return zd::parse_interior_end(len, blk_start, cuts != 0);
}
