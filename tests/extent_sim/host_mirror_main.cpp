// host_mirror_main.cpp -- the C++ mirror's two extent values (zipc_amd/host/zipc_deflate.hpp inflate_extent,
// zlib_decompress_extent) called as a C++ caller calls them, for tests/test_gpu_inflate_extent.py: linked against
// libzipc_host.so, run as a process of its own on the GPU.
//   argv[1]: a file of zlib streams stored back to back.  The program walks it by the recipe -- bound, extent, next stream --
//   with zlib_decompress_extent(arena, nullopt, at), then inflates the first stream's body once more with
//   inflate_extent(arena, nullopt, 2, len - 2), and asks both for a range outside the string.
//   stdout: a line "zlib <used> <out_len>" per stream, "raw <used> <out_len>", "range <n caught>", then "error ..." lines
//   for what failed; argv[2]: where the walk's plain bytes go, end to end.
#include <stdio.h>

#include <fstream>
#include <iterator>
#include <string>

#include "../../zipc_amd/host/zipc_deflate.hpp"

namespace zd = zipc_deflate;

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s arena plain_out\n", argv[0]); return 2; }
  std::ifstream in(argv[1], std::ios::binary);
  const std::string arena((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  std::ofstream out(argv[2], std::ios::binary);
  std::size_t at = 0;
  while (at < arena.size()) {
    const auto r = zd::zlib_decompress_extent(arena, std::nullopt, at);
    if (!r.ok) { printf("error zlib at %zu: %s\n", at, r.error.c_str()); return 1; }
    printf("zlib %zu %zu\n", r.value.second, r.value.first.size());
    out.write(r.value.first.data(), (std::streamsize)r.value.first.size());
    at += r.value.second;
  }
  const auto raw = zd::inflate_extent(arena, std::nullopt, 2, arena.size() - 2);
  if (!raw.ok) { printf("error raw: %s\n", raw.error.c_str()); return 1; }
  printf("raw %zu %zu\n", raw.value.second, raw.value.first.size());
  int caught = 0;
  try { zd::inflate_extent(arena, std::nullopt, arena.size() + 1); } catch (const std::invalid_argument &) { caught++; }
  try { zd::zlib_decompress_extent(arena, std::nullopt, 1, arena.size()); } catch (const std::invalid_argument &) { caught++; }
  printf("range %d\n", caught);
  const auto bad = zd::zlib_decompress_extent(arena, std::nullopt, 1);  // (not a zlib header there)
  printf("bad %d\n", bad.ok ? 1 : 0);
  return 0;
}
