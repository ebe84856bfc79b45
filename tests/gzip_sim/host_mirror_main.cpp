// host_mirror_main.cpp -- the C++ mirror's three gzip values (zipc_amd/host/zipc_deflate.hpp gzip_compress, gzip_size,
// gzip_decompress) called as a C++ caller calls them, for tests/test_gpu_gzip.py: linked against libzipc_host.so and
// libzipc_hip.so, run as a process of its own on the GPU.
//   argv[1]: a gzip file; argv[2]: where its plain bytes go; argv[3]: where the file made of those bytes again goes -- one
//   plain member (`Fast), then BGZF members of 65 280 bytes each (`Default), then BGZF's end-of-file block.
// It prints what gzip_size and gzip_decompress say of argv[1] and of the file it made, what a file with a wrong CRC-32
// gives, and how many of two range errors were caught.
#include <stdio.h>

#include <fstream>
#include <iterator>
#include <string>

#include "../../zipc_amd/host/zipc_deflate.hpp"

namespace zd = zipc_deflate;

static const unsigned char BGZF_EOF[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

int main(int argc, char **argv) {
  if (argc != 4) { fprintf(stderr, "usage: %s file plain_out file_out\n", argv[0]); return 2; }
  std::ifstream in(argv[1], std::ios::binary);
  const std::string file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  const auto sized = zd::gzip_size(file);
  if (!sized.ok) { printf("error size: %s\n", sized.error.message.c_str()); return 1; }
  printf("size %zu %zu %zu\n", sized.value.length, sized.value.used, sized.value.members);
  const auto got = zd::gzip_decompress(file);
  if (!got.ok) { printf("error decompress: %s\n", got.error.message.c_str()); return 1; }
  printf("decompress %zu %zu %zu\n", got.value.value.size(), got.value.used, got.value.members);
  std::ofstream(argv[2], std::ios::binary).write(got.value.value.data(), (std::streamsize)got.value.value.size());
  const std::string &plain = got.value.value;
  std::string made;
  const auto first = zd::gzip_compress(plain, zd::level::Fast, false, 0, plain.size() < 1000 ? plain.size() : 1000);
  if (!first.ok) { printf("error compress: %s\n", first.error.c_str()); return 1; }
  made += first.value;
  std::size_t n_bgzf = 0;
  for (std::size_t at = plain.size() < 1000 ? plain.size() : 1000; at < plain.size(); at += 65280, n_bgzf++) {
    const auto m = zd::gzip_compress(plain, zd::level::Default, true, at, plain.size() - at < 65280 ? plain.size() - at : 65280);
    if (!m.ok) { printf("error bgzf: %s\n", m.error.c_str()); return 1; }
    made += m.value;
  }
  made.append((const char *)BGZF_EOF, sizeof BGZF_EOF);
  std::ofstream(argv[3], std::ios::binary).write(made.data(), (std::streamsize)made.size());
  const auto back = zd::gzip_decompress(made);
  printf("again %d %d %zu %zu\n", back.ok ? 1 : 0, back.ok && back.value.value == plain ? 1 : 0, back.value.used == made.size() ? n_bgzf + 2 : 0,
         back.value.members);
  const auto big = zd::gzip_compress(std::string(70000, 'x') + plain, zd::level::None, true);  // (no BGZF member holds 70 000 stored bytes)
  printf("too_big %d\n", big.ok ? 1 : 0);
  std::string bad = made;
  bad[first.value.size() - 8] ^= 1;  // the first member's CRC-32
  const auto wrong = zd::gzip_decompress(bad);
  printf("wrong %d %d\n", wrong.ok ? 1 : 0, wrong.error.found ? 1 : 0);
  int caught = 0;
  try { zd::gzip_size(file, file.size() + 1); } catch (const std::invalid_argument &) { caught++; }
  try { zd::gzip_decompress(file, 1, file.size()); } catch (const std::invalid_argument &) { caught++; }
  printf("range %d\n", caught);
  return 0;
}
