// sim_recode.cpp -- zipc_amd/csrc/recode_rules.h compiled with g++: open, link and close of a recode as the kernels of
// recode.hip and the host form's plan (host_pipeline.h) apply them, over a table of streams read from stdin, with arrays standing in
// for the context's scratch and a stub standing in for the codec.  Test tooling only (tests/test_recode_rules.py builds it
// plain and under the address and undefined-behaviour sanitizers, and runs it as a process of its own).
//
// stdin:   n max_mid_cap deflate_refuses_batch
//          then per stream: src_off src_len mid_off mid_cap dst_off dst_cap limit flags expect_crc32
//                           inflate_status inflate_checksum inflate_out_len deflate_status deflate_out_len
//          (what inflate / deflate say of the stream IF it reaches them; a "no stream" descriptor gets what the kernels
//          say of one: inflate ST_CORRUPTED, deflate ST_DST_TOO_SMALL, no bytes; deflate_refuses_batch: its device-side
//          check of the declared sizes trips, and every stream of the batch gets ST_INVALID_ARG from it)
// stdout:  per stream one line: the verdict after open, inflate's descriptor, the verdict after link, deflate's
//          descriptor, the result
#include <stdio.h>

#include <vector>

#include "../../zipc_amd/csrc/recode_rules.h"

using namespace zd;

static bool is_no_stream(const StreamDesc &d) { return d.src_len == 0 && d.dst_cap == 0 && d.flags == 0; }
static void print_desc(const StreamDesc &d) {
  printf(" | %llu %llu %llu %llu %llu %u %u", (unsigned long long)d.src_off, (unsigned long long)d.src_len, (unsigned long long)d.dst_off,
         (unsigned long long)d.dst_cap, (unsigned long long)d.limit, d.flags, d.reserved);
}
static void print_verdict(const RecodeVerdict &v) { printf(" | %u %u %u %llu", v.status, v.stage, v.checksum, (unsigned long long)v.mid_len); }

int main() {
  unsigned long long n = 0, max_mid_cap = 0;
  int refused = 0;
  if (scanf("%llu %llu %d", &n, &max_mid_cap, &refused) != 3 || n > 100000) return 2;
  std::vector<RecodeDesc> descs(n);
  std::vector<StreamResult> would_inflate(n), would_deflate(n);
  for (size_t i = 0; i < n; i++) {
    unsigned long long a[7], io, dl;
    unsigned f, e, is, ic, ds;
    if (scanf("%llu %llu %llu %llu %llu %llu %llu %u %u %u %u %llu %u %llu", &a[0], &a[1], &a[2], &a[3], &a[4], &a[5], &a[6], &f, &e, &is, &ic,
              &io, &ds, &dl) != 14)
      return 2;
    descs[i] = RecodeDesc{a[0], a[1], a[2], a[3], a[4], a[5], a[6], f, e};
    would_inflate[i] = StreamResult{is, ic, io};
    would_deflate[i] = StreamResult{ds, 0, dl};
  }
  // the context's scratch: the descriptors the codec runs with, its results, the verdicts
  std::vector<StreamDesc> inner(n), inflate_descs(n);
  std::vector<StreamResult> inner_res(n);
  std::vector<RecodeVerdict> verdicts(n), opened(n);
  std::vector<RecodeResult> results(n);
  for (size_t i = 0; i < n; i++) verdicts[i] = recode_open(descs[i], max_mid_cap, &inner[i]);  // recode_open_kernel
  inflate_descs = inner;
  opened = verdicts;
  for (size_t i = 0; i < n; i++) inner_res[i] = is_no_stream(inner[i]) ? StreamResult{ST_CORRUPTED, 0, 0} : would_inflate[i];  // inflate + CRC-32
  for (size_t i = 0; i < n; i++) verdicts[i] = recode_link(descs[i], verdicts[i], inner_res[i], &inner[i]);  // recode_link_kernel
  for (size_t i = 0; i < n; i++)  // deflate
    inner_res[i] = refused ? StreamResult{ST_INVALID_ARG, 0, 0} : is_no_stream(inner[i]) ? StreamResult{ST_DST_TOO_SMALL, 0, 0} : would_deflate[i];
  for (size_t i = 0; i < n; i++) results[i] = recode_close(verdicts[i], inner_res[i]);  // recode_close_kernel
  for (size_t i = 0; i < n; i++) {
    const RecodeResult &r = results[i];
    const StreamResult p = recode_plain_result(r);
    printf("%zu", i);
    print_verdict(opened[i]);
    print_desc(inflate_descs[i]);
    print_verdict(verdicts[i]);
    print_desc(inner[i]);
    printf(" | %u %u %llu %llu %u %u | %u %u %llu\n", r.status, r.checksum, (unsigned long long)r.out_len, (unsigned long long)r.mid_len, r.stage,
           r.reserved, p.status, p.checksum, (unsigned long long)p.out_len);
  }
  return 0;
}
