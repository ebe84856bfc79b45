// sim_zlib.cpp -- zipc_amd/csrc/zlib_container.h compiled with g++: the container's rules as the kernels of zlib.hip and
// the host forms of api.hip and many.hip apply them, for tests/test_zlib_rules.py to hold against the oracle.  Test tooling only.
#include "../../zipc_amd/csrc/zlib_container.h"

extern "C" {

unsigned sim_zlib_open_status(unsigned long long len, unsigned cmf, unsigned flg) { return zd::zlib_open_status(len, cmf, flg); }
// out[65536]: the status of every (cmf, flg) pair at one length, cmf-major
void sim_zlib_open_status_all(unsigned long long len, unsigned char *out) {
  for (unsigned cmf = 0; cmf < 256; cmf++)
    for (unsigned flg = 0; flg < 256; flg++) out[cmf * 256 + flg] = (unsigned char)zd::zlib_open_status(len, cmf, flg);
}
unsigned sim_zlib_cmf(void) { return zd::zlib_cmf(); }
unsigned sim_zlib_flg(int level) { return zd::zlib_flg(level); }
unsigned long long sim_zlib_body_off(unsigned long long off) { return zd::zlib_body_off(off); }
unsigned long long sim_zlib_body_len(unsigned long long len) { return zd::zlib_body_len(len); }
unsigned sim_zlib_expect(const unsigned char *last4) { return zd::zlib_expect(last4); }
void sim_zlib_put_trailer(unsigned char *p, unsigned adler) { zd::zlib_put_trailer(p, adler); }
// a stream's result from the check's verdict and the codec's: out = {status, checksum, out_len}
void sim_zlib_close_decompress(unsigned pre, unsigned expect, unsigned status, unsigned checksum, unsigned long long out_len,
                               unsigned long long *out) {
  const zd::StreamResult r = zd::zlib_close_decompress(pre, expect, zd::StreamResult{status, checksum, out_len});
  out[0] = r.status; out[1] = r.checksum; out[2] = r.out_len;
}
int sim_zlib_close_compress(unsigned pre, unsigned status, unsigned checksum, unsigned long long out_len, unsigned long long *out) {
  bool wrap;
  const zd::StreamResult r = zd::zlib_close_compress(pre, zd::StreamResult{status, checksum, out_len}, &wrap);
  out[0] = r.status; out[1] = r.checksum; out[2] = r.out_len;
  return wrap ? 1 : 0;
}

}  // extern "C"
