// Hash-chain links on the host.  TEST TOOLING ONLY.  Three things, in this order:
//   * sim_chain_reference: a plain serial reading of the reference's insert_hash (Lz77.hash4 and insert_hash,
//     zipc_deflate.ml:1145-1152) on the source bytes alone -- the second opinion every link of lz_chain is held to
//     (tests/test_chain_rules.py, tests/test_gpu_chain_links.py).  It shares nothing with the kernels: its own hash, its own
//     head table of absolute positions.  Nothing of zipc_amd/csrc is included above the line further down.
//   * the host model of lz_chain_kernel's round algorithm (zipc_amd/csrc/deflate.hip), whole streams and by segments.  The
//     kernel relies on "of several lanes storing to one LDS address, exactly one store lands"; the model replays the same
//     steps for 1024 virtual threads with the landing store chosen at random, and its links must equal the reference's for
//     any choice.
//   * a short model of lz_chain_xchg_segments_kernel: a serial exchange over a segment and the window before it.
// tests/test_chain_rules.py patches single lines of all three (its MUTANTS table): keep the statements it names on lines
// of their own.
#include <stdint.h>
#include <vector>

static const uint32_t CHAIN_REF_NO_POS = 0xFFFFFFFFu;  // lz77_no_pos

static uint32_t chain_ref_hash4(const uint8_t *s, uint32_t i) {  // zd.ml:1145-1148: 15 bits of the little-endian word times a constant
  uint32_t v = (uint32_t)s[i] | ((uint32_t)s[i + 1] << 8) | ((uint32_t)s[i + 2] << 16);
  v |= (uint32_t)s[i + 3] << 24;
  return (uint32_t)(v * 0x9E3779B1u) >> (32 - 15);
}
extern "C" uint32_t sim_chain_ref_hash4(const uint8_t *four) { return chain_ref_hash4(four, 0); }

// links[p] for p = 0 .. len - 4: the distance to the nearest earlier position of equal hash if that is at most 32768 (the
// window test of every walk, zd.ml:1187), else 0.  Nothing is written for a stream of fewer than 4 bytes, nor behind len - 4.
extern "C" void sim_chain_reference(const uint8_t *src, uint32_t len, uint16_t *links) {
  if (len < 4) return;
  const uint32_t last = len - 4;  // max_pos: the last position that has four bytes (zd.ml:1223)
  std::vector<uint32_t> head(1u << 15, CHAIN_REF_NO_POS);
  for (uint32_t p = 0; p <= last; p++) {
    const uint32_t h = chain_ref_hash4(src, p);
    const uint32_t q = head[h];
    uint32_t link = 0;
    if (q != CHAIN_REF_NO_POS && p - q <= 32768) link = p - q;
    links[p] = (uint16_t)link;
    head[h] = p;  // insert_hash zd.ml:1150-1152: every position, whatever its link
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Below this line: the models of the kernels, with the kernels' own hash (zd_common.h).
#include "../../zipc_amd/csrc/zd_common.h"

using namespace zd;

// B_first, own_lo, own_hi: lz_chain_segments_kernel's form -- rounds from B_first on with an empty table, the links of
// [own_lo, own_hi] stored, nothing inserted behind own_hi (the whole stream: 0, 0, len - 4)
static void chain_rounds(const uint8_t *s, uint32_t len, uint16_t *prev, uint32_t seed, int *max_turns,
                         uint32_t B_first, uint32_t own_lo, uint32_t own_hi);
extern "C" void sim_chain(const uint8_t *s, uint32_t len, uint16_t *prev, uint32_t seed, int *max_turns) {
  *max_turns = 0;
  if (len < 4) return;
  chain_rounds(s, len, prev, seed, max_turns, 0, 0, len - 4);
}
// the stream's links made segment by segment of seg_positions (a multiple of 16384), each from 32768 positions before
extern "C" void sim_chain_segments(const uint8_t *s, uint32_t len, uint16_t *prev, uint32_t seed, uint32_t seg_positions) {
  if (len < 4) return;
  int mt = 0;
  for (uint32_t lo = 0; lo <= len - 4; lo += seg_positions) {
    const uint32_t hi = len - 4 - lo >= seg_positions ? lo + seg_positions - 1 : len - 4;
    chain_rounds(s, len, prev, seed + lo, &mt, lo > 32768 ? lo - 32768 : 0, lo, hi);
  }
}
static void chain_rounds(const uint8_t *s, uint32_t len, uint16_t *prev, uint32_t seed, int *max_turns,
                         uint32_t B_first, uint32_t own_lo, uint32_t own_hi) {
  const uint32_t T = 1024, SWEEP_PERIOD = 16384, SWEEP_MARK = 20000;  // CHAIN_ROUND positions per round
  const int PLAIN_TURNS = 4;
  const int NEAR = 8;
  std::vector<uint16_t> head(32768);
  std::vector<uint16_t> hs(T + 2 * NEAR, 0xFFFF);
  const uint32_t max_pos = own_hi;
  (void)len;
  uint32_t rng = seed * 2654435761u + 1u;  // (a generator of the call's own: streams run side by side in the tests)
  auto rnd = [&rng] { rng ^= rng << 13; rng ^= rng >> 17; rng ^= rng << 5; return rng; };
  std::vector<uint32_t> h(T), e_old(T), near_pred(T), order;
  std::vector<char> active(T), reader(T), writer(T), pending(T), notmax(T);
  std::vector<int> pred_local(T);
  for (uint32_t B = B_first; B <= max_pos; B += T) {
    if ((B % SWEEP_PERIOD) == 0) {
      const uint16_t mark = (uint16_t)(B + SWEEP_MARK);
      for (uint32_t i = 0; i < 32768; i++) {
        bool keep = false;
        if (B != B_first) { uint32_t d = (B - head[i]) & 0xFFFFu; keep = d >= 1 && d <= 32768; }
        if (!keep) head[i] = mark;
      }
    }
    near_pred.assign(T, 0);
    notmax.assign(T, 0);
    pred_local.assign(T, -1);
    for (uint32_t t = 0; t < T; t++) {
      uint32_t p = B + t;
      active[t] = p <= max_pos;
      h[t] = active[t] ? hash4(load_u32_le(s + p)) : 0xFFFFu;
      hs[NEAR + t] = (uint16_t)h[t];
    }
    for (uint32_t t = 0; t < T; t++) e_old[t] = active[t] ? head[h[t]] : 0;
    for (uint32_t t = 0; t < T; t++) { reader[t] = active[t]; writer[t] = active[t]; pending[t] = active[t]; }
    int turns = 0;
    for (;;) {
      if (turns == PLAIN_TURNS) {
        for (uint32_t t = 0; t < T; t++) {
          bool has_succ = false;
          if (active[t]) {
            for (int k = NEAR; k >= 1; k--) if (hs[NEAR + t - k] == h[t]) near_pred[t] = k;
            for (int k = 1; k <= NEAR; k++) has_succ |= hs[NEAR + t + k] == h[t];
          }
          reader[t] = active[t] && near_pred[t] == 0;
          if (has_succ) { writer[t] = 0; pending[t] = 0; }
        }
      }
      turns++;
      // all pending threads store; a random one per address lands: apply in random order
      order.clear();
      for (uint32_t t = 0; t < T; t++) if (pending[t]) order.push_back(t);
      for (size_t i = order.size(); i > 1; i--) { size_t j = rnd() % i; std::swap(order[i - 1], order[j]); }
      for (uint32_t t : order) head[h[t]] = (uint16_t)(B + t);
      bool any = false;
      for (uint32_t t = 0; t < T; t++) {
        if (reader[t] || writer[t]) {
          uint32_t r_local = ((uint32_t)head[h[t]] - B) & 0xFFFFu;
          if (r_local == t) pending[t] = 0;
          else if (r_local < t) { if (reader[t] && (int)r_local > pred_local[t]) pred_local[t] = (int)r_local; }
          else notmax[t] = 1;
        }
      }
      for (uint32_t t = 0; t < T; t++) any |= pending[t];
      if (!any) break;
    }
    if (turns > *max_turns) *max_turns = turns;
    for (uint32_t t = 0; t < T; t++) if (writer[t] && !notmax[t]) head[h[t]] = (uint16_t)(B + t);
    for (uint32_t t = 0; t < T; t++) {
      if (!active[t]) continue;
      uint32_t p = B + t, d;
      if (near_pred[t]) d = near_pred[t];
      else if (pred_local[t] >= 0) d = t - (uint32_t)pred_local[t];
      else { d = (p - e_old[t]) & 0xFFFFu; if (d > 32768) d = 0; }
      if (p >= own_lo) prev[p] = (uint16_t)d;
    }
  }
}

// the reference's serial chain (insert_hash zd.ml:1150-1152) as distances
extern "C" void sim_chain_serial(const uint8_t *s, uint32_t len, uint16_t *prev) {
  if (len < 4) return;
  std::vector<int64_t> head(32768, -1);
  for (uint32_t p = 0; p + 4 <= len; p++) {
    uint32_t h = hash4(load_u32_le(s + p));
    int64_t q = head[h];
    prev[p] = (q >= 0 && p - q <= 32768) ? (uint16_t)(p - q) : 0;
    head[h] = p;
  }
}

// lz_chain_xchg_segments_kernel (lz_chain_xchg_kernel for seg_positions = 0: one segment, the whole stream): every segment
// of seg_positions starts from an empty table, exchanges the positions from 32768 before its first one up to its last one
// in order (one ds_wrxchg per position: the old entry out, the position in) and stores the links of its own positions.
extern "C" void sim_chain_xchg_segments(const uint8_t *s, uint32_t len, uint16_t *links, uint32_t seg_positions) {
  if (len < 4) return;
  const uint32_t XCHG_NONE = 0xFFFF0000u, stream_max_pos = len - 4;
  for (uint64_t lo = 0; lo <= stream_max_pos; lo += seg_positions ? seg_positions : (uint64_t)stream_max_pos + 1) {
    const uint32_t own_lo = (uint32_t)lo;
    const uint32_t own_hi = seg_positions && stream_max_pos - own_lo >= seg_positions ? own_lo + seg_positions - 1 : stream_max_pos;
    const uint32_t first = own_lo > 32768 ? own_lo - 32768 : 0;
    std::vector<uint32_t> head(32768, XCHG_NONE);
    for (uint32_t p = first; p <= own_hi; p++) {
      uint32_t &entry = head[hash4(load_u32_le(s + p))];
      const uint32_t d = p - entry;  // (from XCHG_NONE: p + 65536, beyond the window)
      entry = p;
      if (p >= own_lo) links[p] = (uint16_t)(d <= 32768 ? d : 0u);
    }
  }
}
