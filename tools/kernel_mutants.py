#!/usr/bin/env python3
"""Shows that the suite kills one-line mutants of the kernels' block chooser.

The reference chooses a block's kind by two `<=` (zd.ml:1102-1103) from three estimates, the stored one padding 8
bits, not 0, when the type bits end a byte (Q3, zd.ml:1045-1047).  The kernels hold that rule three times:
wave_choose (deflate_emit_kernel, many streams), the inline chooser of deflate_scan_kernel (few long streams) and
coder_choose (zipc_amd/csrc/deflate_lane.h, the host models in tests/host_sim).  Each mutant below changes one of those
lines into its "obvious" version.  Only the choice arithmetic is touched: a wrong choice still writes a valid block
within deflate_bound, so no mutant can write out of bounds.

  tools/kernel_mutants.py --build        each GPU mutant of zipc_amd/csrc/deflate.hip into zipc_amd/lib/mutants/
                                          (build again after any change of zipc_amd/csrc)
  tools/kernel_mutants.py                 (on the MI355X) the vector tests of tests/test_gpu_parity.py against each
                                          mutant library (ZIPC_HIP_LIB), once; every mutant must make them fail
  tools/kernel_mutants.py --inflate ...   the same for the inflate mutants below, against tests/test_gpu_inflate_rules.py

Inflate: the accept / reject rules (zd.ml:355-391, 564-709) are written out again in inflate_lane.h (the plain step,
the fixed path, the serial header and stored code, which the host models compile too), in inflate.hip's wave forms
(wave_init_decoder, wave_tables, wave_dynamic_lengths) and in the refusals of inflate_span.h.  On the GPU a mutant only
makes a check STRICTER -- it refuses more or stops earlier -- so it touches no memory the real kernel does not.  Each
one of the decoding copies must make the rule tests fail.  The span's refusals hand a symbol to the plain step, so a
stricter refusal must change NO result: those are listed as expected to survive, and the rule tests (under every
override) passing under them is what shows the hand-off right.  The relaxed mutants (LANE_INFLATE_RELAXED) run only in
the host models, in child processes: tests/test_host_sim.py::test_inflate_lane_mutants_are_killed.

The mutants of the Adler-32 chunk chain (ADLER_MUTANTS, zipc_amd/csrc/adler_chain.h) are killed on the CPU only:
tests/test_adler_chain_sim.py::test_adler_chain_mutants_are_killed.
The mutants of inflate's room (ROOM_MUTANTS: where a stream's bytes may go) are killed on the CPU only, and are never built
for the GPU: tests/test_inflate_room_rules.py::test_room_mutants_are_killed.
The mutants of the span decoder's token form (TOKEN_MUTANTS) are killed on the CPU only, and are never built for the GPU:
tests/test_token_rules.py::test_token_mutants_are_killed.
The coder_choose mutants are killed on the CPU: tests/test_host_sim.py::test_coder_choose_mutants_are_killed.
Each text must occur exactly once in its file, so a change of the kernels cannot quietly make a mutant a no-op.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zipc_amd", "csrc")
OUT = os.path.join(ROOT, "zipc_amd", "lib", "mutants")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# zipc_amd/csrc/Makefile's flags
HIPFLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function"]

# (name, file under zipc_amd/csrc, text, replacement)
GPU_MUTANTS = [
    ("wave_choose_stored_strict", "deflate.hip",
     "  if (nlen <= dlen && nlen <= flen) return 0;", "  if (nlen < dlen && nlen < flen) return 0;"),
    ("wave_choose_fixed_strict", "deflate.hip", "  if (flen <= dlen) return 1;", "  if (flen < dlen) return 1;"),
    ("wave_choose_q3_mod_8", "deflate.hip",
     "(uint64_t)(8 - ((pending_bits + 3) % 8))", "(uint64_t)((8 - ((pending_bits + 3) % 8)) % 8)"),
    ("scan_stored_strict", "deflate.hip", "(nlen <= dlen && nlen <= flen) ? 0u", "(nlen < dlen && nlen < flen) ? 0u"),
    ("scan_fixed_strict", "deflate.hip", ": flen <= dlen ? 1u : 2u", ": flen < dlen ? 1u : 2u"),
    ("scan_q3_mod_8", "deflate.hip", "(uint64_t)(8 - ((pending + 3) % 8))", "(uint64_t)((8 - ((pending + 3) % 8)) % 8)"),
]
LANE_MUTANTS = [
    ("coder_choose_stored_strict", "deflate_lane.h",
     "  if (nlen <= dlen && nlen <= flen) return 0;", "  if (nlen < dlen && nlen < flen) return 0;"),
    ("coder_choose_fixed_strict", "deflate_lane.h", "  if (flen <= dlen) return 1;", "  if (flen < dlen) return 1;"),
    ("coder_choose_q3_mod_8", "deflate_lane.h",
     "(uint64_t)(8 - ((pending_bits + 3) % 8))", "(uint64_t)((8 - ((pending_bits + 3) % 8)) % 8)"),
]
# (name, file, text, replacement, expected): stricter only, so safe on the GPU.  Expected: "killed"; "survives" (a span
# refusal: the plain step decodes the symbol); "host-only" (the serial header code -- setup_dynamic_lengths and the
# lane init_decoder -- which the kernels replace by wave_dynamic_lengths / wave_tables: killed in the host models);
# "unreached" (the plain step's check of a dynamic block's distance symbol 29: no rule case brings a distance 29 to the
# plain step on the GPU, where the wide table decodes it -- a gap, killed in the host models only)
INFLATE_GPU_MUTANTS = [
    ("lane_dist_eq_out_refused", "inflate_lane.h", "if (dist > d.out_pos) { d.fail", "if (dist >= d.out_pos) { d.fail", "killed"),
    ("lane_litlen_285_refused", "inflate_lane.h", "if (sym > d.lit_max_sym || sym > LITLEN_SYM_MAX) { d.fail",
     "if (sym > d.lit_max_sym || sym >= LITLEN_SYM_MAX) { d.fail", "killed"),
    ("lane_dist_29_refused", "inflate_lane.h", "dsym > d.dist_max_sym || dsym > DIST_SYM_MAX) { d.fail",
     "dsym > d.dist_max_sym || dsym >= DIST_SYM_MAX) { d.fail", "unreached"),
    ("lane_fixed_litlen_285_refused", "inflate_lane.h", "if (sym > LITLEN_SYM_MAX) { d.fail(ST_CORRUPTED); return SYM_STOP; }",
     "if (sym >= LITLEN_SYM_MAX) { d.fail(ST_CORRUPTED); return SYM_STOP; }", "killed"),
    ("lane_fixed_dist_29_refused", "inflate_lane.h", "if (dsym > DIST_SYM_MAX) { d.fail", "if (dsym >= DIST_SYM_MAX) { d.fail", "killed"),
    ("lane_hlit_286_refused", "inflate_lane.h", "if (hlit > 286 || hdist > 30)", "if (hlit > 285 || hdist > 30)", "killed"),
    ("lane_hdist_30_refused", "inflate_lane.h", "if (hlit > 286 || hdist > 30)", "if (hlit > 286 || hdist > 29)", "killed"),
    ("lane_cl16_second_refused", "inflate_lane.h", "if (num == 0) return -1;  // zd.ml:653", "if (num <= 1) return -1;", "host-only"),
    ("lane_repeat_to_end_refused", "inflate_lane.h", "if (repeat > (uint32_t)(total - num)) return -1;",
     "if (repeat >= (uint32_t)(total - num)) return -1;", "host-only"),
    ("lane_eob_length_1_refused", "inflate_lane.h", "if (L.u16(LDS_LENGTHS, 256) == 0) return -1;",
     "if (L.u16(LDS_LENGTHS, 256) <= 1) return -1;", "host-only"),
    ("lane_single_code_refused", "inflate_lane.h", "(num_codes == 1 && L.u16(counts_off, 1) != 1))\n    return false;",
     "(num_codes == 1))\n    return false;", "host-only"),
    ("lane_stored_len_eq_input_refused", "inflate_lane.h", "if (d.src_len - pos < length)", "if (d.src_len - pos <= length)", "killed"),
    ("lane_stored_header_5", "inflate_lane.h", "d.src_len - pos < 4)", "d.src_len - pos < 5)", "killed"),
    ("wave_single_code_refused", "inflate.hip", "(num_codes == 1 && L.u16(counts_off, 1) != 1)) return false;",
     "(num_codes == 1)) return false;", "killed"),
    ("wave_tables_empty_code_refused", "inflate.hip", "(job == 0 && max_sym == -1)) {", "(max_sym == -1)) {", "killed"),
    ("wave_cl16_second_refused", "inflate.hip", "(sym == 16u && start == 0u)", "(sym == 16u && start <= 1u)", "killed"),
    ("wave_repeat_to_end_refused", "inflate.hip", "repeat > total - start);", "repeat >= total - start);", "killed"),
    ("wave_eob_length_1_refused", "inflate.hip", "if (L.u16(LDS_LENGTHS, 256) == 0) return -1;",
     "if (L.u16(LDS_LENGTHS, 256) <= 1) return -1;", "killed"),
    ("span_refuses_the_top_litlen_symbol", "inflate_span.h", "sym > lit_max_sym || sym > LITLEN_SYM_MAX) {",
     "sym >= lit_max_sym || sym > LITLEN_SYM_MAX) {", "survives"),
    ("span_refuses_the_top_dist_symbol", "inflate_span.h", "dsym > dist_max_sym || dsym > DIST_SYM_MAX) {",
     "dsym >= dist_max_sym || dsym > DIST_SYM_MAX) {", "survives"),
]
# the host models' copies: the inflate_lane.h mutants above, and relaxed ones (accept more) that stay in bounds
LANE_INFLATE_MUTANTS = [m[:4] for m in INFLATE_GPU_MUTANTS if m[1] == "inflate_lane.h"]
LANE_INFLATE_RELAXED = [
    ("lane_nlen_unchecked", "inflate_lane.h", "if (length != ((~inv) & 0xFFFFu))", "if (0 && length != ((~inv) & 0xFFFFu))"),
    ("lane_single_code_any_length", "inflate_lane.h",
     "if ((num_codes > 1 && available > 0) || (num_codes == 1 && L.u16(counts_off, 1) != 1))",
     "if (num_codes > 1 && available > 0)"),
    ("lane_incomplete_ok", "inflate_lane.h",
     "if ((num_codes > 1 && available > 0) || (num_codes == 1 && L.u16(counts_off, 1) != 1))",
     "if (num_codes == 1 && L.u16(counts_off, 1) != 1)"),
]
# (name, file, text, replacement, killer): one-line mutants of the Adler-32 chunk chain's arithmetic, killed on the CPU only --
# each built into a host model of its own (tests/host_sim/sim_adler.cpp) and run in a child process by
# tests/test_adler_chain_sim.py::test_adler_chain_mutants_are_killed.  killer: the case of tests/checksum_cases.py
# mutation_cases() whose result it must change, or ("equivalent", why): it must change none.
# (The ambiguity bounds the other way -- `<=` for `<` -- only replay a chunk more: equivalent by construction, not listed.)
ADLER_MUTANTS = [
    ("amb_low_bound_less_1", "adler_chain.h", "return C < ADLER_BASE ||", "return C < ADLER_BASE - 1 ||",
     ("equivalent", "|s2| <= 65520, so a chunk with C = 65520 never goes negative: the bound is one wider than it must be")),
    ("amb_low_bound_less_2", "adler_chain.h", "return C < ADLER_BASE ||", "return C < ADLER_BASE - 2 ||", "low_bound_stays_negative_last"),
    ("amb_mid_lower_bound_plus_1", "adler_chain.h", "(C > 0x80000000ull - ADLER_BASE &&", "(C > 0x80000000ull - ADLER_BASE + 1 &&",
     "mid_lower_bound"),
    ("amb_mid_upper_bound_less_1", "adler_chain.h", "C < 0x80000000ull + ADLER_BASE);", "C < 0x80000000ull + ADLER_BASE - 1);",
     ("equivalent", "s2 >= -65520, so C = 2^31 + 65520 stays at or above 2^31: the bound is one wider than it must be")),
    ("amb_mid_upper_bound_less_2", "adler_chain.h", "C < 0x80000000ull + ADLER_BASE);", "C < 0x80000000ull + ADLER_BASE - 2);",
     "mid_upper_bound"),
    ("a_term_without_225", "adler_chain.h", "hi_k ? ADLER_BASE - 225u : 0u", "hi_k ? 0u : 0u", "ff_chunks"),
    ("hi_k_strict", "adler_chain.h", "return C >= 0x80000000ull;", "return C > 0x80000000ull;",
     ("equivalent", "C = 2^31 is ambiguous: the chunk is replayed exactly, its a term is taken back out by the same function, "
                    "and the branch of an ambiguous chunk is read by nobody (the next chunk takes exact_next or does not care)")),
    ("zero_residue_negative", "adler_chain.h", "(rr == 0 ? 0 : (int32_t)rr - (int32_t)ADLER_BASE)", "((int32_t)rr - (int32_t)ADLER_BASE)",
     "zero_behind_hi_then_mid"),
    ("exact_at_ignored", "adler_chain.h", "k == st.exact_at ? st.exact_next : adler_signed_s2(rr, prev)", "adler_signed_s2(rr, prev)",
     "adjacent_exact"),
    ("prev_branch_no_walk_back", "adler_chain.h", "  while (run >= 0 && run_last_hi[run] == 0xFFFFFFFFu) run--;\n", "",
     ("equivalent", "run (k - 1) / per holds chunk k - 1, so it is never empty: the walk back never takes a step")),
    ("prev_branch_of_k", "adler_chain.h", "int64_t run = (int64_t)((k - 1) / per);", "int64_t run = (int64_t)(k / per);",
     "opens_run_behind_hi"),
    ("delta_not_carried", "adler_chain.h", "const uint32_t rr = addmod(res, st.delta);", "const uint32_t rr = addmod(res, 0u);",
     "delta_carried"),
    ("final_without_delta", "adler_chain.h", "(total_res + st.delta) % ADLER_BASE", "(total_res + 0u) % ADLER_BASE", "mid_upper_bound"),
    ("final_ignores_exact_at", "adler_chain.h", "if (st.exact_at == n_chunks) final_s2", "if (false && st.exact_at == n_chunks) final_s2",
     "low_bound_stays_negative_last"),
    ("fallback_at_the_limit", "adler_chain.h", "n_amb > amb_cap || n_amb > replay_max", "n_amb > amb_cap || n_amb >= replay_max",
     "replay_at_its_limit"),
    ("per_rounded_down", "adler_chain.h", "(n_chunks + n_runs - 1) / n_runs : 1", "n_chunks / n_runs : 1", "ten_chunks_four_runs"),
    ("rfc_chain_bytes_not_reduced", "adler_chain.h", "(nb[i] % ADLER_BASE) * c1", "nb[i] * c1",
     ("equivalent", "a run's bytes stay below 2^37 for any length the launches take and c1 < 2^16: the 64-bit product cannot wrap")),
]
# (name, file, text, replacement, killer): one-line mutants of the many-stream forms' plan (host_pipeline.h plan_many), killed on
# the CPU only -- each built into a model of its own (tests/host_sim/sim_many.cpp) by
# tests/test_many_plan.py::test_plan_mutants_are_killed.  killer: the row of that file's ROWS it must fail.  A wrong cut still
# gives right bytes: no parity test would notice any of these.
MANY_PLAN_MUTANTS = [
    ("taper_shares_not_doubled", "host_pipeline.h", "taper ? 2 * g - 1 : g;", "taper ? g : g;", "taper_K4"),
    ("taper_divides_by_K", "host_pipeline.h", "so / shares * before", "so / K * before", "taper_K4"),
    ("shrink_either_clause", "host_pipeline.h", "n / K < least && so / K < least * 65536", "n / K < least || so / K < least * 65536",
     "shrink_bytes_at_the_limit"),
    ("slot_without_its_gap", "host_pipeline.h", "return (len + 255) / 256 * 256 + 256;", "return (len + 255) / 256 * 256;", "slots"),
    ("mid_off_runs_on", "host_pipeline.h", "uint64_t mo = 0;", "uint64_t mo = p.mid_arena;", "recode_mid_arena"),
    ("six_from_two_gib", "host_pipeline.h", "staged_bytes >= ((uint64_t)1 << 30)", "staged_bytes >= ((uint64_t)1 << 31)", "count_at_a_gib"),
]
# (name, file, text, replacement, killer): one-line mutants of inflate's ROOM -- where a stream's bytes may go and when it
# is refused for want of room -- killed on the CPU only, by tests/test_inflate_room_rules.py::test_room_mutants_are_killed:
# each is built into a host model of its own and run in a child process over the items of tests/inflate_room_cases.py.
# killer: (the host model's mode, the item that must fail), or ("equivalent", why): no item may fail in any mode.
# THESE MUTANTS WRITE OUT OF THEIR ROOM BY DESIGN (up to 15 bytes; the test's 64-byte guards hold that inside its own
# buffer).  They are never built into a GPU library: they are in no list that --build or a GPU run reads, and must not be.
# Each runs in the ONE mode its entry names: the two literal mutants leave out_pos one past cap_min, and the wide turn's
# `cap_min - out_pos` would then wrap (its child would write all over its heap) -- "plain" decodes symbol by symbol.
ROOM_MUTANTS = [
    ("lane_copy_gate_without_its_8", "inflate_lane.h", "(uint64_t)pos + len + 8 <= hard_cap", "(uint64_t)pos + len <= hard_cap",
     ("plain", "lane/L9_d8_g0/R=79/limit R, cap R")),
    ("span_flush_quad_over_the_tail", "inflate_span.h", "if (i + 16u <= tile_len) {", "if (i < tile_len) {", ("span_a", "span/skewed_k5_d17/R=10220/no limit, cap R")),
    ("lane_literal_at_cap_min", "inflate_lane.h", "\n      if (d.out_pos >= d.cap_min) { d.overflow(",
     "\n      if (d.out_pos > d.cap_min) { d.overflow(", ("plain", "literal_last/n20000/R=19999/no limit, cap R")),
    ("lane_fixed_literal_at_cap_min", "inflate_lane.h", "\n    if (d.out_pos >= d.cap_min) { d.overflow(",
     "\n    if (d.out_pos > d.cap_min) { d.overflow(", ("plain", "literal_last/n1/R=0/no limit, cap R")),
    ("lane_match_to_cap_min_refused", "inflate_lane.h",
     "if ((uint64_t)d.out_pos + length > d.cap_min) { d.overflow((uint64_t)d.out_pos + length); return SYM_STOP; }",
     "if ((uint64_t)d.out_pos + length >= d.cap_min) { d.overflow((uint64_t)d.out_pos + length); return SYM_STOP; }",
     ("plain", "lane/L3_d1_g0/R=73/limit R, cap R")),
    ("lane_stored_to_cap_min_refused", "inflate_lane.h",
     "if ((uint64_t)d.out_pos + length > d.cap_min) { d.overflow((uint64_t)d.out_pos + length); return true; }",
     "if ((uint64_t)d.out_pos + length >= d.cap_min) { d.overflow((uint64_t)d.out_pos + length); return true; }",
     ("plain", "stored/len16_behind0/R=16/limit R, cap R")),
    ("cap_min_from_hard_cap_alone", "inflate_lane.h", "d.cap_min = d.limit < d.hard_cap ? d.limit : d.hard_cap;", "d.cap_min = d.hard_cap;",
     ("plain", "lane/L9_d8_g5/R=83/limit R, cap R+40")),
    ("span_far_pass_ungated", "inflate_span.h", "if (out_pos + 32u <= hard_cap && wv::any(has_far != 0u)) {", "if (wv::any(has_far != 0u)) {",
     ("equivalent", "the gate keeps 16-byte LOADS of far sources inside the room; the pass stores into the tile (LDS) only, and what it "
                    "does not fetch the rounds behind it copy: the host model, whose guards are readable, gives the same bytes")),
]
# (name, file, text, replacement, killer): one-line mutants of the TOKEN parts of the span decoder (inflate_span.h: what a byte of a
# match is written down as a copy of), killed on the CPU only and never built for the GPU, in the manner of ROOM_MUTANTS: each is
# built into a host model of its own and run in child processes by tests/test_token_rules.py::test_token_mutants_are_killed, which
# holds every word of tok[] to tests/token_ref.py.  killer: the stream of tests/token_cases.py whose words it must break, or
# ("equivalent", why): it must break none.  The test prints per mutant whether the BYTES alone would have caught it.
TOKEN_MUTANTS = [
    ("follow_from_off_by_one", "inflate_span.h", "const uint32_t from = dp + 32768u - dist;", "const uint32_t from = dp + 32767u - dist;",
     "len_dist_grid"),
    ("follow_in_tile_test_strict", "inflate_span.h", "if (sp >= 32768u && (mbits[(sp - 32768u) >> 5] >> (sp & 31u)) & 1u)",
     "if (sp > 32768u && (mbits[(sp - 32768u) >> 5] >> (sp & 31u)) & 1u)",
     ("equivalent", "(tile_edges has sources that begin at a tile's first byte) sp == 32768 is tile position 0: not following it inside the tile leaves the byte a copy of tile byte 0, a byte of "
                    "the same chain one link further from the literal -- a longer way, never a wrong one")),
    ("follow_sweep_test_strict", "inflate_span.h", "v[u] = sp >= 32768u ? out_pos", "v[u] = sp > 32768u ? out_pos",
     ("equivalent", "sp == 32768 then reads tok[out_pos], the word of tile byte 0 itself: out_pos while nobody has written it, or what "
                    "tile byte 0 is a copy of -- the same chain either way")),
    ("follow_wrap_dropped", "inflate_span.h", "r = r + 1u == dist ? 0u : r + 1u;", "r = r + 1u;",
     ("equivalent", "without the wrap byte i >= dist of an overlapping match is written down as a copy of byte i - dist of the match "
                    "itself, which is src[i] to the letter: one link more per period, the same chain")),
    ("plain_source_not_advanced", "inflate_span.h", "tok[at + i] = from + i;", "tok[at + i] = from;", "len_dist_grid"),
    ("follow_step_reads_the_neighbour", "inflate_span.h", "srcpos[b] = srcpos[sp - 32768u];", "srcpos[b] = srcpos[sp - 32767u];",
     "len_dist_grid"),
    ("follow_store_inverted", "inflate_span.h", "if (v[u] != out_pos + b) tok[out_pos + b] = v[u];",
     "if (v[u] == out_pos + b) tok[out_pos + b] = v[u];", "len_dist_grid"),
]
# what runs against each GPU mutant: the vectors under the default form, then under every override (one process each)
TESTS = "tests/test_gpu_parity.py"
SELECT = "second_readings_vectors"
INFLATE_TESTS = "tests/test_gpu_inflate_rules.py"


def mutated_tree(mutant, into):
    """copies of zipc_amd/csrc and include/ under `into` (the relative includes resolve), one mutant applied"""
    name, fname, old, new = mutant[:4]
    csrc = os.path.join(into, "zipc_amd", "csrc")
    shutil.copytree(CSRC, csrc, ignore=shutil.ignore_patterns("build"))
    shutil.copytree(os.path.join(ROOT, "include"), os.path.join(into, "include"))
    path = os.path.join(csrc, fname)
    text = open(path).read()
    n = text.count(old)
    if n != 1:
        raise SystemExit("%s: %r occurs %d times in %s, not once" % (name, old, n, fname))
    with open(path, "w") as f:
        f.write(text.replace(old, new))
    return csrc


def makefile_units():
    """the units zipc_amd/csrc/Makefile links into libzipc_hip.so (its SRCS line): the library does not load without one of them"""
    m = re.search(r"^SRCS\s*:?=\s*(.+)$", open(os.path.join(CSRC, "Makefile")).read(), re.M)
    units = [w[:-4] for w in m.group(1).split() if w.endswith(".hip")]
    assert "inflate" in units and "deflate" in units, units
    return units


def build(mutant):
    """libzipc_hip.so with the mutated unit (deflate.hip, or inflate.hip for the inflate files) and the product's other
    objects -> its path"""
    name = mutant[0]
    unit = "inflate" if mutant[1].startswith("inflate") else "deflate"
    so = os.path.join(OUT, "libzipc_hip_%s.so" % name)
    with tempfile.TemporaryDirectory() as tmp:
        csrc = mutated_tree(mutant, tmp)
        obj = os.path.join(tmp, unit + ".o")
        subprocess.run([HIPCC] + HIPFLAGS + ["-c", os.path.join(csrc, unit + ".hip"), "-o", obj], check=True)
        others = [os.path.join(CSRC, "build", o + ".o") for o in makefile_units() if o != unit]
        os.makedirs(OUT, exist_ok=True)
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", so, obj] + others, check=True)
    return so


def run(name, so, tests=TESTS, select=SELECT):
    """the vector tests against one mutant library: -> (killed, the failing test)"""
    env = dict(os.environ, ZIPC_HIP_LIB=so)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-rf", "-m", "gpu", "-p", "no:cacheprovider", tests]
                       + (["-k", select] if select else []), cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=1200)
    out = r.stdout.decode()
    if r.returncode < 0 or r.returncode in (134, 139):  # an abort or a fault is not a kill: start nothing more
        sys.stderr.write(out[-3000:])
        raise SystemExit("%s: the test process ended with status %d; stopping" % (name, r.returncode))
    failed = re.findall(r"^FAILED (\S+)(.*)$", out, re.M)
    if r.returncode == 0:
        return False, "-"
    if not failed:  # not a test failure (an import or collection error): not a kill
        sys.stderr.write(out[-3000:])
        return False, "error rc %d" % r.returncode
    test, why = failed[0]
    return True, "%s%s" % (test.split("::")[-1], why[:100])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--build", action="store_true", help="build the mutant libraries only")
    ap.add_argument("--inflate", action="store_true", help="the inflate mutants (INFLATE_GPU_MUTANTS)")
    ap.add_argument("only", nargs="*", help="mutant names (default: all)")
    a = ap.parse_args()
    subprocess.run(["make", "-s", "-C", CSRC, "-j4", "all"], check=True)
    table = INFLATE_GPU_MUTANTS if a.inflate else [m + ("killed",) for m in GPU_MUTANTS]
    mutants = [m for m in table if not a.only or m[0] in a.only]
    sos = {}

    def one(m):  # (built once, before the GPU run: a run uses what --build left)
        so = os.path.join(OUT, "libzipc_hip_%s.so" % m[0])
        return build(m) if a.build or not os.path.exists(so) else so

    import concurrent.futures
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
        for m, so in zip(mutants, ex.map(one, mutants)):
            sos[m[0]] = so
    if a.build:
        print("\n".join(sos.values()))
        return 0
    rows = []
    for m in mutants:
        if a.inflate:  # killers: the rule tests in this process; the expected survivors also under every override
            killed, by = run(m[0], sos[m[0]], INFLATE_TESTS, "not overrides" if m[4] == "killed" else None)
        else:
            killed, by = run(m[0], sos[m[0]])
        rows.append((m[0], m[4], killed, by))
        print("%-36s %-9s %s" % (m[0], "killed" if killed else "SURVIVED", by), flush=True)
    wrong = [n for n, want, k, _ in rows if k != (want == "killed")]
    print("\nkernel %s mutants: %d of %d as expected, %d not" % ("inflate" if a.inflate else "chooser", len(rows) - len(wrong),
                                                              len(rows), len(wrong)))
    print("  %-36s %-9s %-9s %s" % ("mutant", "expected", "got", "first failing test"))
    for n, want, k, by in rows:
        print("  %-36s %-9s %-9s %s" % (n, want, "killed" if k else "survived", by))
    return 1 if wrong else 0


if __name__ == "__main__":
    sys.exit(main())
