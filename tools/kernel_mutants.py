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
override) passing under them is what shows the hand-off right.

Every table here is one a GPU library may be built from.  LANE_MUTANTS and LANE_INFLATE_MUTANTS are the host models'
copies of the GPU ones, killed on the CPU by tests/test_host_sim.py (test_coder_choose_mutants_are_killed,
test_inflate_lane_mutants_are_killed).  Mutants that only ever run in a host model on the CPU -- relaxed checks, the
Adler-32 chunk chain, the many-stream plan, inflate's destination room, the span decoder's tokens -- are tables of the tests
that run them (tests/test_host_sim.py, test_adler_chain_sim.py, test_many_plan.py, test_inflate_room_rules.py,
test_token_rules.py); they share mutated_tree through tests/mutation.py and nothing else of this file.
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
# the host models' copies: the inflate_lane.h mutants above
LANE_INFLATE_MUTANTS = [m[:4] for m in INFLATE_GPU_MUTANTS if m[1] == "inflate_lane.h"]
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
