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
# what runs against each GPU mutant: the vectors under the default form, then under every override (one process each)
TESTS = "tests/test_gpu_parity.py"
SELECT = "second_readings_vectors"


def mutated_tree(mutant, into):
    """copies of zipc_amd/csrc and include/ under `into` (the relative includes resolve), one mutant applied"""
    name, fname, old, new = mutant
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


def build(mutant):
    """libzipc_hip.so with the mutated deflate.hip and the product's other objects -> its path"""
    name = mutant[0]
    so = os.path.join(OUT, "libzipc_hip_%s.so" % name)
    with tempfile.TemporaryDirectory() as tmp:
        csrc = mutated_tree(mutant, tmp)
        obj = os.path.join(tmp, "deflate.o")
        subprocess.run([HIPCC] + HIPFLAGS + ["-c", os.path.join(csrc, "deflate.hip"), "-o", obj], check=True)
        others = [os.path.join(CSRC, "build", o + ".o") for o in ("api", "inflate", "checksum")]
        os.makedirs(OUT, exist_ok=True)
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", so, obj] + others, check=True)
    return so


def run(name, so):
    """the vector tests against one mutant library: -> (killed, the failing test)"""
    env = dict(os.environ, ZIPC_HIP_LIB=so)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-rf", "-m", "gpu", "-p", "no:cacheprovider", TESTS,
                        "-k", SELECT], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=3000)
    out = r.stdout.decode()
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
    ap.add_argument("only", nargs="*", help="mutant names (default: all)")
    a = ap.parse_args()
    subprocess.run(["make", "-s", "-C", CSRC, "-j4", "all"], check=True)
    mutants = [m for m in GPU_MUTANTS if not a.only or m[0] in a.only]
    sos = {}
    for m in mutants:  # (built once, before the GPU run: a run uses what --build left)
        so = os.path.join(OUT, "libzipc_hip_%s.so" % m[0])
        sos[m[0]] = build(m) if a.build or not os.path.exists(so) else so
    if a.build:
        print("\n".join(sos.values()))
        return 0
    rows = []
    for m in mutants:
        killed, by = run(m[0], sos[m[0]])
        rows.append((m[0], killed, by))
        print("%-28s %-9s %s" % (m[0], "killed" if killed else "SURVIVED", by), flush=True)
    survivors = [n for n, k, _ in rows if not k]
    print("\nkernel chooser mutants: %d of %d killed, %d surviving" % (len(rows) - len(survivors), len(rows), len(survivors)))
    for n, k, by in rows:
        print("  %-28s %-9s %s" % (n, "killed" if k else "SURVIVED", by))
    return 1 if survivors else 0


if __name__ == "__main__":
    sys.exit(main())
