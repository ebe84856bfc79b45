"""What the mutation tests share: a one-line change of a text that must match exactly once, the g++ line, the builds of
a host model over a mutated copy of the kernels' headers, a child process that prints JSON, and the rule of a kill
table -- a named killer must change, an equivalent mutant must change nothing.  A plain module: no fixtures, no pytest
settings.  The tables, their judges' own columns and what they print stay with the tests that run them."""
import concurrent.futures
import json
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def patched(text, old, new, where):
    """`text` with `old` replaced by `new`; `old` must occur exactly once, or the mutant would be a silent no-op"""
    n = text.count(old)
    if n != 1:
        raise AssertionError("%s: the mutant's text occurs %d times, not once: %r" % (where, n, old[:80]))
    return text.replace(old, new)


def workers():
    """the width of every pool of builds or children (a run may use 16 CPUs however many the machine has)"""
    return min(16, os.cpu_count() or 1)


def gxx(out, sources, *, shared=True, opt="-O2", include=(), defines=(), extra=()):
    """the one g++ line: `sources` into the shared library (or the program) `out` -> out"""
    cmd = ["g++", opt, "-std=c++17"] + (["-fPIC", "-shared"] if shared else []) + list(extra)
    for d in include:
        cmd += ["-I", str(d)]
    subprocess.run(cmd + ["-D" + d for d in defines] + ["-o", str(out)] + [str(s) for s in sources], check=True)
    return str(out)


def host_model(mutant, into):
    """libhost_sim.so of every file of tests/host_sim, copied under `into` beside tools/kernel_mutants.py's mutated tree (so
    that the models' relative includes find the mutated header) -> its path"""
    import host_sim
    from tools import kernel_mutants as KM

    KM.mutated_tree(mutant, str(into))
    sim_dir = os.path.join(str(into), "tests", "host_sim")
    os.makedirs(sim_dir)
    for f in os.listdir(host_sim.HERE):
        if f.endswith((".cpp", ".h")):
            shutil.copy(os.path.join(host_sim.HERE, f), sim_dir)
    return gxx(os.path.join(sim_dir, "libhost_sim.so"), [os.path.join(sim_dir, s) for s in host_sim.SRCS], include=[sim_dir],
               extra=["-Wno-unknown-pragmas"])


def single_model(sim_cpp, header_name, csrc_dir, so):
    """one file of tests/host_sim alone, its include of zipc_amd/csrc/`header_name` pointed at the copy in `csrc_dir` -> so"""
    src = patched(open(sim_cpp).read(), '#include "../../zipc_amd/csrc/%s"' % header_name,
                  '#include "%s"' % os.path.join(csrc_dir, header_name), sim_cpp)
    cpp = so[:-3] + ".cpp"
    with open(cpp, "w") as f:
        f.write(src)
    return gxx(so, [cpp], opt="-O1", extra=["-Wno-unknown-pragmas"])


def header_model(sim_cpp, define, header, line, mutated, so, rewrite_includes=(), top=None, **flags):
    """a model that takes its header's path from -D`define`, over a copy of `header` beside `so` with `line` changed -> so.
    rewrite_includes: quoted includes of the header that are to find the file beside the original.  top: the header `define`
    names where the mutant is of one IT includes: copied there too, its quoted includes look beside it first."""
    d = os.path.dirname(so)
    os.makedirs(d, exist_ok=True)
    src = patched(open(header).read(), line, mutated, header)
    for inc in rewrite_includes:
        src = patched(src, '#include "%s"' % inc, '#include "%s"' % os.path.join(os.path.dirname(header), inc), header)
    if top:
        shutil.copy(top, d)
    with open(os.path.join(d, os.path.basename(header)), "w") as f:
        f.write(src)
    return gxx(so, [sim_cpp], defines=['%s="%s"' % (define, os.path.join(d, os.path.basename(top or header)))], **flags)


def build_all(fn, items):
    """[fn(item)] side by side"""
    with concurrent.futures.ThreadPoolExecutor(max_workers=workers()) as ex:
        return list(ex.map(fn, items))


def run_child(code, *args, env=None, timeout=900, every_line=False):
    """python -c `code` `args` -> (return code, what its last line of output says as JSON or None, the end of its stderr).
    every_line: every JSON list it printed, not the last alone (a child that may end early prints as it goes).  What a
    return code other than 0 means is the caller's to say."""
    r = subprocess.run([sys.executable, "-c", code] + [str(a) for a in args], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=timeout)
    lines = r.stdout.decode().strip().splitlines()
    try:
        said = [json.loads(ln) for ln in lines if ln.startswith("[")] if every_line else json.loads(lines[-1])
    except (IndexError, ValueError):
        said = None
    return r.returncode, said, r.stderr.decode()[-2000:]


def verdict(killer, changed, crashed=False):
    """is a mutant's row as its table says?  A named killer must be among `changed`; ("equivalent", why) must have changed
    nothing, in a child that ran to its end."""
    if isinstance(killer, tuple) and killer[0] == "equivalent":
        return not changed and not crashed
    return killer in changed
