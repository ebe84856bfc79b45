#!/usr/bin/env python3
"""Line-attributed instruction counts of a kernel's loops, from device assembly made with
  hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S -gline-tables-only X.hip -o X.s

  tools/asm_loop_counts.py X.s KERNEL FILE:LO-HI [FILE:LO-HI ...] [--skip FILE:LO-HI ...] [--lines]

For every source range given (say inflate_span.h:308-359, the walk loop) the innermost loops of KERNEL (the
compiler's own "Loop Header" / "in Loop: Header=" comments) that hold instructions of those lines are listed with
their vector, scalar, LDS, memory, branch and wait instructions.  Blocks of a loop most of whose instructions come
from a --skip range (the rare, divergent forms: span_symbol_slow) are counted apart: the wave jumps over them.
--lines adds the count per source line.  A static count: what one trip through the loop's common path issues."""
import collections
import re
import sys


def klass(op):
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith(("s_waitcnt", "s_nop", "s_barrier", "s_sleep")):
        return "wait"
    if op.startswith("s_load") or op.startswith("s_buffer_load"):
        return "smem"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("v_"):
        return "valu"
    return "other"


def parse_range(s):
    f, r = s.split(":")
    lo, hi = r.split("-")
    return f, int(lo), int(hi)


def main():
    args = sys.argv[1:]
    per_line = "--lines" in args
    args = [a for a in args if a != "--lines"]
    skip = []
    if "--skip" in args:
        i = args.index("--skip")
        skip = [parse_range(a) for a in args[i + 1:]]
        args = args[:i]
    path, kernel, wants = args[0], args[1], [parse_range(a) for a in args[2:]]
    blocks = []  # {label, header, depth, insts: [(op, [(file, line), ...: where it was inlined])]}
    inside = False
    cur = None
    loc = []
    fn = "0"
    for raw in open(path):
        if not inside:
            if re.match(r"_Z\w*%s\w*:" % re.escape(kernel), raw):
                inside = True
                cur = {"label": "entry", "header": None, "depth": 0, "insts": []}
                blocks.append(cur)
            continue
        if raw.startswith(".Lfunc_end"):
            break
        m = re.match(r"\.Lfunc_begin(\d+):", raw)
        if m:
            fn = m.group(1)
            continue
        m = re.match(r"\.L(BB\d+_\d+):", raw) or re.match(r"; %bb\.(\d+):", raw)
        if m:
            label = m.group(1) if m.group(1).startswith("BB") else "BB%s_%s" % (fn, m.group(1))
            cur = {"label": label, "header": None, "depth": 0, "insts": []}
            blocks.append(cur)
        m = re.search(r"; =>\s*This (?:Inner )?Loop Header: Depth=(\d+)", raw)
        if m and not cur["insts"]:
            cur["header"] = cur["label"]
            cur["depth"] = int(m.group(1))
            continue
        m = re.search(r";\s+in Loop: Header=(BB\d+_\d+) Depth=(\d+)", raw)
        if m and not cur["insts"]:
            cur["header"] = m.group(1)
            cur["depth"] = int(m.group(2))
            continue
        if raw.startswith((".LBB", "; %bb.")):
            continue
        m = re.match(r"\s*\.loc\s+\d+\s+\d+[^;]*;\s*(.*)", raw)
        if m:  # innermost first, then the places it was inlined at
            loc = [(c.split("/")[-1].split(":")[0], int(c.split(":")[1])) for c in re.findall(r"[\w./+-]+:\d+:\d+", m.group(1))]
            continue
        m = re.match(r"\s+([a-z][a-z0-9_]+)\b", raw)
        if m and not raw.lstrip().startswith((";", ".")):
            cur["insts"].append((m.group(1), loc))

    def within(chain, ranges):
        return any(f == rf and lo <= ln <= hi for f, ln in chain for rf, lo, hi in ranges)

    def place(chain, want):  # the line of the wanted range the instruction was inlined into, or its own
        for f, ln in chain:
            if f == want[0] and want[1] <= ln <= want[2]:
                return f, ln
        return chain[0] if chain else ("?", 0)

    loops = collections.OrderedDict()
    for b in blocks:
        if b["header"] is not None:
            loops.setdefault(b["header"], []).append(b)
    for want in wants:
        print("== %s:%d-%d" % want)
        for header, bs in loops.items():
            hits = sum(1 for b in bs for op, ch in b["insts"] if within(ch, [want]))
            total = sum(len(b["insts"]) for b in bs)
            if hits == 0 or hits * 5 < total:
                continue
            common, rare = collections.Counter(), collections.Counter()
            lines = collections.Counter()
            for b in bs:
                n_skip = sum(1 for op, ch in b["insts"] if within(ch, skip))
                is_rare = b["insts"] and n_skip * 2 > len(b["insts"])
                for op, ch in b["insts"]:
                    (rare if is_rare else common)[klass(op)] += 1
                    if not is_rare:
                        lines[place(ch, want) + (klass(op),)] += 1
            order = ["valu", "salu", "lds", "vmem", "smem", "branch", "wait", "other"]
            print("loop %s depth %d blocks %d: common path %s | rare blocks %s" % (
                header, bs[0]["depth"], len(bs), " ".join("%s %d" % (k, common[k]) for k in order if common[k]),
                " ".join("%s %d" % (k, rare[k]) for k in order if rare[k]) or "-"))
            if per_line:
                by = collections.defaultdict(collections.Counter)
                for (f, ln, k), n in lines.items():
                    by[(f, ln)][k] += n
                for (f, ln), c in sorted(by.items()):
                    print("    %-16s %5d  %s" % (f, ln, " ".join("%s %d" % (k, c[k]) for k in order if c[k])))


main()
