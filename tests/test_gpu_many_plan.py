"""The library's many-stream calls run the plan of zipc_amd/csrc/host_pipeline.h plan_many: what a call prints under
ZIPC_HIP_HOST_TIMING=1 -- its streams, the ends of its staging arenas, its sub-batches and how many streams each holds --
equals what tests/host_sim's sim_many_plan gives for the same lengths (tests/test_many_plan.py holds that function to rows
written out by hand).  A wrong cut still gives right bytes, so the bytes are held to the oracle beside it.  The settings are
read once per process: every case is a child process of its own."""
import os
import pickle
import random
import re
import subprocess
import sys
import zlib

import pytest

import util
import host_sim

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(util.HERE)
LEVEL = 2

_CHILD = r"""
import ctypes as C, pickle, sys
sys.path.insert(0, sys.argv[3])
import numpy as np
import zipc_amd
from zipc_amd import _lib

job = pickle.load(open(sys.argv[1], "rb"))
lib, ctx = _lib.lib(), zipc_amd.Context(0)
n = len(job["plain"])
def srcs(datas):
    keep = [np.frombuffer(d, np.uint8) if d else np.zeros(1, np.uint8) for d in datas]
    return keep, (C.c_void_p * n)(*[a.ctypes.data for a in keep]), (C.c_size_t * n)(*[len(d) for d in datas])
def dsts(caps):
    keep = [np.full(c + 16, 0xA5, np.uint8) for c in caps]
    return keep, (C.c_void_p * n)(*[a.ctypes.data for a in keep]), (C.c_size_t * n)(*caps)
def taken(res, bufs, caps):
    assert all(bool((b[c:] == 0xA5).all()) for b, c in zip(bufs, caps)), "bytes behind a capacity"
    return [(int(r.status), int(r.checksum), bufs[i][:int(r.out_len)].tobytes()) for i, r in enumerate(res)]
out = {}
sizes = (C.c_size_t * n)(*[len(d) for d in job["plain"]])
k1, sp, sl = srcs(job["plain"])
d1, dp, dc = dsts(job["deflate_caps"])
res = (_lib.StreamResult * n)()
out["deflate_status"] = lib.zipc_hip_deflate_many(ctx.handle, n, sp, sl, job["level"], 1, dp, dc, res)
out["deflate"] = taken(res, d1, job["deflate_caps"])
k2, cp, cl = srcs(job["comp"])
d2, ip, ic = dsts([len(d) for d in job["plain"]])
res = (_lib.StreamResult * n)()
out["inflate_status"] = lib.zipc_hip_inflate_many(ctx.handle, n, cp, cl, sizes, 1, ip, ic, res)
out["inflate"] = taken(res, d2, [len(d) for d in job["plain"]])
d3, rp, rc = dsts(job["recode_caps"])
rres = (_lib.RecodeResult * n)()
out["recode_status"] = lib.zipc_hip_recode_many(ctx.handle, n, cp, cl, sizes, (C.c_uint32 * n)(*job["crcs"]), sizes, job["level"], rp, rc, rres)
out["recode"] = taken(rres, d3, job["recode_caps"])
out["recode_more"] = [(int(r.mid_len), int(r.stage)) for r in rres]
pickle.dump(out, open(sys.argv[2], "wb"))
"""


@pytest.fixture(scope="module")
def job(oracle):
    """29 streams of 0 to 3000 bytes and one of 70 000 among them, as the oracle deflates them: computed once, never changed"""
    rnd = random.Random(29)
    lens = [rnd.randrange(0, 3001) for _ in range(29)]
    lens[3], lens[17] = 0, 70000
    plain = [bytes(util.text(ln, i)) if i % 3 else bytes(util.rand_bytes(ln, i, 3)) for i, ln in enumerate(lens)]
    fast = [oracle.deflate(d, level=1)[1] for d in plain]  # what inflate and recode are handed
    want = [oracle.deflate(d, level=LEVEL)[1] for d in plain]
    caps = [oracle.deflate_bound(len(d)) for d in plain]
    return dict(plain=plain, comp=fast, want=want, crcs=[zlib.crc32(d) for d in plain], deflate_caps=caps, recode_caps=caps, level=LEVEL)


def _printed(stderr, form):
    """(n, src_arena, dst_arena, sub-batches, [(g, streams)]) of the one call of that form"""
    lines = stderr.splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith("zipc_hip %s_many " % form)]
    assert len(at) == 1, (form, stderr[-3000:])
    m = re.match(r"zipc_hip \w+_many n=(\d+) src_arena=(\d+) dst_arena=(\d+) ms: .*\(threads \d+ sub-batches (\d+)\)$", lines[at[0]])
    assert m, lines[at[0]]
    subs = []
    for ln in lines[at[0] + 1:]:
        s = re.match(r"  sub-batch (\d+) \((\d+) streams\): ", ln)
        if not s:
            break
        subs.append((int(s.group(1)), int(s.group(2))))
    return tuple(int(v) for v in m.groups()) + (subs,)


def _planned(p, n):
    cut = p["cut"]
    return (n, p["src_arena_end"], p["dst_arena_end"], p["K"], [(g, cut[g + 1] - cut[g]) for g in range(p["K"]) if cut[g + 1] > cut[g]])


@pytest.mark.parametrize("chunks", [None, 3, 2], ids=["chunks-unset", "chunks-3", "chunks-2"])
def test_the_calls_run_the_plan_of_the_header(job, chunks, tmp_path):
    env = dict(os.environ, ZIPC_HIP_HOST_TIMING="1", ZIPC_HIP_HOST_CHUNK_MIN="2")
    env.pop("ZIPC_HIP_HOST_CHUNKS", None)
    if chunks is not None:
        env["ZIPC_HIP_HOST_CHUNKS"] = str(chunks)
    job_path, out_path = str(tmp_path / "job.pickle"), str(tmp_path / "out.pickle")
    with open(job_path, "wb") as f:
        pickle.dump(job, f)
    r = subprocess.run([sys.executable, "-c", _CHILD, job_path, out_path, ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    with open(out_path, "rb") as f:
        out = pickle.load(f)
    n = len(job["plain"])
    # ---- the bytes, against the oracle
    assert (out["deflate_status"], out["inflate_status"], out["recode_status"]) == (0, 0, 0)
    for i, d in enumerate(job["plain"]):
        assert out["deflate"][i] == (0, job["crcs"][i], job["want"][i]), ("deflate", i)
        assert out["inflate"][i] == (0, job["crcs"][i], d), ("inflate", i)
        assert out["recode"][i] == (0, job["crcs"][i], job["want"][i]) and out["recode_more"][i] == (len(d), 0), ("recode", i)
    # ---- the plan, against the header's
    L = host_sim.lib()
    sizes, comp = [len(d) for d in job["plain"]], [len(c) for c in job["comp"]]
    kw = dict(chunks=chunks or 0, chunk_min=2)
    plans = {"deflate": host_sim.many_plan(L, host_sim.MANY_DEFLATE, sizes, job["deflate_caps"], **kw),
             "inflate": host_sim.many_plan(L, host_sim.MANY_INFLATE, comp, sizes, limit=sizes, **kw),
             "recode": host_sim.many_plan(L, host_sim.MANY_RECODE, comp, job["recode_caps"], limit=sizes, mid_cap=sizes, expect_crc32=job["crcs"], **kw)}
    for form, p in plans.items():
        print(form, _printed(r.stderr, form))
        assert _printed(r.stderr, form) == _planned(p, n), form
    assert plans["deflate"]["K"] == (chunks or 4)  # (29 streams hold 2 a sub-batch: the count is the setting's)
