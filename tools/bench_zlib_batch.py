#!/usr/bin/env python3
"""What the zlib container costs on the device: zipc_hip_zlib_compress_batch / _decompress_batch against
zipc_hip_deflate_batch / _inflate_batch with crc_op ADLER32 on the same data, in one process, at C2's shape (16 384
streams x 64 KiB of 4-bit symbols, `Default).  The four calls are timed in alternation, ROUNDS times over, each timing a
host clock around REPS enqueues and one synchronize (tools/bench_configs.py's way); the spread of the raw forms over the
rounds is what a ratio has to be read against.  One JSON line."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import zipc_amd
from zipc_amd import batch, synth

N, L, BITS, LEVEL = int(os.environ.get("ZLIB_BENCH_STREAMS", 16384)), 65536, 4, 2
ROUNDS, REPS = 9, 3
dev = torch.device("cuda", 0)
ctx = zipc_amd.Context(0)


def timed(fn):
    t0 = time.perf_counter()
    for _ in range(REPS): fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) / REPS * 1e3


src = synth.batch_bytes_torch(2, 0, N, L, BITS, dev)
cap = batch.zlib_bound(L)
descs = batch.uniform_layout(N, L, cap)
slot = int(descs["dst_off"][1])
d_descs = batch.to_device(descs, dev)
comp_raw = torch.zeros(N * slot + 256, dtype=torch.uint8, device=dev)
comp_z = torch.zeros(N * slot + 256, dtype=torch.uint8, device=dev)
out = torch.zeros(N * L + 256, dtype=torch.uint8, device=dev)
d_res = [torch.zeros(N * 16, dtype=torch.uint8, device=dev) for _ in range(4)]
batch.reserve(ctx, N, L, N * L)
calls = {
    "deflate_batch_adler32": lambda: batch.deflate_batch(ctx, src, comp_raw, d_descs, d_res[0], N, L, N * L, LEVEL, 2, sync=False),
    "zlib_compress_batch": lambda: batch.zlib_compress_batch(ctx, src, comp_z, d_descs, d_res[1], N, L, N * L, LEVEL, sync=False),
}
for fn in calls.values(): fn()
ctx.synchronize()
res_raw, res_z = batch.results_from_device(d_res[0]), batch.results_from_device(d_res[1])
assert (res_raw["status"] == 0).all() and (res_z["status"] == 0).all()
assert (res_z["out_len"] == res_raw["out_len"] + 6).all() and (res_z["checksum"] == res_raw["checksum"]).all()
d_iraw = batch.to_device(batch.compact_descs(res_raw, descs, L), dev)
d_iz = batch.to_device(batch.compact_descs(res_z, descs, L), dev)
calls["inflate_batch_adler32"] = lambda: batch.inflate_batch(ctx, comp_raw, out, d_iraw, d_res[2], N, L, 2, sync=False)
calls["zlib_decompress_batch"] = lambda: batch.zlib_decompress_batch(ctx, comp_z, out, d_iz, d_res[3], N, L, sync=False)
ok = True
for name in ("inflate_batch_adler32", "zlib_decompress_batch"):
    out.zero_(); torch.cuda.synchronize()
    calls[name](); ctx.synchronize()
    r = batch.results_from_device(d_res[2 if name.startswith("inflate") else 3])
    ok = ok and bool((r["status"] == 0).all()) and bool(torch.equal(out[:N * L], src)) and bool((r["checksum"] == res_raw["checksum"]).all())
for fn in calls.values(): fn()  # warm
ctx.synchronize()
ms = {k: [] for k in calls}
for _ in range(ROUNDS):
    for k, fn in calls.items(): ms[k].append(timed(fn))
ctx.set_profiling(True); ctx.reset_kernel_times()
calls["zlib_compress_batch"](); calls["zlib_decompress_batch"](); ctx.synchronize()
kt = {a: round(b[1] / b[0], 4) for a, b in ctx.kernel_times().items() if a.startswith("zlib_")}
ctx.set_profiling(False)
med = {k: statistics.median(v) for k, v in ms.items()}
print(json.dumps({
    "config": "C2 shape: %d streams x %d B of %d-bit symbols, level default, Adler-32 (the reference's)" % (N, L, BITS),
    "rounds": ROUNDS, "reps_per_timing": REPS, "round_trip_ok": ok,
    "ms_median": {k: round(v, 3) for k, v in med.items()},
    "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
    "spread_of_raw_forms": {k: round((max(ms[k]) - min(ms[k])) / med[k], 4) for k in ("deflate_batch_adler32", "inflate_batch_adler32")},
    "ratio_compress": round(med["zlib_compress_batch"] / med["deflate_batch_adler32"], 4),
    "ratio_decompress": round(med["zlib_decompress_batch"] / med["inflate_batch_adler32"], 4),
    "container_kernels_ms_per_launch": kt}))
