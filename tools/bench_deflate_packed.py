#!/usr/bin/env python3
"""What the packed encode (zipc_hip_deflate_packed_batch) costs beside the call it is built around, and what its copy kernel
costs beside a plain copy of the same bytes.  Device-resident streams, `Default, CRC_NOP, in one process and one context:
  c2      16 384 streams x 64 KiB of 4-bit symbols (the benchmark's C2 data);
  ragged  4096 streams of 1 B .. 64 KiB of text.
Per shape, timed in alternation, ROUNDS times over, after a warm-up of each (a timing is a host clock around one call with
one synchronize at its end):
  packed         zipc_hip_deflate_packed_batch into an arena of the bound, align 16;
  deflate_batch  zipc_hip_deflate_batch alone over the same batch into slots of zipc_hip_deflate_bound: the path there was
                 before, and the yardstick for the call;
  memcpy         a device-to-device copy of `need` bytes (torch's copy_ of a contiguous uint8 slice: one hipMemcpyAsync):
                 the yardstick for dpacked_copy.
Then the kernels of REPS packed calls by HIP events through the context's kernel times, at align 1 and at align 16
(dpacked_stage, dpacked_layout, dpacked_copy and dpacked_close among them), and the scratch the call takes beside deflate's
own.  The packed arena is compared with deflate_batch's slots before anything is timed.  One JSON object on stdout (and in
--out FILE).  Run from the repository's root."""
import json
import os
import statistics
import sys
import time
import zipfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import zipc_amd  # noqa: E402
from zipc_amd import batch, synth  # noqa: E402

N_C2, L_C2 = int(os.environ.get("DPACKED_BENCH_STREAMS", 16384)), 65536
N_RAGGED = int(os.environ.get("DPACKED_BENCH_RAGGED", 4096))
ROUNDS, REPS, LEVEL = int(os.environ.get("DPACKED_BENCH_ROUNDS", 7)), 3, 2
dev = torch.device("cuda", 0)
ctx = zipc_amd.Context(0)


def text_bytes():
    z = zipfile.ZipFile(os.path.join(ROOT, "tests", "golden", "zip-docs.zip"))
    return z.read("zip-docs/APPNOTE.TXT") + z.read("zip-docs/rfc1951.txt")


def timed(fn):
    ctx.synchronize()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(calls):
    for fn in calls.values():
        timed(fn)
    ms = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, fn in calls.items():
            ms[k].append(timed(fn))
    return ms


def run(name, plain, offs, lens):
    n, total, max_len = len(lens), int(lens.sum()), int(lens.max())
    uniq = np.unique(lens)
    caps = np.array([batch.deflate_bound(int(v)) for v in uniq], np.uint64)[np.searchsorted(uniq, lens)]
    slots = (caps + np.uint64(255)) // np.uint64(256) * np.uint64(256)
    slot_off = np.concatenate([[0], np.cumsum(slots)[:-1]]).astype(np.uint64)
    comp = torch.zeros(int(slots.sum()) + 256, dtype=torch.uint8, device=dev)
    d_slot_descs = batch.to_device(batch.make_descs(offs, lens, slot_off, caps), dev)
    d_descs = batch.to_device(batch.make_descs(offs, lens, np.zeros(n, np.uint64), np.zeros(n, np.uint64)), dev)
    d_res = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    d_packed = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    d_need = torch.zeros(8, dtype=torch.uint8, device=dev)
    arena_len = {a: batch.deflate_packed_bound(n, total, a) for a in (1, 16)}
    arena = torch.zeros(arena_len[16] + 256, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def packed(align=16):
        batch.deflate_packed_batch(ctx, plain, arena, d_descs, d_packed, n, max_len, total, LEVEL, 0, align, d_need,
                                   dst_arena_len=arena_len[align], sync=False)

    def deflate_alone():
        batch.deflate_batch(ctx, plain, comp, d_slot_descs, d_res, n, max_len, total, LEVEL, 0, sync=False)

    packed(); deflate_alone(); ctx.synchronize()
    p, r = batch.packed_results_from_device(d_packed), batch.results_from_device(d_res)
    need = int(d_need.cpu().numpy().view(np.uint64)[0])
    equal = bool((p["status"] == 0).all() and (r["status"] == 0).all() and (p["out_len"] == r["out_len"]).all() and need <= arena_len[16])
    for i in list(range(0, n, max(1, n // 64))) + [n - 1]:
        a, b, k = int(p["dst_off"][i]), int(slot_off[i]), int(r["out_len"][i])
        equal = equal and torch.equal(arena[a:a + k], comp[b:b + k])
    other = torch.zeros(need + 256, dtype=torch.uint8, device=dev)

    def memcpy():
        other[:need].copy_(arena[:need])

    ms = alternate({"packed": packed, "deflate_batch": deflate_alone, "memcpy_need_bytes": memcpy})
    kernels = {}
    for align in (1, 16):
        ctx.set_profiling(True)
        ctx.reset_kernel_times()
        for _ in range(REPS):
            packed(align)
        ctx.synchronize()
        kernels["align %d" % align] = {k: {"launches_per_call": round(c / REPS, 2), "ms_per_call": round(t / REPS, 4)}
                                       for k, (c, t) in sorted(ctx.kernel_times().items()) if c}
        ctx.set_profiling(False)
    med = {k: statistics.median(v) for k, v in ms.items()}
    copy_ms = {a: kernels[a]["dpacked_copy"]["ms_per_call"] for a in kernels}
    return {"shape": name, "streams": n, "plain_bytes": total, "need_bytes": need, "results_and_bytes_equal": equal,
            "ms": {k: {"median": round(med[k], 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in ms.items()},
            "packed_minus_deflate_batch_ms": round(med["packed"] - med["deflate_batch"], 4),
            "packed_over_deflate_batch": round(med["packed"] / med["deflate_batch"], 4),
            "dpacked_copy_ms": copy_ms,
            "dpacked_copy_over_memcpy": {a: round(v / med["memcpy_need_bytes"], 3) for a, v in copy_ms.items()},
            "dpacked_copy_GBps_read_plus_written": {a: round(2 * need / v / 1e6, 1) for a, v in copy_ms.items()},
            "memcpy_GBps_read_plus_written": round(2 * need / med["memcpy_need_bytes"] / 1e6, 1),
            "scratch_beside_deflates_own_bytes": {"staging": batch.deflate_packed_bound(n, total, 16) + 16, "per_stream_records": 256 + 88 * n},
            "kernels_of_a_packed_call": kernels}


def main():
    out = {"rounds": ROUNDS, "level": LEVEL, "crc_op": 0, "shapes": []}
    only = os.environ.get("DPACKED_BENCH_ONLY", "c2,ragged").split(",")
    if "c2" in only:
        src = synth.batch_bytes_torch(2, 0, N_C2, L_C2, 4, dev)
        out["shapes"].append(run("c2: %d x %d B of 4-bit symbols" % (N_C2, L_C2), src, np.arange(N_C2, dtype=np.uint64) * np.uint64(L_C2),
                                 np.full(N_C2, L_C2, np.uint64)))
        del src
        torch.cuda.empty_cache()
    if "ragged" in only:
        text = text_bytes()
        lens = np.random.default_rng(1).integers(1, 65537, N_RAGGED).astype(np.uint64)
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
        host = np.frombuffer((text * (int(lens.sum()) // len(text) + 1))[:int(lens.sum())], np.uint8).copy()
        out["shapes"].append(run("ragged: %d streams of 1 B .. 64 KiB of text" % N_RAGGED, torch.from_numpy(host).to(dev), offs, lens))
    print(json.dumps(out))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
