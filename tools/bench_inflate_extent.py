#!/usr/bin/env python3
"""What the extent forms cost beside the forms they mirror: zipc_hip_inflate_extent_batch against zipc_hip_inflate_batch
and zipc_hip_inflate_size_extent_batch against zipc_hip_inflate_size_batch on bench.py's own batch -- 16 384 streams x
64 KiB of 4-bit symbols deflated at `Default, device-resident, CRC_NOP (and the decode pair once more with CRC-32).  The
only intended difference is the result store: 32 bytes a stream instead of 16.  The calls are timed in alternation, ROUNDS
times over, after a warm-up of each; a timing is a host clock around one call with one synchronize at its end.  Before
anything is timed the extent calls' results are compared with their siblings' and src_used with the streams' lengths.
--parent: only the two existing calls (for a run on the parent commit, which has no extent forms).  One JSON object on
stdout (and in --out FILE).  Run from the repository's root.
One more row isolates what the CRC-32 pair differs in beside the store: zipc_hip_inflate_batch with CRC-32 cut into ONE
slice (zipc_hip_debug_set_slices(1), set around that call alone) -- its default is two slices on queues of their own, the
checksum pass of the first beside the inflate kernel of the second, where the extent form is one launch by design."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import zipc_amd  # noqa: E402
from zipc_amd import _lib, batch, synth  # noqa: E402

N, L = int(os.environ.get("EXTENT_BENCH_STREAMS", 16384)), 65536
ROUNDS, LEVEL = int(os.environ.get("EXTENT_BENCH_ROUNDS", 7)), 2
dev = torch.device("cuda", 0)
ctx = zipc_amd.Context(0)


def timed(fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(calls):
    for fn in calls.values():
        timed(fn)
    ms = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, fn in calls.items():
            ms[k].append(timed(fn))
    return {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in ms.items()}


def main():
    parent = "--parent" in sys.argv
    src = synth.batch_bytes_torch(2, 0, N, L, 4, dev)
    cap = batch.deflate_bound(L)
    descs = batch.uniform_layout(N, L, cap)
    slot = int(descs["dst_off"][1])
    comp = torch.zeros(N * slot + 256, dtype=torch.uint8, device=dev)
    d_res = torch.zeros(N * 16, dtype=torch.uint8, device=dev)
    batch.deflate_batch(ctx, src, comp, batch.to_device(descs, dev), d_res, N, L, N * L, LEVEL, 0)
    res = batch.results_from_device(d_res)
    assert (res["status"] == 0).all()
    # src_len is the slot: an upper bound, as a caller of the extent forms would have it -- for every call alike
    idescs = batch.make_descs(descs["dst_off"], np.full(N, slot, np.uint64), np.arange(N, dtype=np.uint64) * np.uint64(L), np.full(N, L, np.uint64))
    d_idescs = batch.to_device(idescs, dev)
    out_buf = torch.zeros(N * L + 256, dtype=torch.uint8, device=dev)
    r16, r32 = torch.zeros(N * 16, dtype=torch.uint8, device=dev), torch.zeros(N * 32, dtype=torch.uint8, device=dev)
    calls = {}
    for name, op in (("crc_nop", 0), ("crc32", 1)):
        calls["inflate_batch/" + name] = lambda op=op: batch.inflate_batch(ctx, comp, out_buf, d_idescs, r16, N, L, op, sync=False)
        if not parent:
            calls["inflate_extent_batch/" + name] = lambda op=op: batch.inflate_extent_batch(ctx, comp, out_buf, d_idescs, r32, N, L, op, sync=False)
    def one_slice():
        _lib.lib().zipc_hip_debug_set_slices(1)
        batch.inflate_batch(ctx, comp, out_buf, d_idescs, r16, N, L, 1, sync=False)
        _lib.lib().zipc_hip_debug_set_slices(0)

    calls["inflate_batch/crc32, one slice"] = one_slice
    calls["inflate_size_batch"] = lambda: batch.inflate_size_batch(ctx, comp, d_idescs, r16, N, sync=False)
    if not parent:
        calls["inflate_size_extent_batch"] = lambda: batch.inflate_size_extent_batch(ctx, comp, d_idescs, r32, N, sync=False)
    out = {"streams": N, "stream_plain_bytes": L, "stream_bytes": int(res["out_len"].sum()), "rounds": ROUNDS, "level": "default"}
    if not parent:
        calls["inflate_extent_batch/crc32"]()
        ctx.synchronize()
        e = batch.extent_results_from_device(r32)
        assert torch.equal(out_buf[:N * L], src[:N * L])
        calls["inflate_batch/crc32"]()
        ctx.synchronize()
        p = batch.results_from_device(r16)
        equal = bool((e["status"] == p["status"]).all() and (e["checksum"] == p["checksum"]).all() and (e["out_len"] == p["out_len"]).all() and
                     (e["src_used"] == res["out_len"]).all())
        calls["inflate_size_extent_batch"]()
        ctx.synchronize()
        s = batch.extent_results_from_device(r32)
        out["results_equal_and_src_used_is_the_stream_length"] = bool(equal and (s["src_used"] == res["out_len"]).all() and (s["out_len"] == L).all())
    out["ms"] = alternate(calls)
    print(json.dumps(out))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
