#!/usr/bin/env python3
"""What sizing costs: zipc_hip_inflate_size_batch against zipc_hip_inflate_batch (CRC_NOP) on the same streams, and one
long stream through zipc_hip_inflate_size (its one wave) against zipc_hip_inflate with the exact capacity (by blocks).
  batches  C2's shape (16 384 streams x 64 KiB of 4-bit symbols, `Default) and tools/bench_text.py's text batch (64 KiB
           chunks of APPNOTE.TXT / rfc1951.txt, 16 384 streams), device-resident: the two calls alternate, ROUNDS times
           over, a synchronize before and behind every timed call;
  one      1 MiB and 64 MiB of that text as ONE stream at `Default: the host forms (copy in; inflate also copies its
           bytes back), and the same two on the device alone (the batch forms of one stream) alternating likewise.
One JSON object on stdout (and in --out FILE).  Run from the repository's root.

  --blocks  instead: sizing BY BLOCKS (zipc_hip_inflate_size_blocks_batch; zipc_hip_inflate_size goes through it) -- one
           stream of that text at `Default, 1 MiB and 64 MiB: zipc_hip_inflate_size, the one-wave kernel (a
           zipc_hip_inflate_size_batch of one: what zipc_hip_inflate_size was before) and zipc_hip_inflate at the exact
           capacity, as host forms and on the device alone, nine rounds of the three in turn; the kernels of one sizing
           by blocks (HIP events); 64 x 1 MiB through the new batch form against zipc_hip_inflate_batch; and, for the
           constants of forms.h size_blocks_pick, the one-wave kernel and this path in ms per MiB of INPUT on text and on
           C2's 4-bit symbols (one stream of 1 MiB and of 16 MiB each: slope and intercept).  profiles/inflate_size_blocks.json."""
import ctypes as C
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
from zipc_amd import _lib, batch, synth  # noqa: E402

N, L, LEVEL = int(os.environ.get("SIZE_BENCH_STREAMS", 16384)), 65536, 2
LONG_MIB = [int(v) for v in os.environ.get("SIZE_BENCH_LONG_MIB", "1,64").split(",")]
ROUNDS = 7
dev = torch.device("cuda", 0)
ctx = zipc_amd.Context(0)
lib = _lib.lib()


def timed(fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(calls, rounds=ROUNDS):
    """{name: [ms]}: a warm-up of every call, then the calls in turn, rounds times"""
    for fn in calls.values():
        timed(fn)
    ms = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            ms[k].append(timed(fn))
    return ms


def summary(ms):
    return {k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)} for k, v in ms.items()}


def text_bytes():
    z = zipfile.ZipFile(os.path.join(ROOT, "tests", "golden", "zip-docs.zip"))
    return z.read("zip-docs/APPNOTE.TXT"), z.read("zip-docs/rfc1951.txt")


def bench_batch(name, src):
    """src: N streams of L bytes, device-resident -> the batch's figures"""
    cap = batch.deflate_bound(L)
    descs = batch.uniform_layout(N, L, cap)
    slot = int(descs["dst_off"][1])
    comp = torch.zeros(N * slot + 256, dtype=torch.uint8, device=dev)
    out = torch.zeros(N * L + 256, dtype=torch.uint8, device=dev)
    d_res = [torch.zeros(N * 16, dtype=torch.uint8, device=dev) for _ in range(3)]
    batch.deflate_batch(ctx, src, comp, batch.to_device(descs, dev), d_res[0], N, L, N * L, LEVEL, 0)
    res = batch.results_from_device(d_res[0])
    assert (res["status"] == 0).all()
    d_id = batch.to_device(batch.compact_descs(res, descs, L, limit_exact=False), dev)
    calls = {
        "inflate_size_batch": lambda: batch.inflate_size_batch(ctx, comp, d_id, d_res[1], N, sync=False),
        "inflate_batch_nop": lambda: batch.inflate_batch(ctx, comp, out, d_id, d_res[2], N, L, 0, sync=False),
    }
    ms = alternate(calls)
    sized, inflated = batch.results_from_device(d_res[1]), batch.results_from_device(d_res[2])
    ok = bool((sized["status"] == 0).all() and (sized["out_len"] == L).all() and (sized["checksum"] == 0).all()
              and (inflated["status"] == 0).all() and (inflated["out_len"] == L).all() and torch.equal(out[:N * L], src))
    s = summary(ms)
    return {"data": name, "streams": N, "stream_bytes": L, "compressed_ratio": round(float(res["out_len"].sum()) / (N * L), 4),
            "results_ok": ok, "rounds": ROUNDS, **s,
            "size_over_inflate": round(s["inflate_size_batch"]["median_ms"] / s["inflate_batch_nop"]["median_ms"], 4)}


def bench_one(mib, text):
    n = mib << 20
    plain = (text * (n // len(text) + 1))[:n]
    cap = lib.zipc_hip_deflate_bound(n)
    buf = C.create_string_buffer(cap)
    ol, ck = C.c_size_t(), C.c_uint32()
    assert lib.zipc_hip_deflate(ctx.handle, plain, n, LEVEL, 0, buf, cap, C.byref(ol), C.byref(ck)) == 0
    stream = buf.raw[:ol.value]
    del buf
    dst = C.create_string_buffer(n)
    got = {}

    def host_size():
        v = C.c_size_t()
        got["size"] = (lib.zipc_hip_inflate_size(ctx.handle, stream, len(stream), 0, 0, C.byref(v)), v.value)

    def host_inflate():
        v, k = C.c_size_t(), C.c_uint32()
        got["inflate"] = (lib.zipc_hip_inflate(ctx.handle, stream, len(stream), 0, 0, 0, dst, n, C.byref(v), C.byref(k)), v.value)
        got["blocks"] = ctx.last_inflate_blocks()

    rounds = 5 if mib <= 8 else 3
    host = alternate({"zipc_hip_inflate_size": host_size, "zipc_hip_inflate_exact_cap": host_inflate}, rounds)
    ok = got["size"] == (0, n) and got["inflate"] == (0, n) and dst.raw == plain
    # the same on the device alone: no copy in, none back
    src = torch.from_numpy(np.frombuffer(stream + b"\0" * 64, dtype=np.uint8).copy()).to(dev)
    out = torch.zeros(n + 256, dtype=torch.uint8, device=dev)
    d_desc = batch.to_device(batch.make_descs([0], [len(stream)], [0], [n]), dev)
    d_res = [torch.zeros(16, dtype=torch.uint8, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    device = alternate({
        "inflate_size_batch_of_one": lambda: batch.inflate_size_batch(ctx, src, d_desc, d_res[0], 1, sync=False),
        "inflate_batch_of_one_exact_cap": lambda: batch.inflate_batch(ctx, src, out, d_desc, d_res[1], 1, n, 0, sync=False),
    }, rounds)
    r0, r1 = batch.results_from_device(d_res[0]), batch.results_from_device(d_res[1])
    ok = ok and (int(r0["status"][0]), int(r0["out_len"][0])) == (0, n) and (int(r1["status"][0]), int(r1["out_len"][0])) == (0, n)
    return {"data": "%d MiB of text (APPNOTE.TXT + rfc1951.txt, repeated), one stream, level default" % mib, "plain_bytes": n,
            "stream_bytes": len(stream), "results_ok": bool(ok), "rounds": rounds, "inflate_by_blocks": got["blocks"],
            "host_forms": summary(host), "device_only": summary(device)}


def deflate_host(plain):
    cap = lib.zipc_hip_deflate_bound(len(plain))
    buf = C.create_string_buffer(cap)
    ol, ck = C.c_size_t(), C.c_uint32()
    assert lib.zipc_hip_deflate(ctx.handle, plain, len(plain), LEVEL, 0, buf, cap, C.byref(ol), C.byref(ck)) == 0
    return buf.raw[:ol.value]


BLOCK_ROUNDS = 9


def device_three(streams, plains, rounds=BLOCK_ROUNDS, with_inflate=True):
    """the three device-resident calls over a batch of streams, in turn: sizing by blocks, the one-wave sizing kernel,
    inflate_batch (CRC_NOP) at the exact capacities -> (summary, results ok, blocks of the last sizing by blocks)"""
    n = len(streams)
    lens = [len(x) for x in streams]
    caps = [len(x) for x in plains]
    slots = [(k + 255) // 256 * 256 for k in caps]
    src = torch.from_numpy(np.frombuffer(b"".join(streams) + b"\0" * 64, dtype=np.uint8).copy()).to(dev)
    out = torch.zeros(sum(slots) + 256, dtype=torch.uint8, device=dev)
    d_desc = batch.to_device(batch.make_descs(np.cumsum([0] + lens[:-1]).astype(np.uint64), lens,
                                              np.cumsum([0] + slots[:-1]).astype(np.uint64), caps), dev)
    d_res = [torch.zeros(n * 16, dtype=torch.uint8, device=dev) for _ in range(3)]
    torch.cuda.synchronize()
    seen = {}

    def by_blocks():
        batch.inflate_size_blocks_batch(ctx, src, d_desc, d_res[0], n)
        seen["blocks"] = ctx.last_size_blocks()

    calls = {"inflate_size_blocks_batch": by_blocks,
             "inflate_size_batch_one_wave": lambda: batch.inflate_size_batch(ctx, src, d_desc, d_res[1], n, sync=False)}
    if with_inflate:
        calls["inflate_batch_exact_cap"] = lambda: batch.inflate_batch(ctx, src, out, d_desc, d_res[2], n, max(caps), 0, sync=False)
    ms = alternate(calls, rounds)
    ok = True
    for r in d_res[:3 if with_inflate else 2]:
        v = batch.results_from_device(r)
        ok = ok and bool((v["status"] == 0).all()) and [int(x) for x in v["out_len"]] == caps
    if with_inflate:
        o = out.cpu().numpy()
        at = 0
        for k, p in zip(slots, plains):
            ok = ok and o[at:at + len(p)].tobytes() == p
            at += k
    return summary(ms), ok, seen["blocks"]


def blocks_one(mib, text):
    n = mib << 20
    plain = (text * (n // len(text) + 1))[:n]
    stream = deflate_host(plain)
    dst = C.create_string_buffer(n)
    got = {}

    def host_size():
        v = C.c_size_t()
        got["size"] = (lib.zipc_hip_inflate_size(ctx.handle, stream, len(stream), 0, 0, C.byref(v)), v.value)
        got["size_blocks"] = ctx.last_size_blocks()

    def host_inflate():
        v, k = C.c_size_t(), C.c_uint32()
        got["inflate"] = (lib.zipc_hip_inflate(ctx.handle, stream, len(stream), 0, 0, 0, dst, n, C.byref(v), C.byref(k)), v.value)
        got["blocks"] = ctx.last_inflate_blocks()

    host = alternate({"zipc_hip_inflate_size": host_size, "zipc_hip_inflate_exact_cap": host_inflate}, BLOCK_ROUNDS)
    ok = got["size"] == (0, n) and got["inflate"] == (0, n) and dst.raw == plain
    device, ok_d, blocks = device_three([stream], [plain])
    # the kernels of one sizing by blocks
    ctx.set_profiling(True)
    ctx.reset_kernel_times()
    host_size()
    kernels = {k: {"launches": c, "ms": round(t, 4)} for k, (c, t) in sorted(ctx.kernel_times().items()) if c}
    ctx.set_profiling(False)
    return {"data": "%d MiB of text (APPNOTE.TXT + rfc1951.txt, repeated), one stream, level default" % mib, "plain_bytes": n,
            "stream_bytes": len(stream), "results_ok": bool(ok and ok_d), "rounds": BLOCK_ROUNDS, "size_blocks": got["size_blocks"],
            "inflate_by_blocks": got["blocks"], "host_forms": summary(host), "device_only": device,
            "kernels_of_one_sizing_by_blocks": kernels}


def blocks_constants(text):
    """ms per MiB of input: one stream of 1 MiB and of 16 MiB of plain bytes, text and C2's 4-bit symbols"""
    out = []
    for name, make in (("text", lambda n: (text * (n // len(text) + 1))[:n]),
                       ("C2 4-bit symbols", lambda n: synth.stream_bytes_np(2, 7, n, 4).tobytes())):
        pts = []
        for mib in (1, 16):
            plain = make(mib << 20)
            stream = deflate_host(plain)
            s, ok, blocks = device_three([stream], [plain], rounds=5, with_inflate=False)
            pts.append({"plain_mib": mib, "input_mib": round(len(stream) / 1048576.0, 4), "results_ok": ok, "size_blocks": blocks, **s})
        (a, b) = pts
        d_in = b["input_mib"] - a["input_mib"]
        per = {k: round((b[k]["median_ms"] - a[k]["median_ms"]) / d_in, 4) for k in ("inflate_size_blocks_batch", "inflate_size_batch_one_wave")}
        fixed = round(a["inflate_size_blocks_batch"]["median_ms"] - per["inflate_size_blocks_batch"] * a["input_mib"], 4)
        out.append({"data": name, "points": pts, "ms_per_mib_of_input": per, "blocks_fixed_ms": fixed})
    return out


def main_blocks():
    app, rfc = text_bytes()
    text = app + rfc
    out = {"one_stream": [], "batch_64x1MiB": None, "constants": None}
    for mib in LONG_MIB:
        out["one_stream"].append(blocks_one(mib, text))
    plains = [(text[7919 * i % len(text):] + text * 2)[:1 << 20] for i in range(64)]
    streams = [deflate_host(p) for p in plains]
    out["batches_of_1MiB"] = []
    for n in (8, 16, 24, 64):
        s, ok, blocks = device_three(streams[:n], plains[:n])
        row = {"data": "%d streams of 1 MiB of that text, level default" % n, "streams": n, "stream_bytes": sum(len(x) for x in streams[:n]),
               "results_ok": ok, "rounds": BLOCK_ROUNDS, "size_blocks": blocks, **s}
        out["batches_of_1MiB"].append(row)
        if n == 64:
            out["batch_64x1MiB"] = row
    out["constants"] = blocks_constants(text)
    print(json.dumps(out))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


def main():
    if "--blocks" in sys.argv:
        return main_blocks()
    app, rfc = text_bytes()
    out = {"batches": [], "one_stream": []}
    src = synth.batch_bytes_torch(2, 0, N, L, 4, dev)
    out["batches"].append(bench_batch("C2 shape: 4-bit symbols, level default", src))
    del src
    chunks = [app[0:L], app[L:2 * L], (rfc + rfc)[:L], app[100000:100000 + L]]
    host = np.frombuffer(b"".join(chunks[i % len(chunks)] for i in range(N)), np.uint8).copy()
    out["batches"].append(bench_batch("real text (APPNOTE / rfc1951, 4 distinct 64 KiB chunks repeated), level default",
                                      torch.from_numpy(host).to(dev)))
    torch.cuda.empty_cache()
    for mib in LONG_MIB:
        out["one_stream"].append(bench_one(mib, app + rfc))
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
