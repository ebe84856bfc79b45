#!/usr/bin/env python3
"""What the gzip container costs on top of the forms it is made of (include/zipc_hip.h at zipc_hip_gzip_decompress_batch).
Four comparisons, each call timed between two synchronizes, a warm-up of every call and then ROUNDS rounds of the calls in
turn; median, min and max of every call, and for a pair the difference of the medians beside the yardstick's own spread.

  (a) decode on the device   zipc_hip_gzip_decompress_batch over N BGZF members of 64 KiB of 4-bit symbols (bench.py's shape)
                             against zipc_hip_inflate_extent_batch with CRC-32 over the same bodies -- the parent's form;
  (b) compress on the device zipc_hip_gzip_compress_batch (BGZF, `Default) against zipc_hip_deflate_batch with CRC-32;
  (c) host, a BGZF file      zipc_hip_gzip_decompress over the file of those N members from host memory against a loop of
                             zipc_hip_inflate_extent per member over the same bytes -- the parent's only way;
  (d) host, one long member  one .gz member of LONG_MIB MiB of text through zipc_hip_gzip_decompress against
                             zipc_hip_inflate over its body with the length given.
With (a) and (b): what gzip_open and the close kernel take by HIP events (zipc_hip_kernel_times) in one profiled call.
One JSON object on stdout and in --out FILE (profiles/gzip_batch.json).  Run from the repository's root.
GZIP_BENCH_STREAMS, GZIP_BENCH_LONG_MIB scale it down."""
import ctypes as C
import json
import os
import statistics
import sys
import time
import zipfile
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import zipc_amd  # noqa: E402
from zipc_amd import _lib, batch, synth  # noqa: E402

N, L, LEVEL = int(os.environ.get("GZIP_BENCH_STREAMS", 16384)), 65536, 2
LONG_MIB = int(os.environ.get("GZIP_BENCH_LONG_MIB", 64))
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
    torch.cuda.synchronize()  # (the arenas were made on torch's stream)
    for fn in calls.values():
        timed(fn)
    ms = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            ms[k].append(timed(fn))
    return ms


def summary(ms, new, yardstick):
    s = {k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)} for k, v in ms.items()}
    s["difference_of_medians_ms"] = round(s[new]["median_ms"] - s[yardstick]["median_ms"], 3)
    s["yardstick_spread_ms"] = round(s[yardstick]["max_ms"] - s[yardstick]["min_ms"], 3)
    s["new_over_yardstick"] = round(s[new]["median_ms"] / s[yardstick]["median_ms"], 4)
    return s


def container_kernels(fn):
    """the container's kernels in one profiled call: {name: ms}"""
    ctx.set_profiling(True)
    ctx.reset_kernel_times()
    fn()
    ctx.synchronize()
    t = ctx.kernel_times()
    ctx.set_profiling(False)
    return {k: round(v[1], 4) for k, v in t.items() if k.startswith("gzip_")}


def device_forms():
    src = synth.batch_bytes_torch(2, 0, N, L, 4, dev)
    cap = batch.gzip_bound(L, batch.GZIP_BGZF)
    descs = batch.uniform_layout(N, L, cap)
    slot = int(descs["dst_off"][1])
    d_descs = batch.to_device(descs, dev)
    comp = torch.zeros(N * slot + 256, dtype=torch.uint8, device=dev)
    raw = torch.zeros(N * slot + 256, dtype=torch.uint8, device=dev)
    d_res = [torch.zeros(N * 16, dtype=torch.uint8, device=dev) for _ in range(2)]
    calls = {
        "gzip_compress_batch": lambda: batch.gzip_compress_batch(ctx, src, comp, d_descs, d_res[0], N, L, N * L, LEVEL, batch.GZIP_BGZF, sync=False),
        "deflate_batch_crc32": lambda: batch.deflate_batch(ctx, src, raw, d_descs, d_res[1], N, L, N * L, LEVEL, 1, sync=False),
    }
    ms_c = alternate(calls)
    res, plain = batch.results_from_device(d_res[0]), batch.results_from_device(d_res[1])
    ok_c = bool((res["status"] == 0).all() and (plain["status"] == 0).all() and (res["out_len"] == plain["out_len"] + 26).all()
                and (res["checksum"] == plain["checksum"]).all())
    k_c = container_kernels(calls["gzip_compress_batch"])
    # decode: the members where compress left them; the yardstick gets the same bodies (everything behind the 18 header bytes)
    members = batch.make_descs(descs["dst_off"], res["out_len"], np.arange(N, dtype=np.uint64) * np.uint64(L), np.full(N, L, np.uint64))
    bodies = members.copy()
    bodies["src_off"] += 18
    bodies["src_len"] -= 18
    d_m, d_b = batch.to_device(members, dev), batch.to_device(bodies, dev)
    out = [torch.zeros(N * L + 256, dtype=torch.uint8, device=dev) for _ in range(2)]
    d_r = [torch.zeros(N * 32, dtype=torch.uint8, device=dev) for _ in range(2)]
    calls = {
        "gzip_decompress_batch": lambda: batch.gzip_decompress_batch(ctx, comp, out[0], d_m, d_r[0], N, L, sync=False),
        "inflate_extent_batch_crc32": lambda: batch.inflate_extent_batch(ctx, comp, out[1], d_b, d_r[1], N, L, 1, sync=False),
    }
    ms_d = alternate(calls)
    g, e = batch.gzip_results_from_device(d_r[0]), batch.extent_results_from_device(d_r[1])
    ok_d = bool((g["status"] == 0).all() and (e["status"] == 0).all() and (g["src_used"] == res["out_len"]).all() and (g["checksum"] == e["checksum"]).all()
                and torch.equal(out[0][:N * L], src) and torch.equal(out[1][:N * L], src))
    k_d = container_kernels(calls["gzip_decompress_batch"])
    file = b"".join(comp[int(o):int(o) + int(n)].cpu().numpy().tobytes() for o, n in zip(descs["dst_off"], res["out_len"]))
    shape = {"streams": N, "stream_bytes": L, "data": "4-bit symbols (bench.py's C2)", "compressed_ratio": round(float(res["out_len"].sum()) / (N * L), 4)}
    return ({"what": "(b) compress on the device, BGZF members at `Default", **shape, "results_ok": ok_c, "rounds": ROUNDS,
             **summary(ms_c, "gzip_compress_batch", "deflate_batch_crc32"), "container_kernels_ms": k_c},
            {"what": "(a) decode on the device", **shape, "results_ok": ok_d, "rounds": ROUNDS,
             **summary(ms_d, "gzip_decompress_batch", "inflate_extent_batch_crc32"), "container_kernels_ms": k_d},
            file, res["out_len"].astype(np.int64), src.cpu().numpy().tobytes())


def host_bgzf(file, lens, plain):
    dst = C.create_string_buffer(len(plain))
    got = {}
    offs = np.concatenate(([0], np.cumsum(lens)[:-1]))

    def whole():
        n, used, members, crc = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_uint32()
        got["file"] = (lib.zipc_hip_gzip_decompress(ctx.handle, file, len(file), dst, len(plain), C.byref(n), C.byref(used), C.byref(members), C.byref(crc)),
                       n.value, used.value, members.value)

    view = (C.c_char * len(file)).from_buffer_copy(file)
    base, dbase = C.addressof(view), C.addressof(dst)

    def loop():
        n, used, crc = C.c_size_t(), C.c_size_t(), C.c_uint32()
        bad = 0
        for i in range(len(lens)):
            st = lib.zipc_hip_inflate_extent(ctx.handle, base + int(offs[i]) + 18, int(lens[i]) - 18, 0, 0, dbase + i * L, L, 1, C.byref(n), C.byref(used),
                                             C.byref(crc))
            bad += st != 0 or n.value != L
        got["loop"] = bad

    ms = alternate({"gzip_decompress_file": whole, "inflate_extent_per_member": loop}, 5)
    ok = got["file"] == (0, len(plain), len(file), len(lens)) and got["loop"] == 0 and dst.raw == plain
    return {"what": "(c) host decode of a BGZF file against a loop of zipc_hip_inflate_extent per member", "members": len(lens), "file_bytes": len(file),
            "plain_bytes": len(plain), "results_ok": bool(ok), "rounds": 5, **summary(ms, "gzip_decompress_file", "inflate_extent_per_member")}


def host_long():
    z = zipfile.ZipFile(os.path.join(ROOT, "tests", "golden", "zip-docs.zip"))
    text = z.read("zip-docs/APPNOTE.TXT") + z.read("zip-docs/rfc1951.txt")
    n = LONG_MIB << 20
    plain = (text * (n // len(text) + 1))[:n]
    cap = lib.zipc_hip_gzip_bound(n, 0)
    buf, m = C.create_string_buffer(cap), C.c_size_t()
    assert lib.zipc_hip_gzip_compress(ctx.handle, plain, n, LEVEL, 0, buf, cap, C.byref(m)) == 0
    member = buf.raw[:m.value]
    del buf
    body = member[10:-8]
    dst = C.create_string_buffer(n)
    got = {}

    def gz():
        k, used, members, crc = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_uint32()
        got["gzip"] = (lib.zipc_hip_gzip_decompress(ctx.handle, member, len(member), dst, n, C.byref(k), C.byref(used), C.byref(members), C.byref(crc)),
                       k.value, used.value, members.value)
        got["blocks"] = ctx.last_inflate_blocks()

    def raw():
        k, crc = C.c_size_t(), C.c_uint32()
        got["raw"] = (lib.zipc_hip_inflate(ctx.handle, body, len(body), 0, 0, 1, dst, n, C.byref(k), C.byref(crc)), k.value, crc.value)

    ms = alternate({"gzip_decompress_one_member": gz, "inflate_body_length_given": raw}, 5)
    ok = got["gzip"] == (0, n, len(member), 1) and got["raw"] == (0, n, zlib.crc32(plain)) and dst.raw == plain
    return {"what": "(d) host decode of one long member against zipc_hip_inflate over its body with the length given", "plain_bytes": n,
            "member_bytes": len(member), "inflate_by_blocks": got["blocks"], "results_ok": bool(ok), "rounds": 5,
            **summary(ms, "gzip_decompress_one_member", "inflate_body_length_given")}


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    b, a, file, lens, plain = device_forms()
    print("device forms done", file=sys.stderr, flush=True)
    c = host_bgzf(file, lens, plain)
    print("host BGZF file done", file=sys.stderr, flush=True)
    result = {"device": torch.cuda.get_device_name(0), "decode_device": a, "compress_device": b, "host_bgzf_file": c, "host_long_member": host_long()}
    text = json.dumps(result, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
