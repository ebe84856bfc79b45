#!/usr/bin/env python3
"""What a prefix (zipc_hip_inflate_prefix_batch: the first dst_cap bytes of every stream) costs against what there was
before it for the same need: zipc_hip_inflate_batch of the WHOLE streams into rooms of their true size.  Device-resident
streams, CRC_NOP, three batches:
  c2      16 384 streams x 64 KiB of 4-bit symbols at `Default (the benchmark's C2 data);
  long    64 streams of 1 MiB of text (inflate_batch decodes them by a wave per block; the prefix form never does);
  ragged  10 000 streams of 1 B .. 64 KiB of text.
Prefixes of 64, 4096 and 32 768 bytes (dst_cap = the prefix for every stream, so a stream shorter than it simply ends).
Per batch and prefix three calls are timed in alternation, ROUNDS times over, after a warm-up of each: the prefix call,
inflate_batch over the whole streams, and inflate_batch with dst_cap set to the prefix -- every longer stream reports
DST_TOO_SMALL there: the same walk without the cut, so the difference to the prefix call is what the cut itself costs.  A
timing is a host clock around one call with one synchronize at its end.  Before anything is timed the prefix call's
results and bytes are compared with the whole decode.  One JSON object on stdout (and in --out FILE).  Run from the
repository's root."""
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

N_C2, L_C2 = int(os.environ.get("PREFIX_BENCH_STREAMS", 16384)), 65536
N_LONG, LONG = int(os.environ.get("PREFIX_BENCH_LONG", 64)), 1 << 20
N_RAGGED = int(os.environ.get("PREFIX_BENCH_RAGGED", 10000))
ROUNDS, LEVEL = int(os.environ.get("PREFIX_BENCH_ROUNDS", 7)), 2
PREFIXES = (64, 4096, 32768)
dev = torch.device("cuda", 0)
ctx = zipc_amd.Context(0)


def text_bytes():
    z = zipfile.ZipFile(os.path.join(ROOT, "tests", "golden", "zip-docs.zip"))
    return z.read("zip-docs/APPNOTE.TXT") + z.read("zip-docs/rfc1951.txt")


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


def run(name, plain, offs, lens):
    """plain: a uint8 cuda tensor, stream i of it lens[i] bytes at offs[i]"""
    n, total = len(lens), int(lens.sum())
    u = np.unique(lens)
    caps = np.array([batch.deflate_bound(int(v)) for v in u], np.uint64)[np.searchsorted(u, lens)]
    slots = (caps + np.uint64(255)) // np.uint64(256) * np.uint64(256)
    comp_off = np.concatenate([[0], np.cumsum(slots)[:-1]]).astype(np.uint64)
    comp = torch.zeros(int(slots.sum()) + 256, dtype=torch.uint8, device=dev)
    d_res = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    batch.deflate_batch(ctx, plain, comp, batch.to_device(batch.make_descs(offs, lens, comp_off, caps), dev), d_res, n, int(lens.max()), total, LEVEL, 0)
    res = batch.results_from_device(d_res)
    assert (res["status"] == 0).all()
    whole = torch.zeros(total + 256, dtype=torch.uint8, device=dev)
    d_whole = batch.to_device(batch.make_descs(comp_off, res["out_len"], offs, lens), dev)
    max_len = int(lens.max())

    def decode_whole():
        batch.inflate_batch(ctx, comp, whole, d_whole, d_res, n, max_len, 0, sync=False)

    decode_whole()
    ctx.synchronize()
    assert torch.equal(whole[:total], plain[:total])
    host = whole.cpu().numpy()
    out = {"batch": name, "streams": n, "plain_bytes": total, "stream_bytes": int(res["out_len"].sum()),
           "inflate_batch of the whole streams goes by blocks": ctx.last_inflate_blocks() > 0, "prefixes": []}
    for p in PREFIXES:
        room_off = np.arange(n, dtype=np.uint64) * np.uint64(p)
        rooms = torch.zeros(n * p + 256, dtype=torch.uint8, device=dev)
        d_pre = batch.to_device(batch.make_descs(comp_off, res["out_len"], room_off, np.full(n, p, np.uint64)), dev)
        d_pres = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
        d_small = torch.zeros(n * 16, dtype=torch.uint8, device=dev)

        def prefix():
            batch.inflate_prefix_batch(ctx, comp, rooms, d_pre, d_pres, n, sync=False)

        def too_small():
            batch.inflate_batch(ctx, comp, rooms, d_pre, d_small, n, p, 0, sync=False)

        prefix()
        ctx.synchronize()
        got, o = batch.prefix_results_from_device(d_pres), rooms.cpu().numpy()
        want_len = np.minimum(lens, np.uint64(p))
        equal = bool((got["status"] == 0).all() and (got["out_len"] == want_len).all() and (got["ended"] == (lens <= p)).all() and
                     all(np.array_equal(o[i * p:i * p + int(want_len[i])], host[int(offs[i]):int(offs[i]) + int(want_len[i])])
                         for i in range(0, n, max(1, n // 500))))
        ms = alternate({"prefix": prefix, "inflate_batch_whole": decode_whole, "inflate_batch_dst_cap_is_the_prefix": too_small})
        out["prefixes"].append({"prefix_bytes": p, "streams_cut": int((lens > p).sum()), "results_and_bytes_equal": equal, "ms": ms,
                                "whole_over_prefix": round(ms["inflate_batch_whole"]["median"] / ms["prefix"]["median"], 2),
                                "prefix_minus_too_small_ms": round(ms["prefix"]["median"] - ms["inflate_batch_dst_cap_is_the_prefix"]["median"], 4)})
        del rooms
    return out


def main():
    out = {"rounds": ROUNDS, "crc_op": 0, "level": "default", "batches": []}
    only = os.environ.get("PREFIX_BENCH_ONLY", "c2,long,ragged").split(",")
    text = text_bytes()
    if "c2" in only:
        src = synth.batch_bytes_torch(2, 0, N_C2, L_C2, 4, dev)
        out["batches"].append(run("c2: %d x %d B of 4-bit symbols" % (N_C2, L_C2), src, np.arange(N_C2, dtype=np.uint64) * np.uint64(L_C2),
                                  np.full(N_C2, L_C2, np.uint64)))
        del src
        torch.cuda.empty_cache()
    for key, lens in (("long", np.full(N_LONG, LONG, np.uint64)),
                      ("ragged", np.random.default_rng(3).integers(1, 65537, N_RAGGED).astype(np.uint64))):
        if key not in only:
            continue
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
        parts = []
        for i, n in enumerate(lens.tolist()):  # every stream begins somewhere else in the text
            at = 7919 * i % len(text)
            parts.append((text[at:] + text * (n // len(text) + 1))[:n])
        src = torch.from_numpy(np.frombuffer(b"".join(parts), np.uint8).copy()).to(dev)
        name = "long: %d x 1 MiB of text" % N_LONG if key == "long" else "ragged: %d streams of 1 B .. 64 KiB of text" % N_RAGGED
        out["batches"].append(run(name, src, offs, lens))
        del src
        torch.cuda.empty_cache()
    print(json.dumps(out))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
