#!/usr/bin/env python3
"""What the packed decode (zipc_hip_inflate_packed_batch) costs against the way there was before it, INTEGRATION.md's
size-then-decode recipe on the same build: a sizing call, a synchronize, n x 16 bytes of results copied back, the layout
in numpy, n x 48 bytes of descriptors uploaded, zipc_hip_inflate_batch.  Device-resident streams, CRC_NOP, align 256:
  c2      16 384 streams x 64 KiB of 4-bit symbols at `Default (the benchmark's C2 data): sized by one wave a stream, the
          packed call enqueue-only;
  ragged  10 000 streams of 1 B .. 3000 B of text: the same path where the fixed costs are all there is;
  long    64 streams of 1 MiB of text among 3200 short ones (the block-path test's batch, scaled), max_out_len 1 MiB: both
          ways size by blocks and decode by blocks, and both synchronise on the way.
Per shape the three forms -- packed, recipe, and zipc_hip_inflate_batch alone over descriptors that are already there (the
floor: what is left when the sizes are known) -- are timed in alternation, ROUNDS times over, after a warm-up of each; a
timing is a host clock around one call with one synchronize at its end (the recipe's own synchronize and copies lie inside
it, as they do for its callers).  Results and arenas of the two ways are compared before anything is timed.  Then the
kernels of REPS packed calls by HIP events (packed_layout and packed_close among them).  One JSON object on stdout (and in
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

N_C2, L_C2 = int(os.environ.get("PACKED_BENCH_STREAMS", 16384)), 65536
N_RAGGED = int(os.environ.get("PACKED_BENCH_RAGGED", 10000))
N_LONG, LONG, SHORT_PER_LONG = int(os.environ.get("PACKED_BENCH_LONG", 64)), 1 << 20, 50
ROUNDS, REPS, ALIGN, LEVEL = int(os.environ.get("PACKED_BENCH_ROUNDS", 7)), 3, 256, 2
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
    return ms


class Shape:
    """plain: a uint8 cuda tensor, stream i of it lens[i] bytes at offs[i] -> the streams deflated on the device, and the three forms"""

    def __init__(self, name, plain, offs, lens, max_out_len):
        self.name, self.n, self.max_out_len, self.total = name, len(lens), max_out_len, int(np.sum(lens))
        caps = np.array([batch.deflate_bound(int(v)) for v in np.unique(lens)], np.uint64)[np.searchsorted(np.unique(lens), lens)]
        slots = (caps + np.uint64(255)) // np.uint64(256) * np.uint64(256)
        comp_off = np.concatenate([[0], np.cumsum(slots)[:-1]]).astype(np.uint64)
        self.comp = torch.zeros(int(slots.sum()) + 256, dtype=torch.uint8, device=dev)
        d_res = torch.zeros(self.n * 16, dtype=torch.uint8, device=dev)
        batch.deflate_batch(ctx, plain, self.comp, batch.to_device(batch.make_descs(offs, lens, comp_off, caps), dev), d_res, self.n,
                            int(lens.max()), self.total, LEVEL, 0)
        res = batch.results_from_device(d_res)
        assert (res["status"] == 0).all()
        self.src_bytes = int(res["out_len"].sum())
        # what a caller of either way has: the streams, no sizes
        self.descs = batch.make_descs(comp_off, res["out_len"], np.zeros(self.n, np.uint64), np.zeros(self.n, np.uint64))
        self.d_descs = batch.to_device(self.descs, dev)
        rooms = (lens.astype(np.uint64) + np.uint64(ALIGN - 1)) // np.uint64(ALIGN) * np.uint64(ALIGN)
        self.arena_len = int(rooms.sum())
        self.dst = [torch.zeros(self.arena_len + 256, dtype=torch.uint8, device=dev) for _ in range(2)]
        self.d_packed = torch.zeros(self.n * 32, dtype=torch.uint8, device=dev)
        self.d_sized = torch.zeros(self.n * 16, dtype=torch.uint8, device=dev)
        self.d_res = torch.zeros(self.n * 16, dtype=torch.uint8, device=dev)
        self.d_need = torch.zeros(8, dtype=torch.uint8, device=dev)
        known = self.descs.copy()
        known["dst_off"] = np.concatenate([[0], np.cumsum(rooms)[:-1]]).astype(np.uint64)
        known["dst_cap"] = lens
        self.known = known
        self.d_known = batch.to_device(known, dev)
        self.by_blocks = max_out_len >= 256 << 10
        torch.cuda.synchronize()

    def packed(self):
        batch.inflate_packed_batch(ctx, self.comp, self.dst[0], self.d_descs, self.d_packed, self.n, self.max_out_len, ALIGN, 0, self.d_need,
                                   dst_arena_len=self.arena_len, sync=False)

    def recipe(self):
        if self.by_blocks:
            batch.inflate_size_blocks_batch(ctx, self.comp, self.d_descs, self.d_sized, self.n)  # (synchronises by itself)
        else:
            batch.inflate_size_batch(ctx, self.comp, self.d_descs, self.d_sized, self.n, sync=False)
            ctx.synchronize()
        sized = batch.results_from_device(self.d_sized)
        ok = (sized["status"] == 0) & (sized["out_len"] <= self.max_out_len)
        size = np.where(ok, sized["out_len"], 0).astype(np.uint64)
        rooms = (size + np.uint64(ALIGN - 1)) // np.uint64(ALIGN) * np.uint64(ALIGN)
        d = self.descs.copy()
        d["dst_off"] = np.concatenate([[0], np.cumsum(rooms)[:-1]]).astype(np.uint64)
        d["dst_cap"] = size
        d["src_len"] = np.where(ok, d["src_len"], 0)
        d_dev = batch.to_device(d, dev)
        torch.cuda.current_stream(dev).synchronize()
        batch.inflate_batch(ctx, self.comp, self.dst[1], d_dev, self.d_res, self.n, self.max_out_len, 0, sync=False)
        self.last = d

    def floor(self):
        batch.inflate_batch(ctx, self.comp, self.dst[1], self.d_known, self.d_res, self.n, self.max_out_len, 0, sync=False)

    def run(self, plain_check):
        self.packed(); self.recipe(); ctx.synchronize()
        p, r = batch.packed_results_from_device(self.d_packed), batch.results_from_device(self.d_res)
        need = int(self.d_need.cpu().numpy().view(np.uint64)[0])
        equal = bool((p["status"] == 0).all() and (r["status"] == 0).all() and (p["out_len"] == r["out_len"]).all()
                     and (p["dst_off"] == self.last["dst_off"]).all() and (p["dst_off"] == self.known["dst_off"]).all()
                     and need <= self.arena_len and torch.equal(self.dst[0], self.dst[1]) and plain_check(self.dst[0]))
        blocks = (ctx.last_size_blocks(), ctx.last_inflate_blocks())
        ms = alternate({"packed": self.packed, "recipe": self.recipe, "inflate_batch_known_sizes": self.floor})
        ctx.set_profiling(True)
        ctx.reset_kernel_times()
        for _ in range(REPS):
            self.packed()
        ctx.synchronize()
        kernels = {k: {"launches_per_call": round(c / REPS, 2), "ms_per_call": round(t / REPS, 4)} for k, (c, t) in sorted(ctx.kernel_times().items()) if c}
        ctx.set_profiling(False)
        med = {k: statistics.median(v) for k, v in ms.items()}
        return {"shape": self.name, "streams": self.n, "plain_bytes": self.total, "stream_bytes": self.src_bytes, "max_out_len": self.max_out_len,
                "sizing": "by blocks (synchronises)" if self.by_blocks else "one wave a stream (enqueue-only)",
                "last_size_blocks, last_inflate_blocks after the recipe": blocks, "results_and_arenas_equal": equal,
                "ms": {k: {"median": round(med[k], 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in ms.items()},
                "packed_over_recipe": round(med["packed"] / med["recipe"], 4), "packed_minus_recipe_ms": round(med["packed"] - med["recipe"], 4),
                "kernels_of_a_packed_call": kernels}


def main():
    out = {"rounds": ROUNDS, "align": ALIGN, "crc_op": 0, "shapes": []}
    only = os.environ.get("PACKED_BENCH_ONLY", "c2,ragged,long").split(",")
    text = text_bytes()
    if "c2" in only:
        src = synth.batch_bytes_torch(2, 0, N_C2, L_C2, 4, dev)
        s = Shape("c2: %d x %d B of 4-bit symbols, level default" % (N_C2, L_C2), src, np.arange(N_C2, dtype=np.uint64) * np.uint64(L_C2),
                  np.full(N_C2, L_C2, np.uint64), L_C2)
        out["shapes"].append(s.run(lambda dst: torch.equal(dst[:N_C2 * L_C2], src)))
        del s, src
        torch.cuda.empty_cache()
    if "ragged" in only:
        lens = np.random.default_rng(1).integers(1, 3001, N_RAGGED).astype(np.uint64)
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
        host = np.frombuffer((text * (int(lens.sum()) // len(text) + 1))[:int(lens.sum())], np.uint8).copy()
        src = torch.from_numpy(host).to(dev)
        s = Shape("ragged: %d streams of 1 B .. 3000 B of text, level default" % N_RAGGED, src, offs, lens, 3000)

        def check(dst, offs=offs, lens=lens, host=host):
            o = dst.cpu().numpy()
            at = np.concatenate([[0], np.cumsum((lens + np.uint64(ALIGN - 1)) // np.uint64(ALIGN) * np.uint64(ALIGN))[:-1]]).astype(np.int64)
            return all(np.array_equal(o[at[i]:at[i] + int(lens[i])], host[int(offs[i]):int(offs[i]) + int(lens[i])]) for i in range(0, len(lens), 97))

        out["shapes"].append(s.run(check))
        del s, src
        torch.cuda.empty_cache()
    if "long" in only:
        lens = []
        rng = np.random.default_rng(2)
        for _ in range(N_LONG):
            k = SHORT_PER_LONG // 2
            lens += list(rng.integers(200, 5000, k)) + [LONG] + list(rng.integers(200, 5000, SHORT_PER_LONG - k))
        lens = np.array(lens, np.uint64)
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
        total = int(lens.sum())
        # every long stream begins somewhere else in the text
        parts = []
        for i, n in enumerate(lens.tolist()):
            at = 7919 * i % len(text)
            parts.append((text[at:] + text * (n // len(text) + 1))[:n])
        host = np.frombuffer(b"".join(parts), np.uint8).copy()
        assert len(host) == total
        src = torch.from_numpy(host).to(dev)
        s = Shape("long: %d streams of 1 MiB of text among %d of 200 B .. 5000 B, level default" % (N_LONG, N_LONG * SHORT_PER_LONG), src, offs,
                  lens, LONG)

        def check_long(dst, offs=offs, lens=lens, host=host):
            o = dst.cpu().numpy()
            at = np.concatenate([[0], np.cumsum((lens + np.uint64(ALIGN - 1)) // np.uint64(ALIGN) * np.uint64(ALIGN))[:-1]]).astype(np.int64)
            return all(np.array_equal(o[at[i]:at[i] + int(lens[i])], host[int(offs[i]):int(offs[i]) + int(lens[i])]) for i in range(0, len(lens), 17))

        out["shapes"].append(s.run(check_long))
    print(json.dumps(out))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
