#!/usr/bin/env python3
"""What the ragged checksum pass (zipc_hip_checksum_batch) costs, against the only way there was before it: a loop of
zipc_hip_checksum_device calls, one range each.  In one process, on device-resident random bytes:
  uniform  16 384 ranges x 64 KiB (1 GiB): the batch call, CRC alone and both checksums; the loop it replaces (timed over
           LOOP_RANGES of the ranges and scaled: every call is the same work); one checksum_device call over the same
           1 GiB, which is the ceiling -- one range, the rectangular pass, the parallel Adler chain;
  ragged   one range of 64 MiB among 10 000 ranges of 1 to 3000 bytes: the batch call; its parts alone (the long range as a
           batch of one, the short ones as a batch of their own); the loop over all of them;
  long     the 64 MiB range alone, both checksums: the batch (its Adler-32 finish walks the 12 088 chunk sums on one lane)
           against checksum_device (runs, scans, replay).
The forms of a group are timed in alternation, ROUNDS times over, after a warm-up; a timing is a host clock around REPS
calls enqueued back to back with one synchronize at the end (the loop: one synchronize per call, as its callers have to,
because every call writes the same two words).  Results are compared before anything is timed.  One JSON line."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import zipc_amd
from zipc_amd import _lib, batch

N_UNI, L_UNI = int(os.environ.get("CHECKSUM_BENCH_RANGES", 16384)), 65536
N_SHORT, LONG = int(os.environ.get("CHECKSUM_BENCH_SHORT", 10000)), int(os.environ.get("CHECKSUM_BENCH_LONG", 64 << 20))
LOOP_RANGES = int(os.environ.get("CHECKSUM_BENCH_LOOP", 1024))
ROUNDS, REPS = int(os.environ.get("CHECKSUM_BENCH_ROUNDS", 7)), 3
dev = torch.device("cuda", 0)
ctx = zipc_amd.Context(0)
lib = _lib.lib()

arena = torch.randint(0, 256, (max(N_UNI * L_UNI, LONG + 3000 * N_SHORT + 64),), dtype=torch.uint8, device=dev)
out2 = torch.zeros(2, dtype=torch.int32, device=dev)
torch.cuda.synchronize()


class Batch:
    def __init__(self, off, length):
        self.n, self.total = len(off), int(np.sum(length))
        self.off, self.len = off, length
        self.d_ranges = batch.to_device(batch.make_ranges(off, length), dev)
        self.d_res = torch.zeros(self.n * 16, dtype=torch.uint8, device=dev)

    def call(self, crc, adler):
        batch.checksum_batch(ctx, arena, self.d_ranges, self.d_res, self.n, self.total, crc, adler, sync=False)

    def results(self):
        ctx.synchronize()
        return batch.checksum_results_from_device(self.d_res)


def device_one(off, n, crc, adler):
    ctx.check(lib.zipc_hip_checksum_device(ctx.handle, arena.data_ptr() + int(off), int(n), int(crc), int(adler), out2.data_ptr()))


def loop(b, crc, adler, count):
    for k in range(count):
        device_one(b.off[k], b.len[k], crc, adler)
        ctx.synchronize()


def timed(fn, reps=REPS):
    t0 = time.perf_counter()
    for _ in range(reps): fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def measure(forms):
    """forms: {name: (fn, reps, scale)} -> {name: [ms per call, one per round]}, alternating"""
    for fn, _, _ in forms.values(): fn()
    ctx.synchronize()
    ms = {k: [] for k in forms}
    for _ in range(ROUNDS):
        for k, (fn, reps, scale) in forms.items():
            ms[k].append(timed(fn, reps) * scale)
    return ms


def same_as_device(b, picks):
    res = b.results()
    ok = bool((res["status"] == 0).all())
    for k in picks:
        device_one(b.off[k], b.len[k], 1, 1)
        ctx.synchronize()
        v = out2.cpu().numpy().view(np.uint32)
        ok = ok and (int(res["crc32"][k]), int(res["adler32"][k])) == (int(v[0]), int(v[1]))
    return ok


i = np.arange(N_UNI, dtype=np.uint64)
uni = Batch(i * np.uint64(L_UNI), np.full(N_UNI, L_UNI, np.uint64))
rng = np.random.default_rng(1)
short_len = rng.integers(1, 3001, N_SHORT).astype(np.uint64)
short_off = np.uint64(LONG) + np.concatenate([[0], np.cumsum(short_len)[:-1]]).astype(np.uint64)
mid = N_SHORT // 2
rag = Batch(np.concatenate([short_off[:mid], [0], short_off[mid:]]).astype(np.uint64), np.concatenate([short_len[:mid], [LONG], short_len[mid:]]).astype(np.uint64))
shorts = Batch(short_off, short_len)
long1 = Batch(np.array([0], np.uint64), np.array([LONG], np.uint64))

uni.call(1, 1); rag.call(1, 1); long1.call(1, 1)
equal = {"uniform": same_as_device(uni, range(0, N_UNI, max(N_UNI // 16, 1))), "ragged": same_as_device(rag, [0, mid, rag.n - 1]),
         "long": same_as_device(long1, [0])}
loop_n = min(LOOP_RANGES, N_UNI)
groups = {
    "uniform": measure({
        "batch_crc": (lambda: uni.call(1, 0), REPS, 1.0),
        "batch_both": (lambda: uni.call(1, 1), REPS, 1.0),
        "loop_crc": (lambda: loop(uni, 1, 0, loop_n), 1, N_UNI / loop_n),
        "loop_both": (lambda: loop(uni, 1, 1, loop_n), 1, N_UNI / loop_n),
        "one_call_crc": (lambda: device_one(0, N_UNI * L_UNI, 1, 0), REPS, 1.0),
        "one_call_both": (lambda: device_one(0, N_UNI * L_UNI, 1, 1), REPS, 1.0)}),
    "ragged": measure({
        "batch_crc": (lambda: rag.call(1, 0), REPS, 1.0),
        "batch_both": (lambda: rag.call(1, 1), REPS, 1.0),
        "long_alone_crc": (lambda: long1.call(1, 0), REPS, 1.0),
        "short_alone_crc": (lambda: shorts.call(1, 0), REPS, 1.0),
        "long_alone_both": (lambda: long1.call(1, 1), REPS, 1.0),
        "short_alone_both": (lambda: shorts.call(1, 1), REPS, 1.0),
        "loop_crc": (lambda: loop(rag, 1, 0, min(LOOP_RANGES, mid)), 1, rag.n / min(LOOP_RANGES, mid))}),
    "long": measure({
        "batch_both": (lambda: long1.call(1, 1), REPS, 1.0),
        "batch_adler": (lambda: long1.call(0, 1), REPS, 1.0),
        "checksum_device_both": (lambda: device_one(0, LONG, 1, 1), REPS, 1.0),
        "checksum_device_adler": (lambda: device_one(0, LONG, 0, 1), REPS, 1.0)}),
}
ctx.set_profiling(True)
ctx.reset_kernel_times()
for _ in range(REPS): rag.call(1, 1)
ctx.synchronize()
kernels_ragged = {k: round(v[1] / v[0], 4) for k, v in ctx.kernel_times().items() if v[0]}
ctx.reset_kernel_times()
for _ in range(REPS): uni.call(1, 1)
ctx.synchronize()
kernels_uniform = {k: round(v[1] / v[0], 4) for k, v in ctx.kernel_times().items() if v[0]}
ctx.set_profiling(False)
print(json.dumps({
    "config": {"uniform": "%d ranges x %d B" % (N_UNI, L_UNI), "ragged": "one range of %d B among %d of 1 to 3000 B (%d B)" % (LONG, N_SHORT, rag.total),
               "long": "one range of %d B" % LONG, "loop": "checksum_device per range with a synchronize each, timed over %d ranges and scaled" % loop_n},
    "rounds": ROUNDS, "reps_per_timing": REPS, "equal_to_checksum_device": equal,
    "ms_median": {g: {k: round(statistics.median(v), 4) for k, v in ms.items()} for g, ms in groups.items()},
    "ms_min_max": {g: {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()} for g, ms in groups.items()},
    "kernel_ms_per_launch": {"ragged_both": kernels_ragged, "uniform_both": kernels_uniform},
    "note": "the ragged loop is timed over short ranges only and scaled by the number of ranges: it leaves out the long range's own call"}))
