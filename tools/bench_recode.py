#!/usr/bin/env python3
"""What recoding on the device saves: 4096 streams x 64 KiB of C2's generator (4-bit symbols), compressed at `Best,
recoded to `Default, in one process:
  (a) device-resident: zipc_hip_recode_batch against zipc_hip_inflate_batch (CRC-32), the results read back, the link
      rule on the host (numpy), the descriptors sent, zipc_hip_deflate_batch -- the three steps the header defines it by;
  (b) host-resident:   zipc_hip_recode_many against zipc_hip_inflate_many followed by zipc_hip_deflate_many, which is
      what `zipc-hip recode --deflate` did before Archive::recode_deflated.
The two calls of a pair are timed in alternation, ROUNDS times over, after a warm-up; a timing is a host clock around
REPS calls (device forms: enqueued back to back, one synchronize at the end).  The bytes that cross the bus are counted
from the descriptors and results.  One JSON line."""
import ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import zipc_amd
from zipc_amd import _lib, batch, synth

N, L, BITS = int(os.environ.get("RECODE_BENCH_STREAMS", 4096)), 65536, 4
FROM_LEVEL, TO_LEVEL = 3, 2
ROUNDS, REPS = int(os.environ.get("RECODE_BENCH_ROUNDS", 9)), 3
dev = torch.device("cuda", 0)
ctx = zipc_amd.Context(0)
lib = _lib.lib()

# ---- the workload: the streams as `Best leaves them, in their slots of deflate's bound
plain = synth.batch_bytes_torch(2, 0, N, L, BITS, dev)
cap = batch.deflate_bound(L)
cdescs = batch.uniform_layout(N, L, cap)
slot = int(cdescs["dst_off"][1]) if N > 1 else (cap + 255) // 256 * 256
comp = torch.zeros(N * slot + 256, dtype=torch.uint8, device=dev)
d_cres = torch.zeros(N * 16, dtype=torch.uint8, device=dev)
batch.deflate_batch(ctx, plain, comp, batch.to_device(cdescs, dev), d_cres, N, L, N * L, FROM_LEVEL, 1)
cres = batch.results_from_device(d_cres)
assert (cres["status"] == 0).all()
src_len, crc = cres["out_len"].copy(), cres["checksum"].copy()
i = np.arange(N, dtype=np.uint64)

# ---- (a) on the device
rdescs = batch.make_recode_descs(i * np.uint64(slot), src_len, i * np.uint64(L), np.full(N, L, np.uint64), i * np.uint64(slot),
                                 np.full(N, cap, np.uint64), limit=np.full(N, L, np.uint64), expect_crc32=crc)
d_rdescs = batch.to_device(rdescs, dev)
mid = torch.zeros(N * L + 256, dtype=torch.uint8, device=dev)
out_r = torch.zeros(N * slot + 256, dtype=torch.uint8, device=dev)
out_3 = torch.zeros(N * slot + 256, dtype=torch.uint8, device=dev)
d_rres = torch.zeros(N * 32, dtype=torch.uint8, device=dev)
d_ires = torch.zeros(N * 16, dtype=torch.uint8, device=dev)
d_dres = torch.zeros(N * 16, dtype=torch.uint8, device=dev)
idescs = batch.make_descs(rdescs["src_off"], src_len, rdescs["mid_off"], rdescs["mid_cap"], limit=rdescs["limit"])
d_idescs = batch.to_device(idescs, dev)
batch.reserve(ctx, N, L, N * L)


def recode_batch():
    batch.recode_batch(ctx, comp, mid, out_r, d_rdescs, d_rres, N, L, N * L, TO_LEVEL, sync=False)


def three_steps():
    batch.inflate_batch(ctx, comp, mid, d_idescs, d_ires, N, L, 1, sync=False)
    ctx.synchronize()
    ires = batch.results_from_device(d_ires)
    go = (ires["status"] == 0) & (ires["checksum"] == crc)  # the link rule
    dd = batch.make_descs(rdescs["mid_off"], np.where(go, ires["out_len"], 0), rdescs["dst_off"], np.where(go, rdescs["dst_cap"], 0))
    batch.deflate_batch(ctx, mid, out_3, batch.to_device(dd, dev), d_dres, N, L, N * L, TO_LEVEL, 0, sync=False)


def timed_device(fn):
    t0 = time.perf_counter()
    for _ in range(REPS): fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) / REPS * 1e3


for fn in (recode_batch, three_steps): fn()
ctx.synchronize()
rres, dres = batch.recode_results_from_device(d_rres), batch.results_from_device(d_dres)
ok_a = bool((rres["status"] == 0).all() and (dres["status"] == 0).all() and (rres["out_len"] == dres["out_len"]).all()
            and (rres["checksum"] == crc).all() and (rres["mid_len"] == L).all() and torch.equal(out_r, out_3) and torch.equal(mid[:N * L], plain))
ms = {"recode_batch": [], "inflate_batch+host_link+deflate_batch": [], "recode_many": [], "inflate_many+deflate_many": []}
for _ in range(ROUNDS):
    ms["recode_batch"].append(timed_device(recode_batch))
    ms["inflate_batch+host_link+deflate_batch"].append(timed_device(three_steps))
out_len = rres["out_len"].copy()

# ---- (b) from host memory
comp_h = comp.cpu().numpy()
h_src = [comp_h[k * slot:k * slot + int(src_len[k])].copy() for k in range(N)]
del comp, out_r, out_3, mid, plain
P, S = C.c_void_p * N, C.c_size_t * N
p_src, s_src = P(*[a.ctypes.data for a in h_src]), S(*[int(v) for v in src_len])
h_out_r = [np.zeros(cap, np.uint8) for _ in range(N)]
h_mid = [np.zeros(L, np.uint8) for _ in range(N)]
h_out_2 = [np.zeros(cap, np.uint8) for _ in range(N)]
p_out_r, p_mid, p_out_2 = (P(*[a.ctypes.data for a in arrs]) for arrs in (h_out_r, h_mid, h_out_2))
s_L, s_cap = S(*([L] * N)), S(*([cap] * N))
u_crc = (C.c_uint32 * N)(*[int(v) for v in crc])
res_r, res_i, res_d = (_lib.RecodeResult * N)(), (_lib.StreamResult * N)(), (_lib.StreamResult * N)()


def recode_many():
    assert lib.zipc_hip_recode_many(ctx.handle, N, p_src, s_src, s_L, u_crc, s_L, TO_LEVEL, p_out_r, s_cap, res_r) == 0


def inflate_then_deflate_many():
    assert lib.zipc_hip_inflate_many(ctx.handle, N, p_src, s_src, s_L, 1, p_mid, s_L, res_i) == 0
    assert lib.zipc_hip_deflate_many(ctx.handle, N, p_mid, s_L, TO_LEVEL, 1, p_out_2, s_cap, res_d) == 0


def timed_host(fn):
    t0 = time.perf_counter()
    for _ in range(REPS): fn()
    return (time.perf_counter() - t0) / REPS * 1e3


for fn in (recode_many, inflate_then_deflate_many): fn()  # warm: buffer growth, first touch of the pinned memory
ok_b = all(int(res_r[k].status) == 0 and int(res_d[k].status) == 0 and int(res_r[k].out_len) == int(res_d[k].out_len) == int(out_len[k])
           and int(res_r[k].checksum) == int(res_d[k].checksum) == int(crc[k]) for k in range(N))
ok_b = ok_b and all(np.array_equal(h_out_r[k][:int(out_len[k])], h_out_2[k][:int(out_len[k])]) for k in range(0, N, 61))
for _ in range(ROUNDS):
    ms["recode_many"].append(timed_host(recode_many))
    ms["inflate_many+deflate_many"].append(timed_host(inflate_then_deflate_many))

med = {k: statistics.median(v) for k, v in ms.items()}
src_total, out_total, packed_total = int(src_len.sum()), int(out_len.sum()), int(((out_len + 15) // 16 * 16).sum())
print(json.dumps({
    "config": "%d streams x %d B of %d-bit symbols (C2's generator), compressed at best, recoded to default" % (N, L, BITS),
    "rounds": ROUNDS, "reps_per_timing": REPS, "device_forms_equal": ok_a, "host_forms_equal": ok_b,
    "ms_median": {k: round(v, 3) for k, v in med.items()},
    "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
    "ratio_batch": round(med["recode_batch"] / med["inflate_batch+host_link+deflate_batch"], 4),
    "ratio_many": round(med["recode_many"] / med["inflate_many+deflate_many"], 4),
    "decompressed_bytes": N * L, "compressed_bytes_in": src_total, "compressed_bytes_out": out_total,
    "bus_bytes": {
        "recode_batch": {"to_device": 0, "to_host": 0},
        "inflate_batch+host_link+deflate_batch": {"to_device": N * 48, "to_host": N * 16},
        "recode_many": {"to_device": src_total + N * (48 + 64), "to_host": packed_total + N * (16 + 32)},
        "inflate_many+deflate_many": {"to_device": src_total + N * L + 2 * N * 48, "to_host": N * L + packed_total + 2 * N * 16}},
    "note": "bus_bytes: payload, descriptors and results; the many-stream forms send a stream's source up to its 256-byte slot "
            "boundary, which is not counted"}))
