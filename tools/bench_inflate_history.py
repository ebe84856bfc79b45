#!/usr/bin/env python3
"""What the history forms (zipc_hip_inflate_history_batch and its siblings; csrc/inflate_history.h) cost, against the calls
there were before them.  Device-resident streams, three measurements:

  null     16 384 streams x 64 KiB of 4-bit symbols at `Default (the benchmark's C2 data), CRC_NOP: the history form with a
           null d_hist against zipc_hip_inflate_batch over the same descriptors.  It is the same wave: a difference outside
           the spread of the plain call is a finding.
  dict     the same shape as zlib streams made by Python's zlib (level 1) against a dictionary of 4 KiB and of 32 KiB,
           through zipc_hip_zlib_decompress_dict_batch, against zipc_hip_zlib_decompress_batch over the same records made
           without one: what the dictionary's checksum, the open and the seed cost.  DICT_DISTINCT records are compressed on
           the host and the arena repeats them (the decode does not know); the context compares RFC 1950's Adler-32.
  chunks   one stream of 64 MiB of text, deflated by Python's zlib with a Z_SYNC_FLUSH every CHUNK bytes of input (an access
           point per chunk at a byte boundary, start_bit 0, the window kept: every chunk needs the 32 KiB in front of it),
           read as chunks through zipc_hip_inflate_prefix_history_batch, each in a room of its own with its history in
           front -- all chunks in one call, and one chunk from the middle alone -- against zipc_hip_inflate_batch of the
           whole stream, which goes by blocks and is the only way there was to read the middle of it.  Access points at
           other bits of a byte are not measured here (tests/test_gpu_inflate_history.py decodes from all eight).

Per measurement the calls are timed in alternation, ROUNDS times over, after a warm-up of each; a timing is a host clock
around one call with one synchronize at its end.  Results and bytes are compared before anything is timed.  One JSON
object on stdout (and in --out FILE).  Run from the repository's root."""
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
from zipc_amd import batch, synth  # noqa: E402

N, L = int(os.environ.get("HISTORY_BENCH_STREAMS", 16384)), 65536
DICT_DISTINCT = int(os.environ.get("HISTORY_BENCH_DISTINCT", 256))
LONG = int(os.environ.get("HISTORY_BENCH_LONG", 64 << 20))
CHUNK = int(os.environ.get("HISTORY_BENCH_CHUNK", 256 << 10))
ROUNDS, LEVEL = int(os.environ.get("HISTORY_BENCH_ROUNDS", 7)), 2
HIST = 32768
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


def to_dev(b):
    return torch.from_numpy(np.frombuffer(b, np.uint8).copy()).to(dev)


def null_records():
    src = synth.batch_bytes_torch(2, 0, N, L, 4, dev)
    cap = batch.deflate_bound(L)
    descs = batch.uniform_layout(N, L, cap)
    comp = torch.zeros(N * int(descs["dst_off"][1]) + 256, dtype=torch.uint8, device=dev)
    d_res = torch.zeros(N * 16, dtype=torch.uint8, device=dev)
    batch.deflate_batch(ctx, src, comp, batch.to_device(descs, dev), d_res, N, L, N * L, LEVEL, 0)
    res = batch.results_from_device(d_res)
    assert (res["status"] == 0).all()
    d_in = batch.to_device(batch.compact_descs(res, descs, L), dev)
    out_a = torch.zeros(N * L + 256, dtype=torch.uint8, device=dev)
    out_b = torch.zeros(N * L + 256, dtype=torch.uint8, device=dev)
    r_a, r_b = torch.zeros(N * 16, dtype=torch.uint8, device=dev), torch.zeros(N * 16, dtype=torch.uint8, device=dev)
    plain = lambda: batch.inflate_batch(ctx, comp, out_a, d_in, r_a, N, L, 0, sync=False)
    hist = lambda: batch.inflate_history_batch(ctx, comp, out_b, d_in, None, r_b, N, L, 0, sync=False)
    plain(), hist()
    ctx.synchronize()
    equal = bool(torch.equal(out_a, out_b) and torch.equal(r_a, r_b) and torch.equal(out_a[:N * L], src))
    ms = alternate({"inflate_batch": plain, "inflate_history_batch_null_d_hist": hist})
    return {"measurement": "null: %d x %d B of 4-bit symbols, CRC_NOP" % (N, L), "results_and_bytes_equal": equal, "ms": ms,
            "history_minus_plain_ms": round(ms["inflate_history_batch_null_d_hist"]["median"] - ms["inflate_batch"]["median"], 4),
            "spread_of_the_plain_call_ms": round(ms["inflate_batch"]["max"] - ms["inflate_batch"]["min"], 4)}


def dictionaries():
    k = min(DICT_DISTINCT, N)
    records = [synth.stream_bytes_np(2, j, L, 4).tobytes() for j in range(k)]
    out = {"measurement": "dict: %d zlib streams of %d B (%d distinct, level 1), RFC 1950's Adler-32" % (N, L, k), "dictionaries": []}
    ctx.set_adler_rfc1950(True)

    def arena(streams):
        lens = [len(s) for s in streams]
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
        pick = np.arange(N) % k
        return to_dev(b"".join(streams) + b"\0" * 64), offs[pick], np.array(lens, np.uint64)[pick]

    plain_src, plain_off, plain_len = arena([zlib.compress(r, 1) for r in records])
    for dict_len in (4096, HIST):
        d = synth.stream_bytes_np(2, 99999, HIST, 4).tobytes()[:dict_len]
        streams = []
        for r in records:
            co = zlib.compressobj(1, zlib.DEFLATED, 15, zdict=d)
            streams.append(co.compress(r) + co.flush())
        src, off, lens = arena(streams)
        stride = HIST + L + 256
        dst_off = np.arange(N, dtype=np.uint64) * np.uint64(stride) + np.uint64(HIST)
        dst = torch.zeros(N * stride + 256, dtype=torch.uint8, device=dev)
        d_dict = batch.to_device(batch.make_descs(off, lens, dst_off, np.full(N, L, np.uint64)), dev)
        d_plain = batch.to_device(batch.make_descs(plain_off, plain_len, dst_off, np.full(N, L, np.uint64)), dev)
        r_a, r_b = torch.zeros(N * 16, dtype=torch.uint8, device=dev), torch.zeros(N * 16, dtype=torch.uint8, device=dev)
        dict_dev = to_dev(d)
        with_dict = lambda: batch.zlib_decompress_dict_batch(ctx, src, dst, d_dict, r_a, N, L, dict_dev, dict_len, sync=False)
        without = lambda: batch.zlib_decompress_batch(ctx, plain_src, dst, d_plain, r_b, N, L, sync=False)
        with_dict()
        ctx.synchronize()
        ra = batch.results_from_device(r_a)
        host = dst.cpu().numpy()
        equal = bool((ra["status"] == 0).all() and (ra["out_len"] == L).all() and
                     all(host[int(dst_off[i]):int(dst_off[i]) + L].tobytes() == records[i % k] and
                         host[int(dst_off[i]) - dict_len:int(dst_off[i])].tobytes() == d for i in range(0, N, max(1, N // 200))))
        del host
        without()
        ctx.synchronize()
        assert (batch.results_from_device(r_b)["status"] == 0).all()
        ms = alternate({"zlib_decompress_dict_batch": with_dict, "zlib_decompress_batch_without_a_dictionary": without})
        out["dictionaries"].append({"dict_bytes": dict_len, "stream_bytes_with": int(lens.sum()), "stream_bytes_without": int(plain_len.sum()),
                                    "results_bytes_and_gaps_equal": equal, "ms": ms,
                                    "dict_minus_plain_ms": round(ms["zlib_decompress_dict_batch"]["median"] -
                                                                 ms["zlib_decompress_batch_without_a_dictionary"]["median"], 4)})
        del dst, src
        torch.cuda.empty_cache()
    ctx.set_adler_rfc1950(False)
    return out


def chunks():
    z = zipfile.ZipFile(os.path.join(ROOT, "tests", "golden", "zip-docs.zip"))
    text = z.read("zip-docs/APPNOTE.TXT") + z.read("zip-docs/rfc1951.txt")
    plain = (text * (LONG // len(text) + 1))[:LONG]
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    parts, points, pos = [], [], 0
    for at in range(0, LONG, CHUNK):
        points.append(pos)  # the access point of this chunk: a byte of the stream, bit 0
        last = at + CHUNK >= LONG
        piece = co.compress(plain[at:at + CHUNK]) + (co.flush() if last else co.flush(zlib.Z_SYNC_FLUSH))
        parts.append(piece)
        pos += len(piece)
    raw = b"".join(parts)
    n = len(points)
    src = to_dev(raw + b"\0" * 64)
    d_plain = to_dev(plain)
    stride = HIST + CHUNK + 256
    room_off = np.arange(n, dtype=np.uint64) * np.uint64(stride) + np.uint64(HIST)
    rooms = torch.zeros(n * stride + 256, dtype=torch.uint8, device=dev)
    hist_len = np.minimum(np.arange(n, dtype=np.uint64) * np.uint64(CHUNK), np.uint64(HIST))
    for i in range(1, n):  # what an index holds beside the position: the 32 KiB in front of it
        o, h = int(room_off[i]), int(hist_len[i])
        rooms[o - h:o] = d_plain[i * CHUNK - h:i * CHUNK]
    caps = np.minimum(np.uint64(CHUNK), np.uint64(LONG) - np.arange(n, dtype=np.uint64) * np.uint64(CHUNK))
    d_descs = batch.to_device(batch.make_descs(np.array(points, np.uint64), np.uint64(len(raw)) - np.array(points, np.uint64), room_off, caps), dev)
    d_hist = batch.to_device(batch.make_history(hist_len), dev)
    d_res = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    mid = n // 2
    all_chunks = lambda: batch.inflate_prefix_history_batch(ctx, src, rooms, d_descs, d_hist, d_res, n, sync=False)
    one_chunk = lambda: batch.inflate_prefix_history_batch(ctx, src, rooms, d_descs[mid * 48:], d_hist[mid * 8:], d_res[mid * 16:], 1, sync=False)
    whole_dst = torch.zeros(LONG + 256, dtype=torch.uint8, device=dev)
    d_whole = batch.to_device(batch.make_descs([0], [len(raw)], [0], [LONG]), dev)
    r_whole = torch.zeros(16, dtype=torch.uint8, device=dev)
    whole = lambda: batch.inflate_batch(ctx, src, whole_dst, d_whole, r_whole, 1, LONG, 0, sync=False)
    all_chunks()
    ctx.synchronize()
    got = batch.prefix_results_from_device(d_res)
    equal = bool((got["status"] == 0).all() and (got["out_len"] == caps).all() and (got["ended"][:-1] == 0).all() and got["ended"][-1] == 1 and
                 all(torch.equal(rooms[int(room_off[i]):int(room_off[i]) + int(caps[i])], d_plain[i * CHUNK:i * CHUNK + int(caps[i])]) for i in range(n)))
    whole()
    ctx.synchronize()
    by_blocks = ctx.last_inflate_blocks()
    assert int(batch.results_from_device(r_whole)["status"][0]) == 0 and torch.equal(whole_dst[:LONG], d_plain)
    ms = alternate({"prefix_history_batch_all_chunks": all_chunks, "prefix_history_batch_one_middle_chunk": one_chunk, "inflate_batch_whole_stream": whole})
    return {"measurement": "chunks: one stream of %d B of text, an access point every %d B (%d chunks), histories of 32 KiB" % (LONG, CHUNK, n),
            "stream_bytes": len(raw), "inflate_batch_blocks": by_blocks, "results_and_bytes_equal": equal, "ms": ms,
            "whole_over_all_chunks": round(ms["inflate_batch_whole_stream"]["median"] / ms["prefix_history_batch_all_chunks"]["median"], 2),
            "whole_over_one_chunk": round(ms["inflate_batch_whole_stream"]["median"] / ms["prefix_history_batch_one_middle_chunk"]["median"], 2)}


def main():
    only = os.environ.get("HISTORY_BENCH_ONLY", "null,dict,chunks").split(",")
    out = {"rounds": ROUNDS, "measurements": []}
    for key, fn in (("null", null_records), ("dict", dictionaries), ("chunks", chunks)):
        if key in only:
            out["measurements"].append(fn())
            torch.cuda.empty_cache()
    print(json.dumps(out))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
