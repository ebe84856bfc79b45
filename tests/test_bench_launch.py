"""bench.py as the launcher of its own ranks (no GPU here): `--gpus N` starts N worker processes
with the torch.distributed environment, each fails cleanly without a GPU, and the launcher
reports that with a non-zero exit; a --gpus that contradicts WORLD_SIZE is refused."""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def run(args, env_extra=None, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, BENCH] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          timeout=timeout)


def test_gpus_n_spawns_n_ranks_and_fails_cleanly_without_a_gpu():
    for n, config in ((2, "c2"), (3, "c4")):
        r = run(["--gpus", str(n), "--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--config", config])
        err = r.stderr.decode()
        ranks = sorted(int(m.group(1)) for m in re.finditer(r"\[bench\] rank (\d+) of %d " % n, err))
        assert ranks == list(range(n)), err  # the spawned world size equals --gpus
        assert r.returncode != 0 and "workers failed" in err
        # the rank that fails first says why (the launcher stops the others at once); nothing falls back to the CPU
        assert 1 <= err.count("ZIPC_HIP_ERR_NO_DEVICE") <= n
        assert r.stdout.decode().strip() == ""  # and no JSON line is made up


def test_a_dead_rank_stops_the_others_at_once():
    """Rank 1 never arrives (it sleeps for an hour), rank 0 dies without a GPU: the launcher must not wait for
    rank 1 -- on a GPU node the survivors would sit in the rendezvous until the RCCL timeout -- but stop it."""
    import time

    t0 = time.time()
    r = run(["--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu-baseline"], {"ZIPC_BENCH_TEST_HANG_RANK": "1"},
            timeout=120)
    took = time.time() - t0
    err = r.stderr.decode()
    assert r.returncode != 0 and "workers failed" in err and "the others were stopped" in err
    assert took < 60, took
    # nothing of the run is left behind
    ps = subprocess.run(["ps", "-eo", "pid,args"], stdout=subprocess.PIPE).stdout.decode()
    assert not [l for l in ps.splitlines() if "bench.py" in l and "--gpus 2" in l and str(os.getpid()) not in l.split()[0:1]], ps


def test_gpus_must_agree_with_world_size():
    r = run(["--gpus", "2"], {"WORLD_SIZE": "4", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 2 and b"WORLD_SIZE=4" in r.stderr


def test_a_plain_run_leaves_the_cpu_baseline_to_full(monkeypatch):
    """a plain run starts no cpu_baseline process (most of a minute of host time the headline does not need); --full starts
    it, with the same arguments, before anything touches the GPU; --alone-pass is refused without --full"""
    import pytest
    import torch

    import bench

    started = []

    class Done:
        returncode = 0
        stdout = b'{"value": 1.0}\n'

    monkeypatch.setattr(bench.subprocess, "run", lambda cmd, **kw: started.append(cmd) or Done())
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    assert bench.main(["--steps", "1", "--warmup", "0"]) == 3 and started == []
    assert bench.main(["--full", "--steps", "1", "--warmup", "0"]) == 3
    assert len(started) == 1 and started[0][2:] == ["--cpu-baseline-only", "--full", "--steps", "1", "--warmup", "0"]
    with pytest.raises(SystemExit):
        bench.parse_args(["--alone-pass"])
    assert bench.parse_args(["--full", "--alone-pass"]).alone_pass


def test_cpu_baseline_leg_reports_one_thread_and_all_threads():
    import bench

    bench.LEGS["quick"] = (("synth", 2, 4), 2, 65536, (0, 1), True, 1.0)
    line = bench.cpu_leg("quick")
    assert line["cores"] == 1 and line["kind"] == "port" and line["value"] > 0
    assert line["nproc"]["cores"] == (os.cpu_count() or 1) and line["nproc"]["value"] > line["value"] * 0.5


def test_cpu_baseline_leg_hands_over_the_oracles_samples():
    """the legs' parity samples: what the oracle makes of a few streams of every leg, worked out in the cpu_baseline
    process (the only place bench.py runs the oracle) -- digest, CRC-32 and length per sampled stream"""
    import hashlib

    import bench
    import oracle

    keep = dict(bench.LEGS)
    try:
        for k in list(bench.LEGS):
            if k not in ("text_default", "one_c1_zeros_1mib"):
                del bench.LEGS[k]
        s = bench.cpu_samples()
    finally:
        bench.LEGS.clear()
        bench.LEGS.update(keep)
    assert sorted(s) == ["one_c1_zeros_1mib", "text_default"] and sorted(s["text_default"]) == ["0", "1", "2", "3"]
    st, comp, crc = oracle.deflate(bench.text_pieces(65536)[2], level=2, crc_op=oracle.CRC_CRC32)
    assert s["text_default"]["2"] == [hashlib.sha256(comp).hexdigest()[:24], crc, len(comp)]


def test_dump_outputs_is_a_bounded_seeded_sample(tmp_path):
    """--dump-outputs on host tensors: every stream's numbers as float64, the bytes of the same seeded sample of streams in
    every run as float32 rows (zero past a stream's length), and all files together within the 64 MB bound -- also when
    one stream alone is longer than that"""
    import numpy as np
    import torch

    import bench

    n, slot = 300, 4352
    buf = torch.randint(0, 256, (n * slot + 256,), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
    offs = np.arange(n, dtype=np.uint64) * np.uint64(slot)
    lens = np.random.default_rng(1).integers(0, slot, n).astype(np.uint64)
    sums = bench.stream_byte_sums(buf, offs, lens)
    host = buf.numpy()
    assert sums.tolist() == [int(host[int(o):int(o) + int(k)].astype(np.int64).sum()) for o, k in zip(offs, lens)]
    for d in ("a", "b"):
        r = bench.dump_outputs(str(tmp_path / d), n, {"out_len": lens, "byte_sum": sums}, {"bytes": (buf, offs, lens, slot)})
        assert r["streams"] == n and r["sampled_streams"] == 64
    for f in sorted(os.listdir(tmp_path / "a")):
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), f
    rows, sample = np.load(tmp_path / "a" / "bytes.npy"), np.load(tmp_path / "a" / "sample_streams.npy").astype(int)
    assert np.array_equal(np.load(tmp_path / "a" / "byte_sum.npy"), sums)
    for i, j in enumerate(sample):
        k = int(lens[j])
        assert np.array_equal(rows[i, :k], host[int(offs[j]):int(offs[j]) + k]) and not rows[i, k:].any()
    big = 48 << 20
    buf = torch.zeros(2 * big, dtype=torch.uint8)
    offs, lens = np.arange(2, dtype=np.uint64) * np.uint64(big), np.full(2, big, np.uint64)
    bench.dump_outputs(str(tmp_path / "c"), 2, {"out_len": lens}, {"x": (buf, offs, lens, big), "y": (buf, offs, lens, big)})
    assert sum(os.path.getsize(tmp_path / "c" / f) for f in os.listdir(tmp_path / "c")) <= 64 * 10 ** 6
