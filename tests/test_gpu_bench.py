"""bench.py on the GPU at a small shape, both forms of its line: a plain run carries the headline and its dump and nothing
that takes runs of its own; --full adds the profiled steps (C2, C4) and the archive check (C4)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "kernels_ms_per_step", "deflate_gib_s", "inflate_gib_s", "cpu_baseline", "text_gib_s", "archive_check")


def bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1"] + list(args),
                       stdout=subprocess.PIPE, timeout=300)
    assert r.returncode == 0
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def test_a_plain_line_is_the_headline_and_its_dump(tmp_path):
    d = bench("--streams", "256", "--dump-outputs", str(tmp_path))
    assert all(k in d for k in HEADLINE) and d["value"] > 0 and d["ms_per_step"] > 0
    assert not [k for k in FULL_ONLY if k in d]
    assert d["dump_outputs"]["streams"] == 256 and (np.load(tmp_path / "deflate_status.npy") == 0).all()
    assert (np.load(tmp_path / "inflate_out_len.npy") == 65536).all()


def test_full_adds_the_profiled_steps_and_the_archive_check():
    d = bench("--full", "--streams", "256", "--no-cpu-baseline", "--no-extra-legs")
    assert all(k in d for k in HEADLINE) and d["inflate_gib_s"] > 0 and min(d["kernels_ms_per_step"].values()) > 0
    assert d["roofline"]["deflate_pipeline"]["ms_per_step"] > 0 and d["config"]["deflate_gib_s"] == d["deflate_gib_s"]
    c4 = bench("--full", "--config", "c4", "--streams", "64", "--no-cpu-baseline")
    assert c4["archive_check"]["members"] == 64 and c4["archive_check"]["zipfile_ok"] and c4["kernels_ms_per_step"]
