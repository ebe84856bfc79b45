"""Stored members of an archive go through ONE checksum call (zipc_deflate::crc_32_many -> zipc_hip_checksum_many) beside
the deflated batch in Archive::extract_all and Archive::test_all: per member, the bytes or the message are what the
single-member path (File.to_binary_string) gives, and `zipc-hip unzip -t` says what it said."""
import os
import subprocess
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOOL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zipc_amd", "bin", "zipc-hip")
BAD = b"m/bad_crc.bin"


@pytest.fixture(scope="module")
def host(gpu_ctx):
    from zipc_amd import zipc_host

    zipc_host.lib()
    return zipc_host


@pytest.fixture(scope="module")
def archives(host):
    """(files, encoded without the bad member, encoded with it): about 300 stored members of 0 to 40 000 bytes, a deflated
    member after every 24th, and one stored member whose recorded CRC-32 is wrong"""
    rng = np.random.default_rng(300)
    sizes = rng.integers(0, 40001, 300).tolist()
    sizes[0], sizes[1], sizes[2] = 0, 40000, 32768
    files, a = {}, host.Archive()
    for k, n in enumerate(sizes):
        path = b"m/%04d.bin" % k
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        files[path] = data
        a.add_file_stored(path, data)
        if k % 24 == 23:
            path = b"m/%04d.txt" % k
            files[path] = (b"line %d of a deflated member\n" % k) * (k + 1)
            a.add_file_deflate(path, files[path], level=1)
    good = a.to_binary_string()
    data = rng.integers(0, 256, 12345, dtype=np.uint8).tobytes()
    a.add_file_made(BAD, 0, data, len(data), zlib.crc32(data) ^ 1)
    return files, good, a.to_binary_string()


def test_extract_all_is_the_single_member_path(host, archives):
    files, good, bad = archives
    for enc, n_bad in ((good, 0), (bad, 1)):
        a = host.Archive.of_binary_string(enc)
        index = {a.member(i)["path"]: i for i in range(a.member_count())}
        got = a.extract_all()
        assert len(got) == len(files) + n_bad and sum(p.endswith(b".bin") for p, _ in got) == 300 + n_bad
        errors = 0
        for path, r in got:
            try:
                one = a.member_to_binary_string(index[path])[0]
            except host.ZipcError as e:
                assert isinstance(r, host.ZipcError) and r.msg == e.msg and path == BAD and "Checksum mismatch" in e.msg, (path, e.msg)
                errors += 1
                continue
            assert not isinstance(r, host.ZipcError) and r == one == files[path], path
        assert errors == n_bad


def test_unzip_t_says_what_it_said(host, archives, tmp_path):
    files, good, bad = archives
    p_good, p_bad = tmp_path / "good.zip", tmp_path / "bad.zip"
    p_good.write_bytes(good)
    p_bad.write_bytes(bad)
    r = subprocess.run([TOOL, "unzip", "-t", "-v", str(p_good)], capture_output=True, timeout=120)
    assert r.returncode == 0 and b"No errors detected in" in r.stdout and b"(%d files)" % len(files) in r.stdout
    assert r.stderr.count(b"[ OK ] ") == len(files) and b"[FAIL]" not in r.stderr
    # ... in two calls: the 300 stored members' CRC-32s in one, the 12 deflated members in the other (the pipeline's own report)
    r = subprocess.run([TOOL, "unzip", "-t", str(p_good)], capture_output=True, timeout=120, env=dict(os.environ, ZIPC_HIP_HOST_TIMING="1"))
    assert r.returncode == 0 and r.stderr.count(b"zipc_hip checksum_many n=300 ") == 1 and r.stderr.count(b"zipc_hip inflate_many n=12 ") == 1
    assert r.stderr.count(b"_many n=") == 2
    r = subprocess.run([TOOL, "unzip", "-t", "-v", str(p_bad)], capture_output=True, timeout=120)
    assert r.returncode == 2 and b"Errors detected in" in r.stdout
    assert r.stderr.count(b"[ OK ] ") == len(files) and r.stderr.count(b"[FAIL] ") == 1
    assert b"[FAIL] " + BAD + b": Checksum mismatch, expected" in r.stderr
