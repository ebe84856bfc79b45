"""inflate's accept / reject rules (tests/golden/inflate_rules.py) through every decoder form on the MI355X: the one-stream
call with each checksum, calls of the batch form of 256 streams and less (inflate_batch_few_kernel) and of more
(inflate_batch_kernel) padded with valid streams, and the many-stream host calls with and without the bytes.  Each
stream's status, length, bytes and checksum against the oracle (which tests/test_oracle_pins.py holds to the cases as
built).  Then the same in processes of their own under the inflate overrides."""
import ctypes as C
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, util.GOLDEN)
import inflate_rules  # noqa: E402

CASES = inflate_rules.wrapped_cases()
SHORT = {n: c for n, c in CASES.items() if not n.endswith("/e")}
LONG = {n: c for n, c in CASES.items() if n.endswith("/e")}
SHORT_CAP = 1 << 16    # every short case's output fits; a batch call below 256 KiB of max_dst_cap stays on its one waves
LONG_CAP = 1 << 20


def _cap(name, c):
    return c.limit if c.limit is not None else (LONG_CAP if name.endswith("/e") else SHORT_CAP)


def _want(oracle, c, limit, crc_op):
    """the oracle's (status, bytes, checksum); crc_op 3 (Adler-32 as RFC 1950 has it): zlib's over the oracle's bytes"""
    if crc_op == 3:
        st, d, _ = oracle.inflate(c.stream, decompressed_size=limit)
        return st, d, zlib.adler32(d) if st == 0 else 0
    return oracle.inflate(c.stream, decompressed_size=limit, crc_op=crc_op)


def _check(oracle, name, c, crc_op, st, out, ck, form):
    st0, d0, k0 = _want(oracle, c, c.limit, crc_op)
    assert st0 == c.status, (name, "the oracle left its case", st0, c.status)
    assert st == st0, (form, name, crc_op, "status", st, st0)
    if st0 == 0:
        assert out == d0, (form, name, crc_op, "bytes", len(out), len(d0))
        if crc_op:
            assert ck == k0, (form, name, crc_op, "checksum", hex(ck), hex(k0))


def test_one_stream_calls(gpu_ctx, oracle):
    from zipc_amd._lib import lib

    L = lib()
    for name, c in CASES.items():
        cap = _cap(name, c)
        for crc_op in (0, 1, 2, 3):
            dst = C.create_string_buffer(cap + 64)
            ol, ck = C.c_size_t(), C.c_uint32()
            st = L.zipc_hip_inflate(gpu_ctx.handle, c.stream, len(c.stream), int(c.limit is not None), c.limit or 0,
                                    crc_op, dst, cap, C.byref(ol), C.byref(ck))
            _check(oracle, name, c, crc_op, st, dst.raw[:ol.value], ck.value, "zipc_hip_inflate")
            if name.endswith("/e") and c.status == 0 and os.environ.get("ZIPC_HIP_INFLATE_BLOCKS") != "0":
                assert gpu_ctx.last_inflate_blocks() >= 4, (name, gpu_ctx.last_inflate_blocks())


def _padding(n):
    """valid streams (zlib, level 1-9) to pad a call past 256 streams"""
    out = []
    for i in range(n):
        plain = util.text(200 + 37 * i, 400 + i)
        c = zlib.compressobj(1 + i % 9, zlib.DEFLATED, -15)
        out.append(("pad%d" % i, inflate_rules.Case(c.compress(plain) + c.flush(), None, 0, plain, "", [len(plain)])))
    return out


def _batch(gpu_ctx, oracle, items, crc_op):
    """one zipc_hip_inflate_batch call over items [(name, Case)], each stream with its own limit or none"""
    import torch

    from zipc_amd import batch

    dev = torch.device("cuda", 0)
    n = len(items)
    caps = [_cap(nm, c) for nm, c in items]
    src_off = np.cumsum([0] + [len(c.stream) for _, c in items[:-1]]).astype(np.uint64)
    slots = [(k + 255) // 256 * 256 + 256 for k in caps]
    dst_off = np.cumsum([0] + slots[:-1]).astype(np.uint64)
    descs = batch.make_descs(src_off, [len(c.stream) for _, c in items], dst_off, caps)
    for i, (_, c) in enumerate(items):
        if c.limit is not None:
            descs["limit"][i] = c.limit
            descs["flags"][i] = 1
    src = torch.from_numpy(np.frombuffer(b"".join(c.stream for _, c in items) + b"\0" * 64, dtype=np.uint8).copy()).to(dev)
    dst = torch.full((int(sum(slots)) + 256,), 0xA5, dtype=torch.uint8, device=dev)
    d_res = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    batch.inflate_batch(gpu_ctx, src, dst, batch.to_device(descs, dev), d_res, n, max(caps), crc_op)
    res = batch.results_from_device(d_res)
    out = dst.cpu().numpy()
    form = "inflate_batch n=%d" % n
    for i, (nm, c) in enumerate(items):
        o, ln = int(dst_off[i]), int(res["out_len"][i])
        _check(oracle, nm, c, crc_op, int(res["status"][i]), out[o:o + ln].tobytes(), int(res["checksum"][i]), form)
        assert (out[o + caps[i]:o + slots[i]] == 0xA5).all(), (form, nm, "wrote past its dst_cap")


@pytest.mark.parametrize("crc_op", [1, 2])
def test_batch_calls_few_and_many(gpu_ctx, oracle, crc_op):
    short = list(SHORT.items())
    for k in range(0, len(short), 200):  # calls of <= 256 streams: inflate_batch_few_kernel
        _batch(gpu_ctx, oracle, short[k:k + 200], crc_op)
    _batch(gpu_ctx, oracle, short + _padding(max(0, 300 - len(short))), crc_op)  # > 256: inflate_batch_kernel
    long_ = list(LONG.items())
    _batch(gpu_ctx, oracle, long_ + _padding(8), crc_op)
    _batch(gpu_ctx, oracle, long_ + short[:120] + _padding(300 - len(long_) - 120), crc_op)


@pytest.mark.parametrize("check_only", [False, True], ids=["inflate_many", "inflate_many_check"])
def test_many_stream_calls(gpu_ctx, oracle, check_only):
    """zipc_hip_inflate_many / _many_check over every case at once: each stream's limit, or its room as the limit"""
    from zipc_amd import _lib

    L = _lib.lib()
    items = list(CASES.items()) + _padding(20)
    n = len(items)
    caps = [_cap(nm, c) for nm, c in items]
    keep = [np.frombuffer(c.stream, np.uint8) for _, c in items]
    P, S = C.c_void_p * n, C.c_size_t * n
    res = (_lib.StreamResult * n)()
    if check_only:
        assert L.zipc_hip_inflate_many_check(gpu_ctx.handle, n, P(*[a.ctypes.data for a in keep]), S(*[len(a) for a in keep]),
                                             S(*caps), 1, S(*caps), res) == 0
    else:
        outs = [np.full(k + 16, 0xA5, np.uint8) for k in caps]
        assert L.zipc_hip_inflate_many(gpu_ctx.handle, n, P(*[a.ctypes.data for a in keep]), S(*[len(a) for a in keep]),
                                       S(*caps), 1, P(*[a.ctypes.data for a in outs]), S(*caps), res) == 0
    for i, (nm, c) in enumerate(items):
        st, ln = int(res[i].status), int(res[i].out_len)
        st0, d0, k0 = _want(oracle, c, caps[i], 1)
        assert st == st0, ("inflate_many", check_only, nm, st, st0)
        if st0 == 0:
            assert ln == len(d0) and int(res[i].checksum) == k0, ("inflate_many", check_only, nm)
            if not check_only:
                assert outs[i][:ln].tobytes() == d0 and (outs[i][caps[i]:] == 0xA5).all(), ("inflate_many", nm)
        else:
            assert ln == 0, ("inflate_many", check_only, nm, ln)


@pytest.mark.parametrize("env", [
    {"ZIPC_HIP_INFLATE_BLOCKS": "0"},                      # every stream on its one wave
    {"ZIPC_HIP_INFLATE_FOLLOW": "1"},                      # sources written down as what they copy
    {"ZIPC_HIP_EXPLORE_STRIDE": "1024", "ZIPC_HIP_RESOLVE_HOPS0": "3", "ZIPC_HIP_RESOLVE_HOPS1": "5"},
], ids=["one-wave", "following", "explorers-everywhere"])
def test_the_rule_cases_under_overrides(env):
    """The tests above in a process of their own under each inflate override (read once per process)."""
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        os.path.join(ROOT, "tests", "test_gpu_inflate_rules.py"), "-k", "not overrides"],
                       cwd=ROOT, env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    tail = r.stdout.decode()[-1500:]
    assert r.returncode == 0, (env, tail)
