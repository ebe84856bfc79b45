"""zipc_hip_zlib_decompress_many / zipc_hip_zlib_compress_many (include/zipc_hip.h): the cases of
tests/test_gpu_zlib_batch.py held in host memory, against the same verdicts of the oracle (tests/zlib_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import util
import zlib_cases as ZC

pytestmark = pytest.mark.gpu


def _ptrs(arrays):
    return (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def _sizes(values):
    return (C.c_size_t * len(values))(*values)


def _results(n):
    from zipc_amd import _lib

    res = (_lib.StreamResult * n)()
    C.memset(res, 0xEE, C.sizeof(res))
    return res


def many_decompress(ctx, cases):
    """one zipc_hip_zlib_decompress_many over cases that all have a limit, or none has: (call status, results, outputs)"""
    from zipc_amd import _lib

    n = len(cases)
    limited = cases[0].limit is not None
    assert all((c.limit is not None) == limited for c in cases)
    src = [np.frombuffer(c.stream + b"\0", dtype=np.uint8).copy() for c in cases]
    outs = [np.full(c.cap + 64, 0xA5, dtype=np.uint8) for c in cases]
    res = _results(n)
    st = _lib.lib().zipc_hip_zlib_decompress_many(ctx.handle, n, _ptrs(src), _sizes([len(c.stream) for c in cases]),
                                                  _sizes([c.limit for c in cases]) if limited else None, _ptrs(outs),
                                                  _sizes([c.cap for c in cases]), res)
    return st, res, outs


def test_ragged_decompress_many_with_every_error(gpu_ctx):
    pairs = [p for p in ZC.decompress_expectations() if not p[0].flags]  # (the host form has no descriptor flags)
    assert {e.status for _, e in pairs} >= ZC.REQUIRED_STATUSES - {18}
    for limited in (True, False):
        group = [p for p in pairs if (p[0].limit is not None) == limited]
        assert group
        st, res, outs = many_decompress(gpu_ctx, [c for c, _ in group])
        assert st == 0
        for (c, e), r, o in zip(group, res, outs):
            assert int(r.status) == e.status, (c.name, int(r.status), e.status)
            if e.status == 0:
                assert int(r.out_len) == len(e.out) and o[:len(e.out)].tobytes() == e.out and int(r.checksum) == e.checksum, c.name
            else:
                assert int(r.out_len) == 0, c.name
            if e.status == 6:
                assert int(r.checksum) == e.checksum, c.name
            if e.header:
                assert (o == 0xA5).all(), (c.name, "a refused stream's destination was written")
            assert (o[c.cap:] == 0xA5).all(), (c.name, "bytes behind dst_cap")


@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_ragged_compress_many(gpu_ctx, level):
    from zipc_amd import _lib

    L = _lib.lib()
    triples = ZC.compress_expectations(level)
    n = len(triples)
    src = [np.frombuffer(c.data + b"\0", dtype=np.uint8).copy() for c, _, _ in triples]
    caps = [L.zipc_hip_zlib_bound(len(c.data)) if cap is None else cap for c, cap, _ in triples]
    outs = [np.full(cap + 64, 0xA5, dtype=np.uint8) for cap in caps]
    res = _results(n)
    assert L.zipc_hip_zlib_compress_many(gpu_ctx.handle, n, _ptrs(src), _sizes([len(c.data) for c, _, _ in triples]), level,
                                         _ptrs(outs), _sizes(caps), res) == 0
    for (c, _, e), r, o, cap in zip(triples, res, outs, caps):
        assert int(r.status) == e.status, (c.name, level, int(r.status), e.status)
        if e.status == 0:
            assert int(r.out_len) == len(e.out) and int(r.checksum) == e.checksum and o[:len(e.out)].tobytes() == e.out, (c.name, level)
        else:
            assert int(r.out_len) == 0, (c.name, level)
        if e.header:
            assert (o == 0xA5).all(), (c.name, level)
        assert (o[cap:] == 0xA5).all(), (c.name, level, "bytes behind dst_cap")


def test_a_null_source_leaves_every_result_defined(gpu_ctx, oracle):
    from zipc_amd import _lib

    L = _lib.lib()
    z = oracle.zlib_compress(util.text(3000, 1), 2)[1]
    a = np.frombuffer(z, dtype=np.uint8).copy()
    outs = [np.full(3064, 0xA5, dtype=np.uint8) for _ in range(3)]
    src = (C.c_void_p * 3)(a.ctypes.data, None, a.ctypes.data)
    for compress in (False, True):
        res = _results(3)
        if compress:
            st = L.zipc_hip_zlib_compress_many(gpu_ctx.handle, 3, src, _sizes([len(z)] * 3), 2, _ptrs(outs), _sizes([3000] * 3), res)
        else:
            st = L.zipc_hip_zlib_decompress_many(gpu_ctx.handle, 3, src, _sizes([len(z)] * 3), None, _ptrs(outs), _sizes([3000] * 3), res)
        assert st == 18
        assert [(int(r.status), int(r.checksum), int(r.out_len)) for r in res] == [(18, 0, 0)] * 3
    # a null source of NO bytes is a stream too short for a header, not a bad argument
    src = (C.c_void_p * 3)(a.ctypes.data, None, a.ctypes.data)
    res = _results(3)
    assert L.zipc_hip_zlib_decompress_many(gpu_ctx.handle, 3, src, _sizes([len(z), 0, len(z)]), None, _ptrs(outs), _sizes([3000] * 3), res) == 0
    assert [int(r.status) for r in res] == [0, oracle.zlib_decompress(b"")[0], 0]
    assert outs[0][:3000].tobytes() == outs[2][:3000].tobytes() == util.text(3000, 1)


def test_python_mirrors(gpu_ctx, oracle):
    """zipc_deflate.zlib_compress_many / zlib_decompress_many: element i is what the single-stream mirror gives"""
    from zipc_amd import zipc_deflate as Z

    datas = [util.text(3000, 1), b"", util.rand_bytes(20000, 2), util.text(70000, 4)]
    got = Z.zlib_compress_many(datas, level="default", ctx=gpu_ctx)
    want = [oracle.zlib_compress(d, 2) for d in datas]
    assert [g.get_ok() for g in got] == [(a, z) for _, z, a in want]
    zs = [z for _, z, _ in want]
    damaged = zs[0][:-1] + bytes([zs[0][-1] ^ 1])
    back = Z.zlib_decompress_many(zs + [damaged, b"\x77\x85" + zs[0][2:]], ctx=gpu_ctx)  # (no sizes: rooms grow until they fit)
    assert [b.get_ok() for b in back[:4]] == [(d, a) for d, (_, _, a) in zip(datas, want)]
    _, _, _, expect, found = oracle.zlib_decompress(damaged)
    assert back[4].error == ((expect, found), Z.crc_error(expect, found))
    assert back[5].error == (None, "Unknown compression method (7)") and oracle.zlib_decompress(b"\x77\x85" + zs[0][2:])[0] == 3
    sized = Z.zlib_decompress_many(zs, decompressed_size=[len(d) for d in datas], ctx=gpu_ctx)
    assert [b.get_ok()[0] for b in sized] == datas
