"""zipc_hip_checksum_many: CRC-32 and Adler-32 of many host-resident streams per call, through the pipeline of the
other many-stream forms (gather, copy in, the ragged checksum pass per sub-batch, 16-byte results back).  Integer work:
equality with the oracle and zlib."""
import ctypes as C
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 5000  # above four times ZIPC_HIP_HOST_CHUNK_MIN's default (1024 streams): the call is cut into four sub-batches


@pytest.fixture(scope="module")
def streams():
    """ragged: 0 to 2000 bytes, every 37th empty, three long ones (one of 0xFF, where the signed remainder bites)"""
    rng = np.random.default_rng(5000)
    lens = rng.integers(0, 2001, N)
    lens[::37] = 0
    lens[[11, 2500, N - 2]] = (100_000, 1_234_567, 70_001)
    out = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in lens]
    out[N - 2] = b"\xff" * 70_001
    return out


@pytest.fixture(scope="module")
def reference(streams, oracle):
    return [(zlib.crc32(s), oracle.adler32(s), zlib.adler32(s)) for s in streams]


def _rows(res):
    assert not res["reserved"].any()
    return list(zip(res["status"].tolist(), res["crc32"].tolist(), res["adler32"].tolist()))


def test_ragged_streams_over_four_sub_batches(gpu_ctx, oracle, streams, reference):
    from zipc_amd import batch

    assert oracle.crc32(streams[11]) == reference[11][0]
    assert _rows(batch.checksum_many(gpu_ctx, streams)) == [(0, c, a) for c, a, _ in reference]
    assert _rows(batch.checksum_many(gpu_ctx, streams, want_adler32=False)) == [(0, c, 0) for c, _, _ in reference]
    assert _rows(batch.checksum_many(gpu_ctx, streams, want_crc32=False)) == [(0, 0, a) for _, a, _ in reference]
    # a batch call on the same context afterwards is what it was (the forms share the context's scratch)
    assert _rows(batch.checksum_many(gpu_ctx, streams[:7])) == [(0, c, a) for c, a, _ in reference[:7]]


def test_rfc_1950_flavour(streams, reference):
    from zipc_amd import Context, batch

    ctx = Context(0)
    try:
        ctx.set_adler_rfc1950(True)
        pick = streams[:50] + streams[N - 3:]
        want = reference[:50] + reference[N - 3:]
        assert _rows(batch.checksum_many(ctx, pick)) == [(0, c, z) for c, _, z in want]
    finally:
        ctx.close()


def test_results_are_defined_on_bad_arguments(gpu_ctx, streams):
    from zipc_amd import _lib, batch

    bad = _lib.ERR_INVALID_ARG
    # a null src[i] with a length: the call fails, every entry carries its status and no checksum
    some = streams[:5]
    src = (C.c_void_p * 5)(*[C.cast(C.c_char_p(s), C.c_void_p) for s in some])
    lens = (C.c_size_t * 5)(*[len(s) for s in some])
    src[3], lens[3] = None, 17
    st, res = batch.checksum_many_raw(gpu_ctx, 5, src, lens, check=False)
    assert st == bad and _rows(res) == [(bad, 0, 0)] * 5
    # ... a null src[i] of no bytes is an empty stream
    lens[3] = 0
    st, res = batch.checksum_many_raw(gpu_ctx, 5, src, lens, check=False)
    assert st == 0 and _rows(res)[3] == (0, 0, 1)
    assert _rows(res)[1] == (0, zlib.crc32(some[1]), zlib.adler32(some[1]))  # (under 2001 bytes: no sum reaches 2^31, both Adler-32s agree)
    # both selectors 0
    st, res = batch.checksum_many_raw(gpu_ctx, 5, src, lens, want_crc32=False, want_adler32=False, check=False)
    assert st == bad and _rows(res) == [(bad, 0, 0)] * 5
    # no streams: OK
    st, res = batch.checksum_many_raw(gpu_ctx, 0, src, lens, check=False)
    assert st == 0 and len(res) == 0
    assert _lib.lib().zipc_hip_checksum_many(None, 5, src, lens, 1, 1, None) == bad
