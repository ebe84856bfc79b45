"""zipc_hip_checksum_device on the inputs of tests/checksum_cases.py: the Adler-32 chunk chain where its branches lie
(thousands of ambiguous chunks of every kind, the replay at its limit and the plain walk behind it, every shape of the
runs) and the CRC-32 finish on both sides of each of its seams.  Integer work: equality with the oracle (and zlib), no
tolerance.  What each case holds is counted on the CPU by tests/test_adler_chain_sim.py, which runs the same inputs
through the host model of zipc_amd/csrc/adler_chain.h."""
import zlib

import numpy as np
import pytest

import checksum_cases as CC
import host_sim

pytestmark = pytest.mark.gpu

N = CC.N
POOL_BYTES = 192 << 20
OFFSETS = (3, 21)  # where a buffer starts in the pool: neither a multiple of 16


@pytest.fixture(scope="module")
def pool(gpu_ctx):
    """the module's one device buffer"""
    import torch

    return torch.empty(POOL_BYTES, dtype=torch.uint8, device=torch.device("cuda", 0))


@pytest.fixture(scope="module")
def host_random():
    return np.random.default_rng(4097).integers(0, 256, 4097 * CC.CRC_SEG + 64, dtype=np.uint8)


@pytest.fixture(scope="module")
def sim():
    return host_sim.lib()


def _put(pool, host, at=0):
    import torch

    assert at + len(host) <= POOL_BYTES
    pool[at:at + len(host)].copy_(torch.from_numpy(host))


def _three_ways(ctx, view, crc=None, adler=None, what=None):
    """Adler alone (adler_chunks_kernel's sums), CRC alone (crc32_segments_kernel), both (crc32_adler_segments_kernel)"""
    from zipc_amd import batch

    if adler is not None:
        assert batch.checksum_device(ctx, view, want_crc32=False)[1] == adler, ("adler alone", what)
    if crc is not None:
        assert batch.checksum_device(ctx, view, want_adler32=False)[0] == crc, ("crc alone", what)
    if crc is not None and adler is not None:
        assert batch.checksum_device(ctx, view) == (crc, adler), ("both", what)


def _prefix_crcs(host, lengths):
    """zlib.crc32 of host[:n] for every n, in one pass over the bytes"""
    out, state, at = {}, 0, 0
    for n in sorted(set(lengths)):
        state = zlib.crc32(host[at:n], state)
        out[n], at = state, n
    return out


# ---- the chunk chain ---------------------------------------------------------------------------------------------------

def test_zeros_at_the_replays_limit_and_behind_it(gpu_ctx, oracle, pool, sim):
    """Every chunk of an all-zero buffer is ambiguous: 4096 of them are the most the replay holds (4 chunks a run), 4097 go
    the plain walk; 1024 | 1025 chunks is one | two chunks a run, the runs behind the last chunk empty.  Which side a
    length falls on is the host model's word (the shared predicate), not the device's."""
    top = max(CC.ZERO_LENGTHS)
    pool[:top + 64].zero_()
    zeros = np.zeros(top, np.uint8)
    shapes = set()
    for n in CC.ZERO_LENGTHS:
        n_chunks, n_runs, per = host_sim.adler_shape(sim, n)
        value, info = host_sim.adler_chain(sim, [0] * n_chunks, [0] * n_chunks, n)
        shapes.add((info["n_amb"], per, info["path"]))
        crc, adler = zlib.crc32(zeros[:n]), oracle.adler32(zeros[:n])
        assert value == adler and crc == oracle.crc32(zeros[:n])
        for off in OFFSETS:
            _three_ways(gpu_ctx, pool[off:off + n], crc, adler, (n, off))
    assert shapes == {(4095, 4, 0), (4096, 4, 0), (4097, 5, 1), (1024, 1, 0), (1025, 2, 0)}


@pytest.mark.parametrize("name", [p[0] for p in CC.PLANS])
def test_planned_ambiguous_chunks(gpu_ctx, oracle, pool, name):
    """The realised plans (600 chunks: one a run; 3000: three a run; 9000: 2048 runs; 17 000: 4096 runs, 16-byte loads
    in the scan; the two large ones spliced into random bytes), and each with three bytes appended: the grid shifted."""
    pl = CC.plan(name)
    for data in (pl.data, np.concatenate([pl.data, np.frombuffer(b"xyz", np.uint8)])):
        crc, adler = zlib.crc32(data), oracle.adler32(data)
        for off in OFFSETS:
            _put(pool, data, off)
            _three_ways(gpu_ctx, pool[off:off + len(data)], crc, adler, (name, len(data), off))


def test_rfc_1950_mode_on_the_same_buffers(oracle, pool):
    """adler_rfc_finish_kernel in a context of its own against zlib.adler32: the plans, zeros at the limits, and random
    bytes of 1023, 1024 and 1025 chunks (one | two chunks a thread)"""
    import zipc_amd
    from zipc_amd import batch

    ctx = zipc_amd.Context(0)
    try:
        ctx.set_adler_rfc1950(True)
        rng = np.random.default_rng(1950)
        datas = [(name, CC.plan(name).data) for name, _, _ in CC.PLANS]
        datas += [("zeros", np.zeros(n, np.uint8)) for n in CC.ZERO_LENGTHS[:6]]
        datas += [("random", rng.integers(0, 256, n, dtype=np.uint8)) for n in CC.RFC_LENGTHS]
        datas.append(("xyz", np.concatenate([CC.plan("p3000").data, np.frombuffer(b"xyz", np.uint8)])))
        for name, data in datas:
            want, crc = zlib.adler32(data), zlib.crc32(data)
            for off in OFFSETS:
                _put(pool, data, off)
                view = pool[off:off + len(data)]
                assert batch.checksum_device(ctx, view, want_crc32=False)[1] == want, (name, len(data), off)
                assert batch.checksum_device(ctx, view) == (crc, want), (name, len(data), off)
    finally:
        ctx.close()


# ---- the CRC-32 finish -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fill", ["random", "ff"])
def test_crc_finish_seams(gpu_ctx, oracle, pool, host_random, fill):
    """S * 32768 + d bytes for S = 16 | 17 (one thread | the tree), 256 | 257 (one row | two), 2048 | 2049 (one batch of eight
    rows | two), 4096 | 4097 (256 | 1024 threads) and d = -32767, -1, 0, 1: the first segment nearly empty, full, and a
    segment more, so the grid's pad is at both ends of its range.  CRC alone at every length, both checksums in one pass
    up to 2049 segments and at the two largest."""
    from zipc_amd import batch

    host = host_random if fill == "random" else np.full(len(host_random), 255, np.uint8)
    lengths = [S * CC.CRC_SEG + d for S in CC.CRC_SEAMS for d in CC.CRC_DELTAS]
    _put(pool, host)
    pads = set()
    for off in OFFSETS:
        h = host[off:]
        crcs = _prefix_crcs(h, lengths)
        assert crcs[max(lengths)] == oracle.crc32(h[:max(lengths)])
        for n in lengths:
            nseg, nt, rows, padp = CC.crc_shape(n)
            pads.add((nseg, nt, rows, padp))
            if nseg <= 257:
                assert crcs[n] == oracle.crc32(h[:n])
            view = pool[off:off + n]
            assert batch.checksum_device(gpu_ctx, view, want_adler32=False)[0] == crcs[n], (fill, n, off)
            if off == OFFSETS[0] and (nseg <= 2049 or n >= 4097 * CC.CRC_SEG):
                assert batch.checksum_device(gpu_ctx, view) == (crcs[n], oracle.adler32(h[:n])), (fill, n, off)
    assert {(16, 256, 0, 0), (17, 256, 1, 239), (256, 256, 1, 0), (257, 256, 2, 255), (2048, 256, 8, 0), (2049, 256, 9, 255),
            (4096, 256, 16, 0), (4097, 1024, 5, 1023), (4098, 1024, 5, 1022)} <= pads


def test_both_checksums_on_either_side_of_the_second_queue(gpu_ctx, oracle, pool, host_random):
    """from 64 MiB on the fused call finishes the CRC on a second queue beside the Adler chain"""
    from zipc_amd import batch

    lengths = [CC.FUSED_SIDE_BYTES + d for d in (-1, 0, 5)]
    _put(pool, host_random[:max(lengths) + 64])
    for off in OFFSETS:
        h = host_random[off:]
        crcs = _prefix_crcs(h, lengths)
        for n in lengths:
            assert batch.checksum_device(gpu_ctx, pool[off:off + n]) == (crcs[n], oracle.adler32(h[:n])), (n, off)
            assert batch.checksum_device(gpu_ctx, pool[off:off + n]) == (crcs[n], oracle.adler32(h[:n])), (n, off, "again")


# ---- the launches ------------------------------------------------------------------------------------------------------

CHAIN = {"adler_runs_s1": 1, "adler_scan_runs": 2, "adler_runs_a": 1}


def _launches(ctx, call):
    ctx.set_profiling(True)
    ctx.reset_kernel_times()
    try:
        call()
    finally:
        times = {k: n for k, (n, ms) in ctx.kernel_times().items() if n}
        ctx.set_profiling(False)
    return times


def test_the_kernels_of_a_call_are_the_same(gpu_ctx, oracle, pool):
    """zipc_hip_kernel_times after one call of each way: the names and launch counts of the chain and the finishes"""
    import zipc_amd
    from zipc_amd import batch

    data = CC.plan("p600").data
    _put(pool, data, 3)
    view = pool[3:3 + len(data)]
    crc, adler = zlib.crc32(data), oracle.adler32(data)
    got = {}
    t = _launches(gpu_ctx, lambda: got.update(a=batch.checksum_device(gpu_ctx, view, want_crc32=False)[1]))
    assert t == dict(CHAIN, adler_chunks=1, adler_replay=1) and got["a"] == adler
    t = _launches(gpu_ctx, lambda: got.update(c=batch.checksum_device(gpu_ctx, view, want_adler32=False)[0]))
    assert t == {"crc32_segments": 1, "crc32_finish": 1} and got["c"] == crc
    t = _launches(gpu_ctx, lambda: got.update(b=batch.checksum_device(gpu_ctx, view)))
    assert t == dict(CHAIN, crc32_adler_segments=1, crc32_finish=1, adler_replay=1) and got["b"] == (crc, adler)
    ctx = zipc_amd.Context(0)
    try:
        ctx.set_adler_rfc1950(True)
        t = _launches(ctx, lambda: got.update(r=batch.checksum_device(ctx, view, want_crc32=False)[1]))
        assert t == dict(CHAIN, adler_chunks=1, adler_rfc_finish=1) and got["r"] == zlib.adler32(data)
    finally:
        ctx.close()
