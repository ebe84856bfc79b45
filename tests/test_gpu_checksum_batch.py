"""zipc_hip_checksum_batch on the inputs of tests/checksum_batch_cases.py: CRC-32 and Adler-32 of many ranges of one
arena per call, ragged.  Every case three ways (CRC alone, Adler alone, both) against the oracle and against
zipc_hip_checksum_device of the same view; RFC 1950 mode against zlib; bad ranges and a short declared total; the arena
and the ranges untouched; the same launch counts for 1 and 1001 ranges; the call-level refusals.  Integer work:
equality, no tolerance.  What each case holds is counted on the CPU by tests/test_checksum_ranges_rules.py, which runs
the same inputs through the host model of zipc_amd/csrc/checksum_ranges.h."""
import zlib

import numpy as np
import pytest

import checksum_batch_cases as BC

pytestmark = pytest.mark.gpu

WAYS = ((True, False), (False, True), (True, True))  # (want_crc32, want_adler32)


def _dev():
    import torch

    return torch.device("cuda", 0)


class Loaded:
    """a case on the device: arena, ranges, and copies of both to compare with afterwards"""

    def __init__(self, name):
        import torch
        from zipc_amd import batch

        c = BC.case(name)
        self.case, self.n = c, len(c["ranges"])
        self.arena = torch.from_numpy(c["arena"].copy()).to(_dev())
        self.arena_copy = self.arena.clone()
        self.ranges = batch.to_device(batch.make_ranges([r[0] for r in c["ranges"]], [r[1] for r in c["ranges"]]), _dev())
        self.ranges_copy = self.ranges.clone()

    def run(self, ctx, crc, adler, total=None):
        import torch
        from zipc_amd import batch

        res = torch.full((max(self.n, 1) * 16,), 0xEE, dtype=torch.uint8, device=_dev())
        batch.checksum_batch(ctx, self.arena, self.ranges, res, self.n, self.case["total"] if total is None else total, crc, adler)
        return batch.checksum_results_from_device(res)[:self.n]

    def untouched(self):
        import torch

        return torch.equal(self.arena, self.arena_copy) and torch.equal(self.ranges, self.ranges_copy)


_loaded = {}


def loaded(name):
    if name not in _loaded:
        _loaded.clear()  # (one case on the device at a time)
        _loaded[name] = Loaded(name)
    return _loaded[name]


@pytest.fixture(scope="module")
def rfc_ctx(gpu_ctx):
    from zipc_amd import Context

    ctx = Context(0)
    ctx.set_adler_rfc1950(True)
    yield ctx
    ctx.close()


def _expect(case, ref, crc, adler, pick=1):
    """(status, crc32, adler32) rows: pick 1: the reference's Adler-32, 2: RFC 1950's"""
    return [(BC.INVALID_ARG, 0, 0) if i in case["bad"] else (0, r[0] if crc else 0, r[pick] if adler else 0) for i, r in enumerate(ref)]


def _rows(res):
    assert not res["reserved"].any()
    return list(zip(res["status"].tolist(), res["crc32"].tolist(), res["adler32"].tolist()))


def test_a_few_dozen_short_ranges(gpu_ctx, oracle):
    """the narrowest run of the pass: 48 ranges of 0 to 300 bytes, both checksums, one call"""
    import torch
    from zipc_amd import batch

    rng = np.random.default_rng(48)
    host = rng.integers(0, 256, 20000, dtype=np.uint8)
    lens = rng.integers(0, 301, 48)
    offs = rng.integers(0, 20000 - 300, 48)
    arena = torch.from_numpy(host).to(_dev())
    d_ranges = batch.to_device(batch.make_ranges(offs, lens), _dev())
    d_res = torch.zeros(48 * 16, dtype=torch.uint8, device=_dev())
    batch.checksum_batch(gpu_ctx, arena, d_ranges, d_res, 48, int(lens.sum()))
    res = batch.checksum_results_from_device(d_res)
    for i in range(48):
        b = host[offs[i]:offs[i] + lens[i]]
        assert (int(res["status"][i]), int(res["crc32"][i]), int(res["adler32"][i])) == (0, oracle.crc32(b), oracle.adler32(b)), i


@pytest.mark.parametrize("name", BC.NAMES)
def test_every_case_three_ways(gpu_ctx, rfc_ctx, oracle, name):
    """CRC alone, Adler alone, both: the oracle's values per range, INVALID_ARG with no checksum for the bad ranges and
    their neighbours right; RFC 1950 mode gives zlib's Adler-32; arena and ranges are what they were"""
    L = loaded(name)
    ref = BC.reference(name, oracle)
    for crc, adler in WAYS:
        assert _rows(L.run(gpu_ctx, crc, adler)) == _expect(L.case, ref, crc, adler), (name, crc, adler)
    assert _rows(L.run(rfc_ctx, True, True)) == _expect(L.case, ref, True, True, pick=2), (name, "rfc")
    assert _rows(L.run(rfc_ctx, False, True)) == _expect(L.case, ref, False, True, pick=2), (name, "rfc, adler alone")
    assert L.untouched()


@pytest.mark.parametrize("name", ("lengths_rand", "lengths_ff", "p600", "shapes", "ragged_middle"))
def test_checksum_device_of_the_same_view_agrees(gpu_ctx, rfc_ctx, name):
    """the defining property: what zipc_hip_checksum_device gives for the same bytes with the same context flavour
    (every distinct range of the short cases; of the ragged one the long range and a few short ones)"""
    from zipc_amd import batch

    L = loaded(name)
    picks = [i for i in range(L.n) if i not in L.case["bad"]]
    if name.startswith("ragged"):
        picks = picks[:3] + [500] + picks[-3:]
    for ctx in (gpu_ctx, rfc_ctx):
        res = L.run(ctx, True, True)
        for i in picks:
            off, n = L.case["ranges"][i]
            assert (int(res["crc32"][i]), int(res["adler32"][i])) == batch.checksum_device(ctx, L.arena[off:off + n]), (name, i)
    assert L.untouched()


def test_declared_total_one_too_small(gpu_ctx):
    """every result is INVALID_ARG with no checksum, whatever was asked for; a generous total changes nothing"""
    L = loaded("shapes")
    good = L.run(gpu_ctx, True, True)
    for crc, adler in WAYS:
        res = L.run(gpu_ctx, crc, adler, total=L.case["total"] - 1)
        assert _rows(res) == [(BC.INVALID_ARG, 0, 0)] * L.n
    assert _rows(L.run(gpu_ctx, True, True, total=L.case["total"] + 12345678)) == _rows(good)
    assert sorted(np.nonzero(good["status"])[0].tolist()) == list(L.case["bad"])
    assert L.untouched()


def test_launch_counts_do_not_depend_on_n(gpu_ctx):
    """one range or 1001 (one of them long): a plan, one pass, a finish per checksum (a context of its own: the
    table of kernel names of the session's context has seen every other test)"""
    from zipc_amd import Context

    ctx, counts = Context(0), {}
    try:
        for name in ("n1", "ragged_middle"):
            L = loaded(name)
            L.run(ctx, True, True)
            ctx.set_profiling(True)
            for crc, adler in WAYS:
                ctx.reset_kernel_times()
                L.run(ctx, crc, adler)
                counts[(name, crc, adler)] = {k: v[0] for k, v in ctx.kernel_times().items() if v[0]}
            ctx.set_profiling(False)
    finally:
        ctx.close()
    assert counts[("n1", True, True)] == {"checksum_plan": 1, "crc32_adler_ranges": 1, "crc32_finish_ranges": 1, "adler_finish_ranges": 1}
    assert counts[("n1", True, False)] == {"checksum_plan": 1, "crc32_ranges": 1, "crc32_finish_ranges": 1}
    assert counts[("n1", False, True)] == {"checksum_plan": 1, "crc32_adler_ranges": 1, "adler_finish_ranges": 1}
    for way in WAYS:
        assert counts[("n1",) + way] == counts[("ragged_middle",) + way]
    assert len(BC.case("ragged_middle")["ranges"]) == 1001


def test_call_level_refusals(gpu_ctx):
    import torch
    from zipc_amd import _lib, batch

    lib, h = _lib.lib(), gpu_ctx.handle
    arena = torch.zeros(4096, dtype=torch.uint8, device=_dev())
    d_ranges = batch.to_device(batch.make_ranges([0, 5], [10, 20]), _dev())
    d_res = torch.full((32,), 0xEE, dtype=torch.uint8, device=_dev())
    torch.cuda.synchronize()
    a, r, o = arena.data_ptr(), d_ranges.data_ptr(), d_res.data_ptr()
    bad = _lib.ERR_INVALID_ARG
    assert lib.zipc_hip_checksum_batch(None, a, 4096, r, o, 2, 30, 1, 1) == bad
    assert lib.zipc_hip_checksum_batch(h, a, 4096, None, o, 2, 30, 1, 1) == bad
    assert lib.zipc_hip_checksum_batch(h, a, 4096, r, None, 2, 30, 1, 1) == bad
    assert lib.zipc_hip_checksum_batch(h, None, 4096, r, o, 2, 30, 1, 1) == bad
    assert lib.zipc_hip_checksum_batch(h, a, 4096, r, o, 2, 30, 0, 0) == bad
    assert lib.zipc_hip_checksum_batch(h, a, 4096, r, o, 0x80000000, 30, 1, 1) == bad
    assert lib.zipc_hip_checksum_batch(h, a, 4096, r, o, 2, (0x7FFFFFFF - 1) * 32768, 1, 1) == bad   # segs_bound 2^31
    gpu_ctx.synchronize()
    assert (d_res.cpu().numpy() == 0xEE).all()
    # n_ranges == 0: OK, nothing enqueued, nothing written; a null arena of no bytes is fine
    assert lib.zipc_hip_checksum_batch(h, a, 4096, r, o, 0, 0, 1, 1) == 0
    gpu_ctx.synchronize()
    assert (d_res.cpu().numpy() == 0xEE).all()
    empty = batch.to_device(batch.make_ranges([0, 0], [0, 1]), _dev())
    torch.cuda.synchronize()
    assert lib.zipc_hip_checksum_batch(h, None, 0, empty.data_ptr(), o, 2, 1, 1, 1) == 0
    gpu_ctx.synchronize()
    res = batch.checksum_results_from_device(d_res)
    assert _rows(res) == [(0, 0, 1), (BC.INVALID_ARG, 0, 0)] and zlib.crc32(b"") == 0
