"""Packed encode on the MI355X: zipc_hip_deflate_packed_batch / zipc_hip_zlib_compress_packed_batch -- a batch of streams
deflated into staging slots, laid out end to end in one arena, copied there and reported, in one call.

The expected results of every call: zipc_hip_deflate_batch (zipc_hip_zlib_compress_batch) runs over the same sources at the
same level and crc_op into slots of zipc_hip_deflate_bound (zipc_hip_zlib_bound) bytes, and the layout rule of
include/zipc_hip.h is applied to its results in Python (`rule` below).  The packed call must give equal results and, at
the rule's dst_off, equal bytes; the bytes must also be the oracle's for the same input and level.  Every destination
arena is dst_arena_len + 4096 bytes of poison; the tail, every padding gap and the room of every stream that did not fit
must still hold it after the call, and the source and the descriptors must be unchanged."""
import numpy as np
import pytest

import deflate_packed_cases as DC

pytestmark = pytest.mark.gpu

OK, DST_TOO_SMALL, INVALID_ARG = 0, 16, 18
CRC_NOP, CRC_CRC32, CRC_ADLER32, CRC_ADLER32_RFC = 0, 1, 2, 3
POISON, TAIL = 0xA5, 4096
MAX_STREAM_LEN = 0xFFFF0000


def rule(ref, counted, bad, align, arena_len, crc_op):
    """include/zipc_hip.h's layout rule over deflate_batch's results, serially: per stream (status, checksum, out_len, dst_off,
    roomed), and need.  counted[i]: the descriptor is within the format's range; bad: the declared sizes do not hold"""
    off = need = 0
    out = []
    for i, (st, ck, ol) in enumerate(zip(ref["status"].tolist(), ref["checksum"].tolist(), ref["out_len"].tolist())):
        if bad or not counted[i]:
            out.append((INVALID_ARG, 0, 0, 0, False))
        elif st != OK:
            out.append((st, ck, 0, 0, False))
        else:
            if off + ol <= arena_len:
                out.append((OK, ck, ol, off, True))
            else:
                out.append((DST_TOO_SMALL, ck if crc_op == CRC_CRC32 else 0, 0, off, True))
            need = off + ol
            off += (ol + align - 1) // align * align
    return out, need


def bound_formula(n, total, align, zlib_form):
    return total + 6 * (total // 65534) + 14 * n + (align - 1) * n + (6 * n if zlib_form else 0)


class Batch:
    """a batch of plains on the device, and what the batch form says of it"""

    def __init__(self, gpu_ctx, plains, level, zlib_form=False, too_long=(), flags=None):
        import torch

        from zipc_amd import batch

        self.ctx, self.plains, self.level, self.zlib, self.n = gpu_ctx, plains, level, zlib_form, len(plains)
        self.dev = torch.device("cuda", 0)
        lens = [len(p) for p in plains]
        offs = np.cumsum([0] + [l + 3 for l in lens[:-1]]).astype(np.uint64)  # (three bytes between the streams: odd source addresses)
        self.descs = batch.make_descs(offs, lens, np.full(self.n, 1 << 62, np.uint64), np.full(self.n, 1 << 40, np.uint64))  # (dst_off / dst_cap: not to be looked at)
        if flags is not None:
            self.descs["flags"] = flags
        self.counted = [True] * self.n
        for i in too_long:  # (its source is never read)
            self.descs["src_len"][i] = MAX_STREAM_LEN + 1 + i
            self.counted[i] = False
        self.max_src = max([l for l, c in zip(lens, self.counted) if c], default=0)
        self.total = sum(l for l, c in zip(lens, self.counted) if c)
        self.arena = np.frombuffer(b"".join(p + b"\x5a\x5a\x5a" for p in plains) + b"\0" * 64, dtype=np.uint8).copy()
        self.src = torch.from_numpy(self.arena).to(self.dev)
        self.d_descs = batch.to_device(self.descs, self.dev)
        self._ref, self._oracle = {}, None

    def reference(self, crc_op):
        """deflate_batch (zlib_compress_batch) into slots of the bound: (results, [each stream's bytes])"""
        import torch

        from zipc_amd import batch

        if crc_op not in self._ref:
            d = self.descs.copy()
            lens = [len(p) for p in self.plains]
            d["src_len"] = lens  # (a descriptor beyond the format's range: the others are expected as if it were absent)
            caps = [(batch.zlib_bound if self.zlib else batch.deflate_bound)(l) for l in lens]
            slots = np.cumsum([0] + [(c + 255) // 256 * 256 for c in caps]).astype(np.uint64)
            d["dst_off"], d["dst_cap"] = slots[:-1], caps
            dst = torch.full((int(slots[-1]) + TAIL,), POISON, dtype=torch.uint8, device=self.dev)
            d_res = torch.full((self.n * 16,), 0xEE, dtype=torch.uint8, device=self.dev)
            if self.zlib:
                batch.zlib_compress_batch(self.ctx, self.src, dst, batch.to_device(d, self.dev), d_res, self.n, max(lens), sum(lens), self.level)
            else:
                batch.deflate_batch(self.ctx, self.src, dst, batch.to_device(d, self.dev), d_res, self.n, max(lens), sum(lens), self.level, crc_op)
            res, out = batch.results_from_device(d_res), dst.cpu().numpy()
            self._ref[crc_op] = (res, [out[int(o):int(o) + int(l)] for o, l in zip(slots[:-1], res["out_len"])])
        return self._ref[crc_op]

    def oracle_streams(self, oracle):
        """the oracle's deflate (zlib_compress) of every plain at the batch's level"""
        if self._oracle is None:
            f = oracle.zlib_compress if self.zlib else oracle.deflate
            self._oracle = [f(p, level=self.level)[1] for p in self.plains]
        return self._oracle

    def need(self, align, crc_op=0):
        return rule(self.reference(crc_op)[0], self.counted, False, align, 0, crc_op)[1]

    def bound(self, align):
        from zipc_amd import batch

        return batch.deflate_packed_bound(self.n, self.total, align, zlib=self.zlib)

    def check(self, align, arena_len=None, crc_op=0, with_need=True, sync=True, declared=None, oracle=None, rfc=False):
        """one packed call against the expected results; arena_len: None = exactly `need`; declared: (max_src_len, total_src_len)
        where they are not the batch's own.  -> (results, need as written, the arena)"""
        import torch

        from zipc_amd import batch

        ref, ref_bytes = self.reference(crc_op)
        if arena_len is None:
            arena_len = self.need(align, crc_op)
        max_src, total = declared if declared else (self.max_src, self.total)
        bad = self.max_src > max_src or self.total > total
        want, need = rule(ref, self.counted, bad, align, arena_len, crc_op)
        dst = torch.full((arena_len + TAIL,), POISON, dtype=torch.uint8, device=self.dev)
        d_res = torch.full((self.n * 32,), 0xEE, dtype=torch.uint8, device=self.dev)
        d_need = torch.full((8,), 0xEE, dtype=torch.uint8, device=self.dev) if with_need else None
        kw = dict(align=align, need_dev=d_need, dst_arena_len=arena_len, sync=sync)
        if not sync:
            torch.cuda.synchronize()
        if self.zlib:
            batch.zlib_compress_packed_batch(self.ctx, self.src, dst, self.d_descs, d_res, self.n, max_src, total, self.level, **kw)
        else:
            batch.deflate_packed_batch(self.ctx, self.src, dst, self.d_descs, d_res, self.n, max_src, total, self.level, crc_op=crc_op, **kw)
        if not sync:
            self.ctx.synchronize()  # the one synchronize
        res = batch.packed_results_from_device(d_res)
        out = dst.cpu().numpy()
        got_need = int(d_need.cpu().numpy().view(np.uint64)[0]) if with_need else None
        what = (self.level, align, arena_len, crc_op, declared)
        print("packed call", what, "n", self.n, "need", got_need, "statuses", sorted(set(res["status"].tolist())))
        assert np.array_equal(self.src.cpu().numpy(), self.arena), "the source arena changed"
        assert np.array_equal(batch.to_device(self.descs, "cpu").numpy(), self.d_descs.cpu().numpy()), "the descriptors changed"
        if with_need:
            assert got_need == need, (what, got_need, need)
        may_write = np.zeros(arena_len + TAIL, bool)
        streams = self.oracle_streams(oracle) if oracle is not None else None
        for i, w in enumerate(want):
            got = tuple(int(res[f][i]) for f in ("status", "checksum", "out_len", "dst_off", "reserved"))
            assert got == w[:4] + (0,), (what, i, got, w)
            if w[0] == OK:
                off, ol = w[3], w[2]
                assert off % align == 0 and off + ol <= arena_len
                may_write[off:off + ol] = True
                assert np.array_equal(out[off:off + ol], ref_bytes[i]), (what, i, "bytes differ from the batch form's")
                if streams is not None:
                    mine = out[off:off + ol].tobytes()
                    if self.zlib and rfc:  # (the oracle's trailer is the reference's Adler-32)
                        assert mine[:-4] == streams[i][:-4], (what, i, "bytes differ from the oracle's")
                    else:
                        assert mine == streams[i], (what, i, "bytes differ from the oracle's")
        assert (out[~may_write] == POISON).all(), (what, "a byte outside every fitting stream's bytes was written",
                                                   np.nonzero(out[~may_write] != POISON)[0][:8])
        # the suffix property: the roomed streams that do not fit are exactly those from the first one that does not fit onwards
        roomed = [w for w in want if w[4]]
        fits = [w[0] == OK for w in roomed]
        assert fits == sorted(fits, reverse=True), what
        offs = [int(res["dst_off"][i]) for i, w in enumerate(want) if w[4]]
        assert offs == sorted(offs), what
        return res, got_need, out


# ---- exact output lengths

@pytest.fixture(scope="module")
def exact(gpu_ctx):
    return Batch(gpu_ctx, DC.exact_lengths(), 0)


@pytest.mark.parametrize("align", (1, 2, 16, 4096))
def test_exact_lengths(exact, oracle, align):
    """ZIPC_HIP_LEVEL_NONE: the outputs are 5, 15, 16, 17, 31, 33, 32 767, 32 768, 32 769 and 2 x 32 768 bytes long; at align 1
    dst_off modulo 16 takes every residue and two streams share a 16-byte unit; the arena exactly need, and the bound"""
    b = exact
    res, need, _ = b.check(align, oracle=oracle, crc_op=align % 4)
    assert tuple(res["out_len"].tolist()) == DC.EXACT_OUT_LENS and (res["status"] == OK).all()
    if align == 1:
        assert {int(o) % 16 for o in res["dst_off"]} == set(range(16))
        assert int(res["dst_off"][0]) // 16 == int(res["dst_off"][1]) // 16
        assert need == sum(DC.EXACT_OUT_LENS)
    full = b.bound(align)
    assert full == bound_formula(b.n, b.total, align, False) >= need
    res, _, _ = b.check(align, arena_len=full)
    assert (res["status"] == OK).all()


@pytest.mark.parametrize("align", (1, 16))
def test_the_arenas_end(exact, align):
    """the arena exactly need, one byte short, empty and cut in the middle: need is the same in all four, the streams from
    the first that does not fit onwards say where they would lie and leave their room as it was; d_need may be null"""
    b = exact
    need = b.need(align)
    full, n0, _ = b.check(align, arena_len=need)
    short, n1, _ = b.check(align, arena_len=need - 1)
    none, n2, _ = b.check(align, arena_len=0)
    mid, n3, _ = b.check(align, arena_len=need // 2)
    assert n0 == n1 == n2 == n3 == need
    assert (full["status"] == OK).all() and (short["status"][:-1] == OK).all() and short["status"][-1] == DST_TOO_SMALL
    assert (none["status"] == DST_TOO_SMALL).all() and not none["out_len"].any()
    first = mid["status"].tolist().index(DST_TOO_SMALL)
    assert 0 < first < b.n - 1 and (mid["status"][first:] == DST_TOO_SMALL).all() and (mid["status"][:first] == OK).all()
    for r in (short, none, mid):
        assert np.array_equal(r["dst_off"], full["dst_off"])
    b.check(align, arena_len=need // 2, with_need=False)


def test_two_segments_and_five_bytes(gpu_ctx, oracle):
    """an output of 2 x 32 768 + 5 bytes (`Fast), at a destination off every boundary: two whole segments and a third of 5 bytes"""
    plains, level, k = DC.two_segments_and_five()
    b = Batch(gpu_ctx, plains, level)
    for align in (1, 16):
        res, _, _ = b.check(align, oracle=oracle)
        assert int(res["out_len"][k]) == DC.TWO_SEGMENTS_AND_FIVE and (align != 1 or int(res["dst_off"][k]) % 16 != 0)


# ---- the scans' boundaries

@pytest.fixture(scope="module")
def tiny(gpu_ctx):
    return {n: Batch(gpu_ctx, DC.tiny()[:n], 1 + n % 3) for n in (1, 63, 64, 65, 1023, 1024, 1025, 2049)}


@pytest.mark.parametrize("n", (1, 63, 64, 65, 1023, 1024, 1025, 2049))
def test_scan_boundaries(tiny, oracle, n):
    """tiny streams on both sides of a wave, a tile and two tiles, at align 1 and 2: the arena exactly need and cut in the middle"""
    b = tiny[n]
    res, need, _ = b.check(1, oracle=oracle)
    assert (res["status"] == OK).all() and need == int(res["out_len"].sum())
    b.check(2, arena_len=b.need(2) // 2)


# ---- levels, checksums, the round trip

@pytest.fixture(scope="module")
def mixed(gpu_ctx):
    return {level: Batch(gpu_ctx, DC.mixed(), level) for level in (1, 2, 3)}


@pytest.mark.parametrize("level", (1, 2, 3))
def test_levels(mixed, oracle, level):
    """about 200 ragged streams of text, runs and random bytes at every compressing level: the batch form's results and bytes,
    which are the oracle's; the bound as the arena fits them all"""
    b = mixed[level]
    res, need, _ = b.check(64, oracle=oracle)
    assert (res["status"] == OK).all()
    res, _, _ = b.check(1, arena_len=b.bound(1), crc_op=CRC_CRC32)
    assert (res["status"] == OK).all() and need <= b.bound(64)


@pytest.mark.parametrize("crc_op", (0, 1, 2, 3))
def test_checksums(mixed, oracle, crc_op):
    """every crc_op at `Default, the arena cut in the middle: a stream that fits has deflate_batch's checksum, one that does not has
    the CRC-32 of its source with ZIPC_HIP_CRC_CRC32 and 0 otherwise"""
    import zlib

    b = mixed[2]
    res, _, _ = b.check(8, arena_len=b.need(8, crc_op) // 2, crc_op=crc_op)
    short = res["status"] == DST_TOO_SMALL
    assert short.any() and (~short).any()
    for i, p in enumerate(b.plains):
        want = (0, zlib.crc32(p), oracle.deflate(p, level=2, crc_op=oracle.CRC_ADLER32)[2] if crc_op == CRC_ADLER32 else 0, zlib.adler32(p))[crc_op]
        if short[i]:
            want = want if crc_op == CRC_CRC32 else 0
        assert int(res["checksum"][i]) == want, (crc_op, i)


def test_round_trip(mixed, gpu_ctx):
    """`Default: the packed arena, as it lies, goes through zipc_hip_inflate_packed_batch and gives the plains back"""
    import torch

    from zipc_amd import batch

    b = mixed[2]
    res, need, out = b.check(16)
    d = batch.make_descs(res["dst_off"], res["out_len"], np.zeros(b.n, np.uint64), np.zeros(b.n, np.uint64))
    src = torch.from_numpy(np.concatenate([out[:need], np.zeros(64, np.uint8)])).to(b.dev)
    total = sum(len(p) for p in b.plains)
    dst = torch.full((total + TAIL,), POISON, dtype=torch.uint8, device=b.dev)
    d_res = torch.full((b.n * 32,), 0xEE, dtype=torch.uint8, device=b.dev)
    batch.inflate_packed_batch(gpu_ctx, src, dst, batch.to_device(d, b.dev), d_res, b.n, b.max_src, align=1, dst_arena_len=total)
    back, plain = batch.packed_results_from_device(d_res), dst.cpu().numpy()
    assert (back["status"] == OK).all()
    for i, p in enumerate(b.plains):
        assert plain[int(back["dst_off"][i]):int(back["dst_off"][i]) + int(back["out_len"][i])].tobytes() == p, i


def test_long_stream_by_segments(gpu_ctx, oracle):
    """a stream of 300 KiB of runs among short ones at `Default: deflate parses it by segments; its output is copied by several
    workgroups to a destination off every boundary"""
    b = Batch(gpu_ctx, DC.long_runs_among_short(), 2)
    res, _, _ = b.check(1, oracle=oracle, crc_op=CRC_ADLER32)
    assert (res["status"] == OK).all() and int(res["dst_off"][5]) % 16 != 0
    b.check(4096, arena_len=b.need(4096) - 1)


# ---- the zlib form

@pytest.mark.parametrize("rfc", (False, True))
def test_zlib_form(gpu_ctx, oracle, rfc):
    """whole zlib streams in the arena with both Adler-32 flavours; an unknown flag bit is INVALID_ARG in the stream's own result
    and takes no room"""
    import zlib

    plains = DC.mixed()[:40] + DC.exact_lengths()[:8]
    flags = np.zeros(len(plains), np.uint32)
    flags[3], flags[4] = 2, 1
    gpu_ctx.set_adler_rfc1950(rfc)
    try:
        b = Batch(gpu_ctx, plains, 2, zlib_form=True, flags=flags)
        for align, cut in ((1, False), (16, True), (4096, False)):
            need = b.need(align, 0)
            res, _, out = b.check(align, arena_len=need // 2 if cut else need, oracle=oracle, rfc=rfc)
            assert res["status"][3] == INVALID_ARG and res["dst_off"][3] == 0 and res["status"][4] in (OK, DST_TOO_SMALL)
            for i, p in enumerate(plains):
                if res["status"][i] == OK:
                    assert int(res["checksum"][i]) == (zlib.adler32(p) if rfc else oracle.zlib_compress(p, level=2)[2]), i  # (the reference's: taken block by block)
                    s = out[int(res["dst_off"][i]):int(res["dst_off"][i]) + int(res["out_len"][i])].tobytes()
                    if rfc:
                        assert zlib.decompress(s) == p, i
        res, _, _ = b.check(2, arena_len=b.bound(2))
        assert b.bound(2) == bound_formula(b.n, b.total, 2, True) and (np.delete(res["status"], 3) == OK).all()
    finally:
        gpu_ctx.set_adler_rfc1950(False)


# ---- descriptors and declared sizes

def test_descriptor_beyond_the_formats_range(gpu_ctx):
    """one descriptor in the middle with src_len above ZIPC_HIP_MAX_STREAM_LEN: INVALID_ARG in its own result, no room, and the
    others placed as if it were absent"""
    plains = DC.exact_lengths()[:12]
    with_it = Batch(gpu_ctx, plains, 0, too_long=(5,))
    without = Batch(gpu_ctx, plains[:5] + plains[6:], 0)
    for align in (1, 16):
        a, need_a, out_a = with_it.check(align, crc_op=CRC_CRC32)
        b, need_b, out_b = without.check(align, crc_op=CRC_CRC32)
        assert tuple(a[5]) == (INVALID_ARG, 0, 0, 0, 0) and need_a == need_b
        assert np.array_equal(np.delete(a, 5), b) and np.array_equal(out_a, out_b)


@pytest.mark.parametrize("level", (0, 2))
def test_declared_sizes(gpu_ctx, exact, mixed, level):
    """total_src_len and max_src_len each declared one too small: every result INVALID_ARG with out_len 0 and dst_off 0, need 0,
    the arena all poison"""
    b = exact if level == 0 else mixed[2]
    for declared in ((b.max_src, b.total - 1), (b.max_src - 1, b.total)):
        res, need, out = b.check(16, arena_len=b.bound(16), declared=declared, crc_op=CRC_CRC32)
        assert (res["status"] == INVALID_ARG).all() and not res["out_len"].any() and not res["dst_off"].any() and not res["checksum"].any()
        assert need == 0 and (out == POISON).all()
    res, _, _ = b.check(16, declared=(b.max_src + 1, b.total + 1))
    assert (res["status"] == OK).all()


def test_results_without_a_synchronising_call(mixed, tiny):
    """sync=False: the call enqueues and returns (the scratch is there from the calls before); after ONE synchronize the results are there"""
    mixed[1].check(64, sync=False)
    tiny[1025].check(1, sync=False, crc_op=CRC_ADLER32_RFC)


# ---- bad calls

def test_bad_calls(gpu_ctx, exact):
    """each call-level rule: INVALID_ARG, and no byte of the arena, the results or need changed; n_streams == 0 is OK and
    writes nothing either"""
    import torch

    from zipc_amd import _lib

    L = _lib.lib()
    b = exact
    dst = torch.full((1024 + TAIL,), POISON, dtype=torch.uint8, device=b.dev)
    d_res = torch.full((b.n * 32,), 0xEE, dtype=torch.uint8, device=b.dev)
    d_need = torch.full((8,), 0xEE, dtype=torch.uint8, device=b.dev)
    torch.cuda.synchronize()
    h, s, d, de, r, nd = gpu_ctx.handle, b.src.data_ptr(), dst.data_ptr(), b.d_descs.data_ptr(), d_res.data_ptr(), d_need.data_ptr()
    raw, zl = L.zipc_hip_deflate_packed_batch, L.zipc_hip_zlib_compress_packed_batch
    ok = dict(ctx=h, src=s, dst=d, arena=1024, descs=de, res=r, n=b.n, max_src=b.max_src, total=b.total, level=0, crc_op=0, align=8, need=nd)

    def call(**kw):
        a = dict(ok, **kw)
        return (raw(a["ctx"], a["src"], a["dst"], a["arena"], a["descs"], a["res"], a["n"], a["max_src"], a["total"], a["level"], a["crc_op"],
                    a["align"], a["need"]),
                zl(a["ctx"], a["src"], a["dst"], a["arena"], a["descs"], a["res"], a["n"], a["max_src"], a["total"], a["level"], a["align"], a["need"]))

    bad = (INVALID_ARG, INVALID_ARG)
    assert call(ctx=None) == bad and call(descs=None) == bad and call(res=None) == bad
    assert call(dst=None) == bad                       # a null arena with a length
    assert call(n=0x80000000) == bad
    assert call(total=0x7FFFFFFF * 32768) == bad       # the copy's grid bound above 0x7FFFFFFF
    for align in (0, 3, 12, 4097, 8192, 1 << 40):
        assert call(align=align) == bad, align
    for level in (-1, 4):
        assert call(level=level) == bad, level
    assert call(max_src=MAX_STREAM_LEN + 1) == bad
    for crc_op in (-1, 4):  # (the zlib form has no crc_op: the raw form alone)
        assert raw(h, s, d, 1024, de, r, b.n, b.max_src, b.total, 0, crc_op, 8, nd) == INVALID_ARG, crc_op
    assert call(n=0) == (OK, OK)                       # nothing is enqueued, need is not written
    assert call(n=0, dst=None, arena=0, need=None) == (OK, OK)
    gpu_ctx.synchronize()
    assert (dst.cpu().numpy() == POISON).all() and (d_res.cpu().numpy() == 0xEE).all() and (d_need.cpu().numpy() == 0xEE).all()
