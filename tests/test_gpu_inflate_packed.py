"""Packed decode on the MI355X: zipc_hip_inflate_packed_batch / zipc_hip_zlib_decompress_packed_batch -- a batch of streams of
unknown size sized, laid out end to end in one arena, decoded there and reported, in one call.

The expected results of every call: the sizes come from zipc_hip_inflate_size_batch (zipc_hip_zlib_size_batch), the layout rule
of include/zipc_hip.h is applied in Python (`rule` below), and zipc_hip_inflate_batch (zipc_hip_zlib_decompress_batch) runs
with those descriptors -- dst_off from the rule, dst_cap = out_len -- into a second arena.  The packed call must give equal
results and equal bytes, and the bytes must be the inputs the streams were made from (tests/packed_cases.py).  Every
destination arena is dst_arena_len + 4096 bytes of poison; the tail, every padding gap and the room of every stream that did
not fit must still hold it after the call."""
import os
import zlib

import numpy as np
import pytest

import packed_cases as PC

pytestmark = pytest.mark.gpu

OK, CORRUPTED, CHECKSUM, DST_TOO_SMALL, INVALID_ARG = 0, 1, 6, 16, 18
POISON, TAIL = 0xA5, 4096
MAX_STREAM_LEN = 0xFFFF0000
BLOCKS_ON = os.environ.get("ZIPC_HIP_INFLATE_BLOCKS") != "0"


def rule(sized, max_out_len, align, arena_len):
    """include/zipc_hip.h's layout rule over the sizing results, serially: per stream (status, roomed, dst_off), and need"""
    off = need = 0
    out = []
    for st, ol in zip(sized["status"].tolist(), sized["out_len"].tolist()):
        if st == OK and ol <= max_out_len:
            out.append((OK if off + ol <= arena_len else DST_TOO_SMALL, True, off))
            need = off + ol
            off += (ol + align - 1) // align * align
        else:
            out.append((st if st != OK else INVALID_ARG, False, 0))
    return out, need


class Batch:
    """a batch on the device, and what the sizing form says of it"""

    def __init__(self, gpu_ctx, items, zlib_form=False):
        import torch

        from zipc_amd import batch

        self.ctx, self.items, self.zlib, self.n = gpu_ctx, items, zlib_form, len(items)
        self.dev = torch.device("cuda", 0)
        lens = [len(it.stream) for it in items]
        self.descs = batch.make_descs(np.cumsum([0] + lens[:-1]).astype(np.uint64), lens, np.full(self.n, 1 << 62, np.uint64),
                                      np.full(self.n, 1 << 40, np.uint64))  # (dst_off / dst_cap: not to be looked at)
        for i, it in enumerate(items):
            if it.limit is not None:
                self.descs["limit"][i], self.descs["flags"][i] = it.limit, 1
            if it.flags is not None:
                self.descs["flags"][i] = it.flags
        self.arena = np.frombuffer(b"".join(it.stream for it in items) + b"\0" * 64, dtype=np.uint8).copy()
        self.src = torch.from_numpy(self.arena).to(self.dev)
        self.d_descs = batch.to_device(self.descs, self.dev)
        d_res = torch.full((self.n * 16,), 0xEE, dtype=torch.uint8, device=self.dev)
        (batch.zlib_size_batch if zlib_form else batch.inflate_size_batch)(gpu_ctx, self.src, self.d_descs, d_res, self.n)
        self.sized = batch.results_from_device(d_res)

    def need(self, max_out_len, align):
        return rule(self.sized, max_out_len, align, 0)[1]

    def reference(self, want, max_out_len, arena_len, crc_op):
        """inflate_batch (zlib_decompress_batch) over the rule's descriptors into an arena of its own: (results, arena)"""
        import torch

        from zipc_amd import batch

        d = self.descs.copy()
        for i, (st, _, off) in enumerate(want):
            if st == OK:
                d["dst_off"][i], d["dst_cap"][i] = off, self.sized["out_len"][i]
            else:  # it is not to reach the decoder: nothing to read, no room
                d["src_len"][i], d["dst_off"][i], d["dst_cap"][i], d["flags"][i] = 0, 0, 0, 0
        dst = torch.full((arena_len + TAIL,), POISON, dtype=torch.uint8, device=self.dev)
        d_res = torch.full((self.n * 16,), 0xEE, dtype=torch.uint8, device=self.dev)
        if self.zlib:
            batch.zlib_decompress_batch(self.ctx, self.src, dst, batch.to_device(d, self.dev), d_res, self.n, max_out_len)
        else:
            batch.inflate_batch(self.ctx, self.src, dst, batch.to_device(d, self.dev), d_res, self.n, max_out_len, crc_op)
        return batch.results_from_device(d_res), dst.cpu().numpy()

    def check(self, max_out_len, align, arena_len=None, crc_op=0, with_need=True, sync=True, statuses=None):
        """one packed call against the expected results; arena_len: None = exactly `need`.  -> (results, need as written)"""
        import torch

        from zipc_amd import batch

        if arena_len is None:
            arena_len = self.need(max_out_len, align)
        want, need = rule(self.sized, max_out_len, align, arena_len)
        ref, ref_arena = self.reference(want, max_out_len, arena_len, crc_op)
        dst = torch.full((arena_len + TAIL,), POISON, dtype=torch.uint8, device=self.dev)
        d_res = torch.full((self.n * 32,), 0xEE, dtype=torch.uint8, device=self.dev)
        d_need = torch.full((8,), 0xEE, dtype=torch.uint8, device=self.dev) if with_need else None
        kw = dict(align=align, need_dev=d_need, dst_arena_len=arena_len, sync=sync)
        if not sync:
            torch.cuda.synchronize()
        if self.zlib:
            batch.zlib_decompress_packed_batch(self.ctx, self.src, dst, self.d_descs, d_res, self.n, max_out_len, **kw)
        else:
            batch.inflate_packed_batch(self.ctx, self.src, dst, self.d_descs, d_res, self.n, max_out_len, crc_op=crc_op, **kw)
        if not sync:
            self.ctx.synchronize()  # the one synchronize
        self.blocks = (self.ctx.last_size_blocks(), self.ctx.last_inflate_blocks())
        res = batch.packed_results_from_device(d_res)
        out = dst.cpu().numpy()
        got_need = int(d_need.cpu().numpy().view(np.uint64)[0]) if with_need else None
        what = (max_out_len, align, arena_len, crc_op)
        print("packed call", what, "need", got_need, "statuses", sorted(set(res["status"].tolist())))
        assert np.array_equal(self.src.cpu().numpy(), self.arena), "the source arena changed"
        assert np.array_equal(batch.to_device(self.descs, "cpu").numpy(), self.d_descs.cpu().numpy()), "the descriptors changed"
        if with_need:
            assert got_need == need, (what, got_need, need)
        may_write = np.zeros(arena_len + TAIL, bool)
        for i, ((st, roomed, off), it) in enumerate(zip(want, self.items)):
            got = tuple(int(res[f][i]) for f in ("status", "checksum", "out_len", "dst_off", "reserved"))
            if st == OK:
                size = int(self.sized["out_len"][i])
                assert off % align == 0
                assert got == (int(ref["status"][i]), int(ref["checksum"][i]), int(ref["out_len"][i]), off, 0), (what, it.name, got, ref[i])
                may_write[off:off + size] = True
                if got[0] == OK:
                    assert got[2] == size == len(it.plain), (what, it.name)
                    assert out[off:off + size].tobytes() == it.plain, (what, it.name, "bytes")
                else:
                    assert self.zlib and got[0] == CHECKSUM and got[2] == 0, (what, it.name, got)  # sized OK, decoded, refused by its trailer
            else:
                assert got == (st, 0, 0, off if roomed else 0, 0), (what, it.name, got, st)
        assert np.array_equal(out[may_write], ref_arena[may_write]), (what, "bytes differ from inflate_batch's")
        assert (out[~may_write] == POISON).all(), (what, "a byte outside every fitting stream's room was written",
                                                   np.nonzero(out[~may_write] != POISON)[0][:8])
        assert (ref_arena[~may_write] == POISON).all(), (what, "inflate_batch itself wrote outside [dst_off, dst_off + dst_cap)")
        if statuses is not None:
            assert tuple(res["status"].tolist()) == tuple(statuses), (what, res["status"])
        return res, got_need


# ---- mixed verdicts

@pytest.fixture(scope="module")
def mixed(gpu_ctx):
    from zipc_amd import zipc_deflate as Z

    items, max_out_len, statuses = PC.mixed_verdicts(lambda data: Z.deflate(data, level=2, ctx=gpu_ctx).get_ok())
    return Batch(gpu_ctx, items), max_out_len, statuses


@pytest.mark.parametrize("align", (1, 16, 4096))
def test_mixed_verdicts(mixed, align):
    """two good streams, an empty source, a corrupted stream, a limit exceeded, a limit met exactly, an unknown flag bit, a
    stream of no bytes and one sized above max_out_len, in one batch: four take room, in index order, on multiples of align"""
    b, max_out_len, statuses = mixed
    res, need = b.check(max_out_len, align, statuses=statuses)
    roomed = [i for i in range(b.n) if statuses[i] == OK]
    assert roomed == [0, 1, 5, 7]
    sizes = [len(b.items[i].plain) for i in roomed]
    offs = [int(res["dst_off"][i]) for i in roomed]
    up = lambda v: (v + align - 1) // align * align  # noqa: E731
    assert offs == [0, up(sizes[0]), up(sizes[0]) + up(sizes[1]), up(sizes[0]) + up(sizes[1]) + up(sizes[2])]
    assert need == offs[3] + 0 and sizes[3] == 0
    assert not res["dst_off"][[i for i in range(b.n) if i not in roomed]].any()


def test_results_without_a_synchronising_call(mixed):
    """sync=False, max_out_len below 256 KiB: the call enqueues and returns; after ONE synchronize the results are there"""
    b, max_out_len, statuses = mixed
    b.check(max_out_len, 16, sync=False, statuses=statuses)


# ---- the scan's boundaries

@pytest.fixture(scope="module")
def tiny(gpu_ctx):
    return {n: Batch(gpu_ctx, PC.tiny_pool()[:n]) for n in (1, 63, 64, 65, 1023, 1024, 1025, 2049)}


@pytest.mark.parametrize("align", (1, 8))
@pytest.mark.parametrize("n", (1, 63, 64, 65, 1023, 1024, 1025, 2049))
def test_scan_boundaries(tiny, n, align):
    """tiny streams on both sides of a wave, a tile and two tiles; every 7th corrupted"""
    b = tiny[n]
    res, need = b.check(40, align)
    assert sum(st == CORRUPTED for st in res["status"].tolist()) == n // 7
    assert need == b.need(40, align) and (n < 7 or need > 0)


# ---- the arena's end

@pytest.mark.parametrize("zero_tail", (False, True))
def test_the_arenas_end(gpu_ctx, zero_tail):
    """the arena exactly need, one byte short and empty: need is the same in all three; one byte short the last stream with
    bytes (and what lies behind it) does not fit but says where it would lie; d_need may be null"""
    items = list(PC.tiny_pool()[7:13]) + [PC.Item("text", PC.raw_zlib(b"the arena ends here " * 9), b"the arena ends here " * 9)]
    if zero_tail:
        items += [PC.Item("nothing%d" % k, PC.raw_zlib(b""), b"") for k in range(2)]
    b = Batch(gpu_ctx, tuple(items))
    need = b.need(4096, 4)
    assert need % 4 == 0  # (the last stream with bytes is 180 long)
    res_full, n0 = b.check(4096, 4, arena_len=need)
    res_short, n1 = b.check(4096, 4, arena_len=need - 1)
    res_none, n2 = b.check(4096, 4, arena_len=0)
    assert n0 == n1 == n2 == need
    last = 6
    assert res_full["status"][last] == OK and res_short["status"][last] == DST_TOO_SMALL
    assert res_short["dst_off"][last] == res_full["dst_off"][last] == need - 180
    if zero_tail:  # the rule as it stands: need + 0 <= need - 1 is false
        assert (res_full["status"][7:] == OK).all() and (res_short["status"][7:] == DST_TOO_SMALL).all()
        assert (res_short["dst_off"][7:] == need).all()
    assert (res_none["out_len"] == 0).all()
    assert (res_none["status"][[i for i in range(b.n) if b.items[i].plain]] == DST_TOO_SMALL).all()
    b.check(4096, 4, arena_len=need, with_need=False)
    b.check(4096, 4, arena_len=need - 1, with_need=False)


# ---- checksums

@pytest.fixture(scope="module")
def ragged(gpu_ctx):
    return Batch(gpu_ctx, PC.ragged_batch())


def _reference_adler(oracle, stream):
    """the Adler-32 the reference's inflate gives (its value depends on how inflate hands the bytes over, block by block)"""
    st, _, adler = oracle.inflate(stream, crc_op=oracle.CRC_ADLER32)
    assert st == OK
    return adler


@pytest.mark.parametrize("crc_op", (0, 1, 2, 3))
def test_checksums(ragged, oracle, crc_op):
    """every crc_op over ~200 ragged streams of 1 B .. 70 KiB: inflate_batch's checksums (the check inside Batch.check), which
    are zlib's CRC-32 and Adler-32 and the Adler-32 of the oracle's inflate; the two Adler-32 flavours differ where the header says they do"""
    b = ragged
    sizes = [len(it.plain) for it in b.items]
    assert b.n >= 200 and min(sizes) == 1 and max(sizes) == 70 << 10
    res, _ = b.check(70 << 10, 64, crc_op=crc_op)
    assert (res["status"] == OK).all()
    for i, it in enumerate(b.items):
        want = (0, zlib.crc32(it.plain), _reference_adler(oracle, it.stream), zlib.adler32(it.plain))[crc_op]
        assert int(res["checksum"][i]) == want, (crc_op, it.name)
    high = [it for it in b.items if it.name.startswith("high_")]
    assert len(high) == 2 and all(len(it.plain) >= 6 * 1024 and min(it.plain) > 0x7F for it in high)
    assert all(_reference_adler(oracle, it.stream) != zlib.adler32(it.plain) for it in high)


# ---- the block path

@pytest.mark.parametrize("align", (1, 256))
def test_block_path(gpu_ctx, align):
    """a stream of text that inflates to 500 000 bytes among 50 short ones, max_out_len 512 KiB: sized by blocks, decoded by
    blocks, results and bytes as ever -- also where the long stream's room begins on no boundary at all (align 1)"""
    b = Batch(gpu_ctx, PC.long_among_short())
    res, _ = b.check(PC.MAX_OUT_BLOCKS, align, crc_op=1)
    assert align != 1 or int(res["dst_off"][20]) % 4 != 0
    assert (res["status"] == OK).all() and int(res["out_len"][20]) == PC.LONG_PLAIN_LEN
    print("blocks (sizing, decode):", b.blocks)
    if BLOCKS_ON:
        assert b.blocks[0] > 0 and b.blocks[1] > 0, b.blocks


# ---- the zlib form

def test_zlib_form(gpu_ctx, oracle):
    """good streams, every header failure, a wrong trailer, lengths under 6: a header failure takes no room, a checksum
    mismatch reports the value found, no bytes and the dst_off it was given"""
    import zlib_cases

    cases = PC.zlib_batch()
    exp = [zlib_cases.expect_decompress(c) for c in cases]
    items = tuple(PC.Item(c.name, c.stream, e.out if e.status == OK else None, c.limit, None) for c, e in zip(cases, exp))
    b = Batch(gpu_ctx, items, zlib_form=True)
    for align in (1, 32):
        res, _ = b.check(32768, align, statuses=[e.status for e in exp])
        for i, (c, e) in enumerate(zip(cases, exp)):
            assert int(res["checksum"][i]) == e.checksum, c.name
            if e.header:
                assert int(res["dst_off"][i]) == 0, c.name
        k = [c.name for c in cases].index("trailer_byte_-1")
        assert exp[k].status == CHECKSUM and int(res["out_len"][k]) == 0
        assert int(res["dst_off"][k]) == sum((int(b.sized["out_len"][j]) + align - 1) // align * align for j in range(k) if b.sized["status"][j] == OK) > 0
    assert {e.status for e in exp} >= {0, 1, 3, 4, 5, 6}


# ---- bad calls

def test_bad_calls(gpu_ctx):
    """each call-level rule: INVALID_ARG, and no byte of the arena, the results or need changed; n_streams == 0 is OK and
    writes nothing either"""
    import torch

    from zipc_amd import _lib

    L = _lib.lib()
    b = Batch(gpu_ctx, PC.tiny_pool()[:5])
    dst = torch.full((1024 + TAIL,), POISON, dtype=torch.uint8, device=b.dev)
    d_res = torch.full((b.n * 32,), 0xEE, dtype=torch.uint8, device=b.dev)
    d_need = torch.full((8,), 0xEE, dtype=torch.uint8, device=b.dev)
    torch.cuda.synchronize()
    h, s, d, de, r, nd = gpu_ctx.handle, b.src.data_ptr(), dst.data_ptr(), b.d_descs.data_ptr(), d_res.data_ptr(), d_need.data_ptr()
    raw, zl = L.zipc_hip_inflate_packed_batch, L.zipc_hip_zlib_decompress_packed_batch
    ok = dict(ctx=h, src=s, dst=d, arena=1024, descs=de, res=r, n=b.n, max_out=40, align=8, crc_op=0, need=nd)

    def call(**kw):
        a = dict(ok, **kw)
        return (raw(a["ctx"], a["src"], a["dst"], a["arena"], a["descs"], a["res"], a["n"], a["max_out"], a["align"], a["crc_op"], a["need"]),
                zl(a["ctx"], a["src"], a["dst"], a["arena"], a["descs"], a["res"], a["n"], a["max_out"], a["align"], a["need"]))

    bad = (INVALID_ARG, INVALID_ARG)
    assert call(ctx=None) == bad and call(descs=None) == bad and call(res=None) == bad
    assert call(dst=None) == bad                       # a null arena with a length
    assert call(n=0x80000000) == bad
    for align in (0, 3, 12, 4097, 8192, 1 << 40):
        assert call(align=align) == bad, align
    assert call(max_out=MAX_STREAM_LEN + 1) == bad
    for crc_op in (-1, 4):  # (the zlib form has no crc_op: the raw form alone)
        assert raw(h, s, d, 1024, de, r, b.n, 40, 8, crc_op, nd) == INVALID_ARG, crc_op
    assert call(n=0) == (OK, OK)                       # nothing is enqueued, need is not written
    assert call(n=0, dst=None, arena=0, need=None) == (OK, OK)
    gpu_ctx.synchronize()
    assert (dst.cpu().numpy() == POISON).all() and (d_res.cpu().numpy() == 0xEE).all() and (d_need.cpu().numpy() == 0xEE).all()
