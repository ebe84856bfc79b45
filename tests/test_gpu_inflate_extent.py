"""The extent forms on the MI355X (include/zipc_hip.h at zipc_hip_inflate_extent_batch): where every stream of a batch
ends.  Every case of the catalogue (tests/extent_cases.py) through the six batch forms, one batch per form: the sources
side by side in one arena at every alignment 0 .. 7 of src_off, every room between 64 guard bytes of 0xA5 in a poisoned
destination arena, results that start as 0xEE.  What is expected comes from the catalogue (the oracle's status, length and
bytes, the references' extent), and the forms are held directly to the forms they mirror:

  - raw, decode: results and the WHOLE destination arena equal zipc_hip_inflate_batch's for the same descriptors, with
    ZIPC_HIP_CRC_NOP, CRC-32 and both Adler-32 flavours;
  - raw, size: zipc_hip_inflate_size_batch's results; the blocks form: the wave form's, with zipc_hip_last_size_blocks > 0
    on the 512 KiB streams;
  - the mirrored form with src_len := src_used gives identical results and bytes (zlib: zipc_hip_zlib_decompress_batch and
    zipc_hip_zlib_size_batch, which need the exact length);
  - zipc_hip_last_inflate_blocks is 0 behind the wave forms, whatever max_dst_cap;
  - a stream that ends on the last byte of an arena allocated at exactly that size;
  - the two host forms, and the recipe's walk over zlib streams stored back to back."""
import zlib

import numpy as np
import pytest

import extent_cases as EC
import inflate_room_cases as RC

pytestmark = pytest.mark.gpu
CRC_NOP, CRC_CRC32, CRC_ADLER32, CRC_ADLER32_RFC = 0, 1, 2, 3


class Arena:
    """the cases' sources side by side in a source arena (case i at src_off = i mod 8, mod 8), their rooms between guards in
    a poisoned destination arena"""

    def __init__(self, cases, exact_end=False):
        import torch

        self.cases, self.dev = cases, torch.device("cuda", 0)
        parts, self.src_off, pos = [], [], 0
        for i, c in enumerate(cases):
            pad = (i % 8 - pos) % 8
            parts.append(b"\x5a" * pad)
            pos += pad
            self.src_off.append(pos)
            parts.append(c.src)
            pos += len(c.src)
        blob = b"".join(parts) + (b"" if exact_end else b"\x5a" * 64)
        self.src = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(self.dev)
        self.src_clone = self.src.clone()
        self.src_len = [len(c.src) for c in cases]
        self.caps = [c.cap for c in cases]
        self.dst_off, self.total, self.guards = RC.layout(self.caps, [RC.OFF_MODS[i % 4] for i in range(len(cases))])
        self.max_cap = max(self.caps)

    def fresh(self, width):
        """a poisoned destination arena and poisoned results of `width` bytes each"""
        import torch

        return (torch.full((self.total,), RC.POISON, dtype=torch.uint8, device=self.dev),
                torch.full((len(self.cases) * width,), 0xEE, dtype=torch.uint8, device=self.dev))

    def descs(self, src_len=None):
        from zipc_amd import batch

        d = batch.make_descs(np.array(self.src_off, np.uint64), self.src_len if src_len is None else src_len, self.dst_off, self.caps)
        for i, c in enumerate(self.cases):
            d["flags"][i] = c.flags | (1 if c.limit is not None else 0)
            d["limit"][i] = c.limit or 0
        return batch.to_device(d, self.dev)

    def check_guards(self, dst, form):
        out = dst.cpu().numpy()
        for i, c in enumerate(self.cases):
            assert (out[self.guards[i][0]] == RC.POISON).all() and (out[self.guards[i][1]] == RC.POISON).all(), (form, c.name, "wrote outside its room")
        return out


def _records(res):
    return [tuple(int(res[f][i]) for f in ("status", "checksum", "out_len", "src_used", "reserved")) for i in range(len(res))]


def _checksum(oracle, crc_op, data):
    return {CRC_NOP: 0, CRC_CRC32: zlib.crc32(data), CRC_ADLER32: oracle.adler32(data), CRC_ADLER32_RFC: zlib.adler32(data)}[crc_op]


@pytest.fixture(scope="module")
def raw_arena():
    return Arena(list(EC.raw_cases()))


@pytest.fixture(scope="module")
def raw_wants(oracle):
    return [EC.want(oracle, c) for c in EC.raw_cases()], [EC.want(oracle, c, size=True) for c in EC.raw_cases()]


@pytest.mark.parametrize("crc_op", [CRC_NOP, CRC_CRC32, CRC_ADLER32, CRC_ADLER32_RFC])
def test_raw_decode_is_inflate_batch_with_the_extent(gpu_ctx, oracle, raw_arena, raw_wants, crc_op):
    import torch

    from zipc_amd import batch

    a, n = raw_arena, len(raw_arena.cases)
    descs = a.descs()
    dst, res = a.fresh(32)
    batch.inflate_extent_batch(gpu_ctx, a.src, dst, descs, res, n, a.max_cap, crc_op)
    assert gpu_ctx.last_inflate_blocks() == 0
    got = _records(batch.extent_results_from_device(res))
    out = a.check_guards(dst, "inflate_extent_batch")
    assert torch.equal(a.src, a.src_clone)
    for i, c in enumerate(a.cases):
        st, _, n_out, used, data = raw_wants[0][i]
        want = (st, _checksum(oracle, crc_op, data) if st == 0 else 0, n_out, used, 0)
        assert got[i] == want, (c.name, crc_op, got[i], want)
        assert used <= len(c.src)
        o = int(a.dst_off[i])
        assert out[o:o + n_out].tobytes() == data, (c.name, "bytes")
    # the form it mirrors, on the same descriptors: the same three fields, and the same arena to the last guard byte
    dst2, res2 = a.fresh(16)
    batch.inflate_batch(gpu_ctx, a.src, dst2, descs, res2, n, a.max_cap, crc_op)
    plain = batch.results_from_device(res2)
    assert [(int(plain["status"][i]), int(plain["checksum"][i]), int(plain["out_len"][i])) for i in range(n)] == [g[:3] for g in got]
    assert torch.equal(dst, dst2)
    # ... and with src_len := src_used: identical results and bytes
    exact = [g[3] if g[0] == 0 else a.src_len[i] for i, g in enumerate(got)]
    dst3, res3 = a.fresh(16)
    batch.inflate_batch(gpu_ctx, a.src, dst3, a.descs(exact), res3, n, a.max_cap, crc_op)
    again = batch.results_from_device(res3)
    assert (again["status"] == plain["status"]).all() and (again["checksum"] == plain["checksum"]).all() and (again["out_len"] == plain["out_len"]).all()
    assert torch.equal(dst, dst3)


def test_raw_size_is_inflate_size_batch_with_the_extent(gpu_ctx, raw_arena, raw_wants):
    from zipc_amd import batch

    a, n = raw_arena, len(raw_arena.cases)
    descs = a.descs()
    _, res = a.fresh(32)
    batch.inflate_size_extent_batch(gpu_ctx, a.src, descs, res, n)
    assert gpu_ctx.last_size_blocks() == 0
    got = _records(batch.extent_results_from_device(res))
    for i, c in enumerate(a.cases):
        st, _, n_out, used, _ = raw_wants[1][i]
        assert got[i] == (st, 0, n_out, used, 0), (c.name, got[i], raw_wants[1][i][:4])
    _, res2 = a.fresh(16)
    batch.inflate_size_batch(gpu_ctx, a.src, descs, res2, n)
    plain = batch.results_from_device(res2)
    assert [(int(plain["status"][i]), int(plain["checksum"][i]), int(plain["out_len"][i])) for i in range(n)] == [g[:3] for g in got]
    exact = [g[3] if g[0] == 0 else a.src_len[i] for i, g in enumerate(got)]
    _, res3 = a.fresh(16)
    batch.inflate_size_batch(gpu_ctx, a.src, a.descs(exact), res3, n)
    again = batch.results_from_device(res3)
    assert (again["status"] == plain["status"]).all() and (again["out_len"] == plain["out_len"]).all()
    # the blocks form over the same batch, whichever of its streams it picks: the same results
    _, res4 = a.fresh(32)
    batch.inflate_size_extent_blocks_batch(gpu_ctx, a.src, descs, res4, n)
    assert _records(batch.extent_results_from_device(res4)) == got


@pytest.fixture(scope="module")
def zlib_arena():
    return Arena(list(EC.zlib_cases()))


def test_zlib_decode_and_size(gpu_ctx, oracle, zlib_arena):
    import torch

    from zipc_amd import batch

    a, n = zlib_arena, len(zlib_arena.cases)
    descs = a.descs()
    dst, res = a.fresh(32)
    batch.zlib_decompress_extent_batch(gpu_ctx, a.src, dst, descs, res, n, a.max_cap)
    assert gpu_ctx.last_inflate_blocks() == 0
    got = _records(batch.extent_results_from_device(res))
    out = a.check_guards(dst, "zlib_decompress_extent_batch")
    assert torch.equal(a.src, a.src_clone)
    n_ok = 0
    for i, c in enumerate(a.cases):
        st, ck, n_out, used, data = EC.want(oracle, c)
        assert got[i] == (st, ck, n_out, used, 0), (c.name, got[i], (st, ck, n_out, used))
        assert used <= len(c.src)
        o = int(a.dst_off[i])
        assert out[o:o + n_out].tobytes() == data, (c.name, "bytes")
        n_ok += st == 0
    assert n_ok > 400
    _, res_s = a.fresh(32)
    batch.zlib_size_extent_batch(gpu_ctx, a.src, descs, res_s, n)
    sized = _records(batch.extent_results_from_device(res_s))
    for i, c in enumerate(a.cases):
        st, ck, n_out, used, _ = EC.want(oracle, c, size=True)
        assert sized[i] == (st, ck, n_out, used, 0), (c.name, sized[i])
        if got[i][0] == 0:  # a stream the sizing form sizes OK has the src_used the decode form reports
            assert sized[i][3] == got[i][3]
    _, res_b = a.fresh(32)
    batch.zlib_size_extent_blocks_batch(gpu_ctx, a.src, descs, res_b, n)
    assert _records(batch.extent_results_from_device(res_b)) == sized
    # the forms they mirror need the exact length: with src_len := src_used, identical status, checksum, out_len and bytes
    ok = [i for i in range(n) if got[i][0] == 0]
    sub = Arena([EC.Case(a.cases[i].name, a.cases[i].src[:got[i][3]], a.cases[i].cap, a.cases[i].limit, 0, True) for i in ok])
    d1, r1 = sub.fresh(16)
    batch.zlib_decompress_batch(gpu_ctx, sub.src, d1, sub.descs(), r1, len(ok), sub.max_cap)
    plain = batch.results_from_device(r1)
    o1 = sub.check_guards(d1, "zlib_decompress_batch")
    for k, i in enumerate(ok):
        assert (int(plain["status"][k]), int(plain["checksum"][k]), int(plain["out_len"][k])) == got[i][:3], a.cases[i].name
        assert o1[int(sub.dst_off[k]):int(sub.dst_off[k]) + got[i][2]].tobytes() == out[int(a.dst_off[i]):int(a.dst_off[i]) + got[i][2]].tobytes()
    _, r2 = sub.fresh(16)
    batch.zlib_size_batch(gpu_ctx, sub.src, sub.descs(), r2, len(ok))
    plain = batch.results_from_device(r2)
    assert [(int(plain["status"][k]), int(plain["out_len"][k])) for k in range(len(ok))] == [(0, got[i][2]) for i in ok]


def _long_cases():
    out, second = [], EC.long_streams()[1].raw
    for s in EC.long_streams():
        out.append(EC.Case(s.name + "/exact", s.raw, len(s.plain), None, 0, False))
        out.append(EC.Case(s.name + "/ff4096", s.raw + EC.trailing("ff", 4096, second), len(s.plain), None, 0, False))
    out.append(EC.Case("long/text0/second", EC.long_streams()[0].raw + second, EC.LONG, None, 0, False))
    out.append(EC.Case("long/text0/cut1", EC.long_streams()[0].raw[:-1], EC.LONG, None, 0, False))
    return out + [EC.by_name(n) for n in ("hand/three_kinds/ff5", "span/text48k/second4096", "refuse/far_distance", "refuse/bad_flag")]


def test_long_streams_by_their_one_wave_and_sized_by_blocks(gpu_ctx, oracle):
    """rooms of 512 KiB: zipc_hip_inflate_batch would go by blocks from 256 KiB on, the extent decode form never does; the
    blocks sizing form does, and says where the final block ended"""
    from zipc_amd import batch

    cases = _long_cases()
    a, n = Arena(cases), len(cases)
    descs = a.descs()
    dst, res = a.fresh(32)
    assert a.max_cap >= 512 << 10
    batch.inflate_extent_batch(gpu_ctx, a.src, dst, descs, res, n, a.max_cap, CRC_CRC32)
    assert gpu_ctx.last_inflate_blocks() == 0
    got = _records(batch.extent_results_from_device(res))
    out = a.check_guards(dst, "inflate_extent_batch, long")
    for i, c in enumerate(cases):
        st, _, n_out, used, data = EC.want(oracle, c)
        assert got[i] == (st, zlib.crc32(data) if st == 0 else 0, n_out, used, 0), (c.name, got[i], (st, n_out, used))
        assert out[int(a.dst_off[i]):int(a.dst_off[i]) + n_out].tobytes() == data, c.name
    assert got[0][3] == len(EC.long_streams()[0].raw) == got[4][3]
    dst2, res2 = a.fresh(16)
    batch.inflate_batch(gpu_ctx, a.src, dst2, descs, res2, n, a.max_cap, CRC_CRC32)
    assert gpu_ctx.last_inflate_blocks() > 0  # (the form it mirrors did go by blocks: the same results and bytes)
    plain = batch.results_from_device(res2)
    assert [(int(plain["status"][i]), int(plain["checksum"][i]), int(plain["out_len"][i])) for i in range(n)] == [g[:3] for g in got]
    out2 = a.check_guards(dst2, "inflate_batch, long")
    for i in range(n):  # (what a refused stream leaves in its room is nobody's promise: the block path and the wave differ there)
        o = int(a.dst_off[i])
        assert (out2[o:o + got[i][2]] == out[o:o + got[i][2]]).all(), cases[i].name
    # sizing
    _, r_wave = a.fresh(32)
    batch.inflate_size_extent_batch(gpu_ctx, a.src, descs, r_wave, n)
    assert gpu_ctx.last_size_blocks() == 0
    wave = _records(batch.extent_results_from_device(r_wave))
    for i, c in enumerate(cases):
        st, _, n_out, used, _ = EC.want(oracle, c, size=True)
        assert wave[i] == (st, 0, n_out, used, 0), (c.name, wave[i])
    _, r_blocks = a.fresh(32)
    batch.inflate_size_extent_blocks_batch(gpu_ctx, a.src, descs, r_blocks, n)
    assert gpu_ctx.last_size_blocks() > 0
    assert _records(batch.extent_results_from_device(r_blocks)) == wave
    _, r_plain = a.fresh(16)
    batch.inflate_size_blocks_batch(gpu_ctx, a.src, descs, r_plain, n)
    plain = batch.results_from_device(r_plain)
    assert [(int(plain["status"][i]), int(plain["out_len"][i])) for i in range(n)] == [(w[0], w[2]) for w in wave]
    # ... and the zlib blocks form over the long bodies wrapped
    zc = [EC.Case("zlib/" + c.name, EC.wrap(s.raw, s.plain) + tail, len(s.plain), None, 0, True)
          for s in EC.long_streams() for c, tail in ((s, b""), (s, b"\xff" * 7))]
    z = Arena(zc)
    _, rz = z.fresh(32)
    batch.zlib_size_extent_blocks_batch(gpu_ctx, z.src, z.descs(), rz, len(zc))
    assert gpu_ctx.last_size_blocks() > 0
    sized = _records(batch.extent_results_from_device(rz))
    for i, c in enumerate(zc):
        st, ck, n_out, used, _ = EC.want(oracle, c, size=True)
        assert sized[i] == (0, 0, EC.LONG, len(c.src) - (7 if i % 2 else 0), 0) == (st, ck, n_out, used, 0), (c.name, sized[i])


def test_a_stream_that_ends_on_the_arenas_last_byte(gpu_ctx, oracle):
    from zipc_amd import batch

    cases = [EC.by_name("basic/dynamic35/ff5"), EC.by_name("hand/stored_len65535/exact"), EC.by_name("hand/three_kinds/exact")]
    a = Arena(cases, exact_end=True)
    assert a.src.numel() == a.src_off[-1] + len(cases[-1].src)  # the arena holds nothing behind the last stream
    dst, res = a.fresh(32)
    batch.inflate_extent_batch(gpu_ctx, a.src, dst, a.descs(), res, len(cases), a.max_cap, CRC_ADLER32)
    got = _records(batch.extent_results_from_device(res))
    out = a.check_guards(dst, "arena edge")
    for i, c in enumerate(cases):
        st, _, n_out, used, data = EC.want(oracle, c)
        assert got[i] == (0, oracle.adler32(data), n_out, used, 0) and st == 0, (c.name, got[i])
        assert out[int(a.dst_off[i]):int(a.dst_off[i]) + n_out].tobytes() == data
    assert got[-1][3] == len(cases[-1].src)
    z = Arena([EC.by_name("zlib/hand/stored_len1/exact")], exact_end=True)
    dz, rz = z.fresh(32)
    batch.zlib_decompress_extent_batch(gpu_ctx, z.src, dz, z.descs(), rz, 1, z.max_cap)
    assert _records(batch.extent_results_from_device(rz))[0][::3] == (0, z.src.numel())


def test_argument_rules(gpu_ctx, raw_arena):
    from zipc_amd import _lib

    L, a = _lib.lib(), raw_arena
    descs = a.descs()
    dst, res = a.fresh(32)
    h, s, d, dd, r = gpu_ctx.handle, a.src.data_ptr(), dst.data_ptr(), descs.data_ptr(), res.data_ptr()
    assert L.zipc_hip_inflate_extent_batch(None, s, d, dd, r, 1, 64, 0) == 18
    assert L.zipc_hip_inflate_extent_batch(h, s, d, None, r, 1, 64, 0) == 18
    assert L.zipc_hip_inflate_extent_batch(h, s, d, dd, None, 1, 64, 0) == 18
    assert L.zipc_hip_inflate_extent_batch(h, s, d, dd, r, 0x80000000, 64, 0) == 18
    assert L.zipc_hip_inflate_extent_batch(h, s, d, dd, r, 1, 64, 4) == 18 and L.zipc_hip_inflate_extent_batch(h, s, d, dd, r, 1, 64, -1) == 18
    for fn in (L.zipc_hip_inflate_size_extent_batch, L.zipc_hip_zlib_size_extent_batch, L.zipc_hip_inflate_size_extent_blocks_batch,
               L.zipc_hip_zlib_size_extent_blocks_batch):
        assert fn(None, s, dd, r, 1) == 18 and fn(h, s, None, r, 1) == 18 and fn(h, s, dd, None, 1) == 18 and fn(h, s, dd, r, 0x80000000) == 18
        assert fn(h, s, dd, r, 0) == 0
    assert L.zipc_hip_zlib_decompress_extent_batch(None, s, d, dd, r, 1, 64) == 18 and L.zipc_hip_zlib_decompress_extent_batch(h, s, d, dd, r, 0, 64) == 0
    assert L.zipc_hip_inflate_extent_batch(h, s, d, dd, r, 0, 64, 0) == 0
    gpu_ctx.synchronize()
    assert (res.cpu().numpy() == 0xEE).all() and (dst.cpu().numpy() == RC.POISON).all()  # n_streams == 0 enqueues nothing


def test_the_host_forms_and_the_recipe(gpu_ctx, oracle):
    """zipc_hip_inflate_extent / zipc_hip_zlib_decompress_extent through the Python mirror: a sample of the catalogue, the
    ?start ?len range checks, and zlib streams stored back to back walked by bound, extent, next stream"""
    from zipc_amd import zipc_deflate as Z

    names = ["hand/empty_fixed/exact", "hand/stored_len0/ff5", "hand/stored_len1/second4096", "hand/fixed_then_stored/header4", "hand/three_kinds/zeros3",
             "basic/dynamic35/ff5", "span/text48k/ff3", "refuse/far_distance", "refuse/btype3", "refuse/empty_source"]
    for name in names:
        c = EC.by_name(name)
        st, _, n_out, used, data = EC.want(oracle, c)
        r = Z.inflate_extent(b"\x11\x22\x33" + c.src + b"\x44", start=3, len=len(c.src), ctx=gpu_ctx)
        assert (r.is_ok(), r.value if r.is_ok() else None) == (st == 0, (data, used) if st == 0 else None), name
        assert gpu_ctx.last_inflate_blocks() == 0
    for name in ("zlib/hand/stored_len1/ff5", "zlib/hand/empty_fixed/exact", "zlib/wrong_adler", "zlib/trailer_cut1", "zlib/src_len3", "zlib/header_method"):
        c = EC.by_name(name)
        st, _, n_out, used, data = EC.want(oracle, c)
        r = Z.zlib_decompress_extent(c.src, ctx=gpu_ctx)
        assert (r.is_ok(), r.value if r.is_ok() else None) == (st == 0, (data, used) if st == 0 else None), name
    with pytest.raises(ValueError):
        Z.inflate_extent(b"abc", start=2, len=2, ctx=gpu_ctx)
    # a git object: the inflated size is known, the compressed length is not -- decode with the room set to that size
    s = EC.basic()[333]
    r = Z.zlib_decompress_extent(EC.wrap(s.raw, s.plain) + b"the next object", decompressed_size=len(s.plain), ctx=gpu_ctx)
    assert r.value == (s.plain, len(s.raw) + 6)
    arena, plains = EC.back_to_back()
    at, got = 0, []
    while at < len(arena):
        data, used = Z.zlib_decompress_extent(arena, start=at, ctx=gpu_ctx).value
        got.append(data)
        at += used
    assert got == plains and at == len(arena)


def test_an_output_longer_than_max_dst_cap_with_crc32_is_refused_as_in_inflate_batch(gpu_ctx):
    """max_dst_cap sizes the CRC-32 pass: zipc_hip_inflate_batch reports INVALID_ARG for a stream whose output is longer (its
    checksum would cover only a part), and so must the extent form -- with no checksum, no length and no extent; every other
    stream of the call is untouched by it"""
    from zipc_amd import batch

    cases = _long_cases()
    a, n = Arena(cases), len(cases)
    descs = a.descs()
    dst, res = a.fresh(32)
    batch.inflate_extent_batch(gpu_ctx, a.src, dst, descs, res, n, 1000, CRC_CRC32)
    got = _records(batch.extent_results_from_device(res))
    a.check_guards(dst, "inflate_extent_batch, max_dst_cap 1000")
    dst2, res2 = a.fresh(16)
    batch.inflate_batch(gpu_ctx, a.src, dst2, descs, res2, n, 1000, CRC_CRC32)
    plain = batch.results_from_device(res2)
    full_dst, full_res = a.fresh(32)
    batch.inflate_extent_batch(gpu_ctx, a.src, full_dst, descs, full_res, n, a.max_cap, CRC_CRC32)
    full = _records(batch.extent_results_from_device(full_res))
    refused = 0
    for i, c in enumerate(cases):
        assert got[i][:2] == (int(plain["status"][i]), int(plain["checksum"][i])), (c.name, got[i])
        if full[i][0] == 0 and int(plain["status"][i]) == 18:
            assert got[i] == (18, 0, 0, 0, 0), (c.name, got[i])
            refused += 1
        else:
            assert got[i] == full[i] and got[i][2] == int(plain["out_len"][i]), (c.name, got[i], full[i])
    assert refused >= 5 and any(g[0] == 0 for g in got), got  # (the 512 KiB streams; the short one keeps its CRC-32)
    # the other checksums are not sized by max_dst_cap: nothing is refused
    for op in (CRC_NOP, CRC_ADLER32):
        dst3, res3 = a.fresh(32)
        batch.inflate_extent_batch(gpu_ctx, a.src, dst3, descs, res3, n, 1000, op)
        assert [g[0] for g in _records(batch.extent_results_from_device(res3))] == [f[0] for f in full]


def test_a_length_above_the_longest_stream_is_the_streams_own_invalid_argument(gpu_ctx):
    """src_len or dst_cap above ZIPC_HIP_MAX_STREAM_LEN: INVALID_ARG in the stream's own 32-byte record, every other field 0,
    as the form each mirrors reports it; the streams beside it are untouched"""
    import torch

    from zipc_amd import batch

    names = ("hand/three_kinds/ff5", "basic/dynamic35/ff5", "hand/stored_len1/exact", "hand/fixed_then_stored/zeros3")
    a = Arena([EC.by_name(nm) for nm in names])
    z = Arena([EC.by_name("zlib/" + nm) for nm in ("hand/three_kinds/ff5", "hand/stored_len1/exact", "hand/empty_fixed/exact")])
    n, dev = len(names), a.dev

    def lying(arena, field, value):
        d = batch.make_descs(np.array(arena.src_off, np.uint64), arena.src_len, arena.dst_off, arena.caps)
        d[field][0] = value
        return batch.to_device(d, dev)

    def call(arena, fn, width, descs, *more):
        dst, res = arena.fresh(width)
        args = (gpu_ctx, arena.src, dst, descs, res, len(arena.cases)) if more else (gpu_ctx, arena.src, descs, res, len(arena.cases))
        fn(*args, *more)
        arena.check_guards(dst, fn.__name__)
        return (batch.extent_results_from_device(res) if width == 32 else batch.results_from_device(res)), dst

    honest, _ = call(a, batch.inflate_extent_batch, 32, a.descs(), a.max_cap, CRC_CRC32)
    assert (honest["status"] == 0).all()
    for field, too_long in (("src_len", 1 << 32), ("dst_cap", 1 << 32), ("src_len", 0xFFFF0001), ("dst_cap", 0xFFFF0001)):
        d = lying(a, field, too_long)
        got, dst = call(a, batch.inflate_extent_batch, 32, d, a.max_cap, CRC_CRC32)
        plain, dst2 = call(a, batch.inflate_batch, 16, d, a.max_cap, CRC_CRC32)
        assert _records(got)[0] == (18, 0, 0, 0, 0) and int(plain["status"][0]) == 18 and int(plain["out_len"][0]) == 0, (field, _records(got)[0])
        assert _records(got)[1:] == _records(honest)[1:] and torch.equal(dst, dst2), field
        if field == "src_len":  # (the sizing forms do not look at dst_cap)
            for fn, mirror in ((batch.inflate_size_extent_batch, batch.inflate_size_batch),
                               (batch.inflate_size_extent_blocks_batch, batch.inflate_size_blocks_batch)):
                sized, _ = call(a, fn, 32, d)
                plain, _ = call(a, mirror, 16, d)
                assert _records(sized)[0] == (18, 0, 0, 0, 0) and int(plain["status"][0]) == 18, (fn.__name__, _records(sized)[0])
                assert [(r[0], r[2], r[3]) for r in _records(sized)[1:]] == [(r[0], r[2], r[3]) for r in _records(honest)[1:]]
        else:  # the zlib decode form: the room of the body is the stream's
            zh, _ = call(z, batch.zlib_decompress_extent_batch, 32, z.descs(), z.max_cap)
            zg, _ = call(z, batch.zlib_decompress_extent_batch, 32, lying(z, field, too_long), z.max_cap)
            assert _records(zg)[0] == (18, 0, 0, 0, 0) and _records(zg)[1:] == _records(zh)[1:] and (zh["status"] == 0).all()


def test_the_cpp_mirror(gpu_ctx, tmp_path):
    """inflate_extent and zlib_decompress_extent of zipc_amd/host/zipc_deflate.hpp from a C++ caller (a program of its own,
    linked against libzipc_host.so): the recipe's walk over zlib streams stored back to back, the raw form over a
    sub-range, and the start / len range checks"""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "zipc_amd", "lib")
    exe = str(tmp_path / "host_mirror")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(root, "tests", "extent_sim", "host_mirror_main.cpp"), "-L" + lib,
                    "-lzipc_host", "-lzipc_hip", "-Wl,-rpath," + lib], check=True)
    arena, plains = EC.back_to_back()
    (tmp_path / "arena.bin").write_bytes(arena)
    r = subprocess.run([exe, str(tmp_path / "arena.bin"), str(tmp_path / "plain.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, (r.stdout.decode()[-500:], r.stderr.decode()[-1500:])
    lines = r.stdout.decode().split("\n")
    first = EC.extent_by_zlib(arena, wrapped=True)
    want, at = [], 0
    for p in plains:
        used = EC.extent_by_zlib(arena[at:], wrapped=True)
        want.append("zlib %d %d" % (used, len(p)))
        at += used
    assert lines[:len(plains) + 3] == want + ["raw %d %d" % (first - 6, len(plains[0])), "range 2", "bad 0"], lines
    assert (tmp_path / "plain.bin").read_bytes() == b"".join(plains)
