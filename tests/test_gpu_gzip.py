"""The gzip forms on the MI355X (include/zipc_hip.h at zipc_hip_gzip_decompress_batch).  The whole catalogue
(tests/gzip_cases.py) in ONE arena through the decode form, the size form and the size-by-blocks form: the sources side by
side at every alignment 0 .. 7 of src_off, each followed by what the case says lies behind it, every room between 64 guard
bytes of 0xA5 in a poisoned destination arena, results that start as 0xEE, and the arena allocated so that it ends on the
last byte of a case.  Records and bytes are the catalogue's (the oracle's body, zlib's extent and CRC-32).  Then

  - the two defining properties, against zipc_hip_inflate_batch and zipc_hip_deflate_batch on the same device;
  - compress: every source at every level in both flavours, one call per level and flavour -- header + the oracle's deflate +
    trailer, read back by Python's gzip; rooms of overhead - 1 and of bound - 1 bytes;
  - the argument rules;
  - the host forms over every file of the catalogue, a BGZF run in one decode launch, and the C++ mirror."""
import ctypes as C
import gzip
import os
import subprocess
import zlib

import numpy as np
import pytest

import gzip_cases as GC
import inflate_room_cases as RC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("status", "checksum", "out_len", "src_used", "hdr_len", "flg")
MAX_STREAM_LEN = 0xFFFF0000


class Arena:
    """the cases' sources side by side in a source arena that ends on the last case's last byte, their rooms between guards
    in a poisoned destination arena"""

    def __init__(self, cases):
        import torch

        assert not cases[-1].behind
        self.cases, self.dev = cases, torch.device("cuda", 0)
        parts, self.src_off, pos = [], [], 0
        for i, c in enumerate(cases):
            pad = (i % 8 - pos) % 8
            parts.append(b"\x5a" * pad)
            pos += pad
            self.src_off.append(pos)
            parts.append(c.src + c.behind)
            pos += len(c.src) + len(c.behind)
        self.src = torch.from_numpy(np.frombuffer(b"".join(parts), dtype=np.uint8).copy()).to(self.dev)
        self.src_clone = self.src.clone()
        self.src_len = [len(c.src) for c in cases]
        self.caps = [c.cap for c in cases]
        self.dst_off, self.total, self.guards = RC.layout(self.caps, [RC.OFF_MODS[i % 4] for i in range(len(cases))])
        self.max_cap = max(self.caps)

    def fresh(self, width=32):
        import torch

        return (torch.full((self.total,), RC.POISON, dtype=torch.uint8, device=self.dev),
                torch.full((len(self.cases) * width,), 0xEE, dtype=torch.uint8, device=self.dev))

    def descs(self):
        from zipc_amd import batch

        d = batch.make_descs(np.array(self.src_off, np.uint64), self.src_len, self.dst_off, self.caps)
        for i, c in enumerate(self.cases):
            d["flags"][i] = c.flags | (1 if c.limit is not None else 0)
            d["limit"][i] = c.limit or 0
        return d

    def check_guards(self, dst, form):
        out = dst.cpu().numpy()
        for i, c in enumerate(self.cases):
            assert (out[self.guards[i][0]] == RC.POISON).all() and (out[self.guards[i][1]] == RC.POISON).all(), (form, c.name, "wrote outside its room")
        return out


def records(res):
    return [tuple(int(res[f][i]) for f in FIELDS) for i in range(len(res))]


@pytest.fixture(scope="module")
def arena():
    cases = list(GC.flag_cases() + GC.other_cases() + GC.cut_cases())
    assert cases[-1].name.startswith("cut/31/") and not cases[-1].behind  # the arena ends on the last byte of a truncated member
    return Arena(cases)


@pytest.fixture(scope="module")
def wants(oracle):
    return {c.name: (GC.want(oracle, c), GC.want(oracle, c, size=True)) for c in GC.cases()}


@pytest.fixture(scope="module")
def decoded(gpu_ctx, arena):
    """the catalogue through the decode form, once: (records, the destination arena, the device tensors)"""
    from zipc_amd import batch

    a = arena
    dst, res = a.fresh()
    batch.gzip_decompress_batch(gpu_ctx, a.src, dst, batch.to_device(a.descs(), a.dev), res, len(a.cases), a.max_cap)
    blocks = gpu_ctx.last_inflate_blocks()
    return records(batch.gzip_results_from_device(res)), a.check_guards(dst, "gzip_decompress_batch"), dst, blocks


def test_the_catalogue_through_the_decode_form(gpu_ctx, arena, wants, decoded):
    import torch

    a = arena
    got, out, _, blocks = decoded
    assert blocks == 0  # always a wave per member, whatever max_dst_cap
    assert torch.equal(a.src, a.src_clone)
    n_ok = 0
    for i, c in enumerate(a.cases):
        w = wants[c.name][0]
        assert got[i] == tuple(w[:6]), (c.name, got[i], tuple(w[:6]))
        assert got[i][3] <= len(c.src)
        o = int(a.dst_off[i])
        assert out[o:o + w.out_len].tobytes() == w.data, (c.name, "bytes")
        n_ok += w.status == 0
    assert n_ok >= 45  # (the 32 flag members, and the OK members among the others)


def test_the_catalogue_through_the_two_sizing_forms(gpu_ctx, arena, wants, decoded):
    from zipc_amd import batch

    a, n = arena, len(arena.cases)
    descs = batch.to_device(a.descs(), a.dev)
    _, res = a.fresh()
    batch.gzip_size_batch(gpu_ctx, a.src, descs, res, n)
    assert gpu_ctx.last_size_blocks() == 0
    sized = records(batch.gzip_results_from_device(res))
    for i, c in enumerate(a.cases):
        w = wants[c.name][1]
        assert sized[i] == tuple(w[:6]), (c.name, sized[i], tuple(w[:6]))
        if decoded[0][i][0] == 0:  # a member the sizing form sizes OK has the src_used the decode form reports
            assert sized[i][2:] == decoded[0][i][2:]
    _, res_b = a.fresh()
    batch.gzip_size_blocks_batch(gpu_ctx, a.src, descs, res_b, n)
    assert gpu_ctx.last_size_blocks() > 0  # the call holds the 300 KiB member
    assert records(batch.gzip_results_from_device(res_b)) == sized


def test_an_ok_member_is_inflate_batch_over_its_body(gpu_ctx, arena, decoded):
    """the first defining property: zipc_hip_inflate_batch over [src_off + hdr_len, src_off + src_used - 8) with CRC-32 gives
    the same bytes, length and checksum, the member's whole room compared"""
    from zipc_amd import batch

    a, n = arena, len(arena.cases)
    got, out, _, _ = decoded
    d = a.descs()
    for i, g in enumerate(got):
        if g[0] == 0:
            d["src_off"][i] += g[4]
            d["src_len"][i] = g[3] - g[4] - 8
        else:
            d["src_len"][i] = 0
            d["dst_cap"][i] = 0
            d["flags"][i] = 0
    dst2, res2 = a.fresh(16)
    batch.inflate_batch(gpu_ctx, a.src, dst2, batch.to_device(d, a.dev), res2, n, a.max_cap, 1)
    plain = batch.results_from_device(res2)
    out2 = a.check_guards(dst2, "inflate_batch")
    for i, g in enumerate(got):
        if g[0] == 0:
            assert (int(plain["status"][i]), int(plain["checksum"][i]), int(plain["out_len"][i])) == g[:3], a.cases[i].name
            o = int(a.dst_off[i])
            assert (out[o:o + a.caps[i]] == out2[o:o + a.caps[i]]).all(), a.cases[i].name


@pytest.fixture(scope="module")
def compress_arena():
    import torch

    dev = torch.device("cuda", 0)
    srcs = GC.sources()
    offs, pos = [], 0
    for _, data in srcs:
        offs.append(pos)
        pos += len(data) + 3
    blob = b"".join(data + b"\x5a" * 3 for _, data in srcs)
    return dev, srcs, offs, torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(dev)


@pytest.mark.parametrize("flavour", GC.FLAVOURS)
@pytest.mark.parametrize("level", GC.LEVELS)
def test_compress_is_header_deflate_trailer(gpu_ctx, oracle, compress_arena, level, flavour):
    import torch

    from zipc_amd import batch

    dev, srcs, offs, src = compress_arena
    lens = [len(d) for _, d in srcs]
    # every source three times: a room of the bound, of the bound - 1, of the overhead - 1
    caps = [batch.gzip_bound(n, flavour) for n in lens] + [batch.gzip_bound(n, flavour) - 1 for n in lens] + [GC.overhead(flavour) - 1] * len(lens)
    k = len(caps)
    dst_off, total, guards = RC.layout(caps, [RC.OFF_MODS[i % 4] for i in range(k)])
    descs = batch.make_descs(np.array(offs * 3, np.uint64), lens * 3, dst_off, caps)
    dst = torch.full((total,), RC.POISON, dtype=torch.uint8, device=dev)
    res = torch.full((k * 16,), 0xEE, dtype=torch.uint8, device=dev)
    batch.gzip_compress_batch(gpu_ctx, src, dst, batch.to_device(descs, dev), res, k, max(lens), sum(lens) * 3, level, flavour)
    got, out = batch.results_from_device(res), dst.cpu().numpy()
    # the second defining property's yardstick: zipc_hip_deflate_batch over the same sources, rooms of the bound
    dcaps = [batch.deflate_bound(n) for n in lens]
    d_off, d_total, _ = RC.layout(dcaps, [0] * len(lens))
    ddst = torch.zeros((d_total,), dtype=torch.uint8, device=dev)
    dres = torch.zeros((len(lens) * 16,), dtype=torch.uint8, device=dev)
    batch.deflate_batch(gpu_ctx, src, ddst, batch.to_device(batch.make_descs(np.array(offs, np.uint64), lens, d_off, dcaps), dev), dres, len(lens),
                        max(lens), sum(lens), level, 1)
    raw, rout = batch.results_from_device(dres), ddst.cpu().numpy()
    hdr = 18 if flavour == GC.BGZF else 10
    for i in range(k):
        name, data = srcs[i % len(lens)]
        st, crc, member = GC.compress_want(name, level, flavour, caps[i])
        assert (int(got["status"][i]), int(got["checksum"][i]), int(got["out_len"][i])) == (st, crc, len(member)), (name, level, flavour, caps[i])
        assert (out[guards[i][0]] == RC.POISON).all() and (out[guards[i][1]] == RC.POISON).all(), (name, "wrote outside its room")
        if st:
            continue
        o = int(dst_off[i])
        mine = out[o:o + len(member)].tobytes()
        assert mine == member, (name, level, flavour, "bytes")
        assert gzip.decompress(mine) == data
        j = i % len(lens)
        assert int(raw["status"][j]) == 0 and mine[hdr:-8] == rout[int(d_off[j]):int(d_off[j]) + int(raw["out_len"][j])].tobytes(), (name, "deflate_batch's bytes")
        assert mine[-8:-4] == int(raw["checksum"][j]).to_bytes(4, "little")
    if flavour == GC.PLAIN:  # the bound always suffices
        assert (got["status"][:len(lens)] == 0).all()


def test_argument_rules(gpu_ctx, arena):
    import torch

    from zipc_amd import _lib, batch

    L, h, a = _lib.lib(), gpu_ctx.handle, arena
    n = 4
    d = a.descs()[:n].copy()
    descs = batch.to_device(d, a.dev)
    dst, _ = a.fresh()
    res = torch.full((n * 32,), 0xEE, dtype=torch.uint8, device=a.dev)
    sp, dp, qp, rp = a.src.data_ptr(), dst.data_ptr(), descs.data_ptr(), res.data_ptr()
    INVALID = _lib.ERR_INVALID_ARG
    # nulls
    assert L.zipc_hip_gzip_decompress_batch(None, sp, dp, qp, rp, n, a.max_cap) == INVALID
    assert L.zipc_hip_gzip_decompress_batch(h, sp, dp, None, rp, n, a.max_cap) == INVALID
    assert L.zipc_hip_gzip_decompress_batch(h, sp, dp, qp, None, n, a.max_cap) == INVALID
    assert L.zipc_hip_gzip_size_batch(h, sp, None, rp, n) == INVALID and L.zipc_hip_gzip_size_batch(h, sp, qp, None, n) == INVALID
    assert L.zipc_hip_gzip_size_blocks_batch(h, sp, None, rp, n) == INVALID and L.zipc_hip_gzip_size_blocks_batch(None, sp, qp, rp, n) == INVALID
    assert L.zipc_hip_gzip_compress_batch(h, sp, dp, None, rp, n, 100, 400, 2, 0) == INVALID
    assert L.zipc_hip_gzip_compress_batch(h, sp, dp, qp, None, n, 100, 400, 2, 0) == INVALID
    for fn in (lambda k: L.zipc_hip_gzip_decompress_batch(h, sp, dp, qp, rp, k, a.max_cap), lambda k: L.zipc_hip_gzip_size_batch(h, sp, qp, rp, k),
               lambda k: L.zipc_hip_gzip_size_blocks_batch(h, sp, qp, rp, k), lambda k: L.zipc_hip_gzip_compress_batch(h, sp, dp, qp, rp, k, 100, 400, 2, 0)):
        assert fn(0x80000000) == INVALID
        assert fn(0) == 0  # ... and nothing is enqueued: the poisoned results stay
    # level, flavour and the longest source out of range
    for level, flavour, max_len in ((-1, 0, 100), (4, 0, 100), (2, -1, 100), (2, 2, 100), (2, 0, MAX_STREAM_LEN + 1)):
        assert L.zipc_hip_gzip_compress_batch(h, sp, dp, qp, rp, n, max_len, 400, level, flavour) == INVALID
    gpu_ctx.synchronize()
    assert (res.cpu().numpy() == 0xEE).all() and (dst.cpu().numpy() == RC.POISON).all()
    # in a member's own result: a flag bit, a length above ZIPC_HIP_MAX_STREAM_LEN (nothing of it is read), an output longer than max_dst_cap
    # (the pass behind the decode kernel sums max_dst_cap's segments of 32 KiB, as in zipc_hip_inflate_batch: the member of
    # 65 280 bytes is longer than a max_dst_cap of 32 KiB covers)
    d[3] = a.descs()[[c.name for c in a.cases].index("body/bgzf65280")]
    d["flags"][1] = 4
    d["src_len"][2] = MAX_STREAM_LEN + 1
    batch.gzip_decompress_batch(gpu_ctx, a.src, dst, batch.to_device(d, a.dev), res, n, 32768)
    got = records(batch.gzip_results_from_device(res))
    assert [g[0] for g in got] == [0, INVALID, INVALID, INVALID] and all(g[1:] == (0, 0, 0, 0, 0) for g in got[1:]), got
    batch.gzip_decompress_batch(gpu_ctx, a.src, dst, batch.to_device(d, a.dev), res, n, 65280)
    assert [g[0] for g in records(batch.gzip_results_from_device(res))] == [0, INVALID, INVALID, 0]
    batch.gzip_size_batch(gpu_ctx, a.src, batch.to_device(d, a.dev), res, n)
    assert [g[0] for g in records(batch.gzip_results_from_device(res))] == [0, INVALID, INVALID, 0]
    cres = torch.full((n * 16,), 0xEE, dtype=torch.uint8, device=a.dev)
    d["src_len"][2] = 10
    batch.gzip_compress_batch(gpu_ctx, a.src, dst, batch.to_device(d, a.dev), cres, n, 400, 1600, 2, 0)
    assert int(batch.results_from_device(cres)["status"][1]) == INVALID


# ---- the host forms -------------------------------------------------------------------------------------------------

def host_size(ctx, data):
    from zipc_amd import _lib

    n, used, members = C.c_size_t(77), C.c_size_t(77), C.c_size_t(77)
    st = _lib.lib().zipc_hip_gzip_size(ctx.handle, data, len(data), C.byref(n), C.byref(used), C.byref(members))
    return st, n.value, used.value, members.value


def host_decompress(ctx, data, cap):
    from zipc_amd import _lib

    dst = C.create_string_buffer(cap + 64)
    C.memset(dst, 0xA5, cap + 64)
    n, used, members, found = C.c_size_t(77), C.c_size_t(77), C.c_size_t(77), C.c_uint32(77)
    st = _lib.lib().zipc_hip_gzip_decompress(ctx.handle, data, len(data), dst, cap, C.byref(n), C.byref(used), C.byref(members), C.byref(found))
    assert dst.raw[cap:] == b"\xa5" * 64, "wrote behind the room"
    return st, dst.raw[:n.value], used.value, members.value, found.value


@pytest.mark.parametrize("name", [f.name for f in GC.files()])
def test_host_forms_over_the_files(gpu_ctx, name):
    f = GC.file_by_name(name)
    true_len = len(f.plain) if f.status == 0 else 8 << 20
    sized = host_size(gpu_ctx, f.data)
    if f.status == 0:
        assert sized == (0, len(f.plain), f.src_used, f.members)
    else:
        # (the sizing form compares no CRC-32: the file with a wrong one is sized OK)
        assert sized[0] == (0 if f.status == GC.CHECKSUM else f.status) and (sized[0] == 0 or sized[1:3] == (0, 0)), sized
    gpu_ctx.set_profiling(True)
    gpu_ctx.reset_kernel_times()
    got = host_decompress(gpu_ctx, f.data, true_len)
    times = gpu_ctx.kernel_times()
    gpu_ctx.set_profiling(False)
    if f.status == 0:
        assert got == (0, f.plain, f.src_used, f.members, 0)
        # a run of members of known length is ONE decode launch, not one per member
        assert times.get("inflate_extent", (0, 0))[0] == f.runs, (name, times)
        if f.plain:
            assert host_decompress(gpu_ctx, f.data, len(f.plain) - 1)[:3] == (16, b"", 0)
    else:
        assert got == (f.status, b"", 0, 0, f.found), got[:1] + got[2:]


def test_host_compress_round_trip_and_the_python_mirror(gpu_ctx, oracle):
    from zipc_amd import _lib, zipc_deflate as Z

    L = _lib.lib()
    for name, data in GC.sources()[:12]:
        for flavour in GC.FLAVOURS:
            cap = L.zipc_hip_gzip_bound(len(data), flavour)
            dst, n = C.create_string_buffer(cap), C.c_size_t()
            st = L.zipc_hip_gzip_compress(gpu_ctx.handle, data, len(data), 2, flavour, dst, cap, C.byref(n))
            want = GC.compress_want(name, 2, flavour, cap)
            assert (st, dst.raw[:n.value]) == (want[0], want[2]), (name, flavour)
            if st == 0:
                assert host_decompress(gpu_ctx, dst.raw[:n.value] + b"tail", len(data)) == (0, data, n.value, 1, 0)
    text = dict(GC.sources())["text200000"]
    m = Z.gzip_compress(text, level="fast").get_ok()
    assert gzip.decompress(m) == text and m[:10] == gzip.compress(b"x", 1, mtime=0)[:10]
    parts = [Z.gzip_compress(text, bgzf=True, start=at, len=min(65280, len(text) - at)).get_ok() for at in range(0, len(text), 65280)]
    whole = m + b"".join(parts) + GC.BGZF_EOF
    assert gzip.decompress(whole) == text + text
    assert Z.gzip_size(whole).get_ok() == (2 * len(text), len(whole), len(parts) + 2)
    assert Z.gzip_decompress(whole + b"garbage").get_ok() == (text + text, len(whole), len(parts) + 2)
    assert Z.gzip_compress(bytes(range(256)) * 300, level="none", bgzf=True).is_error()
    bad = bytearray(whole)
    bad[len(m) - 8] ^= 1
    e = Z.gzip_decompress(bytes(bad))
    assert e.is_error() and e.error[0] == zlib.crc32(text)
    assert Z.gzip_decompress(b"\x1f\x8b\x07" + whole[3:]).error == (None, "Unknown compression method (7)")
    assert Z.gzip_size(b"").is_error()


def test_cpp_mirror(tmp_path):
    lib = os.path.join(ROOT, "zipc_amd", "lib")
    exe = str(tmp_path / "gzip_mirror")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "gzip_sim", "host_mirror_main.cpp"), "-L" + lib,
                    "-lzipc_host", "-lzipc_hip", "-Wl,-rpath," + lib], check=True)
    f = GC.file_by_name("plain_then_bgzf_then_plain")
    (tmp_path / "file.gz").write_bytes(f.data)
    r = subprocess.run([exe, str(tmp_path / "file.gz"), str(tmp_path / "plain.bin"), str(tmp_path / "made.gz")], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, (r.stdout.decode()[-500:], r.stderr.decode()[-1500:])
    n_bgzf = (len(f.plain) - 1000 + 65279) // 65280
    assert r.stdout.decode().split("\n")[:6] == ["size %d %d %d" % (len(f.plain), f.src_used, f.members),
                                                 "decompress %d %d %d" % (len(f.plain), f.src_used, f.members),
                                                 "again 1 1 %d %d" % (n_bgzf + 2, n_bgzf + 2), "too_big 0", "wrong 0 1", "range 2"], r.stdout.decode()
    assert (tmp_path / "plain.bin").read_bytes() == f.plain
    assert gzip.decompress((tmp_path / "made.gz").read_bytes()) == f.plain
