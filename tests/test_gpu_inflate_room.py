"""Inflate's room on the MI355X: nothing is written in front of dst_off or behind dst_off + dst_cap, whatever the status
(include/zipc_hip.h at zipc_hip_inflate_batch).  Every item of tests/inflate_room_cases.py -- a stream, a room R around
one of its writes, one of the four ways to declare it, a dst_off of 0, 1, 5 or 15 mod 16 -- through every form inflate
has, its room between 64 guard bytes of 0xA5 on either side:

  batch_few      zipc_hip_inflate_batch, calls of 256 streams and less (inflate_batch_few_kernel)
  batch_many     the same items in calls of more than 256 (inflate_batch_kernel)
  by_blocks      the two long streams by a wave per block: alone, all their rooms in one call, among 40 short streams
  one_stream     zipc_hip_inflate, a call per item;  inflate_many: zipc_hip_inflate_many -- poisoned host buffers
  zlib_batch     zipc_hip_zlib_decompress_batch over the same bodies in the six container bytes
  recode_batch   zipc_hip_recode_batch with mid_cap = the room: the guards stand around the middle room
  one_wave       batch_few, batch_many and by_blocks again in a child process with ZIPC_HIP_INFLATE_BLOCKS=0

Where R >= N: status 0, out_len N, the plain bytes, the oracle's checksum.  Where R < N: the status of the item's
declaration and out_len 0; what lies inside the room is not looked at.  Always: both guards intact, results that
started as 0xEE, and a source arena that equals its clone.  No item is left out of any form.

wave_copy_match, the stored-block copy and the block path's stores have no host model: this file is their coverage."""
import ctypes as C
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import inflate_room_cases as RC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE_WAVE = os.environ.get("ZIPC_HIP_INFLATE_BLOCKS") == "0"
SHORT_FAMILIES = RC.SIM_FAMILIES  # every family but by_blocks: no room of theirs reaches 256 KiB
_SUMS = {}


def _sums(oracle, s):
    """(0, CRC-32, the reference's Adler-32) of a stream's plain bytes: by crc_op"""
    key = (s.family, s.name)
    if key not in _SUMS:
        crc = oracle.crc32(s.plain)
        assert crc == zlib.crc32(s.plain)
        _SUMS[key] = (0, crc, oracle.adler32(s.plain))
    return _SUMS[key]


def _check(oracle, form, its, status, out_len, checksum, room_bytes, guards, crc_op):
    """per item: the result, the bytes of a stream that fits, the guards.  room_bytes(i, n) -> the room's first n bytes;
    guards(i) -> (front, back) as arrays; crc_op: what checksum[] holds (None: not looked at), or a function of the item"""
    for i, it in enumerate(its):
        s = RC.stream_of(it)
        n, ident = len(s.plain), (form, RC.item_id(it), "dst_off mod 16 = %d" % it.off_mod)
        assert int(status[i]) == it.want, ident + ("status", int(status[i]), it.want)
        if it.want == 0:
            assert int(out_len[i]) == n, ident + ("out_len", int(out_len[i]), n)
            got = room_bytes(i, n)
            assert got == s.plain, ident + ("bytes", next(k for k in range(n) if got[k] != s.plain[k]))
            if crc_op is not None:
                op = crc_op(it) if callable(crc_op) else crc_op
                assert int(checksum[i]) == _sums(oracle, s)[op], ident + ("checksum", op, hex(int(checksum[i])))
        else:
            assert int(out_len[i]) == 0, ident + ("out_len of a stream that does not fit", int(out_len[i]))
        front, back = guards(i)
        assert (front == RC.POISON).all(), ident + ("wrote in front of its room",)
        assert (back == RC.POISON).all(), ident + ("wrote %d bytes behind its room" % (int(np.flatnonzero(back != RC.POISON).max()) + 1),)


class Arena:
    """the items' streams once each in a source arena, their rooms between guards in a poisoned destination arena"""

    def __init__(self, its, wrap=None):
        import torch

        self.its, self.dev = its, torch.device("cuda", 0)
        at, parts, self.src_off, self.src_len = {}, [], [], []
        pos = 0
        for it in its:
            key = (it.family, it.stream)
            if key not in at:
                raw = RC.stream_of(it).raw if wrap is None else wrap(RC.stream_of(it))
                at[key] = (pos, len(raw))
                parts.append(raw)
                pos += len(raw)
            self.src_off.append(at[key][0])
            self.src_len.append(at[key][1])
        self.src = torch.from_numpy(np.frombuffer(b"".join(parts) + b"\0" * 64, dtype=np.uint8).copy()).to(self.dev)
        self.src_clone = self.src.clone()
        self.caps = [it.cap for it in its]
        self.dst_off, total, self.guards = RC.layout(self.caps, [it.off_mod for it in its])
        self.dst = torch.full((total,), RC.POISON, dtype=torch.uint8, device=self.dev)

    def descs(self):
        from zipc_amd import batch

        d = batch.make_descs(np.array(self.src_off, np.uint64), self.src_len, self.dst_off, self.caps)
        for i, it in enumerate(self.its):
            if it.limit is not None:
                d["limit"][i] = it.limit
                d["flags"][i] = 1
        return d

    def results(self, record):
        import torch

        return torch.full((len(self.its) * record,), 0xEE, dtype=torch.uint8, device=self.dev)

    def check(self, oracle, form, res, crc_op, out=None):
        import torch

        out = self.dst.cpu().numpy() if out is None else out
        assert torch.equal(self.src, self.src_clone), (form, "the source arena was written")
        offs = [int(o) for o in self.dst_off]
        _check(oracle, form, self.its, res["status"], res["out_len"], res["checksum"],
               lambda i, n: out[offs[i]:offs[i] + n].tobytes(), lambda i: (out[self.guards[i][0]], out[self.guards[i][1]]), crc_op)


def _inflate_batch(ctx, oracle, its, crc_op, form):
    """one zipc_hip_inflate_batch over the items (all of one crc_op)"""
    from zipc_amd import batch

    assert all(it.crc_op == crc_op for it in its)
    a = Arena(its)
    d_res = a.results(16)
    batch.inflate_batch(ctx, a.src, a.dst, batch.to_device(a.descs(), a.dev), d_res, len(its), max(a.caps), crc_op)
    a.check(oracle, "%s n=%d crc_op=%d" % (form, len(its), crc_op), batch.results_from_device(d_res), crc_op)


def _by_crc_op(its):
    return [(op, [it for it in its if it.crc_op == op]) for op in RC.CRC_OPS]


@pytest.mark.parametrize("family", SHORT_FAMILIES)
def test_batch_few(gpu_ctx, oracle, family):
    for op, its in _by_crc_op(RC.items(family)):
        for k in range(0, len(its), 256):
            _inflate_batch(gpu_ctx, oracle, its[k:k + 256], op, "inflate_batch few")


@pytest.mark.parametrize("family", SHORT_FAMILIES)
def test_batch_many(gpu_ctx, oracle, family):
    for op, its in _by_crc_op(RC.items(family)):
        its = its * (256 // len(its) + 1)  # (a short family: its items again, each in a room of its own)
        assert len(its) > 256
        _inflate_batch(gpu_ctx, oracle, its, op, "inflate_batch many")


def test_by_blocks(gpu_ctx, oracle):
    its = RC.items("by_blocks")
    for it in its:  # alone: a call per room that holds the stream
        if it.want == 0:
            _inflate_batch(gpu_ctx, oracle, [it], it.crc_op, "inflate_batch by blocks, alone")
            assert ONE_WAVE or gpu_ctx.last_inflate_blocks() >= 2, (RC.item_id(it), gpu_ctx.last_inflate_blocks())
    for op, group in _by_crc_op(its):  # every room; then among 40 short streams
        assert any(it.want == 0 for it in group) and any(it.want != 0 for it in group)
        _inflate_batch(gpu_ctx, oracle, group, op, "inflate_batch by blocks")
        assert ONE_WAVE or gpu_ctx.last_inflate_blocks() >= 2, (op, gpu_ctx.last_inflate_blocks())
        short = [it for f in ("lane", "stored", "run_short", "literal_last") for it in RC.items(f) if it.crc_op == op][::37][:40]
        assert len(short) == 40
        mixed = [x for pair in zip(short, group) for x in pair] + group[40:] + short[len(group):]
        _inflate_batch(gpu_ctx, oracle, mixed, op, "inflate_batch by blocks among short streams")
        assert ONE_WAVE or gpu_ctx.last_inflate_blocks() >= 2, (op, gpu_ctx.last_inflate_blocks())


def _host_rooms(its):
    """a poisoned host buffer per item: GUARD bytes, the room at its dst_off mod 16, GUARD bytes"""
    bufs, offs = [], []
    for it in its:
        b = np.full(RC.GUARD + 16 + it.cap + RC.GUARD, RC.POISON, np.uint8)
        o = RC.GUARD + (it.off_mod - (b.ctypes.data + RC.GUARD)) % 16
        bufs.append(b)
        offs.append(o)
    return bufs, offs


@pytest.mark.parametrize("family", list(RC.FAMILIES))
def test_one_stream_calls(gpu_ctx, oracle, family):
    from zipc_amd._lib import lib

    L, its = lib(), RC.items(family)
    bufs, offs = _host_rooms(its)
    status, out_len, checksum = [], [], []
    for it, b, o in zip(its, bufs, offs):
        s = RC.stream_of(it)
        ol, ck = C.c_size_t(0xEEEEEEEE), C.c_uint32(0xEEEEEEEE)
        status.append(L.zipc_hip_inflate(gpu_ctx.handle, s.raw, len(s.raw), int(it.limit is not None), it.limit or 0, it.crc_op,
                                         b.ctypes.data + o, it.cap, C.byref(ol), C.byref(ck)))
        out_len.append(ol.value)
        checksum.append(ck.value)
        if family == "by_blocks" and it.want == 0:
            assert ONE_WAVE or gpu_ctx.last_inflate_blocks() >= 2, (RC.item_id(it), gpu_ctx.last_inflate_blocks())
    _check(oracle, "zipc_hip_inflate", its, status, out_len, checksum, lambda i, n: bufs[i][offs[i]:offs[i] + n].tobytes(),
           lambda i: (bufs[i][:offs[i]], bufs[i][offs[i] + its[i].cap:]), lambda it: it.crc_op)


@pytest.mark.parametrize("family", list(RC.FAMILIES))
def test_inflate_many(gpu_ctx, oracle, family):
    """zipc_hip_inflate_many takes one crc_op a call, and limits for every stream or for none: a call per such group"""
    from zipc_amd import _lib

    L = _lib.lib()
    for op, group in _by_crc_op(RC.items(family)):
        for limited in (False, True):
            its = [it for it in group if (it.limit is not None) == limited]
            n = len(its)
            bufs, offs = _host_rooms(its)
            keep = [np.frombuffer(RC.stream_of(it).raw, np.uint8) for it in its]
            P, S = C.c_void_p * n, C.c_size_t * n
            res = (_lib.StreamResult * n)()
            C.memset(res, 0xEE, C.sizeof(res))
            st = L.zipc_hip_inflate_many(gpu_ctx.handle, n, P(*[a.ctypes.data for a in keep]), S(*[len(a) for a in keep]),
                                         S(*[it.limit for it in its]) if limited else None, op,
                                         P(*[b.ctypes.data + o for b, o in zip(bufs, offs)]), S(*[it.cap for it in its]), res)
            assert st == 0, (family, op, limited, st)
            for a, it in zip(keep, its):
                assert a.tobytes() == RC.stream_of(it).raw
            _check(oracle, "zipc_hip_inflate_many crc_op=%d" % op, its, [r.status for r in res], [r.out_len for r in res],
                   [r.checksum for r in res], lambda i, n: bufs[i][offs[i]:offs[i] + n].tobytes(),
                   lambda i: (bufs[i][:offs[i]], bufs[i][offs[i] + its[i].cap:]), op)


@pytest.mark.parametrize("family", list(RC.FAMILIES))
def test_zlib_batch(gpu_ctx, oracle, family):
    """the same bodies between CMF / FLG and the reference's Adler-32: the container's kernels hand inflate the same room"""
    from zipc_amd import batch

    its = RC.items(family)
    a = Arena(its, wrap=lambda s: RC.zlib_wrap(s.raw, _sums(oracle, s)[2]))
    d_res = a.results(16)
    batch.zlib_decompress_batch(gpu_ctx, a.src, a.dst, batch.to_device(a.descs(), a.dev), d_res, len(its), max(a.caps))
    a.check(oracle, "zlib_decompress_batch", batch.results_from_device(d_res), 2)


@pytest.mark.parametrize("family", list(RC.FAMILIES))
def test_recode_batch(gpu_ctx, oracle, family):
    """mid_cap = the room: inflate's bytes go to the middle arena, and that is where the guards stand"""
    import torch

    from zipc_amd import batch

    its = RC.items(family)
    a = Arena(its)  # (its destination arena is the MIDDLE one here)
    n = len(its)
    out_caps = [batch.deflate_bound(c) for c in a.caps]
    out_off = np.cumsum([0] + [c + 64 for c in out_caps[:-1]]).astype(np.uint64)
    descs = batch.make_recode_descs(np.array(a.src_off, np.uint64), a.src_len, a.dst_off, a.caps, out_off, out_caps)
    for i, it in enumerate(its):
        if it.limit is not None:
            descs["limit"][i] = it.limit
            descs["flags"][i] = 1
    out = torch.full((int(out_off[-1]) + out_caps[-1] + 256,), RC.POISON, dtype=torch.uint8, device=a.dev)
    d_res = a.results(32)
    batch.recode_batch(gpu_ctx, a.src, a.dst, out, batch.to_device(descs, a.dev), d_res, n, max(a.caps), sum(a.caps), 0)
    res = batch.recode_results_from_device(d_res)
    for i, it in enumerate(its):
        got = (int(res["stage"][i]), int(res["mid_len"][i]), int(res["reserved"][i]))
        want = (0, len(RC.stream_of(it).plain), 0) if it.want == 0 else (1, 0, 0)
        assert got == want, ("recode_batch", RC.item_id(it), "stage, mid_len, reserved", got, want)
    # (a stream that fits goes on to deflate: out_len is the recoded stream's, not looked at here; mid_len is inflate's)
    lens = np.where(res["status"] == 0, res["mid_len"], 0)
    a.check(oracle, "recode_batch", {"status": res["status"], "out_len": lens, "checksum": res["checksum"]}, 1)


def test_one_wave_child():
    """the batch forms and the long streams again with every stream on its one wave (the override is read once per
    process): one child, under a time limit of its own"""
    env = dict(os.environ, ZIPC_HIP_INFLATE_BLOCKS="0")
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        os.path.join(ROOT, "tests", "test_gpu_inflate_room.py"), "-k", "batch_few or batch_many or by_blocks"],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
