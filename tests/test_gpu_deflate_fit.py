"""Deflate's destination-capacity rule (tests/deflate_fit.py; include/zipc_hip.h at zipc_hip_deflate_batch) in every deflate
form of the library.  Every expectation is deflate_fit.expect()'s, made from the oracle's block trace alone: the verdict at
each capacity of the table, the bytes of a stream that fits, and what a stream that does not fit may leave behind.

One call per form holds every (case, level, cap) of a level as a descriptor of its own over the same source range.  The
destination slots lie at dst_off that are no multiple of 4, each with 64 guard bytes in front of it and behind its
dst_cap, in an arena that ends 256 bytes behind the last slot, so that an overrun lands in memory the test owns.  Each call
runs twice, with the arena filled with 0xA5 and with 0x5A: a byte counts as written if it differs from its fill in either.

The library reads its switches once per process, so the forms other than the default run in a process of their own each
(test_batch_form_applies_the_rule_under_overrides), one after the other."""
import ctypes as C
import functools
import os
import zlib

import numpy as np
import pytest

import deflate_fit as F
import util

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, TAIL = 64, 256
FILLS = (0xA5, 0x5A)
CRC32, ADLER32 = 1, 2

_BY_BLOCKS = {"ZIPC_HIP_PARSE_SEGMENTS": "1", "ZIPC_HIP_PARSE_SEG": "4096"}
_BLOCK_KERNELS = {"deflate_plan", "deflate_scan", "deflate_pack", "deflate_seal"}
# form -> (environment, tuning as host_sim words it, kernels it must launch, kernels it must not, pad the call with short
# streams until n x bps > 2048)
FORMS = {
    "default": ({}, {}, set(), set(), False),
    # a wave per stream: deflate_emit_wave<0>'s test, block by block as it writes
    "one-wave": ({"ZIPC_HIP_PARSE_SEGMENTS": "0"}, dict(parse_segments=0), {"lz_parse", "deflate_emit"}, {"deflate_scan"}, False),
    # a wave per block: deflate_scan_kernel's test before anything is written; few blocks, so deflate_bits runs
    "by-blocks-bits": (_BY_BLOCKS, dict(parse_segments=1, parse_seg=4096), _BLOCK_KERNELS | {"deflate_bits"}, set(), False),
    # ... and more than 2048 block slots in the call: no deflate_bits
    "by-blocks-no-bits": (_BY_BLOCKS, dict(parse_segments=1, parse_seg=4096), _BLOCK_KERNELS, {"deflate_bits"}, True),
}
FORM = os.environ.get("ZIPC_TEST_FIT_FORM", "default")


def _rows(level, padded=False, sim=None):
    rows = [r for r in F.table() if r[1] == level]
    if padded and level:
        import host_sim

        longest = max(len(F.data_of(n)) for n, _, _ in rows)
        bps = host_sim.deflate_forms(sim, len(rows), longest, level=level)[0]["bps"]
        k = 0
        while len(rows) * bps <= 2048:  # the empty and the one-byte input at caps 0..3, over and over
            rows.append((("empty", "one")[k // 4 % 2], level, k % 4))
            k += 1
    return rows


class Layout:
    """where the rows' streams lie: every input once in the source arena, a slot per row in the destination arena.
    room(cap) is the descriptor's dst_cap for a row's cap (the zlib form adds its six bytes)"""

    def __init__(self, rows, room=lambda cap: cap):
        self.rows = rows
        names = sorted({n for n, _, _ in rows})
        self.datas = [F.data_of(n) for n in names]
        at = dict(zip(names, np.cumsum([0] + [len(d) for d in self.datas[:-1]]).tolist()))
        self.caps = [room(cap) for _, _, cap in rows]
        self.src_off = [at[n] for n, _, _ in rows]
        self.src_len = [len(F.data_of(n)) for n, _, _ in rows]
        self.dst_off, pos = [], 0
        for i, cap in enumerate(self.caps):
            off = pos + GUARD
            off += (1 + i % 3 - off) % 4  # dst_off = 1, 2, 3 mod 4 in turn
            self.dst_off.append(off)
            pos = off + cap + GUARD
        self.dst_size = pos + TAIL
        assert all(o % 4 == 1 + i % 3 for i, o in enumerate(self.dst_off))

    def descs(self):
        from zipc_amd import batch

        return batch.make_descs(self.src_off, self.src_len, self.dst_off, self.caps)

    def src(self):
        import torch

        return torch.from_numpy(np.frombuffer(b"".join(self.datas) + b"\0" * 64, dtype=np.uint8).copy()).to(DEV)


def run_batch(ctx, lay, level, crc_op, fill, call="deflate"):
    """one zipc_hip_deflate_batch (or zipc_hip_zlib_compress_batch) over the layout: (results, the destination arena)"""
    import torch

    from zipc_amd import batch

    n = len(lay.rows)
    src = lay.src()
    dst = torch.full((lay.dst_size,), fill, dtype=torch.uint8, device=DEV)
    d_res = torch.full((n * 16,), 0xEE, dtype=torch.uint8, device=DEV)
    d_descs = batch.to_device(lay.descs(), DEV)
    if call == "deflate":
        batch.deflate_batch(ctx, src, dst, d_descs, d_res, n, max(lay.src_len), sum(lay.src_len), level, crc_op)
    else:
        batch.zlib_compress_batch(ctx, src, dst, d_descs, d_res, n, max(lay.src_len), sum(lay.src_len), level)
    ctx.synchronize()
    return batch.results_from_device(d_res), dst.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _checksums(name, level):
    """(CRC-32, the reference's Adler-32 of a deflate: one update a block, Q7) of an input"""
    import oracle

    data = F.data_of(name)
    return oracle.crc32(data), oracle.deflate(data, level=level, crc_op=oracle.CRC_ADLER32)[2]


@functools.lru_cache(maxsize=None)
def _inflates_back(stream, name):
    return zlib.decompress(stream, -15) == F.data_of(name)


class Want:
    """what a row's slot must hold: status; on success the bytes; of a stream that does not fit, the range [lo, hi) of its
    slot that may have been written, with `ref` what a written byte there must be"""

    def __init__(self, status, out, lo, hi, ref):
        self.status, self.out, self.lo, self.hi, self.ref = status, out, lo, hi, ref


def want_deflate(name, level, cap):
    st, out, front = F.expect(F.data_of(name), level, cap)
    return Want(st, out, 0, front, F.trace(F.data_of(name), level)[0])


@functools.lru_cache(maxsize=None)
def _zlib_stream(name, level):
    import oracle

    st, z, adler = oracle.zlib_compress(F.data_of(name), level)
    assert st == 0 and z[2:-4] == F.trace(F.data_of(name), level)[0]
    return z, adler


def want_zlib(name, level, room):
    """the zlib form: a stream fits iff room >= 6 and room - 6 fits by the rule; deflate's bytes lie 2 bytes in"""
    z, _ = _zlib_stream(name, level)
    if room < 6:
        return Want(16, b"", 0, 0, z)
    st, out, front = F.expect(F.data_of(name), level, room - 6)
    return Want(st, z if st == 0 else b"", 2, 2 + front if front else 2, z)


def check_slot(what, want, got, slots, cap, name, container=False):
    """got: (status, out_len); slots: per fill, the slot with its guards as a numpy array (GUARD bytes, cap, GUARD bytes)"""
    st, out_len = got
    assert st in (0, 16) and st == want.status, (what, "status", st, want.status)
    assert out_len == len(want.out), (what, "out_len", out_len, len(want.out))
    for fill, s in zip(FILLS, slots):
        assert (s[:GUARD] == fill).all(), (what, "the guard in front of the slot was written")
        assert (s[GUARD + cap:] == fill).all(), (what, "bytes behind dst_cap were written")
    body = [s[GUARD:GUARD + cap] for s in slots]
    if st == 0:
        for b in body:
            assert b[:out_len].tobytes() == want.out, (what, "the bytes are not the oracle's")
        got_bytes = body[0][:out_len].tobytes()  # (the zlib form: the body alone -- the reference's Adler-32 is not always RFC 1950's, Q6)
        assert _inflates_back(got_bytes[2:-4] if container else got_bytes, name), (what, "Python's zlib does not inflate the bytes back")
        return
    written = np.flatnonzero((body[0] != FILLS[0]) | (body[1] != FILLS[1]))
    if written.size:
        assert want.lo <= written[0] and written[-1] < want.hi, (
            what, "a stream that does not fit was written at or behind the block that does not fit", int(written[0]), int(written[-1]),
            want.lo, want.hi)
        ref = np.frombuffer(want.ref, np.uint8)
        for b in body:
            assert (b[written] == ref[written]).all(), (what, "what lies in front of the block that does not fit is not the stream's")


def check_batch(what, lay, wants, runs, checksum_of):
    """runs: per fill (results, arena); checksum_of(row index, run index, fits) -> the checksum the result must carry"""
    for (res, out), fill in zip(runs, FILLS):
        assert (out[lay.dst_size - TAIL:] == fill).all(), (what, "the arena's end was written")
    for i, ((name, level, cap), w) in enumerate(zip(lay.rows, wants)):
        off, room = lay.dst_off[i], lay.caps[i]
        row = (what, name, level, cap)
        got = [(int(res["status"][i]), int(res["out_len"][i])) for res, _ in runs]
        assert got[0] == got[1], (row, got)
        check_slot(row, w, got[0], [out[off - GUARD:off + room + GUARD] for _, out in runs], room, name, container=what.startswith("zlib"))
        for k, (res, _) in enumerate(runs):
            assert int(res["checksum"][i]) == checksum_of(i, k, w.status == 0), (row, "checksum", k, hex(int(res["checksum"][i])))


def _profiled(ctx):
    ctx.set_profiling(True)
    ctx.reset_kernel_times()


def _launched(ctx):
    names = {k for k, (n, ms) in ctx.kernel_times().items() if n}
    ctx.set_profiling(False)
    return names


_warm = []


def _warm_up(ctx):
    """a context's first deflate batch also checks its chain links: kept out of the profiles"""
    if not _warm:
        lay = Layout([("fox", 2, 64), ("fox", 2, 65), ("fox", 2, 66)])
        run_batch(ctx, lay, 2, CRC32, 0)
        _warm.append(True)


@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_batch_form_applies_the_rule(gpu_ctx, level):
    """zipc_hip_deflate_batch in the form this process runs in (ZIPC_TEST_FIT_FORM names it, default: no override): the
    table's verdicts, bytes, untouched guards and checksums -- of a stream that does not fit 0 with Adler-32 and the source's
    CRC-32 with CRC-32, whose pass runs over the source whatever the verdict -- and the kernels the form must launch"""
    import host_sim

    env, tun, need, never, padded = FORMS[FORM]
    assert all(os.environ.get(k) == v for k, v in env.items()), FORM
    sim = host_sim.lib()
    rows = _rows(level, padded, sim)
    lay = Layout(rows)
    wants = [want_deflate(*r) for r in rows]
    assert {w.status for w in wants} == {0, 16} and (level == 0 or any(w.hi > 0 for w in wants if w.status))
    _warm_up(gpu_ctx)
    runs, launched = [], []
    for crc_op, fill in zip((CRC32, ADLER32), FILLS):
        _profiled(gpu_ctx)
        try:
            runs.append(run_batch(gpu_ctx, lay, level, crc_op, fill))
        finally:
            launched.append(_launched(gpu_ctx))
    for crc_op, names in zip((CRC32, ADLER32), launched):
        if level == 0:
            assert names == {"deflate_stored"} | ({"crc32_segments", "crc32_finish"} if crc_op == CRC32 else set()), (FORM, sorted(names))
            continue
        predicted = host_sim.deflate_kernel_names(sim, len(rows), max(lay.src_len), crc_op=crc_op, total_src_len=sum(lay.src_len),
                                                  level=level, xchg_ok=int(gpu_ctx.lds_exchange_ordered()), **tun)
        assert names == predicted, (FORM, level, sorted(names), sorted(predicted))
        assert need <= names and not (never & names), (FORM, level, sorted(names))

    def checksum_of(i, k, fits):
        crc, adler = _checksums(rows[i][0], level)
        return crc if k == 0 else (adler if fits else 0)

    check_batch("deflate_batch, %s" % FORM, lay, wants, runs, checksum_of)


_died = []


@pytest.mark.parametrize("form", [f for f in FORMS if f != "default"])
def test_batch_form_applies_the_rule_under_overrides(form):
    """the test above, all four levels, in a process of its own under each override that picks another form; the processes
    run one after the other, each under a time limit, and after one that died or ran out of time no other is started"""
    import subprocess
    import sys

    assert not _died, "not started: the process of form %s died or timed out" % _died[0]
    e = dict(os.environ)
    e.update(FORMS[form][0])
    e["ZIPC_TEST_FIT_FORM"] = form
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
           "tests/test_gpu_deflate_fit.py::test_batch_form_applies_the_rule"]
    try:
        r = subprocess.run(cmd, cwd=os.path.dirname(util.HERE), env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    except subprocess.TimeoutExpired as t:
        _died.append(form)
        raise AssertionError((form, "timed out", (t.stdout or b"").decode()[-3000:]))
    out = r.stdout.decode()
    if r.returncode not in (0, 1):  # (pytest's own codes for "passed" and "tests failed": anything else is a process that died)
        _died.append(form)
    assert r.returncode == 0 and "4 passed" in out, (form, r.returncode, out[-3000:])


# ---- the other entry points, in the default form
@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_host_form_applies_the_rule(gpu_ctx, level):
    """zipc_hip_deflate, a call per row and fill: a stream that does not fit returns its status with *out_len = 0 and
    *checksum = 0 (the call sets both before anything else, whatever the checksum asked for)"""
    from zipc_amd import _lib

    L = _lib.lib()
    for name, _, cap in _rows(level):
        data = F.data_of(name)
        src = np.frombuffer(data + b"\0", np.uint8)
        w = want_deflate(name, level, cap)
        slots, got = [], []
        for crc_op, fill in zip((CRC32, ADLER32), FILLS):
            buf = np.full(cap + 2 * GUARD, fill, np.uint8)
            out_len, ck = C.c_size_t(77), C.c_uint32(77)
            st = L.zipc_hip_deflate(gpu_ctx.handle, src.ctypes.data, len(data), level, crc_op, buf.ctypes.data + GUARD, cap,
                                    C.byref(out_len), C.byref(ck))
            slots.append(buf)
            got.append((st, out_len.value))
            assert ck.value == (_checksums(name, level)[crc_op - 1] if w.status == 0 else 0), (name, level, cap, crc_op)
        assert got[0] == got[1], (name, level, cap, got)
        check_slot(("zipc_hip_deflate", name, level, cap), w, got[0], slots, cap, name)


@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_many_form_applies_the_rule(gpu_ctx, level):
    """zipc_hip_deflate_many: the rows of a level in one call per fill, destinations and results in host memory"""
    from zipc_amd import _lib

    L = _lib.lib()
    rows = _rows(level)
    n = len(rows)
    keep = {name: np.frombuffer(F.data_of(name) + b"\0", np.uint8) for name, _, _ in rows}
    caps = [cap for _, _, cap in rows]
    runs = []
    for crc_op, fill in zip((CRC32, ADLER32), FILLS):
        outs = [np.full(cap + 2 * GUARD, fill, np.uint8) for cap in caps]
        res = (_lib.StreamResult * n)()
        C.memset(res, 0xEE, C.sizeof(res))
        assert L.zipc_hip_deflate_many(gpu_ctx.handle, n, (C.c_void_p * n)(*[keep[name].ctypes.data for name, _, _ in rows]),
                                       (C.c_size_t * n)(*[len(F.data_of(name)) for name, _, _ in rows]), level, crc_op,
                                       (C.c_void_p * n)(*[o.ctypes.data + GUARD for o in outs]), (C.c_size_t * n)(*caps), res) == 0
        runs.append((res, outs))
    for i, (name, _, cap) in enumerate(rows):
        w = want_deflate(name, level, cap)
        got = [(int(res[i].status), int(res[i].out_len)) for res, _ in runs]
        assert got[0] == got[1], (name, level, cap, got)
        check_slot(("zipc_hip_deflate_many", name, level, cap), w, got[0], [outs[i] for _, outs in runs], cap, name)
        crc, adler = _checksums(name, level)
        assert int(runs[0][0][i].checksum) == crc, (name, level, cap)  # (the CRC-32 pass runs over the source whatever the verdict)
        assert int(runs[1][0][i].checksum) == (adler if w.status == 0 else 0), (name, level, cap)


@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_zlib_batch_form_applies_the_rule(gpu_ctx, level):
    """zipc_hip_zlib_compress_batch: every row with six bytes more room, and every input with 0 and 5 bytes of room.  A
    stream fits iff its room is at least 6 and six bytes less fit by the rule; a stream that fits is out_len + 6 bytes, the
    oracle's zlib stream, with the reference's Adler-32; one that does not has checksum 0 and no container byte written"""
    rows = _rows(level)
    rows = [(name, level, cap + 6) for name, _, cap in rows] + [(name, level, room) for name in sorted({r[0] for r in rows})
                                                                for room in (0, 5)]
    lay = Layout(rows)
    wants = [want_zlib(*r) for r in rows]
    assert {w.status for w in wants} == {0, 16}
    runs = [run_batch(gpu_ctx, lay, level, None, fill, call="zlib") for fill in FILLS]
    check_batch("zlib_compress_batch", lay, wants, runs, lambda i, k, fits: _zlib_stream(rows[i][0], level)[1] if fits else 0)
