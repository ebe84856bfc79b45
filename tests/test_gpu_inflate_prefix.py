"""The prefix forms on the MI355X (include/zipc_hip.h at zipc_hip_inflate_prefix_batch): the first dst_cap bytes of every
stream of a batch.  Every item of the catalogue's SIM_FAMILIES (tests/inflate_room_cases.py) and every planted case
(tests/inflate_prefix_cases.py) through zipc_hip_inflate_prefix_batch, laid out as tests/test_gpu_inflate_room.py lays
its items out: one poisoned destination arena, 64 guard bytes of 0xA5 on either side of every room, dst_off 0, 1, 5, 15
mod 16, results that start as 0xEE, a source arena compared with its clone -- once in calls of at most 256 streams, once
in one call of all of them.  What is expected comes from the catalogue, the planted cases and the oracle alone:

    want 0 : {0, 1, N} and the plain bytes      want 16: {0, 0, R} and the first R of them      want 2 : {2, 0, 0}

Then the two long streams (always a wave per stream: zipc_hip_last_inflate_blocks is 0), the zlib form over the same
bodies in the six container bytes with header failures and wrong Adler-32s, the call's argument rules, and the form's
defining property on 2000 ragged streams of text: its results are what the rule makes of zipc_hip_inflate_batch's.

wave_copy_match's and wave_copy's clipped copies have no host model: this file is their coverage."""
import random
import zlib

import numpy as np
import pytest

import inflate_prefix_cases as PC
import inflate_room_cases as RC
import util

pytestmark = pytest.mark.gpu
OFF_MODS = RC.OFF_MODS
_ADLER = {}

# a case: (id, stream bytes, plain or None, dst_cap, limit or None, (status, ended, out_len), dst_off mod 16)


def _item_want(it):
    n = len(RC.stream_of(it).plain)
    return {0: (0, 1, n), 16: (0, 0, it.R), 2: (2, 0, 0)}[it.want]


def _catalogue(families):
    return [(RC.item_id(it), RC.stream_of(it).raw, RC.stream_of(it).plain, it.cap, it.limit, _item_want(it), it.off_mod)
            for f in families for it in RC.items(f)]


def _planted():
    return [(p.name, p.raw, p.plain, p.R, p.limit, p.want, OFF_MODS[i % 4]) for i, p in enumerate(PC.planted())]


class Arena:
    """the cases' streams once each in a source arena, their rooms between guards in a poisoned destination arena"""

    def __init__(self, cases, wrap=None):
        import torch

        self.cases, self.dev = cases, torch.device("cuda", 0)
        at, parts, self.src_off, self.src_len, pos = {}, [], [], [], 0
        for c in cases:
            raw = c[1] if wrap is None else wrap(c)
            if raw not in at:
                at[raw] = pos
                parts.append(raw)
                pos += len(raw)
            self.src_off.append(at[raw])
            self.src_len.append(len(raw))
        self.src = torch.from_numpy(np.frombuffer(b"".join(parts) + b"\0" * 64, dtype=np.uint8).copy()).to(self.dev)
        self.src_clone = self.src.clone()
        self.caps = [c[3] for c in cases]
        self.dst_off, total, self.guards = RC.layout(self.caps, [c[6] for c in cases])
        self.dst = torch.full((total,), RC.POISON, dtype=torch.uint8, device=self.dev)
        self.res = torch.full((len(cases) * 16,), 0xEE, dtype=torch.uint8, device=self.dev)

    def descs(self):
        from zipc_amd import batch

        d = batch.make_descs(np.array(self.src_off, np.uint64), self.src_len, self.dst_off, self.caps)
        for i, c in enumerate(self.cases):
            if c[4] is not None:
                d["limit"][i] = c[4]
                d["flags"][i] = 1
        return batch.to_device(d, self.dev)

    def check(self, form):
        import torch

        from zipc_amd import batch

        res = batch.prefix_results_from_device(self.res)
        out = self.dst.cpu().numpy()
        assert torch.equal(self.src, self.src_clone), (form, "the source arena was written")
        for i, (ident, _, plain, cap, _, want, off_mod) in enumerate(self.cases):
            who = (form, ident, "dst_off mod 16 = %d" % off_mod)
            got = (int(res["status"][i]), int(res["ended"][i]), int(res["out_len"][i]))
            assert got == want, who + (got, want)
            o = int(self.dst_off[i])
            if plain is not None and want[0] == 0 and want[2]:
                data = out[o:o + want[2]].tobytes()
                assert data == plain[:want[2]], who + ("byte", next(k for k in range(want[2]) if data[k] != plain[k]))
            front, back = out[self.guards[i][0]], out[self.guards[i][1]]
            assert (front == RC.POISON).all(), who + ("wrote in front of its room",)
            assert (back == RC.POISON).all(), who + ("wrote %d bytes behind its room" % (int(np.flatnonzero(back != RC.POISON).max()) + 1),)


def _call(ctx, a, descs, lo, hi, zlib_form=False):
    """one call over cases [lo, hi) of the arena"""
    from zipc_amd import batch

    fn = batch.zlib_decompress_prefix_batch if zlib_form else batch.inflate_prefix_batch
    fn(ctx, a.src, a.dst, descs[lo * 48:], a.res[lo * 16:], hi - lo)
    assert ctx.last_inflate_blocks() == 0


@pytest.fixture(scope="module")
def short_cases():
    return _catalogue(RC.SIM_FAMILIES) + _planted()


def test_calls_of_at_most_256_streams(gpu_ctx, short_cases):
    a = Arena(short_cases)
    descs = a.descs()
    for lo in range(0, len(short_cases), 256):
        _call(gpu_ctx, a, descs, lo, min(lo + 256, len(short_cases)))
    a.check("inflate_prefix_batch, calls of 256")


def test_one_call_of_all(gpu_ctx, short_cases):
    assert len(short_cases) == 7818 + len(PC.planted())
    a = Arena(short_cases)
    _call(gpu_ctx, a, a.descs(), 0, len(short_cases))
    a.check("inflate_prefix_batch, one call")


def _long_cases():
    out = []
    for i, s in enumerate(RC.by_blocks()):
        n = len(s.plain)
        for j, cap in enumerate((300 << 10, n, n - 1, 256 << 10)):
            out.append(("by_blocks/%s/R=%d" % (s.name, cap), s.raw, s.plain, cap, None, PC.want_of(n, cap), OFF_MODS[(i + j) % 4]))
    return out


def test_long_streams_go_by_their_one_wave(gpu_ctx):
    """rooms of 300 KiB and of N, where zipc_hip_inflate_batch decodes by a wave per block: here by the same rule as every
    stream, alone and in one call, and no block is reported for the call"""
    cases = _long_cases()
    assert {c[5][1] for c in cases} == {0, 1}
    a = Arena(cases)
    _call(gpu_ctx, a, a.descs(), 0, len(cases))
    a.check("inflate_prefix_batch, long streams")
    b = Arena(cases[:1])
    _call(gpu_ctx, b, b.descs(), 0, 1)
    b.check("inflate_prefix_batch, one long stream")


# ---- the zlib form --------------------------------------------------------------------------------------------------

def _adler(oracle, plain):
    if plain not in _ADLER:
        _ADLER[plain] = oracle.adler32(plain)
    return _ADLER[plain]


def test_zlib_form(gpu_ctx, oracle, short_cases):
    """the same bodies between CMF / FLG and the reference's Adler-32, then streams that fail the container's checks, an
    ended stream with a wrong Adler-32 (CHECKSUM, no bytes, not ended) and cut streams with a wrong one (OK: not compared)"""
    cases = list(short_cases) + _long_cases()[:2]
    wrapped = {}

    def wrap(c):
        key = (c[1], c[0].startswith("bad/"))
        if key not in wrapped:
            adler = _adler(oracle, c[2]) if c[2] is not None else 1
            wrapped[key] = RC.zlib_wrap(c[1], adler ^ 0x00010000 if key[1] else adler)
        return wrapped[key]

    lit = next(p for p in PC.planted() if p.name == "start/fixed_literal/R=0")
    n = len(lit.plain)
    good = RC.zlib_wrap(lit.raw, _adler(oracle, lit.plain))
    extra = [("bad/ended_wrong_adler", lit.raw, lit.plain, n, None, (6, 0, 0), 1),
             ("bad/ended_wrong_adler_room_to_spare", lit.raw, lit.plain, n + 9, None, (6, 0, 0), 5),
             ("bad/cut_wrong_adler", lit.raw, lit.plain, n - 1, None, (0, 0, n - 1), 15),
             ("bad/cut_wrong_adler_no_room", lit.raw, lit.plain, 0, None, (0, 0, 0), 0)]
    # (the stream, the container's verdict): the reference's checks in its order (tests/zlib_cases.py has them all)
    def head(cmf, flg):  # FLG's check bits made right
        return bytes([cmf, flg + (31 - (cmf * 256 + flg) % 31) % 31]) + good[2:]

    assert head(0x78, 0x80) == good
    headers = [(good[:5], 1), (bytes([good[0], good[1] ^ 1]) + good[2:], 1), (head(0x79, 0x80), 3), (head(0x88, 0x00), 4), (head(0x78, 0xA0), 5)]
    head_cases = [("header/%d" % i, raw, None, 40, None, (st, 0, 0), OFF_MODS[i % 4]) for i, (raw, st) in enumerate(headers)]
    a = Arena(cases + extra + head_cases, wrap=lambda c: c[1] if c[0].startswith("header/") else wrap(c))
    _call(gpu_ctx, a, a.descs(), 0, len(a.cases), zlib_form=True)
    a.check("zlib_decompress_prefix_batch")


# ---- the call's own rules ---------------------------------------------------------------------------------------------

def test_argument_rules(gpu_ctx):
    from zipc_amd._lib import lib

    L = lib()
    a = Arena(_planted()[:3])
    descs = a.descs()
    for fn in (L.zipc_hip_inflate_prefix_batch, L.zipc_hip_zlib_decompress_prefix_batch):
        args = [gpu_ctx.handle, a.src.data_ptr(), a.dst.data_ptr(), descs.data_ptr(), a.res.data_ptr(), 3]
        for k, bad in ((0, None), (3, None), (4, None), (5, 0x80000000)):
            assert fn(*(args[:k] + [bad] + args[k + 1:])) == 18, (fn.__name__, k)
        assert fn(*(args[:5] + [0])) == 0
        assert fn(gpu_ctx.handle, None, None, descs.data_ptr(), a.res.data_ptr(), 0) == 0
    gpu_ctx.synchronize()
    assert (a.res.cpu().numpy() == 0xEE).all() and (a.dst.cpu().numpy() == RC.POISON).all()  # (nothing was enqueued)


# ---- the defining property ---------------------------------------------------------------------------------------------

def test_the_form_is_what_the_rule_makes_of_inflate_batch(gpu_ctx):
    """2000 ragged streams of text, rooms on every side of their sizes, a third of them with a limit below, inside or
    behind: {status, ended, out_len} is what the rule makes of zipc_hip_inflate_batch's (status, out_len) for the same
    descriptors, and the bytes are zlib's own first R"""
    import torch

    from zipc_amd import batch

    r = random.Random(20260117)
    text = util.text(1 << 20, 77)
    cases = []
    for i in range(2000):
        n = r.choice((0, 1, 30, 300, 3000)) + r.randrange(20000 if i % 10 == 0 else 2000)
        at = r.randrange(len(text) - n)
        c = zlib.compressobj(r.choice((1, 6, 9)), zlib.DEFLATED, -15)
        raw = c.compress(text[at:at + n]) + c.flush()
        cap = r.choice((0, 1, 8, 64, n // 2, max(n - 1, 0), n, n + 1, n + 100, r.randrange(n + 1)))
        limit = r.choice((None, None, cap, max(cap - 1, 0), cap + 3, n, n + 5, r.randrange(n + 2)))
        cases.append(("text/%d" % i, raw, text[at:at + n], cap, limit, None, OFF_MODS[i % 4]))
    a, b = Arena(cases), Arena(cases)
    descs = a.descs()
    batch.inflate_batch(gpu_ctx, a.src, a.dst, descs, a.res, len(cases), max(a.caps), 0)
    ref = batch.results_from_device(a.res)
    _call(gpu_ctx, b, descs, 0, len(cases))
    got = batch.prefix_results_from_device(b.res)
    out = b.dst.cpu().numpy()
    assert torch.equal(b.src, b.src_clone)
    kinds = set()
    for i, (ident, raw, plain, cap, limit, _, _) in enumerate(cases):
        s, n = int(ref["status"][i]), int(ref["out_len"][i])
        want = (0, 1, n) if s == 0 else (0, 0, cap) if s == 16 else (s, 0, 0)
        rec = (int(got["status"][i]), int(got["ended"][i]), int(got["out_len"][i]))
        assert rec == want, (ident, cap, limit, rec, want)
        kinds.add((s, want[1]))
        o = int(b.dst_off[i])
        if want[0] == 0:
            assert out[o:o + want[2]].tobytes() == zlib.decompressobj(-15).decompress(raw, cap)[:want[2]] if cap else want[2] == 0, ident
        assert (out[b.guards[i][0]] == RC.POISON).all() and (out[b.guards[i][1]] == RC.POISON).all(), ident
    assert kinds == {(0, 1), (16, 0), (2, 0)}, kinds
