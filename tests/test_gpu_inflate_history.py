"""The history forms on the MI355X (include/zipc_hip.h at zipc_hip_inflate_history_batch): the whole catalogue of
tests/inflate_history_cases.py through each of the five device forms and the two host forms.  One call per form holds all
its cases together, ragged: one source arena, one poisoned destination arena with every case's [history | room] between 64
guard bytes of 0xA5, dst_off 1..16 mod 16, results that start as 0xEE.  What is expected comes from the catalogue (which
tests/test_inflate_history_rules.py holds to Python's zlib), zlib.crc32 / zlib.adler32 and the oracle's Adler-32 of the
output alone; checked: results, bytes, every byte outside the rooms (guards, histories, the gaps of the dictionary forms),
the sizing forms against the decoding forms, a null d_hist against zipc_hip_inflate_batch / _prefix_batch / _size_batch on
the room catalogue item for item, n_streams = 0 and the null-pointer rules.

wave_copy_match's and the queued copies' reads out of the history have no host twin with the wave's own copy routines:
this file is their coverage."""
import ctypes as C
import zlib

import numpy as np
import pytest

import inflate_history_cases as HC
import inflate_room_cases as RC

pytestmark = pytest.mark.gpu
GUARD, POISON = RC.GUARD, RC.POISON
ROOM_MAX = 1 << 20  # a declared room above this belongs to a case that is refused: none is laid out
FRONT = 8192        # poison in front of the first room: where the cases with a dst_off of their own point


class Rooms:
    """the raw cases in one source arena and one destination arena: [guard | history | room | guard] each"""

    def __init__(self, cases):
        import torch

        self.cases, self.dev = cases, torch.device("cuda", 0)
        parts, self.src_off, pos = [], [], 0
        for c in cases:
            self.src_off.append(pos)
            parts.append(c.raw)
            pos += len(c.raw)
        self.src = torch.from_numpy(np.frombuffer(b"".join(parts) + b"\0" * 64, dtype=np.uint8).copy()).to(self.dev)
        self.src_clone = self.src.clone()
        self.room = [c.cap if c.cap <= ROOM_MAX else 0 for c in cases]
        self.dst_off, cursor = [], FRONT
        for i, c in enumerate(cases):
            if c.dst_off is not None:
                self.dst_off.append(c.dst_off)
                continue
            o = cursor + GUARD + len(c.hist)
            o += (HC.ROOM_MODS[i % 16] - o) % 16
            self.dst_off.append(o)
            cursor = o + self.room[i] + GUARD
        self.init = np.full(cursor + 256, POISON, np.uint8)
        self.outside = np.ones(len(self.init), bool)
        for i, c in enumerate(cases):
            o = self.dst_off[i]
            if c.dst_off is None:
                self.init[o - len(c.hist):o] = np.frombuffer(c.hist, np.uint8)
                self.outside[o:o + self.room[i]] = False
        self.max_cap = max(self.room)

    def fresh(self):
        import torch

        self.dst = torch.from_numpy(self.init.copy()).to(self.dev)
        self.res = torch.full((len(self.cases) * 16,), 0xEE, dtype=torch.uint8, device=self.dev)

    def descs(self):
        from zipc_amd import batch

        d = batch.make_descs(np.array(self.src_off, np.uint64), [len(c.raw) for c in self.cases], np.array(self.dst_off, np.uint64),
                             [c.cap for c in self.cases])
        for i, c in enumerate(self.cases):
            if c.limit is not None:
                d["limit"][i] = c.limit
                d["flags"][i] = 1
            d["flags"][i] |= c.flags_extra
        return batch.to_device(d, self.dev)

    def hist(self):
        from zipc_amd import batch

        return batch.to_device(batch.make_history([c.rec[0] for c in self.cases], [c.rec[1] for c in self.cases]), self.dev)

    def check(self, form, wants, second="checksum", wrote=True):
        """wants: per case ((status, checksum or ended, out_len), bytes or None)"""
        import torch

        from zipc_amd import batch

        res = batch.prefix_results_from_device(self.res) if second == "ended" else batch.results_from_device(self.res)
        assert torch.equal(self.src, self.src_clone), (form, "the source arena was written")
        out = self.dst.cpu().numpy()
        if not wrote:
            assert (out == self.init).all(), (form, "the destination arena was written")
        changed = np.flatnonzero((out != self.init) & self.outside)
        assert len(changed) == 0, (form, "bytes outside every room changed: a guard, a history or the arena's front", changed[:8].tolist())
        for i, c in enumerate(self.cases):
            want, plain = wants[i]
            who = (form, c.name, "dst_off %d" % self.dst_off[i])
            got = (int(res["status"][i]), int(res[second][i]), int(res["out_len"][i]))
            assert got == want, who + (got, want)
            if plain is not None and wrote:
                o = self.dst_off[i]
                data = out[o:o + len(plain)].tobytes()
                assert data == plain, who + ("byte", next(k for k in range(len(plain)) if data[k] != plain[k]))


@pytest.fixture(scope="module")
def rooms():
    return Rooms(HC.cases())


def _want_history(c, checksum_of):
    st, n = HC.expect_history(c)
    return (st, checksum_of(c.plain) if st == 0 else 0, n), (c.plain if st == 0 else None)


@pytest.mark.parametrize("crc_op", [0, 1, 2, 3])
def test_history_batch_the_whole_catalogue_in_one_call(gpu_ctx, oracle, rooms, crc_op):
    """zipc_hip_inflate_history_batch: results, bytes, guards and histories; the checksum is of the output alone --
    zlib.crc32, the oracle's Adler-32 (the reference's flavour), zlib.adler32 (RFC 1950's)"""
    from zipc_amd import batch

    checksum_of = {0: lambda p: 0, 1: zlib.crc32, 2: oracle.adler32, 3: zlib.adler32}[crc_op]
    rooms.fresh()
    batch.inflate_history_batch(gpu_ctx, rooms.src, rooms.dst, rooms.descs(), rooms.hist(), rooms.res, len(rooms.cases), rooms.max_cap, crc_op)
    assert gpu_ctx.last_inflate_blocks() == 0
    rooms.check("inflate_history_batch crc_op %d" % crc_op, [_want_history(c, checksum_of) for c in rooms.cases])


def test_prefix_history_batch_the_whole_catalogue_in_one_call(gpu_ctx, rooms):
    from zipc_amd import batch

    rooms.fresh()
    batch.inflate_prefix_history_batch(gpu_ctx, rooms.src, rooms.dst, rooms.descs(), rooms.hist(), rooms.res, len(rooms.cases))
    assert gpu_ctx.last_inflate_blocks() == 0
    wants = []
    for c in rooms.cases:
        w = HC.expect_prefix(c)
        wants.append((w, c.plain[:w[2]] if w[0] == 0 else None))
    assert sum(1 for w, _ in wants if w[:2] == (0, 0)) >= 7  # (the rooms of a block's own length, and one a byte short: cut)
    rooms.check("inflate_prefix_history_batch", wants, second="ended")


def test_size_history_batch_against_the_catalogue_and_the_decoding_form(gpu_ctx, rooms):
    """zipc_hip_inflate_size_history_batch writes no arena (none is passed); where the first form reports OK the two agree on
    out_len, and where it reports DST_TOO_SMALL sizing gives the length that did not fit"""
    from zipc_amd import batch

    rooms.fresh()
    batch.inflate_size_history_batch(gpu_ctx, rooms.src, rooms.descs(), rooms.hist(), rooms.res, len(rooms.cases))
    assert gpu_ctx.last_size_blocks() == 0
    rooms.check("inflate_size_history_batch", [((HC.expect_size(c)[0], 0, HC.expect_size(c)[1]), None) for c in rooms.cases], wrote=False)
    sized = batch.results_from_device(rooms.res)
    rooms.fresh()
    batch.inflate_history_batch(gpu_ctx, rooms.src, rooms.dst, rooms.descs(), rooms.hist(), rooms.res, len(rooms.cases), rooms.max_cap, 0)
    full = batch.results_from_device(rooms.res)
    n_ok = n_small = 0
    for i, c in enumerate(rooms.cases):
        if full["status"][i] == 0:
            assert sized["status"][i] == 0 and sized["out_len"][i] == full["out_len"][i], c.name
            n_ok += 1
        elif full["status"][i] == 16:
            assert sized["status"][i] == 0 and sized["out_len"][i] > c.cap, c.name
            n_small += 1
    assert n_ok > 80 and n_small >= 7, (n_ok, n_small)


# ---- the dictionary forms ---------------------------------------------------------------------------------------------

class DictRooms:
    """the zlib cases of one call: [guard | gap of dict_len | room | guard] each; with a dictionary longer than 5 bytes, its first
    stream made with the dictionary once more at dst_off 5, where no dictionary fits in front of it"""

    def __init__(self, dname):
        import torch

        self.dev = torch.device("cuda", 0)
        self.d = HC.dicts()[dname]
        self.cases = [z for z in HC.zcases() if z.dict == dname]
        self.no_gap = next((z for z in self.cases if z.seeded and z.status == 0), None) if len(self.d) > 5 else None
        streams = [z.raw for z in self.cases] + ([self.no_gap.raw] if self.no_gap else [])
        self.src_off = np.cumsum([0] + [len(s) for s in streams[:-1]]).astype(np.uint64)
        self.src_len = [len(s) for s in streams]
        self.src = torch.from_numpy(np.frombuffer(b"".join(streams) + b"\0" * 64, dtype=np.uint8).copy()).to(self.dev)
        # (one byte into its tensor: the seed's source is at an odd address)
        self.dict_dev = torch.from_numpy(np.frombuffer(b"\0" + self.d, dtype=np.uint8).copy()).to(self.dev)[1:] if self.d else None
        self.caps = [z.cap for z in self.cases] + ([self.no_gap.cap] if self.no_gap else [])
        self.dst_off, cursor = [], FRONT
        for i, z in enumerate(self.cases):
            o = cursor + GUARD + len(self.d)
            o += (HC.ROOM_MODS[(i * 7) % 16] - o) % 16
            self.dst_off.append(o)
            cursor = o + z.cap + GUARD
        self.init = np.full(cursor + 256, POISON, np.uint8)
        self.after = self.init.copy()  # what lies outside the rooms after the decompress form: the gaps that are seeded hold the dictionary
        self.outside = np.ones(len(self.init), bool)
        for z, o in zip(self.cases, self.dst_off):
            self.outside[o:o + z.cap] = False
            if z.seeded:
                self.after[o - len(self.d):o] = np.frombuffer(self.d, np.uint8)
        if self.no_gap:
            self.dst_off.append(5)
        self.n = len(self.caps)

    def fresh(self):
        import torch

        self.dst = torch.from_numpy(self.init.copy()).to(self.dev)
        self.res = torch.full((self.n * 16,), 0xEE, dtype=torch.uint8, device=self.dev)

    def descs(self):
        from zipc_amd import batch

        return batch.to_device(batch.make_descs(self.src_off, self.src_len, np.array(self.dst_off, np.uint64), self.caps), self.dev)


def _zwant(z, size, adler=zlib.adler32):
    if size:
        st = 0 if z.status in (HC.CHECKSUM, HC.DST_TOO_SMALL) else z.status
        return (st, z.checksum if st == HC.ZLIB_DICT else 0, len(z.plain) if st == 0 else 0)
    if z.plain is not None and z.status in (0, HC.CHECKSUM) and adler is not zlib.adler32:
        found, said = adler(z.plain), int.from_bytes(z.raw[-4:], "big")  # (the context's other flavour: the trailer is zlib's)
        return (0, found, len(z.plain)) if found == said else (HC.CHECKSUM, found, 0)
    return (z.status, z.checksum, len(z.plain) if z.status == 0 else 0)


@pytest.mark.parametrize("dname", HC.ZDICT_CALLS)
def test_zlib_dict_forms_one_call_per_dictionary(gpu_ctx, dname):
    """zipc_hip_zlib_decompress_dict_batch and zipc_hip_zlib_size_dict_batch over every zlib case of the dictionary's call:
    results, bytes, the gap of every seeded stream holds the dictionary, every other byte outside the rooms is untouched"""
    from zipc_amd import batch

    a = DictRooms(dname)
    assert a.cases
    gpu_ctx.set_adler_rfc1950(True)
    try:
        for size in (False, True):
            a.fresh()
            if size:
                batch.zlib_size_dict_batch(gpu_ctx, a.src, a.descs(), a.res, a.n, a.dict_dev, len(a.d))
                assert gpu_ctx.last_size_blocks() == 0
            else:
                batch.zlib_decompress_dict_batch(gpu_ctx, a.src, a.dst, a.descs(), a.res, a.n, max(a.caps), a.dict_dev, len(a.d))
                assert gpu_ctx.last_inflate_blocks() == 0
            res = batch.results_from_device(a.res)
            out = a.dst.cpu().numpy()
            expect = a.init if size else a.after
            changed = np.flatnonzero((out != expect) & a.outside)
            assert len(changed) == 0, (dname, size, "a gap, a guard or the arena's front is not what it must be", changed[:8].tolist())
            if size:
                assert (out == a.init).all()
            for i, z in enumerate(a.cases):
                got = (int(res["status"][i]), int(res["checksum"][i]), int(res["out_len"][i]))
                assert got == _zwant(z, size), (z.name, size, got, _zwant(z, size))
                if not size and z.status == 0:
                    assert out[a.dst_off[i]:a.dst_off[i] + len(z.plain)].tobytes() == z.plain, z.name
            if a.no_gap:  # dst_off 5 < dict_len: the stream's own INVALID_ARG, nothing written; sizing has no destination
                got = (int(res["status"][-1]), int(res["checksum"][-1]), int(res["out_len"][-1]))
                assert got == (_zwant(a.no_gap, True) if size else (HC.INVALID_ARG, 0, 0)), (dname, size, got)
    finally:
        gpu_ctx.set_adler_rfc1950(False)


def test_the_dictid_is_rfc_1950s_whatever_the_contexts_flavour(gpu_ctx, oracle):
    """the big dictionary's two Adler-32 flavours differ: in a context of the other flavour every stream made with it still opens;
    the outputs are then compared in the context's flavour, as zipc_hip_zlib_decompress_batch compares them"""
    from zipc_amd import batch

    a = DictRooms("big")
    assert zlib.adler32(a.d) != oracle.adler32(a.d)
    a.fresh()
    batch.zlib_decompress_dict_batch(gpu_ctx, a.src, a.dst, a.descs(), a.res, a.n, max(a.caps), a.dict_dev, len(a.d))
    res = batch.results_from_device(a.res)
    n_ok = 0
    for i, z in enumerate(a.cases):
        got = (int(res["status"][i]), int(res["checksum"][i]), int(res["out_len"][i]))
        assert got == _zwant(z, False, oracle.adler32), (z.name, got)
        n_ok += got[0] == 0
    assert n_ok >= 8


# ---- a null d_hist is the plain form ----------------------------------------------------------------------------------

def test_a_null_d_hist_is_the_plain_form_item_for_item(gpu_ctx):
    """every item of the room catalogue's SIM_FAMILIES through zipc_hip_inflate_batch / _prefix_batch / _size_batch and through
    the history forms with d_hist null, and with records of zeros: the same results and the same destination arena, byte for byte"""
    import torch

    from zipc_amd import batch

    dev = torch.device("cuda", 0)
    its = [it for f in RC.SIM_FAMILIES for it in RC.items(f)]
    streams, at, src_off, pos = [], {}, [], 0
    for it in its:
        raw = RC.stream_of(it).raw
        if raw not in at:
            at[raw] = pos
            streams.append(raw)
            pos += len(raw)
        src_off.append(at[raw])
    src = torch.from_numpy(np.frombuffer(b"".join(streams) + b"\0" * 64, dtype=np.uint8).copy()).to(dev)
    caps = [it.cap for it in its]
    dst_off, total, _ = RC.layout(caps, [it.off_mod for it in its])
    d = batch.make_descs(np.array(src_off, np.uint64), [len(RC.stream_of(it).raw) for it in its], dst_off, caps)
    for i, it in enumerate(its):
        if it.limit is not None:
            d["limit"][i], d["flags"][i] = it.limit, 1
    descs, n = batch.to_device(d, dev), len(its)
    zeros = batch.to_device(batch.make_history([0] * n), dev)

    def ran(fn):
        dst = torch.full((total,), POISON, dtype=torch.uint8, device=dev)
        res = torch.full((n * 16,), 0xEE, dtype=torch.uint8, device=dev)
        fn(dst, res)
        return dst, res

    for crc_op in (0, 1, 2):
        plain = ran(lambda dst, res: batch.inflate_batch(gpu_ctx, src, dst, descs, res, n, max(caps), crc_op))
        for hist in (None, zeros):
            got = ran(lambda dst, res: batch.inflate_history_batch(gpu_ctx, src, dst, descs, hist, res, n, max(caps), crc_op))
            assert torch.equal(plain[1], got[1]) and torch.equal(plain[0], got[0]), ("inflate", crc_op, hist is None)
    plain = ran(lambda dst, res: batch.inflate_prefix_batch(gpu_ctx, src, dst, descs, res, n))
    for hist in (None, zeros):
        got = ran(lambda dst, res: batch.inflate_prefix_history_batch(gpu_ctx, src, dst, descs, hist, res, n))
        assert torch.equal(plain[1], got[1]) and torch.equal(plain[0], got[0]), ("prefix", hist is None)
    plain = ran(lambda dst, res: batch.inflate_size_batch(gpu_ctx, src, descs, res, n))
    for hist in (None, zeros):
        got = ran(lambda dst, res: batch.inflate_size_history_batch(gpu_ctx, src, descs, hist, res, n))
        assert torch.equal(plain[1], got[1]) and bool((got[0] == POISON).all()), ("size", hist is None)


# ---- the argument rules -----------------------------------------------------------------------------------------------

def test_argument_rules(gpu_ctx, rooms):
    """null ctx, d_descs or d_results, a crc_op out of range, a dictionary above 32768 bytes or null with a length fail the
    call with INVALID_ARG; n_streams == 0 is OK and nothing is written"""
    from zipc_amd import _lib

    L, h = _lib.lib(), gpu_ctx.handle
    rooms.fresh()
    held = (rooms.src, rooms.dst, rooms.descs(), rooms.hist(), rooms.res)  # (the tensors outlive the calls)
    src, dst, descs, hist, res = (t.data_ptr() for t in held)
    IA = 18
    assert L.zipc_hip_inflate_history_batch(None, src, dst, descs, hist, res, 1, 100, 0) == IA
    assert L.zipc_hip_inflate_history_batch(h, src, dst, None, hist, res, 1, 100, 0) == IA
    assert L.zipc_hip_inflate_history_batch(h, src, dst, descs, hist, None, 1, 100, 0) == IA
    assert L.zipc_hip_inflate_history_batch(h, src, dst, descs, hist, res, 1, 100, 4) == IA
    assert L.zipc_hip_inflate_history_batch(h, src, dst, descs, hist, res, 1 << 31, 100, 0) == IA
    assert L.zipc_hip_inflate_prefix_history_batch(None, src, dst, descs, hist, res, 1) == IA
    assert L.zipc_hip_inflate_prefix_history_batch(h, src, dst, None, hist, res, 1) == IA
    assert L.zipc_hip_inflate_prefix_history_batch(h, src, dst, descs, hist, None, 1) == IA
    assert L.zipc_hip_inflate_size_history_batch(None, src, descs, hist, res, 1) == IA
    assert L.zipc_hip_inflate_size_history_batch(h, src, None, hist, res, 1) == IA
    assert L.zipc_hip_inflate_size_history_batch(h, src, descs, hist, None, 1) == IA
    assert L.zipc_hip_zlib_decompress_dict_batch(None, src, dst, descs, res, 1, 100, src, 10) == IA
    assert L.zipc_hip_zlib_decompress_dict_batch(h, src, dst, None, res, 1, 100, src, 10) == IA
    assert L.zipc_hip_zlib_decompress_dict_batch(h, src, dst, descs, None, 1, 100, src, 10) == IA
    assert L.zipc_hip_zlib_decompress_dict_batch(h, src, dst, descs, res, 1, 100, src, 32769) == IA
    assert L.zipc_hip_zlib_decompress_dict_batch(h, src, dst, descs, res, 1, 100, None, 1) == IA
    assert L.zipc_hip_zlib_size_dict_batch(h, src, descs, res, 1, src, 32769) == IA
    assert L.zipc_hip_zlib_size_dict_batch(h, src, descs, res, 1, None, 1) == IA
    assert L.zipc_hip_zlib_size_dict_batch(h, src, None, res, 1, src, 1) == IA
    assert L.zipc_hip_inflate_history_batch(h, src, dst, descs, hist, res, 0, 100, 0) == 0
    assert L.zipc_hip_inflate_prefix_history_batch(h, src, dst, descs, hist, res, 0) == 0
    assert L.zipc_hip_inflate_size_history_batch(h, src, descs, hist, res, 0) == 0
    assert L.zipc_hip_zlib_decompress_dict_batch(h, src, dst, descs, res, 0, 100, src, 10) == 0
    assert L.zipc_hip_zlib_size_dict_batch(h, src, descs, res, 0, src, 10) == 0
    gpu_ctx.synchronize()
    assert bool((rooms.res == 0xEE).all()) and (rooms.dst.cpu().numpy() == rooms.init).all()
    out_len = C.c_size_t()
    assert L.zipc_hip_inflate_history(h, b"\x03\x00", 2, 8, None, 0, 0, 0, None, 0, 0, C.byref(out_len), None) == IA
    assert L.zipc_hip_inflate_history(h, b"\x03\x00", 2, 0, b"x", 32769, 0, 0, None, 0, 0, C.byref(out_len), None) == IA
    assert L.zipc_hip_inflate_history(h, b"\x03\x00", 2, 0, None, 1, 0, 0, None, 0, 0, C.byref(out_len), None) == IA
    assert L.zipc_hip_zlib_decompress_dict(h, b"\x78\x9c", 2, b"x", 32769, None, 0, C.byref(out_len)) == IA
    assert L.zipc_hip_zlib_decompress_dict(h, b"\x78\x9c", 2, None, 1, None, 0, C.byref(out_len)) == IA


# ---- the host forms ---------------------------------------------------------------------------------------------------

def test_host_forms_over_the_catalogue(gpu_ctx):
    """zipc_hip_inflate_history and zipc_hip_zlib_decompress_dict, one stream a call.  They take arguments, not descriptors:
    the record cases whose fault is a descriptor's own (a flag bit, a dst_cap above the longest stream, a dst_off) cannot be
    put to them -- those are counted, every other case runs"""
    from zipc_amd import batch

    not_expressible = 0
    for c in HC.cases():
        if c.flags_extra or c.cap > ROOM_MAX or c.dst_off is not None:
            not_expressible += 1
            continue
        hist = c.hist if c.rec[0] == len(c.hist) else bytes(c.rec[0])
        st, data, ck = batch.inflate_history(gpu_ctx, c.raw, hist, c.rec[1], c.cap, c.limit, 3)
        want = HC.expect_history(c)
        assert (st, len(data)) == want, (c.name, st, len(data), want)
        if st == 0:
            assert data == c.plain and ck == zlib.adler32(c.plain), c.name
    assert not_expressible == 9
    gpu_ctx.set_adler_rfc1950(True)
    try:
        for z in HC.zcases():
            st, data = batch.zlib_decompress_dict(gpu_ctx, z.raw, HC.zdict_of(z), z.cap)
            assert st == z.status and data == (z.plain if st == 0 else b""), (z.name, st)
    finally:
        gpu_ctx.set_adler_rfc1950(False)
