"""Inputs that sit exactly on inflate's accept / reject rules (zd.ml:355-391, 564-709).

A small block assembler over util.BitWriter writes what no encoder would: explicit code-length-code lengths and
HCLEN, explicit code-length items (16 first, repeats past the end), explicit litlen / distance lengths, raw symbols
and raw code bits (a phantom symbol, fixed symbols 286/287 and 30/31).  Every case below knows its status, and its
bytes when accepted, BY CONSTRUCTION -- what was written, not what a decoder made of it.  tests/test_oracle_pins.py
holds the oracle to them, and zlib (`zlib.decompressobj(-15)`) to the accepted bytes; ZLIB_DIFFERS names every case
where zlib and the reference part, with the reason.

INFLATE_RULE_CASES: name -> Case (the stream alone).  wrapped_cases(): name/wrapper -> Case, each case also
  b  behind a valid ~1 KiB block (and 3 bytes after the final block, where the end of the input is not the point);
  c  (symbol rules) deep inside its dynamic or fixed block, after ~10 KiB of output from 8 KiB of symbols;
  d  behind a valid block at an odd bit phase, the case's last byte the input's last;
  e  inside a stream of >= 600 KB of output, as a later block, with many valid blocks after it (one-stream calls go
     by blocks there).
Limits are relative to what a case itself writes: a wrapper adds what comes before it.  CPU only; no GPU import.
"""
import collections
import functools
import os
import random
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from util import BitWriter  # noqa: E402

OK, CORRUPTED, SIZE_EXCEEDED = 0, 1, 2
LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
         8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0] + [i // 2 for i in range(2, 28)]
ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def complete_lengths(n):
    """lengths of a complete prefix code over n symbols (n == 1: the one code of length 1)"""
    if n == 1:
        return [1]
    k = (n - 1).bit_length()
    short = (1 << k) - n
    return [k - 1] * short + [k] * (n - short)


def canonical(lengths):
    """sym -> (code, length) of the canonical code of `lengths` (codes clipped to their lengths: an over-subscribed
    table still gets bits to write)"""
    codes, code = {}, 0
    for ln in range(1, 16):
        for sym, sl in enumerate(lengths):
            if sl == ln:
                codes[sym] = (code & ((1 << ln) - 1), ln)
                code += 1
        code <<= 1
    return codes


# the code every general case uses: all 286 litlen and all 30 distance symbols (HLIT 286, HDIST 30)
FULL_LL = complete_lengths(286)
FULL_DL = complete_lengths(30)
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DL = [5] * 32


@functools.lru_cache(maxsize=None)
def len_sym(length):
    i = max(i for i, b in enumerate(LBASE) if b <= length)
    if i == 28 and length != 258:
        i = 27
    return 257 + i, length - LBASE[i]


@functools.lru_cache(maxsize=None)
def dist_sym(dist):
    i = max(i for i, b in enumerate(DBASE) if b <= dist)
    return i, dist - DBASE[i]


class Writer:
    """util.BitWriter plus named marks: mark(name) tags the next field, marks[name] = (first bit, bit count)"""

    def __init__(self):
        self.w, self.pos, self.marks, self._tag = BitWriter(), 0, {}, None

    def mark(self, name):
        self._tag = name

    def _put(self, fn, v, n):
        if self._tag is not None and n:
            self.marks.setdefault(self._tag, (self.pos, n))
            self._tag = None
        fn(v, n)
        self.pos += n

    def field(self, v, n):
        self._put(self.w.field, v, n)

    def code(self, v, n):
        self._put(self.w.code, v, n)

    def align(self):
        self.field(0, (-self.pos) % 8)

    def raw(self, b):
        assert self.pos % 8 == 0 and self.w.n == 0
        if b:
            self.field(b[0], 8)  # (a mark set for this field)
            self.w.out += b[1:]
            self.pos += 8 * (len(b) - 1)

    def bytes(self):
        return self.w.bytes()


class Out:
    """the plain bytes the written symbols stand for; `bad` once a symbol has none (a too-far match, a raw symbol)"""

    def __init__(self):
        self.b, self.bad = bytearray(), False

    def match(self, length, dist):
        if dist > len(self.b) or dist < 1:
            self.bad = True
            return
        for _ in range(length):
            self.b.append(self.b[-dist])


def _resolve(v, out):
    return v(len(out.b)) if callable(v) else v


def emit_symbols(w, out, syms, lc, dc):
    """literals (int), ('m', length, dist) -- dist may be a function of the output so far --, ('l', sym, extra) and
    ('d', sym, extra) raw symbols, ('code', v, n) raw code bits, ('bits', v, n) raw field bits, ('mark', name)"""
    for s in syms:
        if isinstance(s, int):
            w.code(*lc[s])
            out.b.append(s)
        elif s[0] == "m":
            length, dist = s[1], _resolve(s[2], out)
            assert 3 <= length <= 258 and 1 <= dist <= 32768, s
            ls, le = len_sym(length)
            ds, de = dist_sym(dist)
            w.mark("len_code"); w.code(*lc[ls])
            w.mark("len_extra"); w.field(le, LEXT[ls - 257])
            w.mark("dist_code"); w.code(*dc[ds])
            w.mark("dist_extra"); w.field(de, DEXT[ds])
            out.match(length, dist)
        elif s[0] == "l":
            w.code(*lc[s[1]])
            if 257 <= s[1] <= 285:
                w.field(s[2], LEXT[s[1] - 257])
            out.bad = True
        elif s[0] == "d":
            w.code(*dc[s[1]])
            if s[1] < 30:
                w.field(s[2], DEXT[s[1]])
            out.bad = True
        elif s[0] == "code":
            w.code(s[1], s[2])
            out.bad = True
        elif s[0] == "bits":
            w.field(s[1], s[2])
        elif s[0] == "mark":
            w.mark(s[1])
        else:
            raise ValueError(s)


def rle_items(seq):
    """code-length items of a length sequence: plain lengths, zero runs as 17 / 18"""
    items, i = [], 0
    while i < len(seq):
        run = 1
        while i + run < len(seq) and seq[i + run] == seq[i]:
            run += 1
        if seq[i] == 0 and run >= 3:
            n = min(run, 138)
            items.append((17, n) if n <= 10 else (18, n))
            i += n
        else:
            items.append((seq[i],))
            i += 1
    return items


Blk = collections.namedtuple("Blk", "kind syms opts")


def stored(data=b"", **opts):
    """opts: length, nlen (the header's values), cut (bytes of LEN/NLEN written, the input ending there)"""
    return Blk("stored", data, opts)


def fixed(syms, **opts):
    return Blk("fixed", list(syms), opts)


def dynamic(syms, **opts):
    """opts: ll, dl (lengths), hlit, hdist (counts), hlit_field, hdist_field (raw 5-bit fields), cl (19 lengths by symbol),
    hclen, items ([(sym,) | (16|17|18, repeat) | ('code', v, n)]), eob (False: no end of block)"""
    return Blk("dynamic", list(syms), opts)


def btype3(syms):
    """BTYPE 3, then what a decoder that took it for a fixed block would decode: syms and an end of block"""
    return Blk("btype3", list(syms), {})


def emit_block(w, out, blk, final):
    w.mark("bfinal"); w.field(1 if final else 0, 1)
    o = blk.opts
    if blk.kind == "btype3":
        w.mark("btype"); w.field(3, 2)
        lc, dc = canonical(FIXED_LL), canonical(FIXED_DL)
        emit_symbols(w, out, blk.syms, lc, dc)
        w.code(*lc[256])
        out.bad = True
        return
    if blk.kind == "stored":
        w.mark("btype"); w.field(0, 2)
        w.align()
        data = blk.syms
        length = o.get("length", len(data))
        nlen = o.get("nlen", (~length) & 0xFFFF)
        hdr = bytes([length & 255, length >> 8, nlen & 255, nlen >> 8])[:o.get("cut", 4)]
        w.mark("stored_len"); w.raw(hdr)
        w.raw(data)
        if length != len(data) or nlen != (~length) & 0xFFFF or o.get("cut", 4) < 4:
            out.bad = True
        else:
            out.b += data
        return
    if blk.kind == "fixed":
        w.mark("btype"); w.field(1, 2)
        lc, dc = canonical(FIXED_LL), canonical(FIXED_DL)
        emit_symbols(w, out, blk.syms, lc, dc)
        w.mark("eob"); w.code(*lc[256])
        return
    w.mark("btype"); w.field(2, 2)
    ll, dl = list(o.get("ll", FULL_LL)), list(o.get("dl", FULL_DL))
    hlit = o.get("hlit", max([257] + [i + 1 for i, x in enumerate(ll) if x]))
    hdist = o.get("hdist", max([1] + [i + 1 for i, x in enumerate(dl) if x]))
    seq = (ll + [0] * 300)[:hlit] + (dl + [0] * 40)[:hdist]
    items = o["items"] if "items" in o else rle_items(seq)
    cl = o.get("cl")
    if cl is None:
        used = sorted({it[0] for it in items if it[0] != "code"})
        cl = [0] * 19
        for s, ln in zip(used, complete_lengths(len(used))):
            cl[s] = ln
    hclen = o.get("hclen", max([4] + [i + 1 for i, s in enumerate(ORDER) if cl[s]]))
    w.mark("hlit"); w.field(o.get("hlit_field", hlit - 257), 5)
    w.mark("hdist"); w.field(o.get("hdist_field", hdist - 1), 5)
    w.mark("hclen"); w.field(hclen - 4, 4)
    w.mark("cl_lengths")
    for i in range(hclen):
        w.field(cl[ORDER[i]], 3)
    clc = canonical(cl)
    w.mark("cl_items")
    for it in items:
        if it[0] == "code":
            w.code(it[1], it[2])
            continue
        w.code(*clc[it[0]])
        if it[0] == 16:
            w.mark("repeat_extra"); w.field(it[1] - 3, 2)
        elif it[0] == 17:
            w.mark("repeat_extra"); w.field(it[1] - 3, 3)
        elif it[0] == 18:
            w.mark("repeat_extra"); w.field(it[1] - 11, 7)
    lc, dc = canonical(ll[:hlit]), canonical(dl[:hdist])
    w.mark("symbols")
    emit_symbols(w, out, blk.syms, lc, dc)
    if o.get("eob", True):
        w.mark("eob"); w.code(*lc[256])


Case = collections.namedtuple("Case", "stream limit status plain ref cuts")
# what a case is before it is written: blocks (the last one final unless final_last=False), the limit on what the case
# itself writes, the expected status, the zd.ml lines, where the input ends (cut_at: the mark whose field loses its last
# byte; at_end: the end of the input is part of the rule), and which wrappers apply
Spec = collections.namedtuple("Spec", "blocks limit status ref cut_at at_end final_last trailing wrappers deep")


def spec(blocks, status, ref, limit=None, cut_at=None, at_end=False, final_last=True, trailing=b"", wrappers="abde",
         deep=None):
    """deep: what wrapper c puts in front of the last block's symbols, in that block's code (default _deep_syms())"""
    if cut_at is not None or not final_last:
        at_end = True
    if at_end:
        wrappers = wrappers.replace("e", "")
    return Spec(blocks, limit, status, ref, cut_at, at_end, final_last, trailing, wrappers, deep)


def assemble(blocks, final_last=True, cut_at=None, trailing=b"", pre=None, post=None):
    """-> (stream, plain or None, marks, cuts).  pre: (bytes, plain) before (byte aligned, no final block); post: bytes
    and plain after (the case's blocks then all non-final, an empty stored block aligns them).  cuts: the output length
    at the end of each block (pre and post as one block each), what the reference's per-block checksum update is fed
    by (zd.ml:682-690)"""
    w, out, cuts = Writer(), Out(), []
    if pre is not None:
        w.raw(pre[0])
        out.b += pre[1]
        cuts.append(len(out.b))
    for i, blk in enumerate(blocks):
        final = i == len(blocks) - 1 and final_last and post is None
        emit_block(w, out, blk, final)
        cuts.append(len(out.b))
    if post is not None:
        emit_block(w, out, stored(b""), False)
        w.raw(post[0])
        out.b += post[1]
        cuts.append(len(out.b))
    raw = w.bytes()
    if cut_at is not None:
        start, n = w.marks[cut_at]
        raw = raw[:(start + n - 1) // 8]
    return raw + trailing, (None if out.bad else bytes(out.b)), w.marks, cuts


# ---- the valid blocks the wrappers put around a case --------------------------------------------------------------

def _prefix_block(n_lits9):
    """a fixed block of ~1 KiB output: text-ish literals and matches, then n_lits9 9-bit literals (its end's bit phase)"""
    r = random.Random(7)
    syms = [r.choice(b"abcdefgh ") for _ in range(200)]
    for _ in range(100):
        syms += [("m", r.randrange(3, 12), r.randrange(1, 150))]
    syms += [200 + i for i in range(n_lits9)]
    return fixed(syms)


def _deep_syms():
    """8 KiB of symbols (~10 KiB of output) to put in front of a case's block"""
    r = random.Random(8)
    syms = [r.randrange(256) for _ in range(64)]
    for i in range(4000):  # (distances 4 and up: distance symbols 3-11, which every code of a "c" case holds)
        syms.append(r.randrange(256) if i % 3 else ("m", r.randrange(3, 9), r.randrange(4, 60)))
    return syms


def _zlib_part(seed, n, final):
    r = random.Random(seed)
    words = [b"inflate", b"rules", b"block", b"header", b"symbol", b"distance", b" ", b"\n", b"length", b"stored"]
    plain = bytearray()
    while len(plain) < n:
        plain += r.choice(words) if r.random() < 0.8 else bytes([r.randrange(256)])
    plain = bytes(plain[:n])
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = c.compress(plain) + c.flush(zlib.Z_FINISH if final else zlib.Z_SYNC_FLUSH)
    return raw, plain


_BIG = {}


def big_parts():
    """(pre, post) of wrapper e: 320 KB of output in dynamic blocks before the case, 320 KB after it (zlib level 6)"""
    if not _BIG:
        _BIG["pre"] = _zlib_part(1, 320000, False)
        _BIG["post"] = _zlib_part(2, 320000, True)
    return _BIG["pre"], _BIG["post"]


# ---- the cases --------------------------------------------------------------------------------------------------

def _without(n_total, missing, at):
    """a complete code over n_total symbol slots with `missing` of them (at index `at`) given no code"""
    c = complete_lengths(n_total - missing)
    return c[:at] + [0] * missing + c[at:]


def _specs():
    S = {}
    lits = list(b"rule cases ")  # literals below 144: 8-bit fixed codes

    # -- block type (zd.ml:694-705)
    S["btype3_first"] = spec([btype3(lits)], CORRUPTED, "zd.ml:701")
    S["btype3_later"] = spec([fixed(lits), btype3(lits)], CORRUPTED, "zd.ml:701")
    S["btype3_later_nonfinal"] = spec([fixed(lits), btype3(lits), fixed(lits)], CORRUPTED, "zd.ml:701")
    S["nonfinal_then_end"] = spec([fixed(lits)], CORRUPTED, "zd.ml:694-705,564-579", final_last=False)
    S["nonfinal_stored_then_end"] = spec([stored(b"abc")], CORRUPTED, "zd.ml:694-705,564-579", final_last=False)
    S["trailing_bytes_ignored"] = spec([fixed(lits)], OK, "zd.ml:705", trailing=b"\xff\x00\x13\x37")

    # -- stored blocks (zd.ml:671-680)
    for k in range(4):
        S["stored_hdr_%d_bytes_left" % k] = spec([fixed(lits), stored(b"", cut=k)], CORRUPTED, "zd.ml:672", at_end=True)
    for byte in range(4):
        for bit in (0, 7):
            ln, nl = 5, (~5) & 0xFFFF
            if byte < 2:
                ln ^= 1 << (bit + 8 * byte)
            else:
                nl ^= 1 << (bit + 8 * (byte - 2))
            S["stored_nlen_byte%d_bit%d" % (byte, bit)] = spec([stored(b"hello", length=ln, nlen=nl)], CORRUPTED,
                                                               "zd.ml:675")
    S["stored_len_eq_input_left"] = spec([fixed(lits), stored(b"xyz" * 7)], OK, "zd.ml:677", at_end=True)
    S["stored_len_input_left_plus1"] = spec([fixed(lits), stored(b"xyz" * 7, length=22)], CORRUPTED, "zd.ml:677",
                                            at_end=True)
    S["stored_len_zero"] = spec([stored(b""), fixed(lits)], OK, "zd.ml:671-680")
    S["stored_len_zero_final"] = spec([fixed(lits), stored(b"")], OK, "zd.ml:671-680", at_end=True)
    for ph in range(8):  # a fixed block of 8 * 11 + 10 + 9 * ph bits in front: the stored header at bit phase 2 + ph
        S["stored_phase%d" % ((2 + ph) % 8)] = spec([fixed(lits + [200 + i for i in range(ph)]), stored(b"phase %d" % ph)],
                                                    OK, "zd.ml:671-680")

    # -- HLIT and HDIST (zd.ml:641)
    S["hlit_286"] = spec([dynamic(lits + [("m", 258, 1)])], OK, "zd.ml:641")
    for hl in (287, 288):
        S["hlit_%d" % hl] = spec([dynamic(lits + [("m", 5, 2)], hlit=hl)], CORRUPTED, "zd.ml:641")
    S["hdist_30"] = spec([dynamic(lits + [("m", 4, 11)])], OK, "zd.ml:641")
    for hd in (31, 32):
        S["hdist_%d" % hd] = spec([dynamic(lits + [("m", 5, 2)], hdist=hd)], CORRUPTED, "zd.ml:641")

    # -- the code-length code (zd.ml:624-636, 355-391).  `small`: litlen {65, 256} of length 1, no distance code
    small = dict(ll=[0] * 65 + [1] + [0] * 190 + [1], dl=[0], hlit=257, hdist=1)
    small_items = rle_items(small["ll"] + [0])
    S["codelen_all_zero"] = spec([dynamic([65], cl=[0] * 19, hclen=19, items=[("code", 0, 16)], **small)], CORRUPTED, "zd.ml:635")
    # one code of length 1 (symbol 0): the code is accepted and the block fails on its lengths (all zero) ...
    S["codelen_single_len1"] = spec([dynamic([65], cl=[1] + [0] * 18, items=[(0,)] * 258, **small)], CORRUPTED,
                                    "zd.ml:662,377-378")
    # ... and its phantom symbol (code 1) is refused where it is decoded (zd.ml:389-390, 646)
    items_ph = [(0,)] * 65 + [("code", 1, 1)] + [(0,)] * 190 + [("code", 1, 1), (0,)]
    S["codelen_single_phantom"] = spec([dynamic([65, 65], cl=[1] + [0] * 18, items=items_ph, **small)], CORRUPTED,
                                       "zd.ml:389-390,646")
    for ln in range(2, 8):
        S["codelen_single_len%d" % ln] = spec([dynamic([65], cl=[ln] + [0] * 18, items=[(0,)] * 258, **small)],
                                              CORRUPTED, "zd.ml:377-378")
    over = [0] * 19
    for s_ in (0, 1, 17, 18):
        over[s_] = 1
    S["codelen_oversubscribed"] = spec([dynamic([65], cl=over, items=small_items, **small)], CORRUPTED, "zd.ml:370")
    inc = [0] * 19
    inc[0], inc[1], inc[18] = 2, 2, 2
    S["codelen_incomplete"] = spec([dynamic([65], cl=inc, items=small_items, **small)], CORRUPTED, "zd.ml:377")
    S["codelen_incomplete_two"] = spec([dynamic([65], cl=[2, 2] + [0] * 17, items=[(0,)] * 258, **small)], CORRUPTED,
                                       "zd.ml:377")
    cl4 = [0] * 19
    cl4[16] = cl4[17] = cl4[18] = cl4[0] = 2  # HCLEN 4: lengths for 16, 17, 18 and 0 only -- every length is 0
    S["hclen_4"] = spec([dynamic([65], cl=cl4, hclen=4, items=[(18, 138), (18, 120)], **small)], CORRUPTED, "zd.ml:662")
    S["hclen_19"] = spec([dynamic(lits + [("m", 6, 3)], cl=complete_lengths(19), hclen=19)], OK, "zd.ml:624-636")
    S["hclen_19_oversubscribed"] = spec([dynamic(lits + [("m", 6, 3)], cl=[4] * 19, hclen=19)], CORRUPTED, "zd.ml:370")

    # -- code lengths (zd.ml:646-662)
    ll4 = [0] * 4 + complete_lengths(282)  # literals 0-3 have no code
    rest = rle_items(ll4[4:] + FULL_DL)
    S["cl16_first"] = spec([dynamic(lits, ll=ll4, items=[(16, 4)] + rest)], CORRUPTED, "zd.ml:653")
    S["cl16_second"] = spec([dynamic(lits + [("m", 3, 1)], ll=ll4, items=[(0,), (16, 3)] + rest)], OK, "zd.ml:653")
    # 8 codes of length 3 for litlen (0-5, EOB, 257) and for distance (0-7): a 16 copies the last litlen length into
    # the first distance lengths, a 16 ends exactly at hlit + hdist, and one past it
    ll8, dl8 = [3] * 6 + [0] * 250 + [3, 3], [3] * 8
    S["cl16_across_boundary"] = spec([dynamic([1, 2, 3, ("m", 3, 2)], ll=ll8, dl=dl8,
                                              items=rle_items(ll8[:257]) + [(16, 6), (16, 3)])], OK, "zd.ml:650-658")
    S["cl16_ends_at_hlit_hdist"] = spec([dynamic([4, 5, ("m", 3, 1)], ll=ll8, dl=dl8,
                                                 items=rle_items(ll8) + [(3,), (3,), (16, 6)])], OK, "zd.ml:659")
    S["cl16_one_past"] = spec([dynamic([4, 5], ll=ll8, dl=dl8, items=rle_items(ll8) + [(3,), (3,), (3,), (16, 6)])],
                              CORRUPTED, "zd.ml:659")
    # litlen 0-261, one distance code (0), HLIT 286, HDIST 30: the lengths end in a run of 29 zeros
    llz, dlz = complete_lengths(262) + [0] * 24, [1] + [0] * 29
    itz = rle_items(llz + dlz)
    assert itz[-1] == (18, 29), itz[-1]
    zk = dict(ll=llz, dl=dlz, hlit=286, hdist=30)
    S["cl18_ends_at_hlit_hdist"] = spec([dynamic(lits + [("m", 7, 1)], items=itz, **zk)], OK, "zd.ml:659")
    S["cl18_one_past"] = spec([dynamic(lits + [("m", 7, 1)], items=itz[:-1] + [(18, 30)], **zk)], CORRUPTED, "zd.ml:659")
    S["cl17_ends_at_hlit_hdist"] = spec([dynamic(lits + [("m", 6, 1)], items=itz[:-1] + [(17, 10), (17, 10), (17, 9)], **zk)],
                                        OK, "zd.ml:659")
    S["cl17_one_past"] = spec([dynamic(lits + [("m", 6, 1)], items=itz[:-1] + [(17, 10), (17, 10), (17, 10)], **zk)],
                              CORRUPTED, "zd.ml:659")
    # no code for the end of block, the rest of the code complete: refused at the header, before any size check
    ll_no_eob = _without(286, 1, 256)
    S["lengths256_zero"] = spec([dynamic(lits, ll=ll_no_eob, eob=False)], CORRUPTED, "zd.ml:662", at_end=True)
    S["lengths256_zero_over_limit"] = spec([dynamic(lits * 4, ll=ll_no_eob, eob=False)], CORRUPTED, "zd.ml:662",
                                           limit=10, at_end=True)

    # -- litlen and distance codes (zd.ml:355-391, 593-616)
    eob_only = dict(ll=[0] * 256 + [1], dl=[0], hlit=257, hdist=1)
    S["litlen_eob_only"] = spec([dynamic([], **eob_only)], OK, "zd.ml:377-378")
    S["litlen_eob_only_later"] = spec([fixed(lits), dynamic([], **eob_only)], OK, "zd.ml:377-378")
    S["litlen_eob_only_phantom"] = spec([dynamic([("code", 1, 1)], **eob_only)], CORRUPTED, "zd.ml:389-390,603")
    # EOB alone with a code of length 2 (refused), written as the 1-bit code a lax decoder would read
    S["litlen_single_len2"] = spec([dynamic([("code", 0, 1)], ll=[0] * 256 + [2], dl=[0], hlit=257, hdist=1, eob=False)],
                                   CORRUPTED, "zd.ml:377-378")
    ll_ab = [0] * 97 + [2, 2] + [0] * 157 + [2, 2]  # 'a', 'b', EOB, 257 (length 3)
    r = random.Random(9)
    ab_lits = [r.choice(b"ab") for _ in range(8000)]  # wrapper c's prefix in the a/b code: literals (and matches below)
    S["dist_empty_literals"] = spec([dynamic(list(b"abba"), ll=ll_ab, dl=[0], hlit=258, hdist=1)], OK, "zd.ml:377-378",
                                    wrappers="abcde", deep=ab_lits)
    S["dist_empty_match"] = spec([dynamic(list(b"abba") + [("l", 257, 0), ("code", 0, 1)], ll=ll_ab, dl=[0], hlit=258,
                                          hdist=1)], CORRUPTED, "zd.ml:607-608", wrappers="abcde", deep=ab_lits)
    for ds in (0, 3, 29):
        pre = list(b"ab") * (DBASE[ds] // 2 + 2)
        w = "abcd" if ds == 29 else "abcde"
        dl1 = [0] * ds + [1]
        # (c: 8000 symbols in front, matches at the one distance once the output reaches it)
        deep = ab_lits[:64] + [x if i % 4 or ds == 29 else ("m", 3, DBASE[ds]) for i, x in enumerate(ab_lits)]
        S["dist_single_%d_bit0" % ds] = spec([dynamic(pre + [("m", 3, DBASE[ds])], ll=ll_ab, dl=dl1)], OK,
                                             "zd.ml:377-378", wrappers=w, deep=deep)
        S["dist_single_%d_phantom" % ds] = spec([dynamic(pre + [("l", 257, 0), ("code", 1, 1), ("bits", 0, DEXT[ds])],
                                                         ll=ll_ab, dl=dl1)], CORRUPTED, "zd.ml:389-390,608", wrappers=w,
                                                deep=deep)
    S["dist_single_len2"] = spec([dynamic(list(b"abab") + [("l", 257, 0), ("code", 0, 1)], ll=ll_ab, dl=[2])], CORRUPTED,
                                 "zd.ml:377-378")
    # over-subscribed and incomplete litlen codes, written with the codes a lax decoder would read
    ll_over = [0] * 97 + [1] + [0] * 158 + [2, 2, 2]  # a: 0, EOB: 10, 257: 11 (and 258: one code too many)
    S["litlen_oversubscribed"] = spec([dynamic([("code", 0, 1), ("code", 2, 2)], ll=ll_over, dl=[0], hdist=1, eob=False)],
                                      CORRUPTED, "zd.ml:370")
    S["litlen_incomplete"] = spec([dynamic([97], ll=[0] * 97 + [1] + [0] * 158 + [2], dl=[0], hlit=257, hdist=1)],
                                  CORRUPTED, "zd.ml:377")
    S["dist_incomplete"] = spec([dynamic(list(b"abab") + [("m", 3, 2)], ll=ll_ab, dl=[1, 2])], CORRUPTED, "zd.ml:377")
    S["fixed_litlen_285"] = spec([fixed(lits + [("m", 258, 3)])], OK, "zd.ml:603", wrappers="abcde")
    for s_ in (286, 287):
        S["fixed_litlen_%d" % s_] = spec([fixed(lits + [("l", s_, 0), ("d", 0, 0)])], CORRUPTED, "zd.ml:603",
                                         wrappers="abcde")
    S["fixed_dist_29"] = spec([fixed(lits * 2300 + [("m", 3, 24577)])], OK, "zd.ml:608", wrappers="abd")
    for s_ in (30, 31):
        S["fixed_dist_%d" % s_] = spec([fixed(lits + [("l", 257, 0), ("d", s_, 0)])], CORRUPTED, "zd.ml:608",
                                       wrappers="abcde")
    S["dynamic_litlen_285"] = spec([dynamic(lits + [("m", 258, 1)])], OK, "zd.ml:603", wrappers="abcde")
    S["dynamic_dist_29"] = spec([dynamic(lits * 2400 + [("m", 5, 24580)])], OK, "zd.ml:608", wrappers="abd")

    # -- distance (zd.ml:612-614)
    for kind, blk in (("", dynamic), ("fixed_", fixed)):
        S[kind + "dist_eq_out"] = spec([blk(lits + [("m", 10, lambda o: o)])], OK, "zd.ml:614", wrappers="abcd")
        S[kind + "dist_out_plus1"] = spec([blk(lits + [("m", 10, lambda o: o + 1)])], CORRUPTED, "zd.ml:614",
                                          wrappers="abcd")
        S[kind + "match_first"] = spec([blk([("m", 3, 1)] + lits)], CORRUPTED, "zd.ml:614", wrappers="a")
    S["dist_32768_at_32767"] = spec([stored(bytes(range(256)) * 127 + bytes(255)), fixed([("m", 3, 32768)])], CORRUPTED,
                                    "zd.ml:614", wrappers="a")
    S["dist_32768_at_32768"] = spec([stored(bytes(range(256)) * 128), fixed([("m", 3, 32768), 7])], OK, "zd.ml:614")
    S["dist_32768_at_32768_dynamic"] = spec([stored(bytes(range(256)) * 128), dynamic([("m", 258, 32768), 7])], OK,
                                            "zd.ml:614")

    # -- limits and the order of errors (zd.ml:17-75, 612-616, 671-680)
    for kind, blk in (("", dynamic), ("fixed_", fixed)):
        n_body = len(lits) + 20
        S[kind + "limit_exact"] = spec([blk(lits + [("m", 20, 5)])], OK, "zd.ml:17-38", limit=n_body, wrappers="abcd")
        S[kind + "limit_one_short"] = spec([blk(lits + [("m", 20, 5)])], SIZE_EXCEEDED, "zd.ml:17-38", limit=n_body - 1,
                                           wrappers="abcd")
        S[kind + "limit_one_short_literal"] = spec([blk(lits)], SIZE_EXCEEDED, "zd.ml:17-38", limit=len(lits) - 1,
                                                   wrappers="abcd")
        S[kind + "far_match_over_limit"] = spec([blk(lits + [("m", 200, lambda o: o + 1)])], CORRUPTED,
                                                "zd.ml:614 before :63", limit=len(lits) + 10, wrappers="abcd")
        S[kind + "corrupt_before_limit"] = spec([blk(lits + [("m", 4, lambda o: o + 1)] + lits * 10)], CORRUPTED,
                                                "zd.ml:614", limit=len(lits) + 20, wrappers="abcd")
        S[kind + "corrupt_after_limit"] = spec([blk(lits * 3 + [("m", 4, lambda o: o + 1)])], SIZE_EXCEEDED, "zd.ml:63",
                                               limit=len(lits) + 20, wrappers="abcd")
    S["corrupt_after_limit_phantom"] = spec([fixed(lits * 3 + [("l", 286, 0)])], SIZE_EXCEEDED, "zd.ml:63",
                                            limit=len(lits) + 20, wrappers="abcd")
    S["limit_exact_stored"] = spec([stored(b"stored!" * 9)], OK, "zd.ml:17-38", limit=63, wrappers="abd")
    S["limit_one_short_stored"] = spec([stored(b"stored!" * 9)], SIZE_EXCEEDED, "zd.ml:17-38", limit=62, wrappers="abd")
    S["stored_short_of_input_and_limit"] = spec([fixed(lits), stored(b"abc" * 10, length=40)], CORRUPTED,
                                                "zd.ml:677 before :58", limit=len(lits) + 20, at_end=True)

    # -- truncation: the input ends inside each field (the byte that holds the field's last bit is gone)
    trunc = dynamic(lits + [("m", 11, 5), ("m", 12, 7)] + lits, dl=[0, 0, 0] + complete_lengths(27))
    for mk in ("bfinal", "hlit", "hdist", "hclen", "cl_lengths", "cl_items", "repeat_extra", "symbols", "len_code",
               "len_extra", "dist_code", "dist_extra", "eob"):
        S["truncated_in_%s" % mk] = spec([trunc], CORRUPTED, "zd.ml:564-579", cut_at=mk,
                                         wrappers="abcd" if mk in ("symbols", "len_code", "len_extra", "dist_code",
                                                                   "dist_extra", "eob") else "abd")
    S["truncated_in_fixed_symbol"] = spec([fixed(lits + [("m", 11, 5)] + lits)], CORRUPTED, "zd.ml:564-579",
                                          cut_at="len_code", wrappers="abcd")
    S["truncated_in_stored_len"] = spec([fixed(lits), stored(b"abc")], CORRUPTED, "zd.ml:564-579", cut_at="stored_len")
    # 3 + 8 * 11 + 9 * 6 + 7 = 152 bits: the end of block is the input's last bit
    S["eob_on_last_bit"] = spec([fixed(lits + [200 + i for i in range(6)])], OK, "zd.ml:564-579", at_end=True)
    return S


SPECS = _specs()
# cases where zlib and the reference part: name -> why (tests/test_oracle_pins.py holds zlib to this list)
_NO_LIMIT = "zlib has no ?decompressed_size: the stream is whole and only the limit refuses it"
ZLIB_DIFFERS = {n: _NO_LIMIT for n in (
    "limit_one_short", "limit_one_short_literal", "fixed_limit_one_short", "fixed_limit_one_short_literal",
    "limit_one_short_stored")}


def _case(s, pre=None, post=None, trailing=None):
    raw, plain, _, cuts = assemble(s.blocks, s.final_last, s.cut_at, s.trailing if trailing is None else trailing, pre,
                                   post)
    extra = len(pre[1]) if pre else 0
    limit = None if s.limit is None else s.limit + extra
    if s.status != OK:
        plain = None
    else:
        assert plain is not None
    return Case(raw, limit, s.status, plain, s.ref, cuts)


INFLATE_RULE_CASES = {n: _case(s) for n, s in SPECS.items()}


_WRAPPED = {}


def wrapped_cases(wrappers="abcde"):
    """name/wrapper -> Case, for every wrapper of `wrappers` that applies to the case (a: the case alone)"""
    if wrappers not in _WRAPPED:
        _WRAPPED[wrappers] = _wrapped_cases(wrappers)
    return _WRAPPED[wrappers]


def _wrapped_cases(wrappers):
    out = {}
    for n, s in SPECS.items():
        if "a" in wrappers:
            out[n + "/a"] = INFLATE_RULE_CASES[n]
        for wr, n9, tail in (("b", 0, b"\x00\xff\x5a"), ("d", 3, b"")):
            if wr in wrappers and wr in s.wrappers:
                # behind a valid block (b: 3 bytes after the final block unless the input's end is the point; d: the
                # case begins at another bit phase and ends with the input)
                blocks = [_prefix_block(n9)] + list(s.blocks)
                raw, plain, _, cuts = assemble(blocks, s.final_last, s.cut_at, s.trailing + (b"" if s.at_end else tail))
                pre_out = len(assemble([_prefix_block(n9)], True)[1])
                limit = None if s.limit is None else s.limit + pre_out
                out[n + "/" + wr] = Case(raw, limit, s.status, plain if s.status == OK else None, s.ref, cuts)
        if "c" in wrappers and "c" in s.wrappers:
            last = s.blocks[-1]
            deep = s.deep if s.deep is not None else _deep_syms()
            blocks = s.blocks[:-1] + [Blk(last.kind, deep + last.syms, last.opts)]
            raw, plain, _, cuts = assemble(blocks, s.final_last, s.cut_at, s.trailing)
            deep_out = len(assemble([Blk(last.kind, deep, last.opts)], True)[1])
            limit = None if s.limit is None else s.limit + deep_out
            out[n + "/c"] = Case(raw, limit, s.status, plain if s.status == OK else None, s.ref, cuts)
        if "e" in wrappers and "e" in s.wrappers and s.limit is None:
            pre, post = big_parts()
            out[n + "/e"] = _case(s, pre=pre, post=post, trailing=b"")
    return out
