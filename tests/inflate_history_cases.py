"""What the history forms (include/zipc_hip.h at zipc_hip_inflate_history_batch; csrc/inflate_history.h has the rule) are held
to: the smallest shapes at which a decode that starts in the middle of a stream, or with bytes in front of its output, can
go wrong.  numpy, Python's zlib and tests/token_ref.py only: nothing here calls the code under test.
tests/test_inflate_history_rules.py (the host model) and tests/test_gpu_inflate_history.py (the kernels) run what this lists;
neither may leave a case out.

A Case is a raw deflate piece: `raw` begins with the byte that holds the first block header's first bit, `start_bit` is
that bit (0..7), `hist` the bytes in front of the output, `rec` = (hist_len, start_bit) as the record says them (they
differ from len(hist) and start_bit only in the cases that pin the record's verdicts), `cap` the room, `limit` or None,
`flags_extra` stray descriptor flag bits, `dst_off` None or a destination offset the test must give the room (smaller
than hist_len), `plain` what the piece decodes to from its start point to the end of its final block (None: it has an
error in it, or its record or descriptor is refused), `status` what the all-or-nothing form reports when the room is large
enough.  What each form reports follows from these by the rule (expect_*), never from a decoder under test.

  fixed      hand-assembled fixed-Huffman blocks (zlib's encoder never emits a distance above 32 506, and never a match at
             output position 0): one match at position 0; a run of 258 at distance 1 out of the history; the distance
             exactly hist_len + produced and one more, at hist_len 1, 15, 16, 17, 32767, 32768 and produced 0, 1, 600;
             distance 32768 at position 0; runs of 1, 63, 64, 65 short far matches that read history (the queued copies);
             a dense block long enough for the span decoder, its far fetches landing in the history
  boundary   120 KB of word-like text deflated by zlib with flush(Z_BLOCK) at plain positions 1, 2, 700, 40000, 40001,
             90000, and short texts flushed at many positions until every start_bit 1..7 occurs: each block boundary (b, p)
             with reach r (how far the matches behind it reach in front of it) decoded with the history min(p, 32768), r
             and r - 1 (CORRUPTED), and with a room of the block's own length (the prefix form's cut); a stored block as
             the first block behind a non-zero start_bit
  record     hist_len 32769, start_bit 8, hist_len > dst_off, each alone, beside a flag bit and beside an over-long dst_cap
  rooms      dst_off 1..16 mod 16 (the test lays case i out at ROOM_MODS[i % 16]) with hist_len odd and even

ZCase is a whole zlib stream and the dictionary of the call it belongs to (DICTS): records of 0, 1, 50 and 5000 bytes at
levels 1 and 9 with and without the dictionary, a wrong DICTID, FDICT in 9 bytes, FDICT with no dictionary, a damaged
trailer, a body that reaches one byte beyond the dictionary.  `plain` is the record the stream was made of (None: its body
has an error in it), whatever `status` the decompress form reports; the sizing form compares no trailer and has no room."""
import collections
import functools
import random
import zlib

import token_ref
import util

OK, CORRUPTED, SIZE_EXCEEDED, ZLIB_DICT, CHECKSUM, DST_TOO_SMALL, INVALID_ARG = 0, 1, 2, 5, 6, 16, 18
MAX_STREAM_LEN = 0xFFFF0000
HIST_MAX = 32768
LETTERS = b"abcdefghijklmn"

Case = collections.namedtuple("Case", "name raw start_bit hist rec cap limit flags_extra dst_off plain status")
# seeded: the decompress form writes the dictionary in front of the stream's room (FDICT, and the open passed)
ZCase = collections.namedtuple("ZCase", "name dict raw cap plain status checksum seeded")


# ---- the rule: what each form reports of a case ----------------------------------------------------------------------

def expect_history(c):
    """zipc_hip_inflate_history_batch -> (status, out_len); the bytes are c.plain when the status is OK"""
    if c.status != OK:
        return (c.status, 0)
    n = len(c.plain)
    if c.limit is not None and n > c.limit:
        return (SIZE_EXCEEDED, 0)
    return (OK, n) if n <= c.cap else (DST_TOO_SMALL, 0)


def expect_prefix(c):
    """zipc_hip_inflate_prefix_history_batch -> (status, ended, out_len); the bytes are c.plain[:out_len]"""
    st, n = expect_history(c)
    if st == OK:
        return (OK, 1, n)
    if st == DST_TOO_SMALL:
        return (OK, 0, c.cap)
    return (st, 0, 0)


def expect_size(c):
    """zipc_hip_inflate_size_history_batch -> (status, out_len): the first form into the largest room; it has no
    destination, so neither a record whose history does not fit in front of dst_off nor an over-long dst_cap is an error
    to it (zipc_hip_inflate_size_batch looks at neither field)"""
    if c.status == INVALID_ARG and c.rec[0] <= HIST_MAX and c.rec[1] <= 7 and c.flags_extra == 0:
        return (OK, len(symbols_plain(*_RECORD_STREAM)))
    if c.status != OK:
        return (c.status, 0)
    n = len(c.plain)
    return (SIZE_EXCEEDED, 0) if c.limit is not None and n > c.limit else (OK, n)


# ---- a bit writer and the fixed codes ----------------------------------------------------------------------------------

class Bits:
    """deflate's bit order: fields least significant bit first, Huffman codes most significant bit first"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def field(self, v, nbits):
        self.acc |= v << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, v, nbits):
        self.field(int(format(v, "0%db" % nbits)[::-1], 2), nbits)

    def align(self):
        if self.n:
            self.field(0, 8 - self.n)

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def _sym_of(value, base):
    s = max(i for i, b in enumerate(base) if b <= value)
    return s, value - base[s]


def put_fixed(w, symbols, final=True):
    """one fixed block: symbols are literals (ints) and (length, distance) pairs"""
    w.field(int(final), 1)
    w.field(1, 2)
    for s in symbols:
        if isinstance(s, int):
            if s < 144:
                w.code(0x30 + s, 8)
            else:
                w.code(0x190 + s - 144, 9)
            continue
        length, dist = s
        ls, le = _sym_of(length, token_ref.LBASE)
        if ls < 23:
            w.code(ls + 1, 7)
        else:
            w.code(0xC0 + ls - 23, 8)
        w.field(le, token_ref.LEXT[ls])
        ds, de = _sym_of(dist, token_ref.DBASE)
        w.code(ds, 5)
        w.field(de, token_ref.DEXT[ds])
    w.code(0, 7)


def fixed_stream(symbols, start_bit=0):
    """-> raw: `start_bit` bits of ones, then one final fixed block"""
    w = Bits()
    w.field((1 << start_bit) - 1, start_bit)
    put_fixed(w, symbols)
    return w.bytes()


def symbols_plain(symbols, hist):
    """what the written symbols stand for behind `hist`, read serially -> bytes, or None: a distance reaches in front of the history"""
    buf = bytearray(hist)
    for s in symbols:
        if isinstance(s, int):
            buf.append(s)
            continue
        length, dist = s
        if dist > len(buf):
            return None
        for _ in range(length):
            buf.append(buf[-dist])
    return bytes(buf[len(hist):])


def _letters(r, n):
    return bytes(r.choice(LETTERS) for _ in range(n))


def _case(out, name, raw, start_bit, hist, plain, cap=None, limit=None, rec=None, flags_extra=0, dst_off=None, status=None):
    if status is None:
        status = OK if plain is not None else CORRUPTED
    if cap is None:
        cap = len(plain) if plain is not None else 4096
    out.append(Case(name, raw, start_bit, hist, rec or (len(hist), start_bit), cap, limit, flags_extra, dst_off, plain, status))


EDGE_HIST = (1, 15, 16, 17, 32767, 32768)
EDGE_PRODUCED = (0, 1, 600)
QUEUED_K = (1, 63, 64, 65)  # tests/inflate_prefix_cases.py QUEUED_K: the queue of deferred copies holds 64


@functools.lru_cache(maxsize=None)
def fixed_cases():
    out, r = [], random.Random(1951)
    big = _letters(r, HIST_MAX)

    def add(name, symbols, hist, start_bit=0, **kw):
        _case(out, "fixed/" + name, fixed_stream(symbols, start_bit), start_bit, hist, symbols_plain(symbols, hist), **kw)

    add("match_at_0", [(3, 1)], b"x")
    add("match_at_0_bit5", [(3, 1)], b"x", start_bit=5)
    add("run_258_out_of_history", [(258, 1), ord("b")], b"q")
    add("run_258_out_of_history_period3", [(258, 3), ord("b")], b"xyz")
    n_ok = n_bad = 0
    for h in EDGE_HIST:
        for p in EDGE_PRODUCED:
            lead = list(_letters(r, p))
            for more in (0, 1):
                dist = h + p + more
                if dist > HIST_MAX:  # (not a distance deflate can write)
                    if more == 0:  # the longest there is, which is legal here
                        add("dist_max/h%d_p%d" % (h, p), lead + [(5, HIST_MAX), ord("c")], big[HIST_MAX - h:])
                        n_ok += 1
                    continue
                add("dist_%s/h%d_p%d" % ("exact" if more == 0 else "one_more", h, p), lead + [(5, dist), ord("c")], big[HIST_MAX - h:],
                    cap=p + 6 + 64)
                n_ok += more == 0
                n_bad += more == 1
    assert (n_ok, n_bad) == (18, 13), (n_ok, n_bad)
    add("dist_32768_at_0", [(3, HIST_MAX)], big)
    hist = _letters(r, 700)
    for k in QUEUED_K:  # matches of 3..16 bytes, distance >= 16, every source wholly inside the history
        syms, o = [], 0
        for i in range(k):
            ln = 3 + i % 14
            dist = o + ln + 16 + (i * 31) % 200
            assert 16 <= dist <= len(hist) + o and dist - o >= ln
            syms.append((ln, dist))
            o += ln
        add("queued/k%d" % k, syms + [ord("d")], hist)
        add("queued/k%d_bit3_behind_literals" % k, list(_letters(r, 40)) + [(ln, d + 40) for ln, d in syms] + [ord("d")], hist, start_bit=3)
    # dense literals and matches, 39 KB of input: the span decoder's far fetches land in the history while it is in reach
    syms, o = [], 0
    for i in range(6000):
        syms += list(_letters(r, 4))
        o += 4
        ln = 4 + i % 9
        if o + 64 < HIST_MAX:
            dist = min(HIST_MAX, o + 1 + r.randrange(HIST_MAX - ln))  # its source begins in the history
        else:
            dist = 16 + r.randrange(HIST_MAX - 16)
        syms.append((ln, dist))
        o += ln
    add("span_dense", syms, big)
    add("span_dense_bit6", syms, big, start_bit=6)
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


# ---- boundaries of plain streams -------------------------------------------------------------------------------------

FLUSH_AT = (1, 2, 700, 40000, 40001, 90000)
TEXT_LEN = 120000
Boundary = collections.namedtuple("Boundary", "stream bit out_pos out_len reach last")


def flushed(data, cuts, level=6):
    """`data` as one raw deflate stream, a block boundary forced (Z_BLOCK: no padding, the window kept) at every cut"""
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    raw, at = b"", 0
    for cut in cuts:
        raw += co.compress(data[at:cut]) + co.flush(zlib.Z_BLOCK)
        at = cut
    return raw + co.compress(data[at:]) + co.flush()


def boundaries(raw, which):
    """the block boundaries of `raw` behind its first block, by tests/token_ref.py -> [Boundary]"""
    ref = token_ref.decode(raw)
    out = []
    for k, b in enumerate(ref.blocks[1:], 1):
        behind = ref.m_pos >= b.out_pos
        reach = int((ref.m_dist[behind] - (ref.m_pos[behind] - b.out_pos)).max()) if behind.any() else 0
        out.append(Boundary(which, b.start_bit, b.out_pos, b.out_len, max(reach, 0), k == len(ref.blocks) - 1))
    return ref.plain, out


@functools.lru_cache(maxsize=None)
def boundary_streams():
    """-> {name: (plain, raw, [Boundary])}: the long text, and short ones until every start_bit 1..7 has a boundary"""
    streams = {}
    data = util.text(TEXT_LEN, 1950)
    raw = flushed(data, FLUSH_AT)
    plain, bs = boundaries(raw, "text")
    assert plain == data and {b.out_pos for b in bs} >= set(FLUSH_AT)
    streams["text"] = (data, raw, [b for b in bs if b.out_pos in FLUSH_AT])
    seen = {b.bit & 7 for b in streams["text"][2]}
    seed = 0
    while seen != set(range(8)):
        seed += 1
        assert seed < 64
        short = util.text(3000, 2000 + seed)
        sraw = flushed(short, (500 + 13 * seed, 1700 + 7 * seed))
        _, sbs = boundaries(sraw, "short%d" % seed)
        new = [b for b in sbs if b.bit & 7 not in seen]
        if new:
            streams["short%d" % seed] = (short, sraw, new[:1])
            seen.add(new[0].bit & 7)
    return streams


def stored_behind_bit(start_bit):
    """start_bit ones, a stored block of 300 bytes (not final), a final fixed block that copies out of the stored block and
    out of the history -> (raw, symbols' reading as a function of the history)"""
    r = random.Random(77)
    data = _letters(r, 300)
    w = Bits()
    w.field((1 << start_bit) - 1, start_bit)
    w.field(0, 1)
    w.field(0, 2)
    w.align()
    w.field(300, 16)
    w.field(300 ^ 0xFFFF, 16)
    w.out += data
    tail = [(20, 150), ord("e"), (9, 321 + 40)]  # the second match begins 40 bytes in front of the piece
    put_fixed(w, tail)
    return w.bytes(), lambda hist: symbols_plain(list(data) + tail, hist)


@functools.lru_cache(maxsize=None)
def boundary_cases():
    out = []
    n_bad = 0
    for name, (data, raw, bs) in sorted(boundary_streams().items()):
        for b in bs:
            src, bit, p, rest = raw[b.bit >> 3:], b.bit & 7, b.out_pos, data[b.out_pos:]
            ident = "boundary/%s/p%d_bit%d" % (name, p, bit)
            h = min(p, HIST_MAX)
            _case(out, ident + "/h_all", src, bit, data[p - h:p], rest)
            _case(out, ident + "/h_reach", src, bit, data[p - b.reach:p], rest)
            if b.reach:
                _case(out, ident + "/h_reach_less_1", src, bit, data[p - b.reach + 1:p], None, cap=len(rest))
                n_bad += 1
            if not b.last:  # a room of the block's own length: the all-or-nothing form refuses, the prefix form cuts
                _case(out, ident + "/room_of_the_block", src, bit, data[p - h:p], rest, cap=b.out_len)
    assert n_bad >= 6, n_bad
    assert {c.start_bit for c in out} == set(range(8))
    for bit in (3, 7):
        raw, reading = stored_behind_bit(bit)
        hist = bytes(range(100, 164))
        _case(out, "boundary/stored_first_bit%d" % bit, raw, bit, hist, reading(hist))
        _case(out, "boundary/stored_first_bit%d/h_39" % bit, raw, bit, hist[-39:], reading(hist[-39:]), cap=400)
    assert out[-1].plain is None and out[-2].plain is not None
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


# ---- the record's verdicts -------------------------------------------------------------------------------------------

_RECORD_STREAM = ([ord("a"), ord("b"), (4, 2), ord("c")], b"")


@functools.lru_cache(maxsize=None)
def record_cases():
    out = []
    symbols, _ = _RECORD_STREAM
    raw, plain = fixed_stream(symbols), symbols_plain(symbols, b"")
    assert plain == b"ababab" + b"c"
    beside = (("", {}), ("_and_a_flag_bit", {"flags_extra": 2}), ("_and_a_long_dst_cap", {"cap": MAX_STREAM_LEN + 1}))
    for tail, kw in beside:
        _case(out, "record/hist_len_32769" + tail, raw, 0, b"", None, rec=(HIST_MAX + 1, 0), status=INVALID_ARG, **kw)
        _case(out, "record/start_bit_8" + tail, raw, 0, b"", None, rec=(0, 8), status=INVALID_ARG, **kw)
        _case(out, "record/hist_len_above_dst_off" + tail, raw, 0, b"", None, rec=(4, 0), dst_off=3, status=INVALID_ARG, **kw)
    _case(out, "record/a_flag_bit_alone", raw, 0, b"", None, flags_extra=1 << 31, status=INVALID_ARG)
    _case(out, "record/a_long_dst_cap_alone", raw, 0, b"", None, cap=MAX_STREAM_LEN + 1, status=INVALID_ARG)
    _case(out, "record/none_of_them", raw, 0, b"", plain)
    _case(out, "record/limit_counts_the_streams_own_bytes", raw, 0, b"0123456789", plain, limit=len(plain), cap=len(plain) + 5)
    _case(out, "record/limit_one_short", raw, 0, b"0123456789", plain, limit=len(plain) - 1, cap=len(plain) + 5)
    _case(out, "record/room_one_short", raw, 0, b"0123456789", plain, cap=len(plain) - 1)
    return tuple(out)


ROOM_MODS = tuple(range(1, 17))  # dst_off mod 16 of case i: ROOM_MODS[i % 16] (16: a multiple of 16)


@functools.lru_cache(maxsize=None)
def cases():
    """the whole catalogue of raw pieces, in the order the tests lay them out; hist_len odd and even at every dst_off mod 16"""
    out = fixed_cases() + boundary_cases() + record_cases()
    extra, r = [], random.Random(5)
    for parity in (1, 0):  # 16 consecutive cases with an odd history, then 16 with an even one: both at every alignment
        for k in range(16):
            h = 32 + 2 * k + parity
            hist = _letters(r, h)
            symbols = list(_letters(r, 3)) + [(7, h + 3), (13, h + 10), ord("z")]
            _case(extra, "rooms/%d_h%d" % (k, h), fixed_stream(symbols, k % 8), k % 8, hist, symbols_plain(symbols, hist))
    out += tuple(extra)
    assert len({c.name for c in out}) == len(out)
    return out


def by_name(name):
    return next(c for c in cases() if c.name == name)


# ---- zlib with a preset dictionary -----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def dicts():
    """name -> the dictionary of one call.  big holds bytes of every value: RFC 1950's Adler-32 of it and the signed-remainder
    one of the library's other flavour differ (checked by tests/test_inflate_history_rules.py against the oracle)"""
    r = random.Random(1950)
    words = util.text(HIST_MAX - 8192, 11)
    big = bytes(r.randrange(200, 256) for _ in range(8192)) + words
    reach = b"QWERTYUIOPASDFGHJKLZXCVBNM0123456789" + util.text(200, 13)  # (its first 36 bytes occur once)
    return {"none": b"", "one": b"a", "mid": util.text(257, 12), "big": big, "reach": reach, "exact": reach[1:], "short": reach[2:]}


RECORD_SIZES = (0, 1, 50, 5000)


def zdeflate(plain, level, zdict=None):
    co = zlib.compressobj(level, zlib.DEFLATED, 15, zdict=zdict) if zdict else zlib.compressobj(level, zlib.DEFLATED, 15)
    return co.compress(plain) + co.flush()


def _record(d, size, seed):
    """a record that shares text with the dictionary: its matches reach into it"""
    r = random.Random(seed)
    out = bytearray()
    while len(out) < size:
        if len(d) > 1 and r.random() < 0.7:
            at = r.randrange(len(d))
            out += d[at:at + r.randrange(3, 40)]
        else:
            out += (d[:1] or b"a") * r.randrange(1, 6) if len(d) <= 1 else r.choice(util.WORDS)
    return bytes(out[:size])


@functools.lru_cache(maxsize=None)
def zcases():
    out = []
    D = dicts()

    def add(name, dname, raw, plain, status=OK, checksum=None, cap=None, seeded=None):
        if checksum is None:
            checksum = zlib.adler32(plain) if status == OK else 0
        out.append(ZCase("zlib/%s/%s" % (dname, name), dname, raw, len(plain) + 16 if cap is None else cap, plain,
                         status, checksum, bool(raw[1] & 0x20) and status in (OK, CHECKSUM, DST_TOO_SMALL) if seeded is None else seeded))

    for dname in ("one", "mid", "big"):
        d = D[dname]
        for size in RECORD_SIZES:
            rec = _record(d, size, size + len(d))
            for level in (1, 9):
                add("rec%d_l%d_dict" % (size, level), dname, zdeflate(rec, level, d), rec)
                add("rec%d_l%d_plain" % (size, level), dname, zdeflate(rec, level), rec)
    rec = _record(D["mid"], 50, 3)
    made_with_big = zdeflate(rec, 9, D["big"])
    add("wrong_dictid", "mid", made_with_big, rec, status=ZLIB_DICT, checksum=zlib.adler32(D["big"]))
    good = zdeflate(rec, 9, D["mid"])
    add("fdict_in_9_bytes", "mid", good[:9], rec, status=CORRUPTED)
    add("fdict_in_10_bytes", "mid", good[:6] + good[-4:], rec, status=CORRUPTED, seeded=True)  # (an empty body: no block header)
    # two bytes cut off the end: the last four bytes are still taken for the trailer, so the body [6, len - 4) ends two bytes early
    add("fdict_two_bytes_short", "mid", good[:-2], rec, status=CORRUPTED, seeded=True)
    add("damaged_trailer", "mid", good[:-1] + bytes([good[-1] ^ 1]), rec, status=CHECKSUM, checksum=zlib.adler32(rec))
    add("room_one_short", "mid", good, rec, status=DST_TOO_SMALL, cap=len(rec) - 1)
    # a body that reaches one byte beyond the dictionary: made with `reach` (zlib never copies a window's first byte, so the
    # text begins at its second), decoded with `exact` = reach[1:], whose first byte it copies, and with `short` = reach[2:],
    # the DICTID made to fit each time
    text = D["reach"][1:37] + b"#"
    reaching = zdeflate(text, 9, D["reach"])
    refit = lambda d: reaching[:2] + zlib.adler32(d).to_bytes(4, "big") + reaching[6:]
    _check_reaches_the_first_byte(refit(D["exact"]), D["exact"], refit(D["short"]), D["short"], text)
    add("reaches_the_first_byte", "exact", refit(D["exact"]), text)
    out.append(ZCase("zlib/short/reaches_one_byte_beyond", "short", refit(D["short"]), len(text) + 16, None, CORRUPTED, 0, True))
    # no dictionary at all: a stream with FDICT asks for one, a stream without decodes
    add("fdict_without_a_dictionary", "none", good, rec, status=ZLIB_DICT, checksum=zlib.adler32(D["mid"]))
    add("plain_without_a_dictionary", "none", zdeflate(rec, 6), rec)
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def _check_reaches_the_first_byte(stream, d, stream_short, d_short, text):
    """what `reaches_one_byte_beyond` relies on, by zlib: against `d` the stream is `text`; against d_short, one byte less, it
    reaches too far"""
    assert zlib.decompressobj(15, zdict=d).decompress(stream) == text
    try:
        zlib.decompressobj(15, zdict=d_short).decompress(stream_short)
    except zlib.error as e:
        assert "distance too far back" in str(e), e
    else:
        raise AssertionError("the stream does not reach the dictionary's first byte")


def zdict_of(zc):
    return dicts()[zc.dict]


ZDICT_CALLS = ("one", "mid", "big", "exact", "short", "none")  # the calls of the dictionary forms: one dictionary each
