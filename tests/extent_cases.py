"""What the extent forms (include/zipc_hip.h at zipc_hip_inflate_extent_batch) are held to: streams whose source range is
only an upper bound, and for each the count of source bytes it takes.  Plain data and builders -- numpy, Python's zlib,
the block writers of tests/golden/inflate_rules.py; nothing here calls the code under test or needs a GPU.
tests/test_inflate_extent_rules.py (the two CPU references, the host model) and tests/test_gpu_inflate_extent.py (the
kernels) run what this lists.

A Stream is a valid raw deflate stream and nothing else: its extent is len(raw).  A Case is a source range as a caller
would declare it (src, all of it: src_len == len(src)), a room, a limit or None, extra flag bits, and whether the range
holds a zlib stream.  What a case must give is NOT written here: status, length and bytes are the oracle's for the same
range, the extent comes from the two references (extent_by_zlib here, token_ref in the rule test).

  basic      streams made by zlib, fixed and dynamic blocks, 0 .. 400 bytes of a four-letter alphabet: every residue of
             end_bit mod 8 and ends on 32-bit word boundaries (the rule test asserts that coverage)
  hand       an empty fixed block (10 bits), a final stored block of LEN 0, 1 and 65535, a stored block behind a compressed
             one (pad bits), three blocks of mixed kinds
  golden     the streams of tests/golden/zlib_streams.json
  span       about 48 KiB of text in one dynamic block, and one of long runs: streams the span decoder and the wide turns take
  long       two streams of 512 KiB of text, for the blocks forms
Trailing input of 0, 1, 3, 4, 5 and 4096 bytes in four flavours (zeros, 0xFF, a second whole stream, bytes that read as a
valid block header) behind every short stream; a few of them behind the long ones.
  cut        src_len := extent - 1: whatever the oracle says of the cut stream
  refuse     a corrupted header, a distance beyond the output, a limit exceeded, a room too small, an empty source, a bad flag bit
  zlib       the same bodies wrapped; a wrong Adler-32; the trailer cut off by src_len by 1 .. 4 bytes; src_len 0 .. 5; each of the
             reference's header failures; two zlib streams back to back"""
import collections
import functools
import random
import struct
import sys
import zlib

import util

sys.path.insert(0, util.GOLDEN)
import inflate_rules as R  # noqa: E402

Stream = collections.namedtuple("Stream", "name raw plain")
Case = collections.namedtuple("Case", "name src cap limit flags zlib")

TRAIL_LENS = (0, 1, 3, 4, 5, 4096)
FLAVOURS = ("zeros", "ff", "second", "header")
LONG = 512 << 10


def extent_by_zlib(src, wrapped=False):
    """the second CPU reference: source bytes Python's zlib takes of `src` for one stream (None: it refuses the stream)"""
    d = zlib.decompressobj() if wrapped else zlib.decompressobj(-15)
    try:
        d.decompress(src)
    except zlib.error:
        return None
    return len(src) - len(d.unused_data) if d.eof else None


def deflate_raw(plain, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(plain) + c.flush()


def _letters(r, n):
    return bytes(r.choice(b"acgt") for _ in range(n))


def _text(n, seed):
    return util.text(n, seed)[:n]


@functools.lru_cache(maxsize=None)
def basic():
    """zlib's own streams: every length 0 .. 400 of the four letters, fixed (Z_FIXED) and dynamic in turn"""
    r, out = random.Random(5), []
    for n in range(0, 401):
        fixed = n % 2 == 0
        plain = _letters(r, n)
        out.append(Stream("basic/%s%d" % ("fixed" if fixed else "dynamic", n), deflate_raw(plain, 6, zlib.Z_FIXED if fixed else zlib.Z_DEFAULT_STRATEGY), plain))
    return tuple(out)


def _assembled(name, blocks):
    raw, plain, _, _ = R.assemble(blocks)
    assert plain is not None
    return Stream(name, raw, plain)


@functools.lru_cache(maxsize=None)
def hand():
    r = random.Random(9)
    lits = lambda n: list(_letters(r, n))
    return (
        _assembled("hand/empty_fixed", [R.fixed([])]),
        _assembled("hand/stored_len0", [R.stored(b"")]),
        _assembled("hand/stored_len1", [R.stored(b"Z")]),
        _assembled("hand/stored_len65535", [R.stored(bytes(r.randrange(64) for _ in range(65535)))]),
        _assembled("hand/fixed_then_stored", [R.fixed(lits(5)), R.stored(b"pad bits in front")]),
        _assembled("hand/fixed_then_stored_len0", [R.fixed(lits(6)), R.stored(b"")]),
        _assembled("hand/three_kinds", [R.stored(b"first, stored"), R.fixed(lits(40) + [("m", 20, 7)]), R.dynamic(lits(300) + [("m", 258, 100)])]),
        _assembled("hand/three_kinds_stored_last", [R.dynamic(lits(200)), R.fixed(lits(3)), R.stored(b"the last block is stored")]),
    )


@functools.lru_cache(maxsize=None)
def golden():
    out = []
    for s in util.zlib_streams():
        raw = s["raw"]
        if extent_by_zlib(raw) is None:  # (a whole zlib stream: its body)
            raw = raw[2:-4]
        out.append(Stream("golden/" + s["name"], raw, zlib.decompress(raw, -15)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def span():
    """One dynamic block each.  The stream's wave tries the span decoder in PH_SYMBOLS while d.span_off == 0 and d.in_word >=
    d.span_retry_word (inflate.hip), and span_decode (inflate_span.h) runs when the input ahead, SPAN_TAIL_WORDS kept
    clear, holds SPAN_MIN_LANES regions of SPAN_K_MIN granules of SPAN_G bits -- n_lanes = TG / SPAN_K_MIN >=
    SPAN_MIN_LANES: 8 * 4 * 256 bits, 1 KiB of input -- and hard_cap >= 8.  48 KiB of text deflates to 7.5 KB in one block:
    the span decoder takes it, and its last KiB goes to the wide turns and lane_one_symbol.  The stream of runs is 601
    bytes of input for 300 KB of output, below that gate (SPAN_NONE, span_off): the wide turns, the wave's match copies
    and lane_one_symbol take all of it."""
    text = _text(48 << 10, 3)
    runs = b"".join(bytes([65 + i % 26]) * (300 + 37 * i) for i in range(120))
    return (Stream("span/text48k", deflate_raw(text, 6), text), Stream("span/runs", deflate_raw(runs, 6), runs))


@functools.lru_cache(maxsize=None)
def long_streams():
    return tuple(Stream("long/text%d" % k, deflate_raw(_text(LONG, 11 + k), 6), _text(LONG, 11 + k)) for k in range(2))


def short_streams():
    return basic() + hand() + golden()


HEADER_LIKE = bytes([0x05]) + b"\x00\x00\xff\xff" + bytes([0x03, 0x00])  # a stored block's header, then a final empty fixed block


def trailing(flavour, n, second):
    """n bytes of trailing input of a flavour; `second`: a whole other stream to stand behind the first"""
    if flavour == "zeros":
        return bytes(n)
    if flavour == "ff":
        return b"\xff" * n
    if flavour == "second":
        return (second + bytes(n))[:n] if n < len(second) else second + bytes(n - len(second))
    assert flavour == "header"
    return (HEADER_LIKE * (n // len(HEADER_LIKE) + 1))[:n]


def _trailed(s, i, lens=TRAIL_LENS, flavours=FLAVOURS):
    """the stream with every trailing length in every flavour (length 0 once)"""
    second = short_streams()[(7 * i + 3) % len(short_streams())].raw
    out = [Case(s.name + "/exact", s.raw, len(s.plain), None, 0, False)]
    for n in lens:
        for fl in flavours:
            if n:
                out.append(Case("%s/%s%d" % (s.name, fl, n), s.raw + trailing(fl, n, second), len(s.plain), None, 0, False))
    return out


def wrap(raw, plain, adler=None):
    return b"\x78\x9c" + raw + struct.pack(">I", zlib.adler32(plain) if adler is None else adler)


@functools.lru_cache(maxsize=None)
def raw_cases():
    out = []
    for i, s in enumerate(short_streams()):
        # every stream exact and with 5 bytes of 0xFF; every fourth with the whole table of lengths and flavours
        out += _trailed(s, i) if i % 4 == 0 or s.name.startswith("hand/") else _trailed(s, i, (5,), ("ff",))
        if len(s.raw) > 1:
            out.append(Case(s.name + "/cut1", s.raw[:-1], len(s.plain), None, 0, False))
    for i, s in enumerate(span()):
        out += _trailed(s, i, (3, 4096), ("ff", "second"))
    # ---- refusals: no extent
    r = random.Random(13)
    lits = lambda n: list(_letters(r, n))
    far, far_plain, _, _ = R.assemble([R.fixed(lits(10) + [("m", 8, 11)] + lits(3))])
    assert far_plain is None
    bt3, _, _, _ = R.assemble([R.btype3(lits(4))])
    ok = basic()[300]
    out += [
        Case("refuse/btype3", bt3 + b"\xff" * 5, 64, None, 0, False),
        Case("refuse/far_distance", far + b"\xff" * 5, 64, None, 0, False),
        Case("refuse/limit_exceeded", ok.raw + b"\xff" * 5, len(ok.plain), len(ok.plain) - 1, 0, False),
        Case("refuse/limit_exact", ok.raw + b"\xff" * 5, len(ok.plain), len(ok.plain), 0, False),
        Case("refuse/room_too_small", ok.raw + b"\xff" * 5, len(ok.plain) - 1, None, 0, False),
        Case("refuse/empty_source", b"", 64, None, 0, False),
        Case("refuse/bad_flag", ok.raw, len(ok.plain), None, 2, False),
        Case("refuse/done_flag", ok.raw, len(ok.plain), None, 1 << 31, False),
    ]
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def zlib_cases():
    out = []
    bodies = basic()[::5] + hand() + golden()[::4] + span()
    for i, s in enumerate(bodies):
        z = wrap(s.raw, s.plain)
        second = wrap(*short_streams()[(11 * i + 2) % len(short_streams())][1:])
        name = "zlib/" + s.name
        out.append(Case(name + "/exact", z, len(s.plain), None, 0, True))
        for n, fl in ((1, "zeros"), (3, "ff"), (4, "header"), (5, "ff"), (4096, "second")):
            out.append(Case("%s/%s%d" % (name, fl, n), z + trailing(fl, n, second), len(s.plain), None, 0, True))
    s = basic()[301]
    z = wrap(s.raw, s.plain)
    out.append(Case("zlib/wrong_adler", wrap(s.raw, s.plain, zlib.adler32(s.plain) ^ 0x100) + b"\xff" * 9, len(s.plain), None, 0, True))
    # (the right Adler-32 stands at src_len - 4 of this one: a close that looks there passes it)
    out.append(Case("zlib/wrong_adler_right_one_at_the_end", wrap(s.raw, s.plain, 0x12345678) + b"\x00" + struct.pack(">I", zlib.adler32(s.plain)),
                    len(s.plain), None, 0, True))
    for k in (1, 2, 3, 4):
        out.append(Case("zlib/trailer_cut%d" % k, z[:-k], len(s.plain), None, 0, True))
    for n in range(6):
        out.append(Case("zlib/src_len%d" % n, z[:n], len(s.plain), None, 0, True))
    body = s.raw + struct.pack(">I", zlib.adler32(s.plain)) + b"\xff" * 3
    for what, hdr in (("fcheck", b"\x78\x9d"), ("method", b"\x77\x09"), ("window", b"\x88\x1c"), ("dict", b"\x78\xbb")):
        out.append(Case("zlib/header_" + what, hdr + body, len(s.plain), None, 0, True))
    out.append(Case("zlib/limit_exceeded", z + b"\xff" * 5, len(s.plain), len(s.plain) - 1, 0, True))
    out.append(Case("zlib/bad_flag", z, len(s.plain), None, 2, True))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def back_to_back(n=5):
    """n zlib streams stored end to end, and the plain bytes of each: the recipe's input"""
    picks = [short_streams()[(37 * k + 5) % len(short_streams())] for k in range(n)]
    return b"".join(wrap(s.raw, s.plain) for s in picks), [s.plain for s in picks]


def by_name(name):
    return next(c for c in raw_cases() + zlib_cases() if c.name == name)


# ---- what a case must give, from the oracle and a reference extent (never from the code under test) ----------------

OK, CORRUPTED, SIZE_EXCEEDED, CHECKSUM, DST_TOO_SMALL, INVALID_ARG = 0, 1, 2, 6, 16, 18


def _raw_want(oracle, src, cap, limit, extent_of):
    """(status, out_len, extent, plain) of a raw range in a room of `cap` bytes: the oracle's verdict under the limit, then
    the room (the cases keep the two apart: a limit is never above the room)"""
    assert limit is None or limit <= cap
    st, data, _ = oracle.inflate(src, decompressed_size=limit)
    if st != OK:
        return (st, 0, 0, b"")
    if len(data) > cap:
        return (DST_TOO_SMALL, 0, 0, b"")
    return (OK, len(data), extent_of(src), data)


def want(oracle, c, size=False, extent_of=extent_by_zlib):
    """-> (status, checksum or None, out_len, src_used, bytes).  checksum: the Adler-32 a zlib decode form reports, None for
    a raw form (whose checksum is the caller's crc_op over the bytes).  size: a sizing form -- no room, no bytes, no
    checksum compared."""
    cap = 0xFFFF0000 if size else c.cap
    if c.flags:
        return (INVALID_ARG, 0 if c.zlib else None, 0, 0, b"")
    if not c.zlib:
        st, n, u, data = _raw_want(oracle, c.src, cap, c.limit, extent_of)
        return (st, None, n, u, b"" if size else data)
    n_src = len(c.src)
    pre = open_status(c.src)
    if pre != OK:
        return (pre, 0, 0, 0, b"")
    st, n, u, data = _raw_want(oracle, c.src[2:n_src - 2], cap, c.limit, extent_of)
    if st != OK:
        return (st, 0, 0, 0, b"")
    if 2 + u + 4 > n_src:
        return (CORRUPTED, 0, 0, 0, b"")
    found = oracle.adler32(data)
    if size:
        return (OK, 0, n, u + 6, b"")
    if struct.unpack(">I", c.src[2 + u:2 + u + 4])[0] != found:
        return (CHECKSUM, found, 0, 0, b"")
    return (OK, found, n, u + 6, data)


def open_status(z):
    """RFC 1950's two bytes as the reference judges them, in its order (zd.ml:723-730)"""
    if len(z) < 6 or (256 * z[0] + z[1]) % 31:
        return CORRUPTED
    if z[0] & 0x0F != 8:
        return 3
    if z[0] >> 4 > 7:
        return 4
    if z[1] & 0x20:
        return 5
    return OK
