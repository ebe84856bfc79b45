"""What the gzip forms (include/zipc_hip.h at zipc_hip_gzip_decompress_batch) are held to: members, files of members and
sources to compress.  Plain data and builders -- Python's zlib and struct; nothing here calls the code under test or needs a
GPU.  tests/test_gzip_rules.py (the host model) and tests/test_gpu_gzip.py (the kernels, the host forms) run what this lists.

A Case is a source range as a caller would declare it (src, all of it: src_len == len(src)), what lies behind it in the
arena (behind: never to be read), a room, a limit or None, extra flag bits.  What a case must give is NOT written with it:
want() takes the header's verdict from a second writing of RFC 1952 in Python (parse_header), the body's status and bytes
from the oracle's inflate over [hdr_len, ...), the body's extent from Python's zlib, and the CRC-32 from Python's zlib;
zlib_verdict() is zlib's own reading of the whole member (zlib.decompressobj(wbits=31): status from the map of its messages,
src_used = len - len(unused_data)), and the rule test holds the two to each other on every case but those in DIFFERS.

  flags      all 32 values of FLG & 0x1F over a body of 150 bytes, with an extra field that holds a BC subfield, a name and a
             comment where the bit asks for them, each followed by 1f 8b (src_len is an upper bound)
  cut        every proper prefix of each of those members (cut = 0 .. len - 1): ZIPC_HIP_ERR_CORRUPTED
  small      20 bytes (an empty fixed block), an empty stored block, a 1-byte output
  short      lengths 0, 9, 10 and 17
  header     each magic byte wrong, CM 7 and 0, each reserved flag bit, FHCRC off by one bit, FHCRC correct over every field
  text       a name of 65 535 bytes (OK) and of 65 536 (CORRUPTED: the library's limit, differs from zlib); a name whose zero
             is the byte at src_len - 1; a name whose zero is the byte AT src_len (not inside: CORRUPTED)
  trailer    CRC wrong, ISIZE wrong, both wrong (CHECKSUM), the trailer cut by one byte with src_len = src_used - 1
  body       220 and 65 280 bytes of output, one fixed, one stored and one dynamic final block, a body whose inflate is
             corrupted, one member of about 300 KiB of text (its source: above the 40 KiB from which the blocks path takes a stream, and long enough for its model to pick it among the short ones)
  limit      HAS_LIMIT below, at and above the length; a bad flag bit
  files      FILES: whole files for the host forms and gzip_next
  compress   SOURCES x LEVELS x FLAVOURS"""
import collections
import functools
import random
import struct
import zlib

import util

Case = collections.namedtuple("Case", "name src behind cap limit flags")
Want = collections.namedtuple("Want", "status checksum out_len src_used hdr_len flg data")

OK, CORRUPTED, SIZE_EXCEEDED, METHOD, CHECKSUM, DST_TOO_SMALL, INVALID_ARG = 0, 1, 2, 3, 6, 16, 18
FTEXT, FHCRC, FEXTRA, FNAME, FCOMMENT = 1, 2, 4, 8, 16
MAX_TEXT = 65535
MAX_STREAM_LEN = 0xFFFF0000
PLAIN, BGZF = 0, 1
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
# the cases where the library's verdict is not zlib's, and why
DIFFERS = {
    "text/name65536": "a name of more than 65 535 bytes is refused: the library's documented limit, zlib scans without bound",
    "short/len17_cm7": "src_len < 18 is judged first and nothing is read; zlib reads CM and names the method",
}


def deflate_raw(plain, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(plain) + c.flush()


def stored_raw(plain):
    assert len(plain) <= 65535
    return b"\x01" + struct.pack("<HH", len(plain), len(plain) ^ 0xFFFF) + plain


def header(flg=0, extra=b"", name=b"", comment=b"", mtime=0, xfl=0, os=255, cm=8, magic=b"\x1f\x8b", hcrc_xor=0):
    h = magic + struct.pack("<BBIBB", cm, flg, mtime, xfl, os)
    if flg & FEXTRA:
        h += struct.pack("<H", len(extra)) + extra
    if flg & FNAME:
        h += name + b"\0"
    if flg & FCOMMENT:
        h += comment + b"\0"
    if flg & FHCRC:
        h += struct.pack("<H", (zlib.crc32(h) & 0xFFFF) ^ hcrc_xor)
    return h


def member(plain, raw=None, crc=None, isize=None, **hdr):
    raw = deflate_raw(plain) if raw is None else raw
    return header(**hdr) + raw + struct.pack("<II", zlib.crc32(plain) if crc is None else crc, len(plain) & 0xFFFFFFFF if isize is None else isize)


def bc(bsize):
    return b"BC\x02\x00" + struct.pack("<H", bsize - 1)


def bgzf_member(plain, level=6, bsize_delta=0, isize_delta=0, crc=None):
    raw = deflate_raw(plain, level)
    n = 18 + len(raw) + 8
    assert n <= 65536
    return member(plain, raw, crc=crc, isize=len(plain) + isize_delta, flg=FEXTRA, extra=bc(n + bsize_delta))


def _text(n, seed):
    return util.text(n, seed)[:n]


def _letters(n, seed):
    r = random.Random(seed)
    return bytes(r.choice(b"acgt") for _ in range(n))


def flag_member(flg):
    """the member of the flags family: 150 bytes of body, the fields FLG asks for; the BC subfield says the member's length"""
    plain = _letters(150, 100 + flg)
    fields = dict(flg=flg, name=b"reads.fastq", comment=b"flags %d" % flg)
    n = len(member(plain, extra=b"XY\x03\x00abc" + bc(1), **fields))
    return member(plain, extra=b"XY\x03\x00abc" + bc(n), **fields), plain


def _case(name, src, plain_len, behind=b"", limit=None, flags=0, cap=None):
    return Case(name, src, behind, plain_len if cap is None else cap, limit, flags)


@functools.lru_cache(maxsize=None)
def flag_cases():
    return tuple(_case("flags/%02d" % f, flag_member(f)[0] + b"\x1f\x8b", 150) for f in range(32))


@functools.lru_cache(maxsize=None)
def cut_cases():
    out = []
    for f in range(32):
        m = flag_member(f)[0]
        out += [_case("cut/%02d/%d" % (f, k), m[:k], 150) for k in range(len(m))]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def long_member():
    """300 KiB of text in dynamic blocks without matches (Z_HUFFMAN_ONLY): about 180 KiB of source.  Among many short streams
    the blocks path picks a long one only where its model says that pays (forms.h size_blocks_pick): 0.8 ms fixed and
    0.36 + 0.067 ms a MiB of its source against the one wave's 13.2 ms a MiB, so from about 64 KiB of source MORE than the
    longest stream left (tests/test_gzip_rules.py asserts the inequality over this catalogue); the same text with matches
    is 45 KB of source, above the gate's 40 KiB and below what pays."""
    plain = _text(300 << 10, 21)
    m = member(plain, deflate_raw(plain, 6, zlib.Z_HUFFMAN_ONLY))
    assert len(m) > 40 << 10
    return m, plain


@functools.lru_cache(maxsize=None)
def other_cases():
    out = []
    empty_fixed = b"\x03\x00"
    out += [
        _case("small/empty_fixed", member(b"", empty_fixed), 0),
        _case("small/empty_fixed/ff5", member(b"", empty_fixed) + b"\xff" * 5, 0),
        _case("small/empty_stored", member(b"", stored_raw(b"")), 0),
        _case("small/one_byte", member(b"Z", deflate_raw(b"Z", 6, zlib.Z_FIXED)), 1),
    ]
    assert len(out[0].src) == 20
    base, plain = flag_member(0)[0], _letters(150, 100)
    for n in (0, 9, 10, 17):
        out.append(_case("short/len%d" % n, base[:n], 150))
    out.append(_case("short/len17_cm7", member(plain, cm=7)[:17], 150))
    # ---- headers refused
    out += [
        _case("header/magic0", member(plain, magic=b"\x1e\x8b"), 150),
        _case("header/magic1", member(plain, magic=b"\x1f\x8a"), 150),
        _case("header/cm7", member(plain, cm=7), 150),
        _case("header/cm0", member(plain, cm=0), 150),
        _case("header/reserved20", member(plain, flg=0x20), 150),
        _case("header/reserved40", member(plain, flg=0x40), 150),
        _case("header/reserved80", member(plain, flg=0x80), 150),
        _case("header/fhcrc_bit0", member(plain, flg=FHCRC, hcrc_xor=0x0001), 150),
        _case("header/fhcrc_bit9", member(plain, flg=FHCRC, hcrc_xor=0x0200), 150),
        _case("header/fhcrc_all_fields", member(plain, flg=31, extra=b"AB\x01\x00q", name=b"n", comment=b"c", mtime=0x12345678, xfl=2, os=3) + b"\x00" * 3, 150),
        _case("header/extra_overruns_src_len", header(flg=FEXTRA, extra=b"")[:10] + b"\x40\x00" + b"q" * 30, 150),
        _case("header/subfield_overruns_xlen", member(plain, flg=FEXTRA, extra=b"BC\x09\x00zz"), 150),
        _case("header/bc_of_slen3_is_not_bsize", member(plain, flg=FEXTRA, extra=b"BC\x03\x00zzz"), 150),
    ]
    # ---- text fields
    long_name = bytes(65 + i % 26 for i in range(MAX_TEXT + 1))
    out += [
        _case("text/name65535", member(plain, flg=FNAME, name=long_name[:MAX_TEXT]), 150),
        _case("text/name65536", member(plain, flg=FNAME, name=long_name), 150),
        _case("text/comment65535", member(plain, flg=FCOMMENT, comment=long_name[:MAX_TEXT]), 150),
    ]
    m = member(plain, flg=FNAME, name=b"a-name-that-ends-the-declared-bytes")
    zero = m.index(b"\0", 10)
    assert zero + 1 >= 18
    out += [
        _case("text/zero_at_src_len_minus_1", m[:zero + 1], 150, behind=m[zero + 1:]),
        _case("text/zero_at_src_len", m[:zero], 150, behind=m[zero:]),
    ]
    # ---- trailers
    good = member(plain)
    u = len(good) - 8
    crc = zlib.crc32(plain)
    out += [
        _case("trailer/crc_wrong", member(plain, crc=crc ^ 0x100) + b"\xff" * 9, 150),
        _case("trailer/isize_wrong", member(plain, isize=149) + b"\xff" * 9, 150),
        _case("trailer/both_wrong", member(plain, crc=crc ^ 1, isize=151) + b"\xff" * 9, 150),
        # (the right trailer stands at src_len - 8 of this one: a close that looks there passes it)
        _case("trailer/wrong_but_right_at_the_end", good[:u] + struct.pack("<II", 0x12345678, 7) + b"\0" + good[u:], 150),
        _case("trailer/cut1", good[:-1], 150, behind=good[-1:]),
        _case("trailer/cut8", good[:-8], 150, behind=good[-8:]),
    ]
    # ---- bodies
    r = random.Random(77)
    p220, p65280 = _letters(220, 5), _text(65280, 6)
    noise = bytes(r.randrange(256) for _ in range(3000))
    bad_body = bytearray(member(plain, b"\x07" + deflate_raw(plain)[1:]))  # BTYPE 3
    out += [
        _case("body/220", member(p220) + b"\x1f\x8b\x08", 220),
        _case("body/bgzf65280", bgzf_member(p65280) + BGZF_EOF, 65280),
        _case("body/fixed", member(p220, deflate_raw(p220, 6, zlib.Z_FIXED)), 220),
        _case("body/stored", member(noise, stored_raw(noise)) + b"\x00" * 4, 3000),
        _case("body/dynamic", member(_text(5000, 8)), 5000),
        _case("body/corrupted", bytes(bad_body), 150),
        _case("body/room_too_small", member(p220), 220, cap=219),
        _case("body/text300k", long_member()[0] + b"\x1f\x8b", len(long_member()[1])),
    ]
    # ---- limits, flags
    out += [
        _case("limit/below", good + b"\xff" * 3, 150, limit=149),
        _case("limit/at", good + b"\xff" * 3, 150, limit=150),
        _case("limit/above", good + b"\xff" * 3, 200, limit=200, cap=200),
        _case("limit/bad_flag", good, 150, flags=2),
    ]
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def cases():
    return flag_cases() + other_cases() + cut_cases()


def by_name(name):
    return next(c for c in cases() if c.name == name)


# ---- the references ------------------------------------------------------------------------------------------------

Header = collections.namedtuple("Header", "status hdr_len flg bsize")


def parse_header(s):
    """RFC 1952's header as include/zipc_hip.h reads it, written a second time: -> Header"""
    bad = Header(CORRUPTED, 0, 0, 0)
    n = len(s)
    if n < 18 or s[0] != 0x1F or s[1] != 0x8B:
        return bad
    if s[2] != 8:
        return Header(METHOD, 0, 0, 0)
    flg = s[3]
    if flg & 0xE0:
        return bad
    pos, bsize = 10, 0
    if flg & FEXTRA:
        if pos + 2 > n:
            return bad
        xlen = s[pos] + 256 * s[pos + 1]
        pos += 2
        if pos + xlen > n:
            return bad
        x, at = s[pos:pos + xlen], 0
        while at + 4 <= xlen:
            slen = x[at + 2] + 256 * x[at + 3]
            if at + 4 + slen > xlen:
                break
            if x[at:at + 2] == b"BC" and slen == 2:
                bsize = x[at + 4] + 256 * x[at + 5] + 1
                break
            at += 4 + slen
        pos += xlen
    for bit in (FNAME, FCOMMENT):
        if flg & bit:
            z = s.find(b"\0", pos)
            if z < 0 or z - pos > MAX_TEXT:
                return bad
            pos = z + 1
    if flg & FHCRC:
        if pos + 2 > n or s[pos] + 256 * s[pos + 1] != zlib.crc32(s[:pos]) & 0xFFFF:
            return bad
        pos += 2
    return Header(OK, pos, flg, bsize)


def extent_by_zlib(raw):
    """source bytes Python's zlib takes of a raw deflate stream (None: it refuses it or does not see its end)"""
    d = zlib.decompressobj(-15)
    try:
        d.decompress(raw)
    except zlib.error:
        return None
    return len(raw) - len(d.unused_data) if d.eof else None


ZLIB_MESSAGES = (("incorrect header check", CORRUPTED), ("unknown compression method", METHOD), ("unknown header flags set", CORRUPTED),
                 ("header crc mismatch", CORRUPTED), ("incorrect data check", CHECKSUM), ("incorrect length check", CORRUPTED))


def zlib_verdict(src):
    """zlib's own reading of one member: (status, src_used); a body zlib refuses is status None (inflate's messages are the
    oracle's to give); an unfinished member is CORRUPTED"""
    d = zlib.decompressobj(31)
    try:
        d.decompress(src)
    except zlib.error as e:
        for text, st in ZLIB_MESSAGES:
            if text in str(e):
                return st, 0
        return None, 0
    return (OK, len(src) - len(d.unused_data)) if d.eof else (CORRUPTED, 0)


def refusal(status, found=0):
    return Want(status, found, 0, 0, 0, 0, b"")


def want(oracle, c, size=False):
    """-> Want: what the decode form (size: a sizing form -- no room, no bytes, no CRC-32 compared) must give for a case"""
    if c.flags:
        return refusal(INVALID_ARG)
    h = parse_header(c.src)
    if h.status != OK:
        return refusal(h.status)
    assert c.limit is None or c.limit <= c.cap
    body = c.src[h.hdr_len:]
    st, data, _ = oracle.inflate(body, decompressed_size=c.limit)
    if st != OK:
        return refusal(st)
    if len(data) > (MAX_STREAM_LEN if size else c.cap):
        return refusal(DST_TOO_SMALL)
    u = extent_by_zlib(body)
    # (zlib does not see the body's end inside the declared bytes: a cut body whose missing bits read as the zeros behind
    # the end -- then the trailer is not inside them either)
    if u is None or h.hdr_len + u + 8 > len(c.src):
        return refusal(CORRUPTED)
    crc, isize = struct.unpack("<II", c.src[h.hdr_len + u:h.hdr_len + u + 8])
    found = zlib.crc32(data)
    if not size and crc != found:
        return refusal(CHECKSUM, found)
    if isize != len(data) & 0xFFFFFFFF:
        return refusal(CORRUPTED)
    return Want(OK, 0 if size else found, len(data), h.hdr_len + u + 8, h.hdr_len, h.flg, b"" if size else data)


# ---- files ---------------------------------------------------------------------------------------------------------

File = collections.namedtuple("File", "name data status plain src_used members runs found")


def _run_plains(n=100):
    r = random.Random(31)
    sizes = [0, 1, 65280, 65279] + [r.choice((0, 7, 300, 4096, 20000, 65280, r.randrange(65281))) for _ in range(n - 4)]
    return [_text(k, 300 + i) if i % 3 else _letters(k, 300 + i) for i, k in enumerate(sizes)]


@functools.lru_cache(maxsize=None)
def files():
    """-> (File, ...): data, and what gzip_decompress must say of it -- status, the concatenated output, where the last member
    ends, how many members, how many device batches of known-length members (runs), the CRC-32 found on a mismatch"""
    out = []
    p = [_text(700, 1), _letters(90, 2), _text(3000, 3)]
    three = member(p[0]) + member(p[1], flg=FNAME, name=b"second") + flag_member(31)[0]
    out.append(File("three_plain", three, OK, p[0] + p[1] + flag_member(31)[1], len(three), 3, 1, 0))  # (flags 31 carries a BC subfield: a run of one)
    plains = _run_plains()
    run = [bgzf_member(q) for q in plains]
    whole = b"".join(run)
    out.append(File("bgzf_run", whole + BGZF_EOF, OK, b"".join(plains), len(whole) + 28, 101, 1, 0))
    out.append(File("bgzf_run_garbage", whole + BGZF_EOF + b"garbage", OK, b"".join(plains), len(whole) + 28, 101, 1, 0))
    lying = list(run)
    lying[57] = bgzf_member(plains[57], bsize_delta=1)
    out.append(File("bgzf_bsize_lies", b"".join(lying) + BGZF_EOF, CORRUPTED, b"", 0, 0, 1, 0))
    short = list(run[:8])
    short[3] = bgzf_member(plains[3] or b"x", isize_delta=-1)
    out.append(File("bgzf_isize_small", b"".join(short) + BGZF_EOF, CORRUPTED, b"", 0, 0, 1, 0))
    bad_crc = member(p[0]) + member(p[2], crc=zlib.crc32(p[2]) ^ 0x8000)
    out.append(File("second_crc_wrong", bad_crc, CHECKSUM, b"", 0, 0, 0, zlib.crc32(p[2])))
    out.append(File("plain_then_bgzf_then_plain", member(p[1]) + whole[:len(run[0]) + len(run[1]) + len(run[2])] + member(p[2]) + b"\x00\x00", OK,
                    p[1] + plains[0] + plains[1] + plains[2] + p[2], len(member(p[1])) + len(run[0]) + len(run[1]) + len(run[2]) + len(member(p[2])), 5, 1, 0))
    out.append(File("long_member", long_member()[0], OK, long_member()[1], len(long_member()[0]), 1, 0, 0))
    out.append(File("first_member_bad_method", member(p[0], cm=7), METHOD, b"", 0, 0, 0, 0))
    out.append(File("empty_file", b"", CORRUPTED, b"", 0, 0, 0, 0))
    return tuple(out)


def file_by_name(name):
    return next(f for f in files() if f.name == name)


# ---- compress ------------------------------------------------------------------------------------------------------

LEVELS = (0, 1, 2, 3)
FLAVOURS = (PLAIN, BGZF)
SIZES = (0, 1, 65280, 65535, 65536, 200000)


@functools.lru_cache(maxsize=None)
def sources():
    r = random.Random(41)
    noise = bytes(r.randrange(256) for _ in range(max(SIZES)))
    out = []
    for n in SIZES:
        out += [("text%d" % n, _text(n, 50)), ("zeros%d" % n, bytes(n)), ("random%d" % n, noise[:n])]
    return tuple(out)


def overhead(flavour):
    return 26 if flavour == BGZF else 18


def xfl(level):
    return {3: 2, 1: 4}.get(level, 0)


def compress_header(level, flavour, member_len):
    h = b"\x1f\x8b\x08" + (b"\x04" if flavour == BGZF else b"\x00") + b"\0\0\0\0" + bytes([xfl(level), 255])
    return h + (b"\x06\x00" + bc(member_len) if flavour == BGZF else b"")


@functools.lru_cache(maxsize=None)
def compress_want(name, level, flavour, dst_cap):
    """-> (status, checksum, bytes) of compressing a source into a room of dst_cap bytes: header + the oracle's deflate bytes +
    trailer, by deflate's own capacity rule (tests/deflate_fit.py) over the room behind the header"""
    import deflate_fit as F

    data = dict(sources())[name]
    if dst_cap < overhead(flavour):
        return DST_TOO_SMALL, 0, b""
    room = min(dst_cap, 65536) if flavour == BGZF else dst_cap
    st, body, _ = F.expect(data, level, room - overhead(flavour))
    if st != OK:
        return st, 0, b""
    n = overhead(flavour) + len(body)
    return OK, zlib.crc32(data), compress_header(level, flavour, n) + body + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)
