"""Host-side mirror of the reference's module ``Zipc_deflate`` (src/zipc_deflate.mli).

Same names, argument meaning and error behaviour as the OCaml signature; every
function runs on the GPU through the C ABI of include/zipc_hip.h (host forms).
OCaml's ``result`` is mirrored by :class:`Ok` / :class:`Error` so the parity tests
read like the reference's own (``test/test.ml``):

    cs = zipc_deflate.deflate(s, level="fast").get_ok()
    assert zipc_deflate.inflate(cs).get_ok() == s

Reference quirks kept on purpose: the default ``level`` is
``"best"`` (zipc_deflate.ml:817, although the .mli says `Default); Adler-32 uses
the reference's signed 32-bit remainder.  ``start``/``len`` select the byte range
like ``?start ?len``; for ``deflate`` and ``zlib_*`` the reference mis-handles
``start <> 0`` (Q4/Q5), so here the range is simply sliced first.
"""
from __future__ import annotations

import ctypes as C

from . import _lib
from ._lib import (CRC_ADLER32, CRC_CRC32, CRC_NOP, ERR_CHECKSUM, ERR_DST_TOO_SMALL,
                   ERR_ZLIB_METHOD, OK, default_context, lib)

LEVELS = {"none": 0, "fast": 1, "default": 2, "best": 3,
          "None": 0, "Fast": 1, "Default": 2, "Best": 3}


class Ok:
    __slots__ = ("value",)

    def __init__(self, value):
        self.value = value

    def get_ok(self):
        return self.value

    def is_ok(self):
        return True

    def is_error(self):
        return False

    def __repr__(self):
        return "Ok(%r)" % (self.value,)


class Error:
    __slots__ = ("error",)

    def __init__(self, error):
        self.error = error

    def get_ok(self):
        raise ValueError("Result.get_ok on Error %r" % (self.error,))

    def is_ok(self):
        return False

    def is_error(self):
        return True

    def __repr__(self):
        return "Error(%r)" % (self.error,)


def _range(s, start, length):
    """default_length (zipc_deflate.ml:9-10) + OCaml's bounds checks."""
    s = bytes(s) if not isinstance(s, bytes) else s
    n = len(s) - start if length is None else length
    if start < 0 or n < 0 or start + n > len(s):
        raise ValueError("index out of bounds")  # Invalid_argument in the reference
    return s[start:start + n] if (start or n != len(s)) else s


def _message(status, detail=None):
    msg = lib().zipc_hip_strerror(status).decode()
    if status == ERR_ZLIB_METHOD and detail is not None:
        msg = msg % detail
    return msg


def crc_error(expect, found):
    # crc_error zipc_deflate.ml:103-104 (the unbalanced parenthesis is the reference's)
    return "Checksum mismatch, expected %x found %x)" % (expect, found)


class _Checksum:
    @staticmethod
    def equal(a, b):
        return (a & 0xFFFFFFFF) == (b & 0xFFFFFFFF)

    @classmethod
    def check(cls, expect, found):
        return Ok(None) if cls.equal(expect, found) else Error(crc_error(expect, found))

    @staticmethod
    def pp(crc):
        return "%x" % (crc & 0xFFFFFFFF)


class Crc_32(_Checksum):
    """ZIP CRC-32 checksums (zipc_deflate.mli:24-49)."""

    @staticmethod
    def string(s, start=0, len=None, ctx=None):
        data = _range(s, start, len)
        ctx = ctx or default_context()
        out = C.c_uint32()
        ctx.check(lib().zipc_hip_crc32(ctx.handle, data, data.__len__(), C.byref(out)))
        return out.value


class Adler_32(_Checksum):
    """Adler-32 checksums (zipc_deflate.mli:52-75)."""

    @staticmethod
    def string(s, start=0, len=None, ctx=None):
        data = _range(s, start, len)
        ctx = ctx or default_context()
        out = C.c_uint32()
        ctx.check(lib().zipc_hip_adler32(ctx.handle, data, data.__len__(), C.byref(out)))
        return out.value


def _inflate(s, decompressed_size, start, length, crc_op, ctx):
    data = _range(s, start, length)
    ctx = ctx or default_context()
    n = len(data)
    has_limit = decompressed_size is not None
    # without a limit the reference starts at 3x the input and doubles
    # (zipc_deflate.ml:553, Buf.grow :27-38); same policy for the device buffer
    cap = decompressed_size if has_limit else max(3 * n, 1024)
    if not has_limit and n >= _lib.BLOCKS_MIN_SRC:
        # a long stream is sized first (by a wave per block: less than decoding it costs) and decoded once at its exact
        # size.  A status other than OK is the answer: it is by definition what zipc_hip_inflate would say.  (A stream
        # beyond the longest the sizing forms take is left to the loop.)
        size = C.c_size_t()
        st = lib().zipc_hip_inflate_size(ctx.handle, data, n, 0, 0, C.byref(size))
        if st == OK:
            cap = size.value
        elif st != ERR_DST_TOO_SMALL:
            if st in (_lib.ERR_HIP, _lib.ERR_INVALID_ARG, _lib.ERR_NO_DEVICE, _lib.ERR_NOMEM):
                ctx.check(st)
            return Error(_message(st))
    while True:
        dst = C.create_string_buffer(max(cap, 1))
        out_len, crc = C.c_size_t(), C.c_uint32()
        st = lib().zipc_hip_inflate(ctx.handle, data, n, int(has_limit), decompressed_size or 0,
                                    crc_op, dst, cap, C.byref(out_len), C.byref(crc))
        if st == ERR_DST_TOO_SMALL and not has_limit:
            cap *= 2
            continue
        if st == OK:
            return Ok((dst.raw[:out_len.value], crc.value))
        if st in (_lib.ERR_HIP, _lib.ERR_INVALID_ARG, _lib.ERR_NO_DEVICE, _lib.ERR_NOMEM):
            ctx.check(st)
        return Error(_message(st))


def inflate(s, decompressed_size=None, start=0, len=None, ctx=None):
    """zipc_deflate.mli:79-91"""
    r = _inflate(s, decompressed_size, start, len, CRC_NOP, ctx)
    return Ok(r.value[0]) if r.is_ok() else r


def inflate_size(s, decompressed_size=None, start=0, len=None, ctx=None):
    """What `inflate` of the same arguments would hand back, without the bytes: Ok (decompressed length) | Error msg.  The
    stream is walked on the device with every check of inflate and nothing is stored (zipc_hip_inflate_size); the
    reference has no such value -- it is what its `inflate` without ?decompressed_size finds out by growing a buffer."""
    data = _range(s, start, len)
    ctx = ctx or default_context()
    has_limit = decompressed_size is not None
    out_len = C.c_size_t()
    st = lib().zipc_hip_inflate_size(ctx.handle, data, data.__len__(), int(has_limit), decompressed_size or 0, C.byref(out_len))
    if st == OK:
        return Ok(out_len.value)
    if st in (_lib.ERR_HIP, _lib.ERR_INVALID_ARG, _lib.ERR_NO_DEVICE, _lib.ERR_NOMEM):
        ctx.check(st)
    return Error(_message(st))


def inflate_and_crc_32(s, decompressed_size=None, start=0, len=None, ctx=None):
    """zipc_deflate.mli:93-97"""
    return _inflate(s, decompressed_size, start, len, CRC_CRC32, ctx)


def inflate_and_adler_32(s, decompressed_size=None, start=0, len=None, ctx=None):
    """zipc_deflate.mli:99-103"""
    return _inflate(s, decompressed_size, start, len, CRC_ADLER32, ctx)


def zlib_decompress(s, decompressed_size=None, start=0, len=None, ctx=None):
    """zipc_deflate.mli:104-118: Ok (bytes, adler) | Error ((expect, found) | None, msg)"""
    data = _range(s, start, len)
    ctx = ctx or default_context()
    n = data.__len__()
    has_limit = decompressed_size is not None
    cap = decompressed_size if has_limit else max(3 * n, 1024)
    while True:
        dst = C.create_string_buffer(max(cap, 1))
        out_len = C.c_size_t()
        adler, expect, found = C.c_uint32(), C.c_uint32(), C.c_uint32()
        st = lib().zipc_hip_zlib_decompress(ctx.handle, data, n, int(has_limit),
                                            decompressed_size or 0, dst, cap, C.byref(out_len),
                                            C.byref(adler), C.byref(expect), C.byref(found))
        if st == ERR_DST_TOO_SMALL and not has_limit:
            cap *= 2
            continue
        if st == OK:
            return Ok((dst.raw[:out_len.value], adler.value))
        if st == ERR_CHECKSUM:
            return Error(((expect.value, found.value), crc_error(expect.value, found.value)))
        if st in (_lib.ERR_HIP, _lib.ERR_INVALID_ARG, _lib.ERR_NO_DEVICE, _lib.ERR_NOMEM):
            ctx.check(st)
        return Error((None, _message(st, data[0] & 0x0F if n else 0)))


def _extent(zlib, s, decompressed_size, start, length, crc_op, ctx):
    data = _range(s, start, length)
    ctx = ctx or default_context()
    n = data.__len__()
    has_limit = decompressed_size is not None
    cap = decompressed_size if has_limit else max(3 * n, 1024)
    while True:
        dst = C.create_string_buffer(max(cap, 1))
        out_len, used, crc = C.c_size_t(), C.c_size_t(), C.c_uint32()
        if zlib:
            st = lib().zipc_hip_zlib_decompress_extent(ctx.handle, data, n, int(has_limit), decompressed_size or 0, dst, cap,
                                                       C.byref(out_len), C.byref(used), C.byref(crc))
        else:
            st = lib().zipc_hip_inflate_extent(ctx.handle, data, n, int(has_limit), decompressed_size or 0, dst, cap, crc_op,
                                               C.byref(out_len), C.byref(used), C.byref(crc))
        if st == ERR_DST_TOO_SMALL and not has_limit:
            cap *= 2
            continue
        if st == OK:
            return Ok((dst.raw[:out_len.value], used.value, crc.value))
        if st in (_lib.ERR_HIP, _lib.ERR_INVALID_ARG, _lib.ERR_NO_DEVICE, _lib.ERR_NOMEM):
            ctx.check(st)
        return Error(_message(st, data[0] & 0x0F if n else 0) if zlib else _message(st))


def inflate_extent(s, decompressed_size=None, start=0, len=None, ctx=None):
    """An addition the reference's signature does not have: `inflate` of a stream whose compressed length is not known.
    The range (?start ?len, checked as ever) is an upper bound of the stream; Ok (bytes, used) | Error msg, `used` the
    count of source bytes from `start` that the stream took (zipc_hip_inflate_extent).  The next stream of a run stored
    back to back begins at start + used."""
    r = _extent(False, s, decompressed_size, start, len, CRC_NOP, ctx)
    return Ok(r.value[:2]) if r.is_ok() else r


def zlib_decompress_extent(s, decompressed_size=None, start=0, len=None, ctx=None):
    """The same for a zlib stream (an addition, too): Ok (bytes, used) | Error msg, `used` counting the two header bytes
    and the Adler-32, which is found behind the deflate stream's own end and compared (zipc_hip_zlib_decompress_extent)."""
    r = _extent(True, s, decompressed_size, start, len, CRC_NOP, ctx)
    return Ok(r.value[:2]) if r.is_ok() else r


def _level(level):
    if level is None:
        return LEVELS["best"]  # make_encoder ?(level = `Best) zipc_deflate.ml:817
    if isinstance(level, int):
        return level
    return LEVELS[level]


def _deflate(s, level, start, length, crc_op, ctx):
    data = _range(s, start, length)
    ctx = ctx or default_context()
    n = data.__len__()
    cap = lib().zipc_hip_deflate_bound(n)
    dst = C.create_string_buffer(cap)
    out_len, crc = C.c_size_t(), C.c_uint32()
    st = lib().zipc_hip_deflate(ctx.handle, data, n, _level(level), crc_op, dst, cap,
                                C.byref(out_len), C.byref(crc))
    if st != OK:
        ctx.check(st)
    return Ok((crc.value, dst.raw[:out_len.value]))


def deflate(s, level=None, start=0, len=None, ctx=None):
    """zipc_deflate.mli:128-137"""
    return Ok(_deflate(s, level, start, len, CRC_NOP, ctx).value[1])


def crc_32_and_deflate(s, level=None, start=0, len=None, ctx=None):
    """zipc_deflate.mli:139-143: Ok (crc, bytes)"""
    return _deflate(s, level, start, len, CRC_CRC32, ctx)


def adler_32_and_deflate(s, level=None, start=0, len=None, ctx=None):
    """zipc_deflate.mli:145-149: Ok (adler, bytes)"""
    return _deflate(s, level, start, len, CRC_ADLER32, ctx)


def zlib_compress(s, level=None, start=0, len=None, ctx=None):
    """zipc_deflate.mli:152-162: Ok (adler, bytes)"""
    data = _range(s, start, len)
    ctx = ctx or default_context()
    n = data.__len__()
    cap = lib().zipc_hip_zlib_bound(n)
    dst = C.create_string_buffer(cap)
    out_len, adler = C.c_size_t(), C.c_uint32()
    st = lib().zipc_hip_zlib_compress(ctx.handle, data, n, _level(level), dst, cap,
                                      C.byref(out_len), C.byref(adler))
    if st != OK:
        ctx.check(st)
    return Ok((adler.value, dst.raw[:out_len.value]))


# ---- gzip (RFC 1952; include/zipc_hip.h zipc_hip_gzip_*): additions, the reference has no gzip.  A name or a comment of a
# member's header may be at most 65 535 bytes long (a limit of this library); compress writes MTIME 0 and OS 255.

_FATAL = (_lib.ERR_HIP, _lib.ERR_INVALID_ARG, _lib.ERR_NO_DEVICE, _lib.ERR_NOMEM)


def gzip_compress(s, level=None, bgzf=False, start=0, len=None, ctx=None):
    """One gzip member of the range: Ok bytes | Error msg.  bgzf: a BGZF member (an extra field with the member's length,
    at most 64 KiB in all: cut the input at 65 280 bytes; BGZF's end-of-file block is the caller's to append)."""
    data = _range(s, start, len)
    ctx = ctx or default_context()
    n = data.__len__()
    flavour = _lib.GZIP_BGZF if bgzf else _lib.GZIP_PLAIN
    cap = lib().zipc_hip_gzip_bound(n, flavour)
    dst = C.create_string_buffer(cap)
    out_len = C.c_size_t()
    st = lib().zipc_hip_gzip_compress(ctx.handle, data, n, _level(level), flavour, dst, cap, C.byref(out_len))
    if st == OK:
        return Ok(dst.raw[:out_len.value])
    if st in _FATAL:
        ctx.check(st)
    return Error(_message(st))


def gzip_size(s, start=0, len=None, ctx=None):
    """What `gzip_decompress` of the same range would hand back, without the bytes and without the CRC-32s compared:
    Ok (length, used, members) | Error msg."""
    data = _range(s, start, len)
    ctx = ctx or default_context()
    out_len, used, members = C.c_size_t(), C.c_size_t(), C.c_size_t()
    st = lib().zipc_hip_gzip_size(ctx.handle, data, data.__len__(), C.byref(out_len), C.byref(used), C.byref(members))
    if st == OK:
        return Ok((out_len.value, used.value, members.value))
    if st in _FATAL:
        ctx.check(st)
    return Error(_message(st, data[2] if data.__len__() > 2 else 0))


def gzip_decompress(s, start=0, len=None, ctx=None):
    """A whole gzip FILE -- every member of the range, their outputs concatenated (a .gz, a BGZF file in one batch per run
    of members): Ok (bytes, used, members) | Error (found | None, msg), `used` the source bytes up to the end of the last
    member, `found` the CRC-32 found where a member's own differs."""
    data = _range(s, start, len)
    ctx = ctx or default_context()
    n = data.__len__()
    size, used, members, crc = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_uint32()
    st = lib().zipc_hip_gzip_size(ctx.handle, data, n, C.byref(size), C.byref(used), C.byref(members))
    if st == OK:
        dst = C.create_string_buffer(max(size.value, 1))
        out_len = C.c_size_t()
        st = lib().zipc_hip_gzip_decompress(ctx.handle, data, n, dst, size.value, C.byref(out_len), C.byref(used), C.byref(members),
                                            C.byref(crc))
        if st == OK:
            return Ok((dst.raw[:out_len.value], used.value, members.value))
    if st in _FATAL:
        ctx.check(st)
    if st == ERR_CHECKSUM:
        return Error((crc.value, "Checksum mismatch, found %x" % crc.value))
    return Error((None, _message(st, data[2] if n > 2 else 0)))


# ---- many streams in one call (include/zipc_hip.h zipc_hip_zlib_*_many): what a caller with a pack of git objects, the
# IDAT chunks of many images or a table's pages uses instead of n calls of the two functions above.  The reference has
# no such values; every element of the result is what the single-stream function gives for that stream.

def _many_arrays(bufs):
    n = len(bufs)
    keep = [C.create_string_buffer(b, max(len(b), 1)) if isinstance(b, bytes) else b for b in bufs]
    ptrs = (C.c_void_p * max(n, 1))(*[C.addressof(k) for k in keep])
    return keep, ptrs


def zlib_compress_many(streams, level=None, ctx=None):
    """[zlib_compress(s, level) for s in streams] in one call: a list of Ok((adler, bytes))"""
    ctx = ctx or default_context()
    data = [bytes(s) for s in streams]
    n = len(data)
    if n == 0:
        return []
    caps = [lib().zipc_hip_zlib_bound(len(d)) for d in data]
    keep, sp = _many_arrays(data)  # (the copies the pointers point into live until the call is through)
    outs = [C.create_string_buffer(c) for c in caps]
    _, dp = _many_arrays(outs)
    res = (_lib.StreamResult * n)()
    st = lib().zipc_hip_zlib_compress_many(ctx.handle, n, sp, (C.c_size_t * n)(*[len(d) for d in data]), _level(level), dp,
                                           (C.c_size_t * n)(*caps), res)
    if st != OK:
        ctx.check(st)
    for r in res:
        if r.status != OK:
            ctx.check(r.status)
    del keep
    return [Ok((int(r.checksum), o.raw[:r.out_len])) for r, o in zip(res, outs)]


def zlib_decompress_many(streams, decompressed_size=None, ctx=None):
    """[zlib_decompress(s, decompressed_size[i]) for s in streams] in one call: a list of Ok((bytes, adler)) |
    Error(((expect, found) | None, msg)).  decompressed_size: None, or one size per stream.  Without sizes every stream
    starts with room for three times its length, as zlib_decompress does, and the streams that need more go again."""
    ctx = ctx or default_context()
    data = [bytes(s) for s in streams]
    n = len(data)
    has_limit = decompressed_size is not None
    if has_limit and len(decompressed_size) != n:
        raise ValueError("decompressed_size: one size per stream")
    out = [None] * n
    todo = list(range(n))
    caps = {i: (decompressed_size[i] if has_limit else max(3 * len(data[i]), 1024)) for i in todo}
    while todo:
        m = len(todo)
        keep, sp = _many_arrays([data[i] for i in todo])  # (the copies the pointers point into live until the call is through)
        bufs = [C.create_string_buffer(max(caps[i], 1)) for i in todo]
        _, dp = _many_arrays(bufs)
        res = (_lib.StreamResult * m)()
        lim = (C.c_size_t * m)(*[decompressed_size[i] for i in todo]) if has_limit else None
        st = lib().zipc_hip_zlib_decompress_many(ctx.handle, m, sp, (C.c_size_t * m)(*[len(data[i]) for i in todo]), lim, dp,
                                                 (C.c_size_t * m)(*[caps[i] for i in todo]), res)
        if st != OK:
            ctx.check(st)
        del keep
        again = []
        for i, r, b in zip(todo, res, bufs):
            if r.status == ERR_DST_TOO_SMALL and not has_limit:
                caps[i] *= 2
                again.append(i)
            elif r.status == OK:
                out[i] = Ok((b.raw[:r.out_len], int(r.checksum)))
            elif r.status == ERR_CHECKSUM:
                expect = int.from_bytes(data[i][-4:], "big")  # (the result carries the value found: include/zipc_hip.h)
                out[i] = Error(((expect, int(r.checksum)), crc_error(expect, int(r.checksum))))
            elif r.status in (_lib.ERR_HIP, _lib.ERR_INVALID_ARG, _lib.ERR_NO_DEVICE, _lib.ERR_NOMEM):
                ctx.check(r.status)
            else:
                out[i] = Error((None, _message(r.status, data[i][0] & 0x0F if data[i] else 0)))
        todo = again
    return out


def recode_many(streams, decompressed_size=None, expect_crc32=None, level=None, ctx=None):
    """Every raw deflate stream inflated, its CRC-32 checked and deflated again at `level` in one call
    (zipc_hip_recode_many): what the reference's `recode` does to a member (test/zipc_tool.ml:437-545) -- inflate_and_crc_32,
    Crc_32.check, deflate -- with the decompressed bytes staying on the device.  A list of Ok((crc32, bytes)) |
    Error(message): inflate's message, or Crc_32.check's.  decompressed_size / expect_crc32: None, or one value per stream.
    Without sizes every stream starts with room for three times its length, as inflate does, and the streams that need
    more go again."""
    ctx = ctx or default_context()
    data = [bytes(s) for s in streams]
    n = len(data)
    has_limit = decompressed_size is not None
    if has_limit and len(decompressed_size) != n:
        raise ValueError("decompressed_size: one size per stream")
    if expect_crc32 is not None and len(expect_crc32) != n:
        raise ValueError("expect_crc32: one value per stream")
    out = [None] * n
    todo = list(range(n))
    mids = {i: (decompressed_size[i] if has_limit else max(3 * len(data[i]), 1024)) for i in todo}
    while todo:
        m = len(todo)
        keep, sp = _many_arrays([data[i] for i in todo])  # (the copies the pointers point into live until the call is through)
        caps = [lib().zipc_hip_deflate_bound(mids[i]) for i in todo]
        bufs = [C.create_string_buffer(c) for c in caps]
        _, dp = _many_arrays(bufs)
        res = (_lib.RecodeResult * m)()
        lim = (C.c_size_t * m)(*[decompressed_size[i] for i in todo]) if has_limit else None
        crc = (C.c_uint32 * m)(*[expect_crc32[i] & 0xFFFFFFFF for i in todo]) if expect_crc32 is not None else None
        st = lib().zipc_hip_recode_many(ctx.handle, m, sp, (C.c_size_t * m)(*[len(data[i]) for i in todo]), lim, crc,
                                        (C.c_size_t * m)(*[mids[i] for i in todo]), _level(level), dp, (C.c_size_t * m)(*caps), res)
        if st != OK:
            ctx.check(st)
        del keep
        again = []
        for i, r, b in zip(todo, res, bufs):
            if r.status == ERR_DST_TOO_SMALL and r.stage == 1 and not has_limit:
                mids[i] *= 2
                again.append(i)
            elif r.status == OK:
                out[i] = Ok((int(r.checksum), b.raw[:r.out_len]))
            elif r.status == ERR_CHECKSUM:
                out[i] = Error(crc_error(expect_crc32[i] & 0xFFFFFFFF, int(r.checksum)))
            elif r.status in (_lib.ERR_HIP, _lib.ERR_INVALID_ARG, _lib.ERR_NO_DEVICE, _lib.ERR_NOMEM) or r.stage == 3:
                ctx.check(r.status)  # (stage 3: the destination is deflate's bound -- the library's own failure)
            else:
                out[i] = Error(_message(r.status))
        todo = again
    return out
