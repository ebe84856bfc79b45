"""The streams of the recode tests (tests/test_gpu_recode_batch.py, tests/test_gpu_recode_many.py) and what the oracle says
of each: inflate with CRC-32, Crc_32.check, deflate at a level.  Nothing here runs on the GPU."""
import functools
import zlib

import deflate_fit
import util


class Case:
    """one stream: its source bytes (a raw deflate stream), the room for its decompressed bytes, ?decompressed_size,
    the CRC-32 it is held to, the room for what it recodes to (None: deflate's bound), stray flag bits"""

    def __init__(self, name, stream, mid_cap, limit=None, expect=None, dst_cap=None, flags=0):
        self.name, self.stream, self.mid_cap, self.limit, self.expect, self.dst_cap, self.flags = name, stream, mid_cap, limit, expect, dst_cap, flags


class Expect:
    """(status, stage, checksum, mid_len, out) of zipc_hip_recode_result, and the decompressed bytes where there are any"""

    def __init__(self, status, stage, checksum=0, data=b"", out=b"", would_be=b"", may_write=0):
        self.status, self.stage, self.checksum, self.out = status, stage, checksum, out
        self.mid_len = len(data) if stage in (2, 3) or status == 0 else 0
        self.data = data
        # a stream that stops at stage 3: what it would have recoded to, and how many bytes of that -- the blocks in
        # front of the one that does not fit -- deflate may have left in the device's destination slot (the header's words)
        self.would_be, self.may_write = would_be, may_write


@functools.lru_cache(maxsize=None)
def _inflate(stream, limit):
    import oracle

    return oracle.inflate(stream, decompressed_size=limit, crc_op=oracle.CRC_CRC32)


@functools.lru_cache(maxsize=None)
def _deflate(data, level):
    import oracle

    st, out, _ = oracle.deflate(data, level=level)
    assert st == 0
    return out


def bound(n):
    import oracle

    return oracle.deflate_bound(n)


def expectation(c, level):
    """what the header says of the stream, with the oracle standing in for the codec"""
    if c.flags & ~3:
        return Expect(18, 0)
    st, data, crc = _inflate(c.stream, c.limit)
    if st != 0:
        return Expect(st, 1)
    if c.limit is None and len(data) > c.mid_cap:  # (the reference grows its buffer; here the caller is asked for more room)
        return Expect(16, 1)
    if c.expect is not None and crc != c.expect:
        return Expect(6, 2, crc, data)
    out = _deflate(data, level)
    cap = bound(c.mid_cap) if c.dst_cap is None else c.dst_cap
    if not deflate_fit.fits(data, level, cap):  # (not "len(out) > cap": tests/deflate_fit.py has the rule)
        return Expect(16, 3, crc, data, would_be=out, may_write=blocks_in_front(data, level, out, cap))
    return Expect(0, 0, crc, data, out)


def blocks_in_front(data, level, out, dst_cap):
    """The bytes of `out` that lie in front of the first block that does not fit dst_cap, in whole bytes: what deflate may
    have left of the stream (deflate_fit.expect's whole_bytes_in_front).  One block: none.  `None (stored blocks): none
    either, the whole length is known before a byte is stored."""
    status, _, front = deflate_fit.expect(data, level, dst_cap)
    assert status == 16 and front < len(out)
    return front


@functools.lru_cache(maxsize=None)
def datas():
    """the decompressed inputs the issue names: 0, 1, 100 and 6000 bytes, random and text-like; 70 000 bytes of few symbols
    (more than one block behind the 65 534-symbol cut)"""
    d = []
    for n in (0, 1, 100, 6000):
        d.append(("rand%d" % n, util.rand_bytes(n, 40 + n % 7)))
        d.append(("text%d" % n, util.text(n, 50 + n % 7)))
    d.append(("few70000", util.rand_bytes(70000, 9, bits=2)))
    return d


def zlib_fixed_and_stored():
    """a stream Python's zlib made: fixed blocks of text, ended on a byte by a full flush, then stored blocks of random
    bytes with the final bit"""
    a, b = util.text(2000, 77), util.rand_bytes(3000, 78)
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)
    z = co.compress(a) + co.flush(zlib.Z_FULL_FLUSH)
    assert z[0] & 6 == 2  # BTYPE 01: fixed
    st = zlib.compressobj(0, zlib.DEFLATED, -15)
    z += st.compress(b) + st.flush()
    assert zlib.decompress(z, -15) == a + b
    return a + b, z


@functools.lru_cache(maxsize=None)
def good_cases():
    """about 40 good streams, ragged: every input of datas() as the oracle's deflate makes it at every level (the long one at
    two), with and without ?decompressed_size and an expected CRC-32, some with room to spare"""
    import oracle

    out = []
    k = 0
    for name, data in datas():
        for level in ((1, 3) if len(data) > 10000 else (0, 1, 2, 3)):
            s = _deflate(data, level)
            limit = len(data) if k % 2 == 0 else None
            expect = oracle.crc32(data) if k % 3 != 2 else None
            spare = (0, 1, 300)[k % 3] if limit is None else (0, 17)[k // 2 % 2]
            if limit is not None:
                limit += spare  # (?decompressed_size is the most a stream may inflate to: every other one says more than it does)
            out.append(Case("%s_from_level%d" % (name, level), s, len(data) + spare, limit, expect))
            k += 1
    data, z = zlib_fixed_and_stored()
    out.append(Case("zlib_fixed_and_stored", z, len(data), len(data), zlib.crc32(data)))
    return out


def error_cases():
    """one stream of each way a recode can stop"""
    import oracle

    data = util.text(6000, 61)
    s = _deflate(data, 2)
    crc = oracle.crc32(data)
    return [
        Case("corrupted", bytes([s[0] | 6]) + s[1:], len(data), len(data), crc),                # BTYPE 11
        Case("limit_below_size", s, len(data), len(data) - 1, crc),
        Case("mid_cap_too_small", s, len(data) - 10, None, crc),
        Case("wrong_crc", s, len(data), len(data), crc ^ 0x8000),
        Case("dst_cap_too_small", s, len(data), len(data), crc, dst_cap=20),                     # (one block: less than any level makes of 6000 bytes of words)
        Case("stray_flag", s, len(data), len(data), crc, flags=4),
        two_block_stream_without_room(),
    ] + middle_block_binds()


def two_block_stream_without_room():
    """the 70 000 bytes of few symbols with room for what their first block recodes to, at every level, and not for the
    second (`None: 70 010 bytes, the others 20 969 to 21 786 with a last block of 1300 and more)"""
    import oracle

    data = dict(datas())["few70000"]
    return Case("dst_cap_holds_the_first_block_only", _deflate(data, 1), len(data), len(data), oracle.crc32(data), dst_cap=20900)


def middle_block_binds():
    """196 612 zero bytes with room for what they recode to at `Default (233 bytes) and with the least room the rule takes
    (238): three dynamic blocks and a fixed one, and the third one's estimate decides -- refused at stage 3, then accepted
    (at `Fast and `Best too; at `None both are far too small)"""
    import oracle

    data = deflate_fit.ZEROS196K
    out, blocks = deflate_fit.trace(data, 2)
    clen, least = len(out), deflate_fit.min_cap(blocks)
    assert (clen, least) == (233, 238) and not deflate_fit.fits(data, 2, clen) and deflate_fit.fits(data, 2, least)
    return [Case("zeros196k_room_%s" % what, _deflate(data, 2), len(data), len(data), oracle.crc32(data), dst_cap=cap)
            for what, cap in (("for_the_output", clen), ("the_rule_takes", least))]


def ragged_batch():
    """the good streams with the ones that stop (and the one that just fits) scattered among them"""
    cases = list(good_cases())
    for j, e in enumerate(error_cases()):
        cases.insert(3 + 6 * j, e)
    return cases


def require_coverage(pairs):
    """on the expectation's side: every status and every stage the issue names occurs"""
    assert {e.status for _, e in pairs} == {0, 1, 2, 6, 16, 18}, {e.status for _, e in pairs}
    assert {e.stage for _, e in pairs} == {0, 1, 2, 3}
    assert {(e.status, e.stage) for _, e in pairs} >= {(0, 0), (18, 0), (1, 1), (2, 1), (16, 1), (6, 2), (16, 3)}
