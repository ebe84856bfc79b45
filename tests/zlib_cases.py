"""The zlib streams tests/test_gpu_zlib_batch.py and tests/test_gpu_zlib_many.py run, and what the ORACLE says of each
(oracle.zlib_decompress / oracle.zlib_compress): made once per process, shared, never changed.  Nothing here calls the
code under test."""
import collections
import functools

import deflate_fit
import util

# limit: ?decompressed_size, or None; cap: the destination's room (>= limit); flags: descriptor bits beyond HAS_LIMIT
Case = collections.namedtuple("Case", "name stream limit cap flags")
# status, the bytes, the result's checksum (on a checksum mismatch: the value found); header: the stream never reaches
# the codec (its header, its length or its descriptor's flags are refused), so its destination stays as it was
Expect = collections.namedtuple("Expect", "status out checksum header")

ST_DST_TOO_SMALL, ST_INVALID_ARG = 16, 18
REQUIRED_STATUSES = {0, 1, 2, 3, 4, 5, 6, 16, 18}


def _with_fcheck(cmf, flg):
    """flg with its low five bits set so that cmf, flg is a multiple of 31 (RFC 1950 FCHECK)"""
    flg &= 0xE0
    return flg + (31 - (cmf * 256 + flg) % 31) % 31


@functools.lru_cache(maxsize=None)
def decompress_cases():
    import oracle

    cases = []
    plains = [("trip%d" % i, s) for i, (s, _) in enumerate(util.trip_strings())]
    plains += [("text3000", util.text(3000, 1)), ("rand20000", util.rand_bytes(20000, 2)), ("empty", b"")]
    for level in range(4):
        for name, data in plains:
            st, z, _ = oracle.zlib_compress(data, level)
            assert st == 0
            cases.append(Case("good_%s_l%d" % (name, level), z, len(data), len(data), 0))
    data = util.text(3000, 1)
    z = oracle.zlib_compress(data, 2)[1]
    n, roomy = len(data), 2 * len(data) + 1000

    def bad(name, stream, limit=roomy, cap=None, flags=0):
        cases.append(Case(name, bytes(stream), limit, limit if cap is None else cap, flags))

    for k in range(6):
        bad("len%d" % k, z[:k])
    bad("fcheck_off_by_one", bytes([z[0], z[1] + 1]) + z[2:])
    bad("method7", bytes([0x77, z[1]]) + z[2:])
    bad("method7_fcheck", bytes([0x77, _with_fcheck(0x77, z[1])]) + z[2:])
    bad("window8_fcheck", bytes([0x88, _with_fcheck(0x88, z[1])]) + z[2:])
    bad("dict_fcheck", bytes([z[0], _with_fcheck(z[0], z[1] | 0x20)]) + z[2:])
    for k in range(1, 5):
        b = bytearray(z)
        b[-k] ^= 0x10
        bad("trailer_byte_-%d" % k, b)
    for i, body in enumerate(util.corrupt_variants(z[2:-4], 11, 12)):
        bad("body_damaged_%d" % i, z[:2] + body + z[-4:])
    bad("cut2", z[:-2])        # inflate gets the whole body and nothing else: the trailer read is not the trailer
    bad("cut4", z[:-4])        # inflate runs into what were the body's last bytes
    bad("garbage2", z + b"\x5a\xc3")
    bad("limit_one_short", z, limit=n - 1)
    bad("cap_one_short_no_limit", z, limit=None, cap=n - 1)
    bad("unknown_flag", z, limit=n, flags=2)
    return tuple(cases)


def expect_decompress(case):
    """the oracle's verdict (the reference's Adler-32), with the two boundary statuses the reference has no word for"""
    import oracle

    if case.flags:
        return Expect(ST_INVALID_ARG, b"", 0, True)
    st, out, adler, expect, found = oracle.zlib_decompress(case.stream, decompressed_size=case.limit)
    header = st in (3, 4, 5) or (st == 1 and (len(case.stream) < 6 or (case.stream[0] * 256 + case.stream[1]) % 31 != 0))
    if case.limit is None and st == 0 and len(out) > case.cap:
        return Expect(ST_DST_TOO_SMALL, b"", 0, False)
    if st == 6:
        assert expect == int.from_bytes(case.stream[-4:], "big")
        return Expect(6, b"", found, False)
    return Expect(st, out, adler if st == 0 else 0, header)


@functools.lru_cache(maxsize=None)
def decompress_expectations():
    """[(case, Expect)], and the proof on the oracle's side that every status is there"""
    pairs = tuple((c, expect_decompress(c)) for c in decompress_cases())
    seen = {e.status for _, e in pairs}
    assert seen >= REQUIRED_STATUSES, sorted(REQUIRED_STATUSES - seen)
    assert any(e.header and e.status == 1 for _, e in pairs) and any(not e.header and e.status == 1 for _, e in pairs)
    return pairs


COMPRESS_LENGTHS = (0, 1, 5, 65534, 65535, 70000, 200000)
# name, data, cap: None = zlib_bound(len), "exact" / "exact-1" = the oracle's size (less one), "least" = six bytes more
# than the least room deflate's rule takes (tests/deflate_fit.py), or a number
CCase = collections.namedtuple("CCase", "name data cap")


@functools.lru_cache(maxsize=None)
def compress_cases():
    cases = []
    for n in COMPRESS_LENGTHS:
        cases.append(CCase("text%d" % n, util.text(n, 40 + n % 7), None))
        cases.append(CCase("rand%d" % n, util.rand_bytes(n, 50 + n % 7), None))
    small = util.text(5000, 7)
    for cap in (0, 5, "exact", "exact-1"):
        cases.append(CCase("cap_%s" % cap, small, cap))
    for cap in ("exact", "least"):  # four blocks, the third one's estimate decides: room for the output is refused
        cases.append(CCase("zeros196k_cap_%s" % cap, deflate_fit.ZEROS196K, cap))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def compress_expectations(level):
    """[(case, cap in bytes or None, Expect)] at a level"""
    import oracle

    out = []
    for c in compress_cases():
        st, z, adler = oracle.zlib_compress(c.data, level)
        assert st == 0
        cap = {None: None, "exact": len(z), "exact-1": len(z) - 1, "least": deflate_fit.least_room(c.data, level) + 6}.get(c.cap, c.cap)
        # a stream fits iff there is room for the container and deflate's rule takes the rest (not "cap >= len(z)")
        if cap is not None and (cap < 6 or not deflate_fit.fits(c.data, level, cap - 6)):
            out.append((c, cap, Expect(ST_DST_TOO_SMALL, b"", 0, cap < 6)))
        else:
            out.append((c, cap, Expect(0, z, adler, False)))
    return tuple(out)
