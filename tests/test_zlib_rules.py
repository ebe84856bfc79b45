"""zipc_amd/csrc/zlib_container.h -- the zlib container's rules, one header for the kernels of zlib.hip, the host forms
and this test -- compiled with g++ (tests/zlib_sim/sim_zlib.cpp) and held against the oracle's zlib_decompress /
zlib_compress.  No GPU; the kernels that apply the rules are checked in tests/test_gpu_zlib_batch.py."""
import ctypes as C
import os

import pytest

import mutation
import util  # noqa: F401  (sets sys.path through conftest)

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER_STATUSES = (1, 3, 4, 5)  # what the reference's checks of the first two bytes and the length can say (zd.ml:723-730)


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    L = C.CDLL(mutation.gxx(tmp_path_factory.mktemp("zlib_sim") / "libzlib_sim.so", [os.path.join(HERE, "zlib_sim", "sim_zlib.cpp")],
                            extra=["-Wall", "-Wno-unknown-pragmas"]))
    L.sim_zlib_open_status.restype = C.c_uint
    L.sim_zlib_open_status.argtypes = [C.c_ulonglong, C.c_uint, C.c_uint]
    L.sim_zlib_open_status_all.restype = None
    L.sim_zlib_open_status_all.argtypes = [C.c_ulonglong, C.c_void_p]
    L.sim_zlib_cmf.restype = C.c_uint
    L.sim_zlib_flg.restype = C.c_uint
    L.sim_zlib_flg.argtypes = [C.c_int]
    L.sim_zlib_body_off.restype = L.sim_zlib_body_len.restype = C.c_ulonglong
    L.sim_zlib_body_off.argtypes = L.sim_zlib_body_len.argtypes = [C.c_ulonglong]
    L.sim_zlib_expect.restype = C.c_uint
    L.sim_zlib_expect.argtypes = [C.c_char_p]
    L.sim_zlib_put_trailer.restype = None
    L.sim_zlib_put_trailer.argtypes = [C.c_void_p, C.c_uint]
    L.sim_zlib_close_decompress.restype = None
    L.sim_zlib_close_decompress.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_ulonglong, C.POINTER(C.c_ulonglong)]
    L.sim_zlib_close_compress.restype = C.c_int
    L.sim_zlib_close_compress.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_ulonglong, C.POINTER(C.c_ulonglong)]
    return L


@pytest.mark.parametrize("length", [5, 8])
def test_open_status_of_every_header_is_the_oracles(sim, oracle, length):
    """all 65 536 (CMF, FLG) pairs in front of an empty fixed block and its Adler-32 (cmf flg 03 00 00 00 00 01), whole
    and cut to 5 bytes: the header's verdict is the oracle's, and OK wherever the oracle's verdict is not about the
    header (8 bytes: always -- the body is valid)"""
    got = (C.c_ubyte * 65536)()
    sim.sim_zlib_open_status_all(length, got)
    seen = set()
    for cmf in range(256):
        for flg in range(256):
            stream = (bytes([cmf, flg]) + b"\x03\x00\x00\x00\x00\x01")[:length]
            st0 = oracle.zlib_decompress(stream)[0]
            st = got[cmf * 256 + flg]
            assert st == sim.sim_zlib_open_status(length, cmf, flg)
            assert st == (st0 if st0 in HEADER_STATUSES else 0), (length, cmf, flg, st, st0)
            seen.add(st0)
    assert seen == ({1} if length == 5 else {0, 1, 3, 4, 5}), seen  # (the oracle's side: every check is reached)


def test_open_status_looks_at_the_length_first(sim):
    for length in range(6):
        assert sim.sim_zlib_open_status(length, 0x78, 0x9C) == 1
        assert sim.sim_zlib_open_status(length, 0x77, 0x00) == 1  # (not "unknown method": the reference never gets there)
    assert sim.sim_zlib_open_status(6, 0x78, 0x9C) == 0


def test_header_written_is_the_oracles(sim, oracle):
    for level in range(4):
        st, z, _ = oracle.zlib_compress(b"", level)
        assert st == 0 and bytes([sim.sim_zlib_cmf(), sim.sim_zlib_flg(level)]) == z[:2], level
        assert sim.sim_zlib_open_status(len(z), z[0], z[1]) == 0


def test_body_range_and_trailer(sim, oracle):
    """inflate is handed [2, len - 2) -- two of the trailer's bytes are inside (zd.ml:732) -- and the trailer is the
    big-endian Adler-32, read and written"""
    for data in (b"", b"a", util.text(3000, 1), util.rand_bytes(20000, 2)):
        st, z, adler = oracle.zlib_compress(data, 2)
        off, ln = sim.sim_zlib_body_off(0), sim.sim_zlib_body_len(len(z))
        assert (off, off + ln) == (2, len(z) - 2)
        assert oracle.inflate(z[off:off + ln], crc_op=oracle.CRC_ADLER32) == (0, data, adler)
        assert sim.sim_zlib_expect(z[-4:]) == adler == oracle.zlib_decompress(z)[3]
        buf = C.create_string_buffer(4)
        sim.sim_zlib_put_trailer(buf, adler)
        assert buf.raw == z[-4:]
    assert sim.sim_zlib_body_off(1000) == 1002


def test_close_rules(sim):
    def dec(pre, expect, inner):
        out = (C.c_ulonglong * 3)()
        sim.sim_zlib_close_decompress(pre, expect, *inner, out)
        return tuple(out)

    def comp(pre, inner):
        out = (C.c_ulonglong * 3)()
        wrap = sim.sim_zlib_close_compress(pre, *inner, out)
        return tuple(out), wrap

    assert dec(0, 0xABCD, (0, 0xABCD, 77)) == (0, 0xABCD, 77)
    assert dec(0, 0xABCD, (0, 0x1234, 77)) == (6, 0x1234, 0)       # the value found, no bytes
    for st in (1, 2, 16, 18):
        assert dec(0, 5, (st, 0, 0)) == (st, 0, 0)                 # inflate's own verdicts pass through
    for pre in (1, 3, 4, 5, 18):
        assert dec(pre, 0, (1, 0, 0)) == (pre, 0, 0)               # the container's verdict comes first
        assert dec(pre, 0, (0, 1, 0)) == (pre, 0, 0)
    assert comp(0, (0, 0xABCD, 10)) == ((0, 0xABCD, 16), 1)
    assert comp(0, (16, 0, 0)) == ((16, 0, 0), 0)
    assert comp(0, (18, 0, 0)) == ((18, 0, 0), 0)
    assert comp(16, (16, 0, 0)) == ((16, 0, 0), 0)
    assert comp(18, (18, 0, 0)) == ((18, 0, 0), 0)
    assert comp(16, (0, 1, 2)) == ((16, 0, 0), 0)
