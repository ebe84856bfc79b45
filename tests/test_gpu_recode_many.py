"""zipc_hip_recode_many (include/zipc_hip.h) and what stands on it -- zipc_deflate.recode_many, Archive::recode_deflated:
host-resident deflate streams inflated, CRC-checked and deflated again with the decompressed bytes staying on the device.
Every expectation is the oracle's (tests/recode_cases.py), or, for the archive, the bytes the extract-then-add path writes."""
import ctypes as C
import random
import struct

import numpy as np
import pytest

import recode_cases as RC
import util

pytestmark = pytest.mark.gpu


def _ptrs(arrays):
    return (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def _sizes(values):
    return (C.c_size_t * len(values))(*values)


def many(ctx, cases, level, limits=True, expects=True, null_src=()):
    """one zipc_hip_recode_many over `cases`: (call status, results, outputs, dst_caps).  limits / expects False: the NULL arrays"""
    from zipc_amd import _lib

    n = len(cases)
    src = [np.frombuffer(c.stream + b"\0", dtype=np.uint8).copy() for c in cases]
    caps = [RC.bound(c.mid_cap) if c.dst_cap is None else c.dst_cap for c in cases]
    outs = [np.full(cap + 64, 0xA5, dtype=np.uint8) for cap in caps]
    res = (_lib.RecodeResult * n)()
    C.memset(res, 0xEE, C.sizeof(res))
    sp = _ptrs(src)
    for i in null_src:
        sp[i] = None
    st = _lib.lib().zipc_hip_recode_many(ctx.handle, n, sp, _sizes([len(c.stream) for c in cases]),
                                         _sizes([c.limit for c in cases]) if limits else None,
                                         (C.c_uint32 * n)(*[c.expect for c in cases]) if expects else None,
                                         _sizes([c.mid_cap for c in cases]), level, _ptrs(outs), _sizes(caps), res)
    return st, res, outs, caps


def check(cases, level, res, outs, caps, what):
    seen = set()
    for c, r, o, cap in zip(cases, res, outs, caps):
        e = RC.expectation(c, level)
        got = (int(r.status), int(r.stage), int(r.checksum), int(r.mid_len), int(r.out_len), int(r.reserved))
        assert got == (e.status, e.stage, e.checksum, e.mid_len, len(e.out), 0), (what, c.name, got)
        if e.status == 0:
            assert o[:len(e.out)].tobytes() == e.out, (what, c.name)
            assert (o[cap:] == 0xA5).all(), (what, c.name, "bytes behind dst_cap")
        else:
            assert (o == 0xA5).all(), (what, c.name, "the buffer of a stream that stopped was written")
        seen.add((e.status, e.stage))
    return seen


@pytest.fixture(scope="module")
def many_cases():
    """2500 streams of 1-3 KiB cut from one pool of text and random bytes, as the oracle deflates them at `Best, each with
    its size and CRC-32; nine of them stop: three corrupted, two with a limit below their size, two held to a wrong CRC-32,
    two with no room for what they recode to"""
    import oracle

    r = random.Random(2500)
    pool = util.text(300000, 3) + util.rand_bytes(100000, 4) + util.text(100000, 5)
    cases = []
    for i in range(2500):
        n = r.randrange(1024, 3073)
        at = r.randrange(0, len(pool) - n)
        data = pool[at:at + n]
        cases.append(RC.Case("s%d" % i, RC._deflate(data, 3), n, n, oracle.crc32(data)))
    for k, i in enumerate((0, 7, 700, 1249, 1250, 1251, 1900, 2498, 2499)):
        c = cases[i]
        if k % 4 == 0:
            c.stream, c.name = bytes([c.stream[0] | 6]) + c.stream[1:], c.name + "_corrupted"
        elif k % 4 == 1:
            c.limit, c.name = c.limit - 1, c.name + "_limit_below_size"
        elif k % 4 == 2:
            c.expect, c.name = c.expect ^ 1, c.name + "_wrong_crc"
        else:
            c.dst_cap, c.name = 12, c.name + "_dst_cap_too_small"
    return cases


def test_2500_streams_in_more_than_one_sub_batch(gpu_ctx, many_cases):
    try:  # (every sub-batch launches the recode sequence once: the launches of its first kernel count them)
        gpu_ctx.set_profiling(True)
        gpu_ctx.reset_kernel_times()
        st, res, outs, caps = many(gpu_ctx, many_cases, 2)
        sub_batches = gpu_ctx.kernel_times()["recode_open"][0]
    finally:
        gpu_ctx.set_profiling(False)
    assert st == 0 and sub_batches >= 2, (st, sub_batches)
    seen = check(many_cases, 2, res, outs, caps, "recode_many")
    assert seen == {(0, 0), (1, 1), (2, 1), (6, 2), (16, 3)}, seen  # (the expectation's side: the ways to stop are there)


def test_no_limits_and_no_expected_crcs(gpu_ctx):
    """limit and expect_crc32 both NULL: no stream has a ?decompressed_size (one without room says so at stage 1), and no
    CRC-32 is compared (a wrong one goes unnoticed, as the header says)"""
    cases = []
    for c in RC.ragged_batch():
        if c.flags or c.name == "limit_below_size":
            continue
        cases.append(RC.Case(c.name, c.stream, c.mid_cap, None, None, c.dst_cap))
    st, res, outs, caps = many(gpu_ctx, cases, 1, limits=False, expects=False)
    assert st == 0
    seen = check(cases, 1, res, outs, caps, "recode_many without limits")
    assert seen == {(0, 0), (1, 1), (16, 1), (16, 3)}, seen
    assert any(c.name == "dst_cap_holds_the_first_block_only" for c in cases)  # (nothing of it reaches the caller's buffer: check)


def test_a_null_source_fails_the_call_and_defines_every_result(gpu_ctx, many_cases):
    cases = many_cases[:40]
    st, res, outs, _ = many(gpu_ctx, cases, 2, null_src=(17,))
    assert st == 18
    for r, o in zip(res, outs):
        assert (int(r.status), int(r.stage), int(r.checksum), int(r.mid_len), int(r.out_len), int(r.reserved)) == (18, 0, 0, 0, 0, 0)
        assert (o == 0xA5).all()
    st, res, outs, caps = many(gpu_ctx, cases, 2)  # (nothing sticks)
    assert st == 0
    check(cases, 2, res, outs, caps, "after a refused call")


def test_python_mirror_gives_the_references_messages(gpu_ctx, oracle):
    """zipc_deflate.recode_many: Ok((crc32, bytes)), inflate's message, or Crc_32.check's; without sizes it finds the room
    itself as inflate does"""
    from zipc_amd import zipc_deflate as Z

    datas = [util.text(5000, 1), b"", util.rand_bytes(3000, 2), util.text(2000, 3), util.text(9000, 4)]
    streams = [RC._deflate(d, 3) for d in datas]
    crcs = [oracle.crc32(d) for d in datas]
    streams[3] = bytes([streams[3][0] | 6]) + streams[3][1:]
    crcs[2] ^= 0x10
    sizes = [len(d) for d in datas]
    sizes[4] -= 1
    got = Z.recode_many(streams, decompressed_size=sizes, expect_crc32=crcs, level="fast", ctx=gpu_ctx)
    assert got[0].get_ok() == (crcs[0], RC._deflate(datas[0], 1)) and got[1].get_ok() == (0, RC._deflate(b"", 1))
    assert got[2].error == Z.Crc_32.check(crcs[2], oracle.crc32(datas[2])).error == "Checksum mismatch, expected %x found %x)" % (crcs[2], crcs[2] ^ 0x10)
    assert got[3].error == "Corrupted data stream" and got[4].error == "Expected decompression size exceeded"
    zeros = oracle.deflate(bytes(40000), level=3)[1]  # (a stream that inflates to far more than three times its length)
    got = Z.recode_many([streams[0], zeros], level=None, ctx=gpu_ctx)
    assert got[0].get_ok() == (crcs[0], RC._deflate(datas[0], 3)) and got[1].get_ok() == (oracle.crc32(bytes(40000)), zeros)


def _patch_directory_crc(z, path, value):
    """the archive with the CRC-32 the central directory has for `path` replaced"""
    at = 0
    while True:
        at = z.index(b"PK\x01\x02", at)
        name_len = struct.unpack_from("<H", z, at + 28)[0]
        if z[at + 46:at + 46 + name_len] == path:
            return z[:at + 16] + struct.pack("<I", value) + z[at + 20:]
        at += 4


def _overstate_size(z, path, add):
    """the archive with the decompressed size of `path` raised by `add` in the central directory and in the local header"""
    at = 0
    while True:
        at = z.index(b"PK\x01\x02", at)
        name_len = struct.unpack_from("<H", z, at + 28)[0]
        if z[at + 46:at + 46 + name_len] == path:
            break
        at += 4
    size, local = struct.unpack_from("<I", z, at + 24)[0], struct.unpack_from("<I", z, at + 42)[0]
    assert z[local:local + 4] == b"PK\x03\x04" and struct.unpack_from("<I", z, local + 22)[0] == size
    z = z[:at + 24] + struct.pack("<I", size + add) + z[at + 28:]
    return z[:local + 22] + struct.pack("<I", size + add) + z[local + 26:]


@pytest.mark.parametrize("overstated", [False, True], ids=["fixture", "a_directory_size_above_the_real_one"])
@pytest.mark.parametrize("level", [None, 1])
def test_archive_recode_deflated_writes_the_bytes_of_extract_then_add(gpu_ctx, level, overstated):
    """overstated: the directory says 100 bytes more than the member inflates to, with the right CRC-32.  ?decompressed_size
    is only the most a stream may inflate to, so the member extracts, and File.deflate_of_binary_string gives the recoded
    member the length of what was extracted: so must the device's way"""
    from zipc_amd import zipc_host

    z = util.zip_docs()
    first = util.kat()["zip_docs"]["members"][0]
    if overstated:
        z = _overstate_size(z, first["path"].encode(), 100)
    a = zipc_host.Archive.of_binary_string(z)
    b = zipc_host.Archive.of_binary_string(z)
    n_deflated = 0
    for i, m in enumerate(a.members()):  # the present path: File.to_binary_string |> File.deflate_of_binary_string, same mtime / mode
        if not m["is_dir"] and m["compression"] == 8 and not m["is_encrypted"]:
            b.add_file_deflate(m["path"], a.member_to_binary_string(i)[0], level=level, mtime=m["mtime"], mode=m["mode"])
            n_deflated += 1
    assert n_deflated >= 2
    assert a.member(a.find(first["path"].encode()))["decompressed_size"] == first["decompressed_size"] + (100 if overstated else 0)
    a.recode_deflated(level)
    assert a.to_binary_string() == b.to_binary_string()
    assert a.member(a.find(first["path"].encode()))["decompressed_size"] == first["decompressed_size"]
    assert [(m["path"], m["mtime"], m["mode"], m["decompressed_crc_32"]) for m in a.members()] == \
        [(m["path"], m["mtime"], m["mode"], m["decompressed_crc_32"]) for m in zipc_host.Archive.of_binary_string(z).members()]
    if level == 1:
        assert a.to_binary_string() != z  # (the fixture is not what `Fast makes: the members were replaced)


def test_archive_recode_deflated_reports_the_crc_message_and_changes_nothing(gpu_ctx):
    from zipc_amd import zipc_host

    z = util.zip_docs()
    members = util.kat()["zip_docs"]["members"]
    path, crc = members[-1]["path"].encode(), members[-1]["crc32"]
    bad = _patch_directory_crc(z, path, crc ^ 0x40)
    a = zipc_host.Archive.of_binary_string(bad)
    before = a.to_binary_string()
    with pytest.raises(zipc_host.ZipcError) as e:
        a.recode_deflated(1)
    assert e.value.code == zipc_host.ERROR
    assert e.value.msg == path.decode() + ": Checksum mismatch, expected %x found %x)" % (crc ^ 0x40, crc)
    assert a.to_binary_string() == before
    try:  # (the text File.to_binary_string gives for that member today)
        a.member_to_binary_string(a.find(path))
        raise AssertionError("the patched member extracted")
    except zipc_host.ZipcError as single:
        assert e.value.msg == path.decode() + ": " + single.msg
