"""The lane-serial halves of the kernels (zipc_amd/csrc/*_lane.h) compiled with
g++ and driven on the CPU, against the oracle.  This checks the kernel LOGIC on
the build box; the kernels themselves are checked on the GPU (test_gpu_*.py).
No GPU, and nothing here is a product path."""
import ctypes as C
import random

import pytest

import mutation
import util
from host_sim import lib as sim_lib


@pytest.fixture(scope="module")
def sim():
    return sim_lib()


def sim_inflate(sim, raw, cap, limit=None, crc_op=0, budget=512):
    dst = C.create_string_buffer(max(cap, 1) + 64)
    ol, ck = C.c_uint64(), C.c_uint32()
    st = sim.sim_inflate(raw, len(raw), dst, cap, int(limit is not None), limit or 0, crc_op,
                         C.byref(ol), C.byref(ck), budget)
    return st, dst.raw[:ol.value], ck.value


def sim_deflate(sim, oracle, data, level):
    cap = oracle.deflate_bound(len(data))
    dst = C.create_string_buffer(cap)
    ol, ad, kinds, nk = C.c_uint64(), C.c_uint32(), (C.c_int * 64)(), C.c_int()
    st = sim.sim_deflate(data, len(data), level, dst, cap, C.byref(ol), C.byref(ad), kinds, 64, C.byref(nk))
    return st, dst.raw[:ol.value], ad.value, list(kinds[:min(nk.value, 64)])


def test_inflate_lane_golden_streams(sim, oracle):
    for s in util.zlib_streams():
        st0, d0, a0 = oracle.inflate(s["raw"], crc_op=oracle.CRC_ADLER32)
        for budget in (512, 7):
            st, d, a = sim_inflate(sim, s["raw"], s["plain_len"] + 100, crc_op=2, budget=budget)
            assert (st, d, a) == (st0, d0, a0), s["name"]
        for lim in (s["plain_len"], s["plain_len"] + 1, max(0, s["plain_len"] - 1)):
            st0, d0, _ = oracle.inflate(s["raw"], decompressed_size=lim)
            st, d, _ = sim_inflate(sim, s["raw"], lim, limit=lim)
            assert (st, d) == (st0, d0), (s["name"], lim)


def test_inflate_lane_accept_reject_fuzz(sim, oracle):
    seen = {}
    for i, s in enumerate(util.zlib_streams()):
        if len(s["raw"]) > 40000:
            continue
        cap = s["plain_len"] * 2 + 1000
        for r in util.corrupt_variants(s["raw"], i, 60):
            st0, d0, a0 = oracle.inflate(r, decompressed_size=cap, crc_op=oracle.CRC_ADLER32)
            st, d, a = sim_inflate(sim, r, cap, limit=cap, crc_op=2)
            assert st == st0 and d == d0 and (st != 0 or a == a0), s["name"]
            seen[st] = seen.get(st, 0) + 1
    assert seen.get(0, 0) > 50 and seen.get(1, 0) > 50


def test_inflate_wide_turn_model(sim, oracle, monkeypatch):
    """The kernel's wide turn (64 speculative symbol decodes, chain by pointer
    doubling, parallel commit), modelled on the host: same bytes, same accept /
    reject, on the golden streams and on damaged ones."""
    monkeypatch.setenv("SIM_INFLATE_WIDE", "1")
    seen = {}
    for i, s in enumerate(util.zlib_streams()):
        st0, d0, a0 = oracle.inflate(s["raw"], crc_op=oracle.CRC_ADLER32)
        for budget in (24, 3, 400):
            st, d, a = sim_inflate(sim, s["raw"], s["plain_len"] + 100, crc_op=2, budget=budget)
            assert (st, d, a) == (st0, d0, a0), s["name"]
        lim = max(0, s["plain_len"] - 1)
        assert sim_inflate(sim, s["raw"], lim, limit=lim)[0] == oracle.inflate(s["raw"], decompressed_size=lim)[0]
        if len(s["raw"]) > 40000:
            continue
        cap = s["plain_len"] * 2 + 1000
        for r in util.corrupt_variants(s["raw"], i, 40):
            st0, d0, a0 = oracle.inflate(r, decompressed_size=cap, crc_op=oracle.CRC_ADLER32)
            st, d, a = sim_inflate(sim, r, cap, limit=cap, crc_op=2)
            assert st == st0 and d == d0 and (st != 0 or a == a0), s["name"]
            seen[st] = seen.get(st, 0) + 1
    assert seen.get(0, 0) > 30 and seen.get(1, 0) > 30
    for name, data in util.deflate_cases(small=True).items():
        for lvl in (0, 2):
            c = oracle.deflate(data, level=lvl)[1]
            assert sim_inflate(sim, c, len(data), limit=len(data))[:2] == (0, data), name


def test_deflate_lane_logic_bytes_equal_oracle(sim, oracle):
    for name, data in util.deflate_cases().items():
        for lvl in (0, 1, 2, 3):
            st0, c0, a0, blocks = oracle.deflate_trace(data, level=lvl, crc_op=oracle.CRC_ADLER32)
            st, c, a, kinds = sim_deflate(sim, oracle, data, lvl)
            assert st == 0 and c == c0 and a == a0, (name, lvl)
            assert kinds == [b.kind for b in blocks][:64], (name, lvl)


def test_parse_tiles_model_bytes_equal_oracle(sim, oracle, monkeypatch):
    """lz_parse_kernel's algorithm (pointer doubling + marking per 64-position
    tile instead of a serial walk), modelled on the host, gives the same bytes."""
    monkeypatch.setenv("SIM_PARSE_TILES", "1")
    for name, data in util.deflate_cases().items():
        for lvl in (1, 2, 3):
            st0, c0, a0 = oracle.deflate(data, level=lvl, crc_op=oracle.CRC_ADLER32)
            st, c, a, _ = sim_deflate(sim, oracle, data, lvl)
            assert st == 0 and c == c0 and a == a0, (name, lvl)


def _sim_cases_for_segments():
    """the deflate cases plus what the segment stitch is about: runs of one byte and short periods (paths that stay
    out of phase), long enough for several segments and blocks"""
    cases = dict(util.deflate_cases())
    rnd = random.Random(5)
    for k in (1, 2, 3, 7, 64, 257, 258, 259, 260, 515, 1000):
        pat = bytes(rnd.randrange(256) for _ in range(k))
        cases["period_%d" % k] = (pat * (150000 // k + 1))[:150000 + k]
    t = bytearray(util.text(200000, 9))
    t[50000:120000] = b"ab" * 35000
    t[140000:170000] = bytes(30000)
    cases["text_with_runs"] = bytes(t)
    return cases


@pytest.mark.parametrize("seg", [64, 4096, 8192])
def test_parse_segments_model_bytes_equal_oracle(sim, oracle, monkeypatch, seg):
    """lz_parse by segments (lz_parse_spec / _stitch / _gather_kernel): the algorithm on the host -- every segment
    parsed from its first position, stitched where the true path meets it within a tile, runs of equal steps, the
    block cut at the step that holds the block's byte 65534 -- gives the reference's bytes (64: a segment per tile,
    every boundary case many times over)."""
    monkeypatch.setenv("SIM_PARSE_SEGMENTS", str(seg))
    for name, data in _sim_cases_for_segments().items():
        for lvl in ((1, 2, 3) if seg != 64 else (2,)):
            st0, c0, a0 = oracle.deflate(data, level=lvl, crc_op=oracle.CRC_ADLER32)
            st, c, a, _ = sim_deflate(sim, oracle, data, lvl)
            assert st == 0 and c == c0 and a == a0, (name, lvl, seg)


def test_blocks_coded_independently_model_bytes_equal_oracle(sim, oracle, monkeypatch):
    """deflate_plan / _counts / _codelen / _scan_kernel's split of the block coder: what a block's bits owe to the
    blocks before it is the bit it starts at, the counts of the code-length symbols (never reset, Q1) and nothing
    else; the sizes the scan goes by are the real ones (a stored block's estimate runs 8 high when its type bits end
    a byte, Q3; a dynamic block's counts every block's code-length symbols)."""
    monkeypatch.setenv("SIM_EMIT_BLOCKS", "1")
    monkeypatch.setenv("SIM_PARSE_SEGMENTS", "4096")
    for name, data in _sim_cases_for_segments().items():
        for lvl in (1, 2, 3):
            st0, c0, a0 = oracle.deflate(data, level=lvl, crc_op=oracle.CRC_ADLER32)
            st, c, a, _ = sim_deflate(sim, oracle, data, lvl)
            assert st == 0 and c == c0 and a == a0, (name, lvl)


def test_deflate_lane_logic_fuzz(sim, oracle):
    rnd = random.Random(11)
    for t in range(600):
        n = rnd.randrange(0, 600)
        kind = rnd.randrange(4)
        if kind == 0:
            data = util.rand_bytes(n, t)
        elif kind == 1:
            data = util.rand_bytes(n, t, 2)
        elif kind == 2:
            data = (util.rand_bytes(rnd.randrange(1, 20), t) * (n // 2 + 1))[:n]
        else:
            data = util.text(n, t)
        lvl = rnd.randrange(1, 4)
        st0, c0, a0 = oracle.deflate(data, level=lvl, crc_op=oracle.CRC_ADLER32)
        st, c, a, _ = sim_deflate(sim, oracle, data, lvl)
        assert st == 0 and c == c0 and a == a0, (t, n, kind, lvl)


def test_chain_round_model_equals_serial_chain(sim):
    """lz_chain_kernel's round algorithm, with the surviving LDS store picked at
    random, yields the reference's insert_hash links."""
    cases = {
        "zeros": bytes(70000), "rand": util.rand_bytes(70000, 1), "nib": util.rand_bytes(70000, 2, 4),
        "nib3": util.rand_bytes(100000, 3, 3), "p2": b"ab" * 20000, "p9": b"abcdefghi" * 6000,
        "p300": util.rand_bytes(300, 4) * 200, "text": util.text(80000, 5), "bin": util.rand_bytes(50000, 6, 1),
        "short": b"abcabcabcab", "tiny": b"abcd", "n1027": util.rand_bytes(1027, 7),
        "old": util.rand_bytes(100, 8) + bytes(70000) + util.rand_bytes(100, 8) + bytes(70000),
    }
    for name, d in cases.items():
        n = len(d)
        for seed in (1, 2):
            a, b, mt = (C.c_uint16 * (n + 8))(), (C.c_uint16 * (n + 8))(), C.c_int()
            sim.sim_chain(d, n, a, seed, C.byref(mt))
            sim.sim_chain_serial(d, n, b)
            assert list(a[:max(0, n - 3)]) == list(b[:max(0, n - 3)]), name


def test_chain_links_by_segments_equal_serial_chain(sim):
    """lz_chain_segments_kernel's claim: a link is a function of the 32 KiB before its position, so a stream's links
    can be made a segment at a time, each from an empty table 32 768 positions before its first one."""
    cases = {
        "text": util.text(200000, 5), "nib": util.rand_bytes(150000, 2, 4), "nib3": util.rand_bytes(150000, 3, 3),
        "zeros": bytes(120000), "p300": util.rand_bytes(300, 4) * 500,
        "old": util.rand_bytes(100, 8) + bytes(70000) + util.rand_bytes(100, 8) + bytes(70000),
        "far": util.rand_bytes(40000, 9) + util.text(33000, 1) + util.rand_bytes(40000, 9) + util.text(70000, 2),
    }
    for name, d in cases.items():
        n = len(d)
        b = (C.c_uint16 * (n + 8))()
        sim.sim_chain_serial(d, n, b)
        for seg in (16384, 32768, 131072):
            a = (C.c_uint16 * (n + 8))()
            sim.sim_chain_segments(d, n, a, 3, seg)
            assert list(a[:n - 3]) == list(b[:n - 3]), (name, seg)


def test_symbol_value_closed_forms_equal_rfc_tables(sim):
    assert sim.sim_sym_values_match_tables() == 0


def test_crc_combination_rule(sim, oracle):
    rnd = random.Random(5)
    for _ in range(100):
        a, b = util.rand_bytes(rnd.randrange(0, 5000), rnd.random()), util.rand_bytes(rnd.randrange(0, 5000), rnd.random())
        raw_b = oracle.crc32_update(0, b)
        st_a = oracle.crc32_update(0xFFFFFFFF, a)
        assert sim.sim_crc_advance(st_a, raw_b, len(b)) == oracle.crc32_update(0xFFFFFFFF, a + b)


def test_inflate_models_header_fuzz(sim, oracle, monkeypatch):
    """random complete / perturbed Huffman codes in dynamic headers: plain and wide model vs oracle"""
    streams = util.header_fuzz_streams(78, 150, 450)
    for wide in (False, True):
        if wide:
            monkeypatch.setenv("SIM_INFLATE_WIDE", "1")
        for s in streams:
            st0, d0, c0 = oracle.inflate(s, decompressed_size=1 << 16, crc_op=2)
            st, d, a = sim_inflate(sim, s, 1 << 16, limit=1 << 16, crc_op=2, budget=24)
            assert st == st0
            if st0 == 0:
                assert d == d0 and a == c0


def test_inflate_span_model(sim, oracle, monkeypatch):
    """inflate_span.h (regions per lane, self-synchronising walks, LDS output tiles) -- the very
    code the kernel runs, on the emulated wave (host_sim/wave_emu.h), lanes resumed in ascending
    and in descending order: same bytes, checksums and statuses as the oracle on every input
    shape, under size limits that fall inside a span, and on damaged streams."""
    monkeypatch.setenv("SIM_INFLATE_WIDE", "1")
    stats = (C.c_uint64 * 8).in_dll(sim, "sim_span_stats")
    r = random.Random(2024)
    long_random = []
    while len(long_random) < 24:
        try:
            long_random.append(util.random_dynamic_stream(r, 0, max_symbols=9000))
        except (KeyError, IndexError, ValueError):
            pass
    for order in ("a", "d"):
        monkeypatch.setenv("SIM_INFLATE_SPAN", order)
        for i in range(8):
            stats[i] = 0
        for name, data in util.deflate_cases().items():
            for lvl in (0, 1, 2, 3) if order == "a" else (2,):
                st0, c, a0 = oracle.deflate(data, level=lvl, crc_op=oracle.CRC_ADLER32)
                st, d, a = sim_inflate(sim, c, len(data), limit=len(data), crc_op=2, budget=24)
                assert (st, d, a) == (0, data, a0), (name, lvl, order)
        assert stats[0] > 20 and stats[2] > 900000, list(stats)  # spans ran and produced most of the bytes
        # limits inside the data: the reference's "Expected decompression size exceeded", same prefix rules
        for name in ("nib64k", "text150k", "mixed", "zip-docs/rfc1951.txt"):
            data = util.deflate_cases()[name]
            c = oracle.deflate(data, level=2)[1]
            for lim in (len(data) - 1, len(data) // 2, 5000, len(data) - 300):
                st0, d0, _ = oracle.inflate(c, decompressed_size=lim)
                st, d, _ = sim_inflate(sim, c, lim, limit=lim)
                assert (st, d) == (st0, d0), (name, lim, order)
        for s in util.zlib_streams():
            st0, d0, a0 = oracle.inflate(s["raw"], crc_op=oracle.CRC_ADLER32)
            st, d, a = sim_inflate(sim, s["raw"], s["plain_len"] + 100, crc_op=2, budget=24)
            assert (st, d, a) == (st0, d0, a0), s["name"]
        # binary-like: stretches a span cannot take (zeros, short periods: granules too rich for a tile) between
        # stretches it can -- the span steps aside for the wide turns and comes back (SPAN_LATER), again and again
        rb = random.Random(77)
        for shape in range(3):
            parts = []
            while sum(map(len, parts)) < 150000:
                parts.append(bytes(rb.randrange(256 if shape else 16) for _ in range(rb.randrange(200, 6000))))
                parts.append(bytes([0, 0xFF, 0x90][shape]) * rb.randrange(300, 9000) if rb.random() < 0.7
                             else bytes(rb.randrange(256) for _ in range(rb.randrange(1, 9))) * rb.randrange(100, 1500))
                parts.append(util.deflate_cases()["text150k"][rb.randrange(0, 100000):][:rb.randrange(500, 8000)])
            data = b"".join(parts)
            spans_before = stats[0]
            st0, c, a0 = oracle.deflate(data, level=2, crc_op=oracle.CRC_ADLER32)
            st, d, a = sim_inflate(sim, c, len(data), limit=len(data), crc_op=2, budget=24)
            assert (st, d, a) == (0, data, a0), (shape, order)
            assert stats[0] - spans_before > 6, (shape, list(stats))  # spans kept coming back after the runs
        # more holes than a tile lists (SPAN_LIST_MAX): thousands of 3-byte matches in a row, hand-made
        for length, dist, n, seed in ((3, 3, 6000, None), (3, 1, 3000, None), (3, 4, 8000, 1), (4, 4, 8000, 2), (4, 2, 5000, 3)):
            c, data = util.fixed_block_of_short_matches(n, length, dist, seed=seed)
            st0, d0, a0 = oracle.inflate(c, decompressed_size=len(data), crc_op=2)
            st, d, a = sim_inflate(sim, c, len(data), limit=len(data), crc_op=2, budget=24)
            assert (st0, d0) == (0, data) and (st, d, a) == (0, data, a0), (length, dist, order)
        # random literals and matches at every mix of lengths and distances, hand-made
        for seed in range(8 if order == "a" else 3):
            c, data = util.random_fixed_block(seed, 5000, max_dist=[1, 4, 64, 300, 5000, 3, 16, 32768][seed], max_len=[3, 4, 10, 40, 258][seed % 5],
                                              lit_share=[0.0, 0.05, 0.5][seed % 3])
            st0, d0, a0 = oracle.inflate(c, decompressed_size=len(data), crc_op=2)
            st, d, a = sim_inflate(sim, c, len(data), limit=len(data), crc_op=2, budget=24)
            assert (st0, d0) == (0, data) and (st, d, a) == (0, data, a0), (seed, order)
        # random complete codes (long codes, odd alphabets), thousands of symbols; then damaged
        seen = {}
        for k, s in enumerate(long_random):
            st0, d0, a0 = oracle.inflate(s, decompressed_size=1 << 21, crc_op=2)
            st, d, a = sim_inflate(sim, s, 1 << 21, limit=1 << 21, crc_op=2, budget=24)
            assert st0 == 0 and (st, d, a) == (st0, d0, a0), k
            for v in util.corrupt_variants(s, k, 6 if order == "a" else 2):
                st0, d0, a0 = oracle.inflate(v, decompressed_size=1 << 21, crc_op=2)
                st, d, a = sim_inflate(sim, v, 1 << 21, limit=1 << 21, crc_op=2, budget=24)
                assert st == st0 and (st != 0 or (d == d0 and a == a0)), k
                seen[st] = seen.get(st, 0) + 1
        for i, s in enumerate(util.zlib_streams()):
            if len(s["raw"]) < 2000:
                continue
            cap = s["plain_len"] * 2 + 1000
            for v in util.corrupt_variants(s["raw"], i, 12 if order == "a" else 4):
                if len(v) > 300 and r.random() < 0.5:  # damage past the header too
                    b = bytearray(v)
                    b[r.randrange(200, len(b))] ^= 1 << r.randrange(8)
                    v = bytes(b)
                st0, d0, a0 = oracle.inflate(v, decompressed_size=cap, crc_op=oracle.CRC_ADLER32)
                st, d, a = sim_inflate(sim, v, cap, limit=cap, crc_op=2)
                assert st == st0 and (st != 0 or (d == d0 and a == a0)), s["name"]
                seen[st] = seen.get(st, 0) + 1
        assert seen.get(0, 0) > 5 and seen.get(1, 0) > 20, seen


def test_huffman_two_queues_equal_the_heap(sim):
    """Huffman.lengths_of_freqs (zd.ml:404-473) two ways: the reference's heap (huff_lengths_of_freqs, what the
    oracle restates) and the two queues deflate_emit runs (huff_lengths_of_freqs_tq).  The tree is a function
    of the order of the keys (freq << 10) | link, so frequency ties -- merged nodes before leaves, later merged
    nodes first -- and the flatten-and-retry path are what must agree."""
    import numpy as np

    r = random.Random(20261003)

    def fib(n):
        a, b, out = 1, 1, []
        for _ in range(n):
            out.append(a)
            a, b = b, a + b
        return out

    for it in range(20000):
        kind = it % 9
        max_sym, max_len = ((285, 15), (29, 15), (18, 7))[it % 3]
        n = max_sym + 1
        if kind == 0: fr = [r.choice([0, 1]) for _ in range(n)]
        elif kind == 1: fr = [r.choice([0, 1, 2]) for _ in range(n)]
        elif kind == 2: fr = [r.choice([0, 1, 2, 4, 8, 16]) for _ in range(n)]
        elif kind == 3: fr = [r.randrange(0, 5) for _ in range(n)]
        elif kind == 4: fr = [r.randrange(0, 70000) if r.random() < 0.5 else 0 for _ in range(n)]
        elif kind == 5:
            fr = [0] * n
            fb = fib(min(n, 30))
            for i, v in zip(r.sample(range(n), len(fb)), fb):
                fr[i] = min(v, 65535)
        elif kind == 6:
            fr = [0] * n
            for i in r.sample(range(n), r.randrange(0, min(n, 6) + 1)):
                fr[i] = r.randrange(1, 4)
        elif kind == 7: fr = [int(2 ** r.uniform(0, 16)) if r.random() < 0.7 else 0 for _ in range(n)]
        else:
            base = r.randrange(1, 1000)
            fr = [base * r.choice([0, 1, 1, 2, 3]) for _ in range(n)]
        f = np.array(fr, np.uint32)
        a = np.zeros(n, np.uint32)
        b = np.zeros(n, np.uint32)
        assert sim.sim_huff_lengths(f.ctypes.data, max_sym, max_len, a.ctypes.data, b.ctypes.data) == 0, (it, fr)


def _find_sources():
    import os
    import zlib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = (open(os.path.join(root, "SURVEY.md"), "rb").read() + open(os.path.join(root, "BASELINE.md"), "rb").read() * 40)[:150000]
    assert len(text) == 150000
    rnd = random.Random(11)
    symbols = bytes(rnd.randrange(16) * 17 for _ in range(150000))
    records = b"".join(bytes([rnd.randrange(256), rnd.randrange(64)]) * 2 for _ in range(40000))
    for name, data in (("text", text), ("symbols", symbols), ("records", records)):
        yield name, data, zlib


def test_block_header_search_finds_every_dynamic_block(sim, oracle):
    """inflate_find.h (the search of inflate.hip's one-stream path) over every bit offset of streams of the
    reference's encoder (the oracle) and of zlib: every block with a dynamic header is found where the inflate model
    says it starts, and next to nothing else passes."""
    sim.sim_find_candidates.restype = C.c_uint64
    sim.sim_inflate_block_starts.restype = C.c_uint64
    for name, data, zlib in _find_sources():
        streams = [("oracle-%d" % lv, oracle.deflate(data, level=lv)[1]) for lv in (1, 2)]
        for lv in (1, 6):
            c = zlib.compressobj(lv, zlib.DEFLATED, -15)
            streams.append(("zlib-%d" % lv, c.compress(data) + c.flush()))
        for enc, raw in streams:
            st, d, _ = sim_inflate(sim, raw, len(data), limit=len(data))
            assert st == 0 and d == data, (name, enc)
            bits, types = (C.c_uint64 * 4096)(), (C.c_int * 4096)()
            nb = sim.sim_inflate_block_starts(bits, types, 4096)
            starts = {int(bits[i]) for i in range(nb) if types[i] == 2}
            assert nb >= 2 and len(starts) >= 1, (name, enc, nb)
            cand, nf = (C.c_uint64 * 65536)(), C.c_uint64()
            nc = sim.sim_find_candidates(raw, len(raw), cand, 65536, C.byref(nf))
            found = {int(cand[i]) for i in range(nc)}
            assert 0 in found
            assert starts <= found, (name, enc, sorted(starts - found))
            assert len(found - starts - {0}) <= 1, (name, enc, sorted(found - starts))
            assert nf.value < len(raw) // 32  # what the first test lets through to the second


def test_inflate_token_form_resolves_to_the_plain_decode(sim, oracle):
    """inflate.hip's IM_TOKEN form of the span decoder on the emulated wave (literals stored, a match's bytes written
    down as the positions they copy -- directly, or "following": what those positions copy -- tiles that are refused
    leave nothing behind), spans cut short like those of a wave that leaves at a checkpoint; the copies resolved
    afterwards must give the stream's bytes."""
    import zlib
    rnd = random.Random(5)
    datas = []
    for name, data, _ in _find_sources():
        datas.append((name, data[:90000]))
    datas.append(("runs", b"".join(bytes([rnd.randrange(256)]) * rnd.randrange(1, 700) + bytes(rnd.randrange(256) for _ in range(rnd.randrange(40)))
                                   for _ in range(300))))
    for name, data in datas:
        streams = [("oracle-2", oracle.deflate(data, level=2)[1])]
        for lv, stg in ((6, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED)):
            c = zlib.compressobj(lv, zlib.DEFLATED, -15, 8, stg)
            streams.append(("zlib-%d-%d" % (lv, stg), c.compress(data) + c.flush()))
        for enc, raw in streams:
            for follow, desc, cut in ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 20000), (1, 0, 9000)):
                dst = C.create_string_buffer(len(data) + 64)
                ol = C.c_uint64()
                st = sim.sim_inflate_token(raw, len(raw), dst, len(data), follow, desc, cut, C.byref(ol))
                assert st == 0 and ol.value == len(data) and dst.raw[:len(data)] == data, (name, enc, follow, desc, cut)


def test_coder_choose_mutants_are_killed(oracle, tmp_path):
    """tools/kernel_mutants.py's mutants of coder_choose (the block chooser's two `<=` and Q3's 8 bits of padding, the
    host models' copy of wave_choose and deflate_scan_kernel's): each built into a host model of its own, each must
    change the bytes of an input that sits on its line (util.TIE_CASES).  The GPU copies: tools/kernel_mutants.py."""
    from host_sim import _bind
    from tools import kernel_mutants as KM

    ties = util.tie_cases()
    rows = []
    for m in KM.LANE_MUTANTS:
        msim = _bind(C.CDLL(mutation.host_model(m, tmp_path / m[0])))
        changed = []
        for name, (level, _, _) in util.TIE_CASES.items():
            lv = oracle.LEVELS[level]
            st0, c0, a0 = oracle.deflate(ties[name], level=lv, crc_op=oracle.CRC_ADLER32)
            st, c, a, _ = sim_deflate(msim, oracle, ties[name], lv)
            if (st, c) != (st0, c0):
                changed.append(name)
        rows.append((m[0], changed))
    print("\n".join("%-28s %s" % (n, ("killed by " + " ".join(c)) if c else "SURVIVED") for n, c in rows))
    assert all(c for _, c in rows), rows


def test_inflate_lane_equals_the_oracle_on_the_rule_cases(sim, oracle, monkeypatch):
    """inflate_lane.h (plain step, fixed path, serial header and stored code) and its wide turn on every case of
    tests/golden/inflate_rules.py in every wrapper, at budgets 512 and 7: status, bytes and Adler-32 as the oracle."""
    import sys

    sys.path.insert(0, util.GOLDEN)
    import inflate_rules

    cases = inflate_rules.wrapped_cases()
    for wide in (False, True):
        if wide:
            monkeypatch.setenv("SIM_INFLATE_WIDE", "1")
        for name, c in cases.items():
            cap = c.limit if c.limit is not None else 1 << 20
            st0, d0, a0 = oracle.inflate(c.stream, decompressed_size=cap, crc_op=oracle.CRC_ADLER32)
            for budget in (512, 7):
                st, d, a = sim_inflate(sim, c.stream, cap, limit=cap, crc_op=2, budget=budget)
                assert st == st0 and (st != 0 or (d, a) == (d0, a0)), (name, wide, budget, st, st0)


# (name, file, text, replacement): relaxed mutants of inflate_lane.h -- they accept more, and stay in bounds.  They run only
# in the host models, in child processes, beside the host copies of the stricter ones the GPU runs too
# (tools/kernel_mutants.py LANE_INFLATE_MUTANTS); no GPU library is ever built from these.
LANE_INFLATE_RELAXED = [
    ("lane_nlen_unchecked", "inflate_lane.h", "if (length != ((~inv) & 0xFFFFu))", "if (0 && length != ((~inv) & 0xFFFFu))"),
    ("lane_single_code_any_length", "inflate_lane.h",
     "if ((num_codes > 1 && available > 0) || (num_codes == 1 && L.u16(counts_off, 1) != 1))",
     "if (num_codes > 1 && available > 0)"),
    ("lane_incomplete_ok", "inflate_lane.h",
     "if ((num_codes > 1 && available > 0) || (num_codes == 1 && L.u16(counts_off, 1) != 1))",
     "if (num_codes == 1 && L.u16(counts_off, 1) != 1)"),
]

_LANE_CHILD = r"""
import ctypes as C, json, os, sys
sys.path.insert(0, os.path.join(sys.argv[2], "tests")); sys.path.insert(0, os.path.join(sys.argv[2], "tests", "golden"))
sys.path.insert(0, sys.argv[2])
import oracle, inflate_rules
from host_sim import _bind
sim = _bind(C.CDLL(sys.argv[1]))
changed = []
for name, c in inflate_rules.wrapped_cases().items():
    cap = c.limit if c.limit is not None else 1 << 20
    st0, d0, a0 = oracle.inflate(c.stream, decompressed_size=cap, crc_op=oracle.CRC_ADLER32)
    dst = C.create_string_buffer(cap + 64)
    ol, ck = C.c_uint64(), C.c_uint32()
    st = sim.sim_inflate(c.stream, len(c.stream), dst, cap, 1, cap, 2, C.byref(ol), C.byref(ck), 512)
    if st != st0 or (st == 0 and (dst.raw[:ol.value], ck.value) != (d0, a0)):
        changed.append(name)
print(json.dumps(changed))
"""


def test_inflate_lane_mutants_are_killed(oracle, tmp_path, capsys):
    """The mutants of inflate_lane.h -- the stricter ones the GPU runs too (tools/kernel_mutants.py), and the relaxed ones
    above -- each built into a host model of its own and run over every rule case (tests/golden/inflate_rules.py) in a child
    process, plain and wide: each must change a result.  A relaxed mutant that read out of bounds would end its child,
    not this run (and would count as a kill only through the results it printed: none)."""
    import os

    from tools import kernel_mutants as KM

    muts = [(m, "stricter") for m in KM.LANE_INFLATE_MUTANTS] + [(m, "relaxed") for m in LANE_INFLATE_RELAXED]
    sos = mutation.build_all(lambda m: mutation.host_model(m, tmp_path / m[0]), [m for m, _ in muts])
    rows = []
    for (m, kind), so in zip(muts, sos):
        changed, notes = set(), []
        for wide in ("0", "1"):
            env = dict(os.environ)
            env.pop("SIM_INFLATE_WIDE", None)
            if wide == "1":
                env["SIM_INFLATE_WIDE"] = "1"
            rc, got, _ = mutation.run_child(_LANE_CHILD, so, mutation.ROOT, env=env, timeout=600)
            if rc != 0:
                notes.append("child rc %d" % rc)
                continue
            changed |= set(got)
        rows.append((m[0], kind, sorted(changed), notes))
    with capsys.disabled():
        print("\ninflate_lane.h mutants in the host models against the rule cases")
        for n, kind, changed, notes in rows:
            print("  %-34s %-9s %4d changed  %s %s" % (n, kind, len(changed), changed[0] if changed else "SURVIVED", " ".join(notes)))
        print("  %d of %d killed" % (sum(bool(c) for _, _, c, _ in rows), len(rows)))
    assert all(c and not notes for _, _, c, notes in rows), rows


def test_block_header_search_finds_the_dynamic_headers_around_the_rule_cases(sim, oracle):
    """inflate_find.h on the accepted rule cases inside long streams (tests/golden/inflate_rules.py, wrapper e): every
    dynamic block the inflate model decodes is among the candidates the search lists."""
    import sys

    sys.path.insert(0, util.GOLDEN)
    import inflate_rules

    sim.sim_find_candidates.restype = C.c_uint64
    sim.sim_inflate_block_starts.restype = C.c_uint64
    n = 0
    for name, c in inflate_rules.wrapped_cases("e").items():
        if not name.endswith("/e") or c.status != 0:
            continue
        st, d, _ = sim_inflate(sim, c.stream, len(c.plain), limit=len(c.plain))
        assert st == 0 and d == c.plain, name
        bits, types = (C.c_uint64 * 4096)(), (C.c_int * 4096)()
        nb = sim.sim_inflate_block_starts(bits, types, 4096)
        starts = {int(bits[i]) for i in range(nb) if types[i] == 2}
        cand, nf = (C.c_uint64 * 65536)(), C.c_uint64()
        nc = sim.sim_find_candidates(c.stream, len(c.stream), cand, 65536, C.byref(nf))
        found = {int(cand[i]) for i in range(nc)}
        assert len(starts) >= 4 and starts <= found, (name, sorted(starts - found))
        n += 1
    assert n >= 25


# ---- the launch rules (zipc_amd/csrc/forms.h, tests/host_sim/sim_forms.cpp) ------------------------------------------
# Every expected value below is written out by hand from the rules as launch_deflate_group and inflate_by_blocks stated
# them before they moved into forms.h, with the arithmetic beside it; none is the output of the functions under test.
#   tps  = 1 if L - 4 < 49152 else 2 + (L - 4 - 49152) // 16384      cps = ceil(L / 1024)
#   tpg  = n * tps // 8192 within [1, tps]                           gps = ceil(tps / tpg)
#   segp = 4096 / 8192 / 16384 for L <= 4 MiB / <= 32 MiB / longer, doubled while < 32768 and n * ceil(L / (2 segp)) >= 65536
#   sps  = ceil(L / segp)      bps = L // 65277 + 2
#   segmented = sps >= 8 and (n <= 2048 or (n <= 4096 and L >= 512 KiB) or (n <= 8192 and L >= 1 MiB))
#   slices = 2, one less while n // slices < 2048
import host_sim as H

KIB, MIB, GIB = 1 << 10, 1 << 20, 1 << 30

FORMS_ROWS = [
    # (what, arguments of host_sim.deflate_forms, expected fields of the group, expected fields of the slice)
    # --- the matcher: streams of up to 8192 bytes keep lz_match_kernel, cps = 8 tiles of 1024: grid 4 * 8 = 32
    ("matcher 8192", dict(n=4, max_src_len=8192), dict(cps=8, segmented=0), dict(match_window=0, match_grid=32)),
    # 8193: the window kernel; tps = 1, tpg = 4 * 1 // 8192 = 0 -> 1, gps = 1, gpw = 4 // 2048 = 0 -> 1, 4 workgroups -> 8
    ("matcher 8193", dict(n=4, max_src_len=8193), dict(tps=1, tpg=1, gps=1), dict(match_window=1, gpw=1, match_grid=8)),
    # --- lz_chain by exchange, by segments: n < 1024 and L > 192 KiB
    ("xchg 1023 x 192 KiB", dict(n=1023, max_src_len=192 * KIB), dict(xseg=0, xsegs=1), dict(chain=H.CHAIN_XCHG, chain_grid=1023)),
    # xseg = 98304: 1023 * ceil(196609 / 196608) = 2046 < 2048, no doubling; xsegs = ceil(196609 / 98304) = 3; grid 1023 * 3
    ("xchg 1023 x 192 KiB + 1", dict(n=1023, max_src_len=192 * KIB + 1), dict(xseg=98304, xsegs=3),
     dict(chain=H.CHAIN_XCHG_SEGMENTS, chain_grid=3069)),
    ("xchg 1024 x 192 KiB + 1", dict(n=1024, max_src_len=192 * KIB + 1), dict(xseg=0, xsegs=1), dict(chain=H.CHAIN_XCHG, chain_grid=1024)),
    # 1023 * ceil(393217 / 196608) = 1023 * 3 >= 2048: xseg doubles to 196608; 1023 * ceil(393217 / 393216) = 2046: stays; xsegs = 3
    ("xchg doubling", dict(n=1023, max_src_len=384 * KIB + 1), dict(xseg=196608, xsegs=3), dict(chain=H.CHAIN_XCHG_SEGMENTS, chain_grid=3069)),
    # --- sps 7 / 8 (segp 4096): 28672 = 7 * 4096
    ("sps 7", dict(n=2, max_src_len=28672), dict(segp=4096, sps=7, segmented=0, n_slots=0, tiles=0, seg_syms=0),
     dict(streams=2, segments=0, blocks=0, ppb=0)),
    # sps 8: P = 2 * 28673 + 512 * 2 + 256 = 58626; n_slots = 58626 // 4096 + 2 + 1 = 17; tiles = 58626 // 64 + 4 = 920;
    # seg_syms = 4096 + 576; bps = 0 + 2; slice of 2: 16 segments, 4 blocks <= 2048 -> ppb 8, bits = pack = 32, seal ceil(32 / 256)
    ("sps 8", dict(n=2, max_src_len=28673), dict(segp=4096, sps=8, segmented=1, segments_required=0, bps=2, n_slots=17, tiles=920, seg_syms=4672),
     dict(chain=H.CHAIN_XCHG, chain_grid=2, streams=2, segments=16, blocks=4, ppb=8, bits_grid=32, pack_grid=32, seal_grid=1)),
    # ... the same without the exchange: chain_seg 32768 (2 * 1 <= 512), csegs = 1: the whole-stream peel kernel
    ("sps 8 peel", dict(n=2, max_src_len=28673, xchg_ok=0), dict(xchg_chain=0, chain_seg=32768, csegs=1), dict(chain=H.CHAIN_PEEL, chain_grid=2)),
    # ... and when the parse scratch could not be had: the forms by a wave per stream
    ("sps 8, no scratch", dict(n=2, max_src_len=28673, segments_ok=0), dict(sps=8, segmented=0, n_slots=0), dict(segments=0, ppb=0)),
    # --- n 2048 / 2049 at 32 KiB: sps = 8 (2048 * ceil(32768 / 8192) = 8192 < 65536: segp stays 4096); one slice (2048 // 2 < 2048)
    # P = 2048 * 32768 + 512 * 2048 + 256 = 68157696; n_slots = 16640 + 2048 + 1; tiles = 1064964 + 4
    # blocks = 2048 * 2 = 4096 > 2048: ppb 1, no deflate_bits, pack 4096, seal 4096 / 256 = 16
    ("2048 x 32 KiB", dict(n=2048, max_src_len=32 * KIB), dict(slices=1, sps=8, segmented=1, bps=2, n_slots=18689, tiles=1064968),
     dict(chain=H.CHAIN_XCHG, chain_grid=2048, gpw=1, match_grid=2048, segments=16384, blocks=4096, ppb=1, bits_grid=0, pack_grid=4096, seal_grid=16)),
    ("2049 x 32 KiB", dict(n=2049, max_src_len=32 * KIB), dict(slices=1, sps=8, segmented=0), dict(streams=2049, segments=0)),
    # --- n 4096 / 4097 at 512 KiB: 4096 * ceil(524288 / 8192, / 16384, / 32768) = 262144, 131072, 65536, all >= 65536:
    # segp 32768, sps = 16; two slices
    ("4096 x 512 KiB", dict(n=4096, max_src_len=512 * KIB), dict(slices=2, segp=32768, sps=16, segmented=1), {}),
    ("4097 x 512 KiB", dict(n=4097, max_src_len=512 * KIB), dict(slices=2, segp=32768, sps=16, segmented=0), {}),
    ("4096 x 512 KiB - 1", dict(n=4096, max_src_len=512 * KIB - 1), dict(segp=32768, sps=16, segmented=0), {}),
    # --- n 8192 / 8193 at 1 MiB: segp 32768 the same way, sps = 32
    ("8192 x 1 MiB", dict(n=8192, max_src_len=MIB), dict(segp=32768, sps=32, segmented=1), {}),
    ("8193 x 1 MiB", dict(n=8193, max_src_len=MIB), dict(segp=32768, sps=32, segmented=0), {}),
    ("8192 x 1 MiB - 1", dict(n=8192, max_src_len=MIB - 1), dict(segp=32768, sps=32, segmented=0), {}),
    # --- the segp steps: 4 MiB / 4096 = 1024; (4 MiB + 1) / 8192 -> 513; 32 MiB / 8192 = 4096; (32 MiB + 1) / 16384 -> 2049
    ("segp 4 MiB", dict(n=1, max_src_len=4 * MIB), dict(segp=4096, sps=1024), {}),
    ("segp 4 MiB + 1", dict(n=1, max_src_len=4 * MIB + 1), dict(segp=8192, sps=513), {}),
    ("segp 32 MiB", dict(n=1, max_src_len=32 * MIB), dict(segp=8192, sps=4096), {}),
    ("segp 32 MiB + 1", dict(n=1, max_src_len=32 * MIB + 1), dict(segp=16384, sps=2049), {}),
    # --- the doubling at 65536 waves: 64 KiB streams, ceil(65536 / 8192) = 8: 8191 * 8 = 65528, 8192 * 8 = 65536 (then 8192 * 4: stays)
    ("65528 waves", dict(n=8191, max_src_len=64 * KIB), dict(segp=4096, sps=16, segmented=0), {}),
    ("65536 waves", dict(n=8192, max_src_len=64 * KIB), dict(segp=8192, sps=8, segmented=0), {}),
    # --- the peel kernel by segments: segmented, csegs > 1, m <= 128.  1 MiB: 128 * 32 > 512, 128 * 16 > 1024: chain_seg 131072, csegs 8
    ("peel m 128", dict(n=128, max_src_len=MIB, xchg_ok=0), dict(segmented=1, sps=256, chain_seg=131072, csegs=8),
     dict(chain=H.CHAIN_PEEL_SEGMENTS, chain_grid=1024)),
    ("peel m 129", dict(n=129, max_src_len=MIB, xchg_ok=0), dict(segmented=1, chain_seg=131072, csegs=8), dict(chain=H.CHAIN_PEEL, chain_grid=129)),
    # chain_seg: 16 * 32 = 512 <= 512: 32768; 17 * 32 > 512, 17 * 16 <= 1024: 65536; 64 * 16 = 1024: 65536; 65 * 16 > 1024: 131072
    ("chain_seg 16", dict(n=16, max_src_len=MIB, xchg_ok=0), dict(chain_seg=32768, csegs=32), dict(chain=H.CHAIN_PEEL_SEGMENTS, chain_grid=512)),
    ("chain_seg 17", dict(n=17, max_src_len=MIB, xchg_ok=0), dict(chain_seg=65536, csegs=16), dict(chain_grid=272)),
    ("chain_seg 64", dict(n=64, max_src_len=MIB, xchg_ok=0), dict(chain_seg=65536, csegs=16), dict(chain_grid=1024)),
    ("chain_seg 65", dict(n=65, max_src_len=MIB, xchg_ok=0), dict(chain_seg=131072, csegs=8), dict(chain_grid=520)),
    # --- ppb: m * bps 2048 / 2049.  32 KiB: bps 2, 1024 * 2 = 2048 -> 8 parts: bits = pack = 16384, seal 64; 1025 * 2 = 2050 -> 1
    ("ppb 2048", dict(n=1024, max_src_len=32 * KIB), dict(segmented=1, bps=2), dict(blocks=2048, ppb=8, bits_grid=16384, pack_grid=16384, seal_grid=64)),
    ("ppb 2050", dict(n=1025, max_src_len=32 * KIB), dict(segmented=1, bps=2), dict(blocks=2050, ppb=1, bits_grid=0, pack_grid=2050, seal_grid=9)),
    # 64 KiB: bps = 65536 // 65277 + 2 = 3: 682 * 3 = 2046 -> 8 parts, 16368 waves, seal ceil(16368 / 256) = 64; 683 * 3 = 2049 -> 1, seal 9
    ("ppb 2046", dict(n=682, max_src_len=64 * KIB), dict(segmented=1, bps=3), dict(blocks=2046, ppb=8, bits_grid=16368, pack_grid=16368, seal_grid=64)),
    ("ppb 2049", dict(n=683, max_src_len=64 * KIB), dict(segmented=1, bps=3), dict(blocks=2049, ppb=1, bits_grid=0, pack_grid=2049, seal_grid=9)),
    # --- gpw.  64 KiB: tps = 2 + (65532 - 49152) // 16384 = 2; tpg = 4096 * 2 // 8192 = 1; gps = 2; a slice of 2048:
    # gpw = 2048 * 2 // 2048 = 2, ceil(4096 / 2) = 2048 workgroups; `Best (K = 4096 >= 1024): gpw 1, 4096 workgroups
    ("gpw default", dict(n=4096, max_src_len=64 * KIB, m=2048), dict(K=128, slices=2, tps=2, tpg=1, gps=2), dict(gpw=2, match_grid=2048)),
    ("gpw best", dict(n=4096, max_src_len=64 * KIB, m=2048, level=3), dict(K=4096, tps=2, tpg=1, gps=2), dict(gpw=1, match_grid=4096)),
    ("gpw fast", dict(n=4096, max_src_len=64 * KIB, m=2048, level=1), dict(K=4), dict(gpw=2, match_grid=2048)),
    # 256 KiB: tps = 2 + (262140 - 49152) // 16384 = 14; tpg = 4096 * 14 // 8192 = 7, gps 2; 8192 streams: tpg 14, gps 1
    ("tpg 7", dict(n=4096, max_src_len=256 * KIB), dict(tps=14, tpg=7, gps=2), {}),
    ("tpg 14", dict(n=8192, max_src_len=256 * KIB), dict(tps=14, tpg=14, gps=1), {}),
    # match_tiles_per_group = 1: gps 14; a slice of 2048: gpw = 14 -> 8 at most; ceil(2048 * 14 / 8) = 3584 workgroups
    ("tpg override", dict(n=4096, max_src_len=256 * KIB, m=2048, match_tiles_per_group=1), dict(tps=14, tpg=1, gps=14), dict(gpw=8, match_grid=3584)),
    ("tpg override beyond tps", dict(n=4, max_src_len=256 * KIB, match_tiles_per_group=99), dict(tps=14, tpg=14, gps=1), {}),
    # --- slices: 4095 // 2 < 2048
    ("slices 4095", dict(n=4095, max_src_len=100), dict(slices=1), {}),
    ("slices 4096", dict(n=4096, max_src_len=100), dict(slices=2), {}),
    # slices = 4: 8192 // 4 = 2048; 8191 // 4 = 2047 -> 3 (8191 // 3 = 2730); at most 8; slice_min = 8: 32 // 4 = 8, 31 // 4 = 7 -> 3
    ("slices env 4", dict(n=8192, max_src_len=100, slices=4), dict(slices=4), {}),
    ("slices env 4, short", dict(n=8191, max_src_len=100, slices=4), dict(slices=3), {}),
    ("slices env 100", dict(n=16384, max_src_len=100, slices=100), dict(slices=8), {}),
    ("slice_min 8", dict(n=32, max_src_len=100, slices=4, slice_min=8), dict(slices=4), {}),
    ("slice_min 8, short", dict(n=31, max_src_len=100, slices=4, slice_min=8), dict(slices=3), {}),
    ("slices override", dict(n=8192, max_src_len=100, slices=4, slices_override=1), dict(slices=1), {}),
    # --- parse_segments 0 / 1, parse_seg
    ("segments never", dict(n=2, max_src_len=28673, parse_segments=0), dict(sps=8, segmented=0, segments_required=0), {}),
    ("segments always, 2 segments", dict(n=5000, max_src_len=4097, parse_segments=1), dict(sps=2, segmented=1, segments_required=1), {}),
    ("segments always, 1 segment", dict(n=5000, max_src_len=4096, parse_segments=1), dict(sps=1, segmented=0, segments_required=1), {}),
    ("parse_seg 8192", dict(n=2, max_src_len=28673, parse_seg=8192), dict(segp=8192, sps=4, segmented=0), {}),
    ("parse_seg below the least", dict(n=2, max_src_len=28673, parse_seg=4032), dict(segp=4096, sps=8), {}),
    ("parse_seg no multiple of 64", dict(n=2, max_src_len=28673, parse_seg=8200), dict(segp=4096, sps=8), {}),
    ("parse_seg 1 Mi", dict(n=2, max_src_len=4 * MIB, parse_seg=1 << 20), dict(segp=1 << 20, sps=4), {}),
    ("parse_seg beyond 1 Mi", dict(n=2, max_src_len=4 * MIB, parse_seg=(1 << 20) + 64), dict(segp=4096, sps=1024), {}),
    ("parse_seg and segments always", dict(n=3, max_src_len=8193, parse_segments=1, parse_seg=4096), dict(segp=4096, sps=3, segmented=1, seg_syms=4672), {}),
    # --- the grid guards.  lz_match's fails the call: the longest stream, tps = 2 + (0xFFFF0000 - 4 - 49152) // 16384 = 262138;
    # 8192 * 262138 = 2147434496 <= 2^31 - 1 < 8193 * 262138; 8 chunks of the short matcher: 268435455 * 8 = 2^31 - 8
    ("match grid fits", dict(n=8192, max_src_len=0xFFFF0000, total_src_len=1 << 40, parse_segments=0), dict(tps=262138, grid_too_large=0), {}),
    ("match grid too large", dict(n=8193, max_src_len=0xFFFF0000, total_src_len=1 << 40, parse_segments=0), dict(tps=262138, grid_too_large=1), {}),
    ("short match grid fits", dict(n=268435455, max_src_len=8192, total_src_len=1 << 40), dict(cps=8, grid_too_large=0), {}),
    ("short match grid too large", dict(n=268435456, max_src_len=8192, total_src_len=1 << 40), dict(cps=8, grid_too_large=1), {}),
    # the segmented forms' only turn them off.  1 MiB in segments of 4096: sps 256, bps = 16 + 2: 8388607 * 256 = 2^31 - 256;
    # 8388608 * 256 = 2^31 (n * bps * 8 = 144 n stays below)
    ("segment grid fits", dict(n=8388607, max_src_len=MIB, parse_segments=1, parse_seg=4096), dict(sps=256, bps=18, segmented=1, grid_too_large=0), {}),
    ("segment grid too large", dict(n=8388608, max_src_len=MIB, parse_segments=1, parse_seg=4096), dict(sps=256, segmented=0, grid_too_large=0), {}),
    # 16 MiB in segments of 1 Mi: sps 16, bps = 257 + 2: 1000000 * 259 * 8 = 2072000000 fits, 1048576 * 259 * 8 = 2172649472 does not
    ("block grid fits", dict(n=1000000, max_src_len=16 * MIB, parse_segments=1, parse_seg=1 << 20), dict(sps=16, bps=259, segmented=1, grid_too_large=0), {}),
    ("block grid too large", dict(n=1048576, max_src_len=16 * MIB, parse_segments=1, parse_seg=1 << 20), dict(sps=16, bps=259, segmented=0, grid_too_large=0), {}),
    # --- the edges of the helpers: no stream, streams too short for a match
    ("empty streams", dict(n=3, max_src_len=0), dict(tps=1, cps=1, sps=0, bps=2, segmented=0, csegs=0), dict(match_window=0, match_grid=8, chain_grid=3)),
    ("3 bytes", dict(n=3, max_src_len=3), dict(tps=1, cps=1, sps=1), {}),
]


@pytest.mark.parametrize("row", FORMS_ROWS, ids=[r[0] for r in FORMS_ROWS])
def test_deflate_forms_equal_the_hand_written_rows(sim, row):
    what, args, group, sl = row
    f, s = H.deflate_forms(sim, **args)
    assert {k: f[k] for k in group} == group, (what, f)
    assert {k: s[k] for k in sl} == sl, (what, s)


def test_deflate_grouping_past_the_group_bytes(sim):
    # (n, max_src_len, total, group bytes) -> (streams per group, bytes a group holds at most)
    rows = [
        ((8192, MIB, 8 * GIB, 8 * GIB), (8192, 8 * GIB)),          # not MORE than a group's bytes: one group
        ((8193, MIB, 8193 * MIB, 8 * GIB), (8192, 8 * GIB)),       # 8 GiB // 1 MiB streams, 8192 * 1 MiB < the total
        ((10, 300, 1000, 1000), (10, 1000)),
        ((10, 300, 1001, 1000), (3, 900)),                         # 1000 // 300 = 3 streams, 3 * 300 = 900 < 1001
        ((10, 300, 2500, 1000), (3, 900)),
        ((10, 300, 2500, 100), (1, 300)),                          # 100 // 300 = 0: a stream to a group at least
        ((2, 300, 450, 400), (1, 300)),
        ((10, 300, 2500, 5000), (10, 2500)),
        ((1, 5000, 5000, 1000), (1, 5000)),                        # one stream is never cut
        ((10, 0, 2500, 1000), (10, 2500)),                         # nothing declared to divide by
        ((4, 600, 2400, 2399), (3, 1800)),                         # 2399 // 600 = 3
    ]
    for (n, L, total, gb), want in rows:
        assert H.deflate_grouping(sim, n, L, total, deflate_group_bytes=gb) == want, (n, L, total, gb)


def _scratch_bytes_as_it_was(n_all, max_src_len, total_all, level, group_bytes=8 * GIB):
    """deflate_scratch_bytes as deflate.hip summed it before the layout became one carve function: the independent reading"""
    n, total = n_all, total_all
    if total_all > group_bytes and max_src_len > 0 and n_all > 1:
        n = max(1, min(group_bytes // max_src_len, n_all))
        total = min(n * max_src_len, total_all)
    P = total + (256 + 256) * n + 256
    Bk = total // 65277 + 2 * n + 16
    up = lambda v: (v + 255) // 256 * 256
    b = up(n * 8) * 2 + up(n * 4) * 2 + 256
    if level != 0:
        b += up(P * 2) + 2 * up(P * 4) + up(P * 4)
        b += up(Bk * 16)
    return b + 1024


def test_deflate_scratch_bytes_equal_the_sums_they_were(sim):
    rows = [(1, 0, 0, 2), (1, 1, 1, 1), (1, 100, 100, 2), (1, 1 << 19, 1 << 19, 2), (3, 70001, 150003, 3), (64, 65536, 64 * 65536, 2),
            (64, 65536, 64 * 65536, 0), (1, 100, 100, 0), (33, 777, 20000, 0), (4096, 32768, 4096 * 32768, 3), (8192, MIB, 8 * GIB, 2),
            (8193, MIB, 8193 * MIB, 2), (8193, MIB, 8193 * MIB, 0), (20000, MIB, 9 * GIB, 1)]
    for n, L, total, level in rows:
        assert H.deflate_scratch_bytes(sim, n, L, total, level) == _scratch_bytes_as_it_was(n, L, total, level), (n, L, total, level)
    for n, L, total, level, gb in [(10, 300, 2500, 2, 1000), (10, 300, 2500, 0, 1000), (10, 300, 2500, 3, 100), (7, 70000, 400000, 2, 200000)]:
        assert H.deflate_scratch_bytes(sim, n, L, total, level, deflate_group_bytes=gb) == _scratch_bytes_as_it_was(n, L, total, level, gb), (n, L, total, level, gb)
    # one value by hand: one stream of 100 bytes at `Default: P = 100 + 512 + 256 = 868, Bk = 0 + 2 + 16 = 18;
    # 4 * 256 + 256 | 1792 + 3 * 3584 | 512 | + 1024
    assert H.deflate_scratch_bytes(sim, 1, 100, 100, 2) == 1280 + 1792 + 10752 + 512 + 1024


def test_inflate_gates_at_their_thresholds(sim):
    # one stream: from BLOCKS_MIN_SRC = 40 KiB of capacity; a batch: from BLOCKS_BATCH_MIN_DST = 256 KiB; at most
    # MAX_STREAM_LEN = 0xFFFF0000 of capacity and BLOCKS_MAX_STREAMS = 2^20 streams
    rows = [((1, 40 * KIB), 1), ((1, 40 * KIB - 1), 0), ((2, 256 * KIB), 1), ((2, 256 * KIB - 1), 0), ((2, 40 * KIB), 0),
            ((1, 0xFFFF0000), 1), ((1, 0xFFFF0001), 0), ((64, 0xFFFF0001), 0), ((1 << 20, 256 * KIB), 1), (((1 << 20) + 1, 256 * KIB), 0)]
    for (n, cap), want in rows:
        assert sim.sim_inflate_blocks_gate(n, cap) == want, (n, cap)
    assert [sim.sim_inflate_few_streams(n) for n in (1, 256, 257, 4096)] == [1, 1, 0, 0]


def test_inflate_streams_picked_for_the_block_path(sim):
    """ms = (1 + 0.09 per MiB taken, if any is taken) + 15 per MiB of the longest stream left to its one wave"""
    half = 512 * KIB
    # 64 x 1 MiB: none 15 ms, all 1 + 64 * 0.09 = 6.76 ms, any k between 1 + 0.09 k + 15: every stream, one group (64 * 12 MiB)
    assert H.inflate_blocks_pick(sim, [(half, MIB)] * 64) == (list(range(64)), [64])
    # 4096 x 1 MiB: none 15 ms, all 1 + 4096 * 0.09 = 369.64 ms: none
    assert H.inflate_blocks_pick(sim, [(half, MIB)] * 4096) == ([], [])
    # 1000 members below BLOCKS_MIN_SRC of input (64 KiB of output) and two of 8 MiB: none 8 * 15 = 120 ms, the longer one
    # 1 + 0.72 + 120, both 1 + 16 * 0.09 + 15 / 16 = 3.38 ms
    members = [(20000, 64 * KIB)] * 1002
    members[500] = members[1001] = (4 * MIB, 8 * MIB)
    assert H.inflate_blocks_pick(sim, members) == ([500, 1001], [2])
    # runs: output beyond 64 x the input never goes by blocks (4194368 // 64 = 65537 > 65536); at 64 x it does (1.36 ms against 60)
    assert H.inflate_blocks_pick(sim, [(65536, 64 * 65536 + 64)]) == ([], [])
    assert H.inflate_blocks_pick(sim, [(65536, 64 * 65536 + 63)]) == ([0], [1])
    # what the block path takes at all: 40 KiB .. 0x1FFFFFFF bytes of input, 8 .. 0xFFFF0000 bytes of capacity
    assert H.inflate_blocks_pick(sim, [(40 * KIB - 1, MIB)]) == ([], [])
    assert H.inflate_blocks_pick(sim, [(40 * KIB, MIB)]) == ([0], [1])
    assert H.inflate_blocks_pick(sim, [(0x1FFFFFFF, 0x20000000)]) == ([0], [1])
    assert H.inflate_blocks_pick(sim, [(0x20000000, 0x20000000)]) == ([], [])
    assert H.inflate_blocks_pick(sim, [(1 << 28, 0xFFFF0000)]) == ([0], [1])
    assert H.inflate_blocks_pick(sim, [(1 << 28, 0xFFFF0001)]) == ([], [])
    # a long stream among equal ones that stay: 3000 x 1 MiB and one of 64 MiB: none 960 ms, the long one 1 + 5.76 + 15 = 21.76,
    # one more 1 + 5.85 + 15
    many = [(half, MIB)] * 3001
    many[7] = (32 * MIB, 64 * MIB)
    assert H.inflate_blocks_pick(sim, many) == ([7], [1])


def test_inflate_groups_cut_at_the_token_budget(sim):
    # 12 bytes of scratch per byte of capacity, 1 GiB to a group: 32 MiB members are 384 MiB each, two to a group
    # (all five picked: 1 + 160 * 0.09 = 15.4 ms against 480)
    assert H.inflate_blocks_pick(sim, [(16 * MIB, 32 * MIB)] * 5) == ([0, 1, 2, 3, 4], [2, 4, 5])
    # 2 * 12 * 44739242 = 2^30 - 16 fits, 2 * 12 * 44739243 = 2^30 + 8 does not
    assert H.inflate_blocks_pick(sim, [(16 * MIB, 44739242)] * 3) == ([0, 1, 2], [2, 3])
    assert H.inflate_blocks_pick(sim, [(16 * MIB, 44739243)] * 3) == ([0, 1, 2], [1, 2, 3])
    # a member beyond the budget has a group to itself: 128 MiB is 1.5 GiB of scratch
    assert H.inflate_blocks_pick(sim, [(64 * MIB, 128 * MIB), (512 * KIB, MIB), (64 * MIB, 128 * MIB)]) == ([0, 1, 2], [1, 2, 3])


# ---- inflate by blocks between its launches (zipc_amd/csrc/inflate_blocks.h).  As above, every expected value is the reading of
# the launch code as it stood inline before the rules moved, with the arithmetic beside it; none is the header's own output.
#   first_cap = src_len // 8 + 4096           cand_cap = min(src_len // 512 + 64, 65536)
#   max_explorers = src_len // stride + 1     rec_cap = chain_cap = min(2 * cand_cap + 4 * max_explorers, 262144)
def test_inflate_blocks_caps_equal_the_hand_written_rows(sim):
    rows = [
        # (src_len, stride) -> (first_cap, cand_cap, max_explorers, rec_cap)
        ((40960, 16384), (5120 + 4096, 80 + 64, 2 + 1, 288 + 12)),
        ((67108864, 16384), (8388608 + 4096, 65536, 4096 + 1, 131072 + 16388)),         # cand_cap capped (131072 + 64)
        ((0x1FFFFFFF, 16384), (67108863 + 4096, 65536, 32767 + 1, 262144)),             # 131072 + 4 * 32768: exactly the cap
        ((0x1FFFFFFF, 1024), (67108863 + 4096, 65536, 524287 + 1, 262144)),             # 131072 + 4 * 524288: capped
        # cand_cap reaching 65536: 65471 + 64, 65472 + 64 (the cap itself, not capped), 65473 + 64 (capped)
        ((33521663, 16384), (4190207 + 4096, 65535, 2045 + 1, 131070 + 8184)),
        ((33521664, 16384), (4190208 + 4096, 65536, 2046 + 1, 131072 + 8188)),
        ((33522176, 16384), (4190272 + 4096, 65536, 2046 + 1, 131072 + 8188)),
        ((100000, 16384), (12500 + 4096, 195 + 64, 6 + 1, 518 + 28)),
        ((5000000, 16384), (625000 + 4096, 9765 + 64, 305 + 1, 19658 + 1224)),
    ]
    for args, want in rows:
        assert H.blocks_caps(sim, *args) == want, args


def test_inflate_blocks_candidates_are_read_back_when_lists_are_long_or_many(sim):
    # one stream: the kernels read the count themselves up to a list of 8192 (4161536 // 512 + 64 = 8192 = 4162047 // 512 + 64)
    assert sim.sim_blocks_read_candidates(1, 4161536, 16384) == 0
    assert sim.sim_blocks_read_candidates(1, 4162047, 16384) == 0
    assert sim.sim_blocks_read_candidates(1, 4162048, 16384) == 1      # a list of 8193
    assert sim.sim_blocks_read_candidates(1, 40 * KIB, 16384) == 0
    assert sim.sim_blocks_read_candidates(2, 40 * KIB, 16384) == 1      # two streams, whatever their lists
    assert sim.sim_blocks_read_candidates(64, 4161536, 16384) == 1


_up256 = lambda v: (v + 255) // 256 * 256
FIND_COUNTS_BYTES, BLOCKS_JOB_BYTES = 104, 144  # 4 + 2 words, 13 + 3 words, 4 words; 10 words and 13 pointers


def _blocks_list_bytes(first_cap, cand_cap, rec_cap):
    """a stream's nine lists in the order they lie: first | cand | recs | sorted | sorted_src | chain | chain_end | chain_iv | cks
    (4-byte offsets, 32-byte BlockRec, 16-byte BlockStart, 24-byte BlockEnd, 8-byte ChainIv, 256-byte BlockCk for listed and walked)"""
    return [first_cap * 4, cand_cap * 4, rec_cap * 32, rec_cap * 32, rec_cap * 4, rec_cap * 16, rec_cap * 24, rec_cap * 8,
            (rec_cap + rec_cap) * 256]


def test_inflate_blocks_scratch_is_one_layout_for_the_size_and_the_pointers(sim):
    names = H.BLOCKS_LISTS[1:10]
    # one stream of 40 KiB: caps 9216, 144, 300 (above)
    end, head, lists = H.blocks_scratch(sim, [40960])
    assert end == 256 + 256 + 36864 + 768 + 2 * 9728 + 1280 + 4864 + 7424 + 2560 + 153600 == 227328
    assert end == _up256(FIND_COUNTS_BYTES) + _up256(BLOCKS_JOB_BYTES) + sum(_up256(b) for b in _blocks_list_bytes(9216, 144, 300))
    assert head == (0, 256) and lists[0]["counts"] == 0 and lists[0]["first"] == 512 and lists[0]["stream"] == 100
    # three streams of unequal length, their caps as the rows above have them
    src_lens, caps = [40960, 100000, 5000000], [(9216, 144, 300), (16596, 259, 546), (629096, 9829, 20882)]
    want_end = _up256(3 * FIND_COUNTS_BYTES) + _up256(3 * BLOCKS_JOB_BYTES) + sum(_up256(b) for c in caps for b in _blocks_list_bytes(*c))
    end0, head0, lists0 = H.blocks_scratch(sim, src_lens)
    assert end0 == want_end
    # ... and from a base: every pointer is the base plus the running sum, in the documented order
    for base in (0, (1 << 40) + 0x300):
        end, head, lists = H.blocks_scratch(sim, src_lens, base=base)
        assert end == base + want_end
        assert head == (base, base + _up256(3 * FIND_COUNTS_BYTES))
        at = base + _up256(3 * FIND_COUNTS_BYTES) + _up256(3 * BLOCKS_JOB_BYTES)
        arrays = [(head[0], 3 * FIND_COUNTS_BYTES), (head[1], 3 * BLOCKS_JOB_BYTES)]
        for j, c in enumerate(caps):
            assert lists[j]["counts"] == base + j * FIND_COUNTS_BYTES and lists[j]["stream"] == 100 + j
            for name, size in zip(names, _blocks_list_bytes(*c)):
                assert lists[j][name] == at, (base, j, name)
                arrays.append((at, size))
                at += _up256(size)
        assert at == end
        # every array on a 256-byte boundary, no two overlap, none beyond the end
        assert all(a % 256 == 0 for a, _ in arrays)
        arrays.sort()
        assert all(a + size <= b for (a, size), (b, _) in zip(arrays, arrays[1:])) and arrays[-1][0] + arrays[-1][1] <= end


def test_inflate_blocks_verdicts_after_each_read_back(sim):
    # 1 MiB of input: cand_cap 2048 + 64 = 2112, max_explorers 64 + 1, rec_cap 2 * 2112 + 4 * 65 = 4484; 8388608 bits,
    # an explorer every 16384 * 8 = 131072 of them
    v = lambda **kw: H.blocks_verdicts(sim, src_len=MIB, **kw)
    # after the find: no candidate, or more than the list holds
    assert [v(n_cand=n)["found"] for n in (0, 1, 2112, 2113)] == [0, 1, 1, 0]
    assert [v(n_cand=n, chain_ok=0, miss_bit=5)["chained"] for n in (0, 2112, 2113)] == [0, 2, 0]  # dropped whatever the chain says
    # after the first chain: lost only with a place where it stopped
    assert v(chain_ok=0, miss_bit=0)["chained"] == 2
    assert v(chain_ok=0, miss_bit=H.NO_MISS)["chained"] == 1
    assert v(chain_ok=1, miss_bit=H.NO_MISS)["chained"] == 1
    assert v(chain_ok=1, miss_bit=0)["chained"] == 1
    # explorers: ceil(bits left / 131072) -- exactly three strides before the end 3, one bit earlier 4, the whole stream 64
    lost = lambda miss_bit, n_recs=0, **kw: (lambda d: (d["explorers"], d["waves"]))(v(chain_ok=0, miss_bit=miss_bit, n_recs=n_recs, **kw))
    assert lost(8388608 - 3 * 131072) == (3, 3)
    assert lost(8388608 - 3 * 131072 - 1) == (4, 4)
    assert lost(8388608 - 1) == (1, 1)
    assert lost(0) == (64, 64)
    # ... at most max_explorers.  A place inside the input never needs more (ceil(bits left / stride) <= src_len // stride + 1);
    # the cap is what holds when the counts say a place two strides BEHIND the input, whose distance to the end wraps around:
    # 65, not (2^64 - 262144 + 131071) // 131072
    assert lost(8388608 + 2 * 131072) == (65, 65)
    assert lost(8388608 + 2 * 131072, n_recs=7) == (65, 72)
    assert H.blocks_verdicts(sim, src_len=MIB, explore_stride=1024, chain_ok=0, miss_bit=8388608 + 2 * 8192)["explorers"] == 1024 + 1
    assert H.blocks_verdicts(sim, src_len=MIB, explore_stride=1024, chain_ok=0, miss_bit=8388608 - 8192 - 1)["explorers"] == 2
    # followers: a wave per block listed so far, at most the list (n_recs counts on when it overflows)
    assert lost(8388608 - 3 * 131072, n_recs=10) == (3, 13)
    assert lost(8388608 - 3 * 131072, n_recs=4483) == (3, 3 + 4483)
    assert lost(8388608 - 3 * 131072, n_recs=4484) == (3, 3 + 4484)
    assert lost(8388608 - 3 * 131072, n_recs=4485) == (3, 3 + 4484)
    assert lost(8388608 - 3 * 131072, n_recs=100000) == (3, 3 + 4484)
    # into the token run: a chain of two blocks and more with output
    assert v(chain_ok=1, n_blocks=2, out_len=1)["taken"] == 1
    assert v(chain_ok=1, n_blocks=1, out_len=1)["taken"] == 0
    assert v(chain_ok=1, n_blocks=2, out_len=0)["taken"] == 0
    assert v(chain_ok=0, n_blocks=2, out_len=1)["taken"] == 0
    # after the gather: done unless a block ended elsewhere or the LAST round left bytes short
    assert v(rounds=6)["done"] == 1
    assert v(rounds=6, token_bad=1)["done"] == 0
    assert v(rounds=6, more_at=5)["done"] == 0
    assert v(rounds=6, more_at=4)["done"] == 1
    assert v(rounds=6, more_at=6)["done"] == 1
    assert v(rounds=12, more_at=11)["done"] == 0
    assert v(rounds=12, more_at=5)["done"] == 1


def test_inflate_blocks_token_plan(sim):
    plan = lambda streams, **kw: H.blocks_token_plan(sim, streams, **kw)
    one = lambda src_len, out_len, **kw: plan([(src_len, 1, 5, out_len, 9)], **kw)[0][0]
    # follow from 32 MiB of output of the whole call on: a wave per block (5) instead of one per interval (9)
    assert one(MIB, 32 * MIB - 1) == dict(follow=0, n=9, tok_at=0, out_len=32 * MIB - 1)
    assert one(MIB, 32 * MIB) == dict(follow=1, n=5, tok_at=0, out_len=32 * MIB)
    per, call_out, _ = plan([(MIB, 1, 5, 16 * MIB, 9), (MIB, 1, 5, 16 * MIB, 9)])
    assert call_out == 32 * MIB and [p["follow"] for p in per] == [1, 1]
    per, call_out, _ = plan([(MIB, 1, 5, 16 * MIB, 9), (MIB, 1, 5, 16 * MIB - 1, 9)])
    assert call_out == 32 * MIB - 1 and [p["follow"] for p in per] == [0, 0]
    # (streams that stay out of the token run do not count: one block, no chain)
    per, call_out, _ = plan([(MIB, 1, 1, 16 * MIB, 9), (MIB, 1, 5, 16 * MIB, 9), (MIB, 0, 5, 16 * MIB, 9)])
    assert call_out == 16 * MIB and per[0] is None and per[2] is None and per[1]["follow"] == 0 and per[1]["tok_at"] == 0
    # ... and output of at least 1.5 x the input: out_len * 2 against src_len * 3 = 90000003 / 90000000
    assert one(30000001, 45000001)["follow"] == 0   # 90000002: one short
    assert one(30000001, 45000002)["follow"] == 1
    assert one(30000000, 44999999)["follow"] == 0
    assert one(30000000, 45000000)["follow"] == 1   # equal
    # the override wins both ways
    assert one(MIB, 32 * MIB, follow_env=0) == dict(follow=0, n=9, tok_at=0, out_len=32 * MIB)
    assert one(MIB, 100, follow_env=1) == dict(follow=1, n=5, tok_at=0, out_len=100)
    assert one(MIB, 100, follow_env=-1)["follow"] == 0
    # tok[]: three words per output byte in steps of 64 words -- 21 bytes: 63 -> 64 words, 22: 66 -> 128 -- one stream's behind the other's
    per, _, tok_bytes = plan([(MIB, 1, 2, 21, 2), (MIB, 1, 2, 22, 2)])
    assert [p["tok_at"] for p in per] == [0, 64 * 4] and tok_bytes == (64 + 128) * 4
    per, _, tok_bytes = plan([(MIB, 1, 2, 22, 2), (MIB, 1, 1, 50, 2), (MIB, 1, 2, 21, 2)])
    assert per[1] is None and [per[0]["tok_at"], per[2]["tok_at"]] == [0, 128 * 4] and tok_bytes == (128 + 64) * 4
    assert plan([(MIB, 1, 2, 64, 2)])[2] == 192 * 4 and plan([(MIB, 1, 2, 65, 2)])[2] == 256 * 4
    assert plan([(MIB, 1, 2, 43, 2)])[2] == 192 * 4  # 129 words: one beyond a step is a whole step more
    # resolve rounds: 6 when both hop counts reach 16 (16^6 links), else all 12
    assert [sim.sim_resolve_rounds(*h) for h in ((16, 16), (15, 16), (16, 15), (3, 5), (256, 256))] == [6, 12, 12, 12, 6]
    # the resolve grid: the first round a thread per byte, later rounds 2048 workgroups at most
    assert [sim.sim_resolve_grid(0, g) for g in (2047, 2048, 5000)] == [2047, 2048, 5000]
    assert [sim.sim_resolve_grid(1, g) for g in (2047, 2048, 5000)] == [2047, 2048, 2048]
    assert sim.sim_resolve_grid(5, 2049) == 2048


def test_inflate_blocks_shares_of_the_span_index_and_the_adler_sums(sim):
    # a slot of 64 * 18 * 2 = 2304 bytes per wave; three words per Adler chunk and a chunk to spare
    span_at, span_bytes, sums_at, sums_bytes = H.blocks_shares(sim, [3, 0, 5], [4, 1, 7])
    assert span_at == [0, 3 * 2304, 3 * 2304] and span_bytes == 8 * 2304
    assert sums_at == [0, 4 * 12, 5 * 12] and sums_bytes == (12 + 1) * 12
    assert H.blocks_shares(sim, [1], [0]) == ([0], 2304, [0], 12)
