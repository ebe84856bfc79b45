"""Test-only host build of the lane-serial kernel code (see sim_*.cpp)."""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libhost_sim.so")
SRCS = ["sim_inflate.cpp", "sim_deflate.cpp", "sim_chain.cpp", "sim_forms.cpp", "sim_adler.cpp", "sim_many.cpp", "sim_match.cpp"]


def lib():
    if os.environ.get("ZD_HOST_SIM_LIB"):  # another build of the same sources (tests/test_sanitizers.py: address + undefined sanitizers)
        return _bind(C.CDLL(os.environ["ZD_HOST_SIM_LIB"]))
    deps = [os.path.join(HERE, s) for s in SRCS]
    csrc = os.path.join(HERE, "..", "..", "zipc_amd", "csrc")
    deps += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    deps += [os.path.join(HERE, f) for f in os.listdir(HERE) if f.endswith(".h")]
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in deps):
        sys.path.insert(0, os.path.dirname(HERE))  # (tools/ import this package as tests.host_sim)
        import mutation

        mutation.gxx(LIB, [os.path.join(HERE, s) for s in SRCS], include=[HERE], extra=["-g", "-Wall", "-Wno-unknown-pragmas"])
    return _bind(C.CDLL(LIB))


def _bind(L):
    L.sim_inflate.restype = C.c_int
    L.sim_inflate.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_int,
                              C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_int]
    L.sim_deflate.restype = C.c_int
    L.sim_deflate.argtypes = [C.c_char_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                              C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
    L.sim_huff_lengths.restype = C.c_int
    L.sim_huff_lengths.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    if hasattr(L, "sim_inflate_token_words"):  # (a library of one file alone, as the mutants' tests build them, may lack it)
        L.sim_inflate_token_words.restype = C.c_int
        L.sim_inflate_token_words.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_uint32,
                                              C.POINTER(C.c_uint64), C.c_void_p]
        L.sim_inflate_token_tiles.restype = C.c_uint64
        L.sim_inflate_token_tiles.argtypes = [C.c_void_p, C.c_uint64]
    L.sim_crc_advance.restype = C.c_uint32
    L.sim_crc_advance.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64]
    tun = C.POINTER(C.c_longlong)
    L.sim_deflate_grouping.restype = None
    L.sim_deflate_grouping.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, tun, C.POINTER(C.c_uint64)]
    L.sim_deflate_scratch_bytes.restype = C.c_uint64
    L.sim_deflate_scratch_bytes.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, tun]
    L.sim_deflate_forms.restype = None
    L.sim_deflate_forms.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, tun, C.c_int, C.c_uint64, C.POINTER(C.c_uint64),
                                    C.POINTER(C.c_uint64)]
    L.sim_chain_seg_known.restype = C.c_int
    L.sim_chain_seg_known.argtypes = [C.c_int, C.c_uint64]
    L.sim_inflate_blocks_gate.restype = C.c_int
    L.sim_inflate_blocks_gate.argtypes = [C.c_uint64, C.c_uint64]
    L.sim_inflate_few_streams.restype = C.c_int
    L.sim_inflate_few_streams.argtypes = [C.c_uint64]
    L.sim_inflate_blocks_pick.restype = C.c_uint64
    L.sim_inflate_blocks_pick.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_uint32),
                                          C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    L.sim_blocks_caps.restype = None
    L.sim_blocks_caps.argtypes = [C.c_uint64, C.c_uint64, u64p]
    L.sim_blocks_read_candidates.restype = C.c_int
    L.sim_blocks_read_candidates.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64]
    L.sim_blocks_scratch.restype = C.c_uint64
    L.sim_blocks_scratch.argtypes = [C.c_uint64, u64p, C.c_uint64, C.c_uint64, u64p, u64p]
    L.sim_blocks_verdicts.restype = None
    L.sim_blocks_verdicts.argtypes = [u64p, u64p]
    L.sim_blocks_token_plan.restype = None
    L.sim_blocks_token_plan.argtypes = [u64p, C.c_uint64, C.c_int, u64p, u64p]
    L.sim_resolve_rounds.restype = C.c_int
    L.sim_resolve_rounds.argtypes = [C.c_int, C.c_int]
    L.sim_resolve_grid.restype = C.c_uint32
    L.sim_resolve_grid.argtypes = [C.c_int, C.c_uint32]
    L.sim_blocks_shares.restype = None
    L.sim_blocks_shares.argtypes = [u32p, u32p, C.c_uint64, u64p, u64p, u64p]
    L.sim_match_lane_position.restype = None
    L.sim_match_lane_position.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return bind_chain(bind_match(bind_many(bind_adler(L))))


def bind_chain(L):
    """sim_chain.cpp's entry points (a library of that file alone has no others: the mutants of tests/test_chain_rules.py)"""
    L.sim_chain.restype = None
    L.sim_chain.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_int)]
    L.sim_chain_segments.restype = None
    L.sim_chain_segments.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]
    L.sim_chain_serial.restype = None
    L.sim_chain_serial.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p]
    L.sim_chain_ref_hash4.restype = C.c_uint32
    L.sim_chain_ref_hash4.argtypes = [C.c_char_p]
    L.sim_chain_reference.restype = None
    L.sim_chain_reference.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p]
    L.sim_chain_xchg_segments.restype = None
    L.sim_chain_xchg_segments.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint32]
    return L


def bind_match(L):
    """sim_match.cpp's reference (a library of its top half alone has no other entry points: the mutants of
    tests/test_match_rules.py)"""
    L.sim_match_hash4.restype = C.c_uint32
    L.sim_match_hash4.argtypes = [C.c_char_p]
    L.sim_match_reference.restype = None
    L.sim_match_reference.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.sim_match_parse_reads.restype = None
    L.sim_match_parse_reads.argtypes = [C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def bind_many(L):
    """sim_many.cpp's entry points (a library of that file alone has no others: the mutants of tests/test_many_plan.py)"""
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    L.sim_many_slot.restype = C.c_uint64
    L.sim_many_slot.argtypes = [C.c_uint64]
    L.sim_many_chunks.restype = C.c_uint64
    L.sim_many_chunks.argtypes = [C.c_long, C.c_uint64]
    L.sim_many_plan.restype = C.c_uint64
    L.sim_many_plan.argtypes = [C.c_int, C.c_uint64, u64p, u64p, u64p, u64p, u32p, C.c_long, C.c_long, u64p, u64p, u64p, u64p, u64p, u64p]
    return L


def bind_adler(L):
    """sim_adler.cpp's entry points (a library of that file alone has no others: the mutants of tests/test_adler_chain_sim.py)"""
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    L.sim_adler_shape.restype = None
    L.sim_adler_shape.argtypes = [C.c_uint64, u64p]
    L.sim_adler_chain.restype = C.c_int
    L.sim_adler_chain.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u32p, u64p]
    for f in (L.sim_adler_serial, L.sim_adler_rfc):
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, u32p]
    L.sim_crc_finish_grid.restype = C.c_uint64
    L.sim_crc_finish_grid.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, u64p, u64p]
    return L


# ---- zipc_amd/csrc/forms.h through sim_forms.cpp: the launch rules as dicts of plain numbers
FORMS_FIELDS = ("grid_too_large", "K", "slices", "tps", "cps", "tpg", "gps", "segmented", "segments_required", "segp", "sps", "bps",
                "n_slots", "tiles", "seg_syms", "xchg_chain", "chain_seg", "csegs", "xseg", "xsegs")
SLICE_FIELDS = ("chain", "chain_grid", "match_window", "match_grid", "gpw", "streams", "segments", "blocks", "ppb", "bits_grid",
                "pack_grid", "seal_grid")
CHAIN_XCHG, CHAIN_XCHG_SEGMENTS, CHAIN_PEEL, CHAIN_PEEL_SEGMENTS = 0, 1, 2, 3


def _tun(parse_segments=-1, parse_seg=0, match_tiles_per_group=0, deflate_group_bytes=8 << 30, slices=0, slice_min=0,
         slices_override=0, segments_ok=1):
    """the Tuning fields the deflate rules read (their defaults: api.hip tuning()), the debug override of the slices, and
    whether the parse scratch could be had"""
    return (C.c_longlong * 8)(parse_segments, parse_seg, match_tiles_per_group, deflate_group_bytes, slices, slice_min,
                              slices_override, segments_ok)


def deflate_forms(L, n, max_src_len, total_src_len=None, level=2, xchg_ok=1, m=None, **tun):
    """forms.h deflate_forms of a group, and deflate_slice_forms of a slice of m of its streams (default: the whole group)"""
    out, sl = (C.c_uint64 * len(FORMS_FIELDS))(), (C.c_uint64 * len(SLICE_FIELDS))()
    L.sim_deflate_forms(n, max_src_len, n * max_src_len if total_src_len is None else total_src_len, level, _tun(**tun), xchg_ok,
                        n if m is None else m, out, sl)
    return dict(zip(FORMS_FIELDS, out)), dict(zip(SLICE_FIELDS, sl))


def deflate_grouping(L, n, max_src_len, total_src_len, **tun):
    out = (C.c_uint64 * 2)()
    L.sim_deflate_grouping(n, max_src_len, total_src_len, _tun(**tun), out)
    return out[0], out[1]


def deflate_scratch_bytes(L, n, max_src_len, total_src_len, level, **tun):
    return L.sim_deflate_scratch_bytes(n, max_src_len, total_src_len, level, _tun(**tun))


def inflate_blocks_pick(L, streams):
    """streams: (src_len, dst_cap) pairs -> (the indices that go by blocks, the ends of their groups)"""
    n = len(streams)
    src, cap = (C.c_uint64 * n)(*[s for s, c in streams]), (C.c_uint64 * n)(*[c for s, c in streams])
    picked, ends, ng = (C.c_uint32 * max(n, 1))(), (C.c_uint64 * max(n, 1))(), C.c_uint64()
    k = L.sim_inflate_blocks_pick(src, cap, n, picked, ends, C.byref(ng))
    return list(picked[:k]), list(ends[:ng.value])


def deflate_kernel_names(L, n, max_src_len, crc_op=1, **kw):
    """the names zipc_hip_kernel_times records for one zipc_hip_deflate_batch of n streams at a compressing level
    (deflate.hip launch_deflate_group's ZD_LAUNCH lines, slice by slice)"""
    f, _ = deflate_forms(L, n, max_src_len, **kw)
    names = {"deflate_offsets", "lz_chain", "lz_match"}
    if crc_op == 1:
        names |= {"crc32_segments", "crc32_finish"}
    k = f["slices"]
    for i in range(k):
        _, s = deflate_forms(L, n, max_src_len, m=n * (i + 1) // k - n * i // k, **kw)
        if f["segmented"]:
            names |= {"lz_parse_spec", "lz_parse_meet", "lz_parse_stitch", "lz_parse_gather", "deflate_plan", "deflate_counts",
                      "deflate_codelen", "deflate_scan", "deflate_pack", "deflate_seal"}
            if s["ppb"] != 1:
                names.add("deflate_bits")
        else:
            names |= {"lz_parse", "deflate_emit"}
    return names


# ---- zipc_amd/csrc/inflate_blocks.h through sim_forms.cpp: the rules of inflate by blocks between its launches
BLOCKS_LISTS = ("counts", "first", "cand", "recs", "sorted", "sorted_src", "chain", "chain_end", "chain_iv", "cks", "stream")
NO_MISS = (1 << 64) - 1  # FindCounts::miss_bit: the chain did not stop anywhere


def blocks_caps(L, src_len, explore_stride=16384):
    """(first_cap, cand_cap, max_explorers, rec_cap) of one stream's lists"""
    out = (C.c_uint64 * 4)()
    L.sim_blocks_caps(src_len, explore_stride, out)
    return tuple(out)


def blocks_scratch(L, src_lens, base=0, explore_stride=16384):
    """carve_blocks_scratch -> (the end, where the counts and the job list begin, a dict of addresses per stream)"""
    n = len(src_lens)
    head, lists = (C.c_uint64 * 2)(), (C.c_uint64 * (len(BLOCKS_LISTS) * n))()
    end = L.sim_blocks_scratch(base, (C.c_uint64 * n)(*src_lens), n, explore_stride, head, lists)
    k = len(BLOCKS_LISTS)
    return end, tuple(head), [dict(zip(BLOCKS_LISTS, lists[k * j:k * j + k])) for j in range(n)]


def blocks_verdicts(L, src_len=1 << 20, explore_stride=16384, n_cand=1, chain_ok=1, miss_bit=NO_MISS, n_recs=0, n_blocks=2, out_len=1,
                    token_bad=0, more_at=-1, rounds=6):
    """what the host makes of one stream's counts: dict(found, chained, explorers, waves, taken, done)"""
    out = (C.c_uint64 * 6)()
    L.sim_blocks_verdicts((C.c_uint64 * 11)(src_len, explore_stride, n_cand, chain_ok, miss_bit, n_recs, n_blocks, out_len, token_bad,
                                            more_at & NO_MISS, rounds), out)
    return dict(zip(("found", "chained", "explorers", "waves", "taken", "done"), out))


def blocks_token_plan(L, streams, follow_env=-1):
    """streams: (src_len, chain_ok, n_blocks, out_len, n_intervals) -> (per stream None or dict(follow, n, tok_at, out_len),
    call_out, tok_bytes)"""
    n = len(streams)
    out, total = (C.c_uint64 * (5 * n))(), (C.c_uint64 * 2)()
    L.sim_blocks_token_plan((C.c_uint64 * (5 * n))(*[v for s in streams for v in s]), n, follow_env, out, total)
    per = [dict(zip(("follow", "n", "tok_at", "out_len"), out[5 * j + 1:5 * j + 5])) if out[5 * j] else None for j in range(n)]
    return per, total[0], total[1]


def blocks_shares(L, waves, chunks):
    """-> (span_at, span bytes, sums_at, sums bytes) of streams with that many waves / Adler chunks"""
    n = len(waves)
    span_at, sums_at, total = (C.c_uint64 * n)(), (C.c_uint64 * n)(), (C.c_uint64 * 2)()
    L.sim_blocks_shares((C.c_uint32 * n)(*waves), (C.c_uint32 * n)(*chunks), n, span_at, sums_at, total)
    return list(span_at), total[0], list(sums_at), total[1]


# ---- zipc_amd/csrc/adler_chain.h through sim_adler.cpp: the Adler-32 chunk chain over chunk sums, the CRC-32 finish's grid
ADLER_REPLAY, ADLER_WALK = 0, 1


def adler_shape(L, length):
    """(n_chunks, n_runs, per) that zipc_hip_checksum_device takes for a buffer of that length"""
    out = (C.c_uint64 * 3)()
    L.sim_adler_shape(length, out)
    return tuple(out)


def _sums(S1, S2):
    import numpy as np

    a, b = np.ascontiguousarray(S1, dtype=np.uint32), np.ascontiguousarray(S2, dtype=np.uint32)
    assert a.shape == b.shape and a.ndim == 1
    return a, b


def adler_chain(L, S1, S2, length, n_runs=0, replay_max=0, amb_cap=0, seed=0):
    """the five launches over the chunk sums of a buffer of `length` bytes (chunk 0 is its first length % 5552 bytes)
    -> (value, dict(path, n_amb, n_runs, per)); n_runs, replay_max, amb_cap: 0 for the product's"""
    a, b = _sums(S1, S2)
    v, info = C.c_uint32(), (C.c_uint64 * 4)()
    st = L.sim_adler_chain(a.ctypes.data, b.ctypes.data, len(a), length, n_runs, replay_max, amb_cap, seed, C.byref(v), info)
    assert st == 0, "the sums are not those of %d bytes" % length
    return v.value, dict(zip(("path", "n_amb", "n_runs", "per"), info))


def adler_serial(L, S1, S2, length):
    a, b = _sums(S1, S2)
    v = C.c_uint32()
    assert L.sim_adler_serial(a.ctypes.data, b.ctypes.data, len(a), length, C.byref(v)) == 0
    return v.value


def adler_rfc(L, S1, S2, length):
    a, b = _sums(S1, S2)
    v = C.c_uint32()
    assert L.sim_adler_rfc(a.ctypes.data, b.ctypes.data, len(a), length, C.byref(v)) == 0
    return v.value


def crc_finish_grid(L, nseg, segs=None, threads=0):
    """crc32_finish_kernel's reads of nseg partials -> (used, loaded, dict(threads, rows, padp, one_thread)): the partial
    at every place of the fold in order (-1: a virtual zero), and every index a thread fetches"""
    import numpy as np

    segs = nseg if segs is None else segs
    cap = (nseg // 256 + 16) * 1024 + 16
    used, loaded = np.empty(cap, np.int64), np.empty(cap, np.uint64)
    nl, info = C.c_uint64(), (C.c_uint64 * 4)()
    nu = L.sim_crc_finish_grid(nseg, segs, threads, used.ctypes.data, cap, loaded.ctypes.data, cap, C.byref(nl), info)
    assert nu <= cap and nl.value <= cap
    return used[:nu], loaded[:nl.value], dict(zip(("threads", "rows", "padp", "one_thread"), info))


# ---- zipc_amd/csrc/host_pipeline.h through sim_many.cpp: the plan of a many-stream call
MANY_DEFLATE, MANY_INFLATE, MANY_RECODE = 0, 1, 2
MANY_SCALARS = ("src_arena_end", "dst_arena_end", "max_src", "max_cap", "max_mid", "K", "n_max", "total_max", "mid_arena",
                "mid_total_max", "ahead")
RECODE_DESC_FIELDS = ("src_off", "src_len", "mid_off", "mid_cap", "dst_off", "dst_cap", "limit", "flags", "expect_crc32")


def many_plan(L, op, src_len, dst_cap, limit=None, mid_cap=None, expect_crc32=None, chunks=0, chunk_min=1024):
    """plan_many of a call -> dict of MANY_SCALARS, src_off, dst_off, cut and, for a recode, rdescs (dicts of
    RECODE_DESC_FIELDS) and inflate_descs (tuples: src_off, src_len, dst_off, dst_cap, limit, flags, reserved)"""
    n = len(src_len)
    arr = lambda v, t=C.c_uint64: None if v is None else (t * max(n, 1))(*v)
    scalars, cut = (C.c_uint64 * len(MANY_SCALARS))(), (C.c_uint64 * 65)()
    src_off, dst_off = (C.c_uint64 * max(n, 1))(), (C.c_uint64 * max(n, 1))()
    rd, ind = (C.c_uint64 * (9 * max(n, 1)))(), (C.c_uint64 * (7 * max(n, 1)))()
    k = L.sim_many_plan(op, n, arr(src_len), arr(dst_cap), arr(limit), arr(mid_cap), arr(expect_crc32, C.c_uint32), chunks, chunk_min,
                        scalars, src_off, dst_off, cut, rd, ind)
    out = dict(zip(MANY_SCALARS, scalars), src_off=list(src_off[:n]), dst_off=list(dst_off[:n]), cut=list(cut[:k + 1]))
    if op == MANY_RECODE:
        out["rdescs"] = [dict(zip(RECODE_DESC_FIELDS, rd[9 * i:9 * i + 9])) for i in range(n)]
        out["inflate_descs"] = [tuple(ind[7 * i:7 * i + 7]) for i in range(n)]
    return out


# ---- sim_match.cpp: the serial reference of the match finder, and deflate_lane.h's lz_match_position beside it
MATCH_LEVELS = {1: (4, 1, 4), 2: (128, 32, 8), 3: (4096, 1024, 32)}  # level -> (K, Kq, good_match): level_params zd.ml:754-764
MATCH_SLACK = 512  # zero bytes behind a stream's copy: a mutant that drops the stream-end cap reads up to 258 of them


def _padded(data):
    import numpy as np

    buf = np.zeros(len(data) + MATCH_SLACK, np.uint8)
    buf[:len(data)] = np.frombuffer(data, np.uint8)
    return buf


def match_reference(L, data, level):
    """sim_match_reference -> (best, first): uint32 arrays over the positions 0 .. len - 4 (empty below 4 bytes)"""
    import numpy as np

    K, Kq, _ = MATCH_LEVELS[level]
    n = max(len(data) - 3, 0)
    best, first = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    buf = _padded(data)
    L.sim_match_reference(buf.ctypes.data, len(data), K, Kq, best.ctypes.data, first.ctypes.data)
    return best, first


def match_lane_position(L, data, level):
    """deflate_lane.h lz_match_position at every position, over sim_chain_serial's links -> (best, first)"""
    import numpy as np

    K, Kq, _ = MATCH_LEVELS[level]
    n = max(len(data) - 3, 0)
    best, first = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    links = np.zeros(len(data) + 8, np.uint16)
    buf = _padded(data)
    L.sim_chain_serial(buf.ctypes.data_as(C.c_char_p), len(data), links.ctypes.data)
    L.sim_match_lane_position(buf.ctypes.data, len(data), links.ctypes.data, K, Kq, best.ctypes.data, first.ctypes.data)
    return best, first


def match_parse_reads(L, length, level, best, first):
    """which record the lazy parse reads at every position (0 none, 1 best, 2 first, 3 comes by and reads neither)"""
    import numpy as np

    read = np.zeros(max(length - 3, 0), np.uint8)
    L.sim_match_parse_reads(length, MATCH_LEVELS[level][2], best.ctypes.data, first.ctypes.data, read.ctypes.data)
    return read


# ---- sim_chain.cpp: the serial reference of the hash-chain links, and the models of the four chain forms beside it
LINK_POISON = 0xFFFF  # include/zipc_hip.h ZIPC_HIP_DEBUG_LINK_POISON: no link exceeds 32768


def chain_links(L, data, model="reference", seg_positions=0, seed=1):
    """a stream's links by `model` -- "reference" (sim_chain_reference), "serial" (sim_chain_serial), "peel" (the model of
    lz_chain_kernel, by segments where seg_positions is not 0) or "xchg" (the exchange kernel's, the same) -- as a uint16
    array with one slot per BYTE, filled with LINK_POISON first: the slots of the last three bytes, and all of a stream
    shorter than 4, must still hold it"""
    import numpy as np

    links = np.full(len(data) + 8, LINK_POISON, np.uint16)
    if model == "reference":
        L.sim_chain_reference(data, len(data), links.ctypes.data)
    elif model == "serial":
        L.sim_chain_serial(data, len(data), links.ctypes.data)
    elif model == "peel" and seg_positions:
        L.sim_chain_segments(data, len(data), links.ctypes.data, seed, seg_positions)
    elif model == "peel":
        L.sim_chain(data, len(data), links.ctypes.data, seed, C.byref(C.c_int()))
    elif model == "xchg":
        L.sim_chain_xchg_segments(data, len(data), links.ctypes.data, seg_positions)
    else:
        raise ValueError(model)
    assert (links[len(data):] == LINK_POISON).all()
    return links[:len(data)]
