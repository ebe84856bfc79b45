"""zipc_amd/csrc/parse_tile.h -- the one predicate by which lz_parse_wave (deflate.hip) runs a tile of 64 positions in its
interior form (no clamps, no masks of the stream's end, no block cut) or in the general edge form -- compiled with g++
(tests/parse_tile_sim/sim_parse_tile.cpp) and enumerated.  The expected values are the few lines of arithmetic below, not
the header.  No GPU; the kernels are checked in tests/test_gpu_parse_tiles.py."""
import ctypes as C
import os

import numpy as np
import pytest

import mutation
import util  # noqa: F401  (sets sys.path through conftest)

HERE = os.path.dirname(os.path.abspath(__file__))
SIM = os.path.join(HERE, "parse_tile_sim", "sim_parse_tile.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "zipc_amd", "csrc")
TILE = 64
MAX_BLOCK_SRC_LEN = 65534
STEP_MAX = 255 + 258  # deferral literals + the longest match: the furthest a macro step advances


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    L = C.CDLL(mutation.gxx(tmp_path_factory.mktemp("parse_tile_sim") / "libparse_tile_sim.so", [SIM], include=[CSRC],
                            extra=["-Wall", "-Wno-unknown-pragmas"]))
    L.sim_parse_tile_interior.restype = C.c_int
    L.sim_parse_tile_interior.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    L.sim_parse_tile_forms.restype = None
    L.sim_parse_tile_forms.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
    L.sim_parse_interior_end.restype = C.c_uint32
    L.sim_parse_interior_end.argtypes = [C.c_uint32, C.c_uint32, C.c_int]
    return L


def _forms(sim, ln, blk_start, cuts):
    out = np.zeros((ln + TILE - 1) // TILE + 1, np.uint8)
    sim.sim_parse_tile_forms(ln, blk_start, cuts, out.ctypes.data)
    return out[:(ln + TILE - 1) // TILE]


def _furthest_load(B):
    """the last source byte the tile at B asks for: lane 63's 4-byte word of the tile three ahead"""
    return B + 3 * TILE + 63 + 3


def test_never_interior_where_a_load_would_pass_the_end(sim):
    chosen = 0
    for ln in range(0, 1025):
        for cuts in (0, 1):
            for B in range(0, max(ln, 1), TILE):
                for blk_start in sorted({0, B, max(B - 1, 0), B // 2}):
                    got = sim.sim_parse_tile_interior(B, ln, blk_start, cuts)
                    chosen += got
                    assert not (got and _furthest_load(B) >= ln), (ln, B, blk_start, cuts)
                    # ... and the other way round: these lengths hold no block cut, so the end is all that can refuse a tile
                    assert got or _furthest_load(B) >= ln, (ln, B, blk_start, cuts)
    assert chosen


def test_never_interior_where_a_block_cut_can_fall(sim):
    """a wave that cuts blocks (one wave per stream): the tile's last lane, B + 63, may advance by 513"""
    ln = 3 * 65536
    seen = {0: 0, 1: 0}
    for blk_start in (0, 1, 63, 64, 100, 65534, 65534 + 255, 2 * 65534 - 17):
        for B in range(blk_start // TILE * TILE, min(blk_start + 65536 + 2 * TILE, ln - 5 * TILE), TILE):
            if blk_start > B + 63 + 255:  # (the open block starts in the tile, or a deferral's literals behind it)
                continue
            got = sim.sim_parse_tile_interior(B, ln, blk_start, 1)
            can_cut = B + 63 - blk_start + STEP_MAX > MAX_BLOCK_SRC_LEN
            assert not (got and can_cut), (B, blk_start)
            assert got or can_cut, (B, blk_start)  # (far from the end nothing else refuses a tile)
            seen[got] += 1
            # a wave per segment cuts no blocks: the stitch does
            assert sim.sim_parse_tile_interior(B, ln, blk_start, 0) == 1, (B, blk_start)
    assert seen[0] >= 8 * 4 and seen[1] >= 8 * 1000  # (both sides of the line were met)


def test_interior_for_all_but_the_last_tiles_of_a_64k_stream(sim):
    """An always-false predicate would pass the two tests above.  A stream of 64 KiB has 1024 tiles; the last four reach past
    its end (65536 - 259 = 65277: tile 1019 is the last that fits), so all but the last 5 are interior where no block is cut
    (a wave per segment).  The wave that cuts blocks meets byte 65534 in the same stream: of the tiles before the last 5, those
    the rule of the test above refuses (B + 63 + 513 > 65534: tiles 1015 ..) are the only ones not chosen."""
    ln = 65536
    f = _forms(sim, ln, 0, 0)
    assert len(f) == 1024 and f[:1024 - 5].all() and not f[1024 - 4:].any()
    g = _forms(sim, ln, 0, 1)
    for t in range(1024 - 5):
        assert g[t] == (t * TILE + 63 + STEP_MAX <= MAX_BLOCK_SRC_LEN), t
    assert int(g.sum()) == 1015 and not g[1015:].any()
    # behind the cut the rest of the stream is the edge form by its end alone, whatever the block's start
    h = _forms(sim, ln, 65534, 1)
    assert not h[1024 - 4:].any()


def test_the_loops_bound_is_the_predicate(sim):
    """parse_interior_end, the one compare a tile the kernel's loop makes: B < end exactly where the predicate holds"""
    cases = [(ln, b, c) for ln in list(range(0, 1025)) + [65534, 65535, 65536, 65536 + 320, 3 * 65536, 0xFFFF0000]
             for b in (0, 64, 100) if b <= ln for c in (0, 1)]
    cases += [(3 * 65536, b, 1) for b in (65534, 65534 + 255, 2 * 65534 - 17)] + [(0xFFFF0000, 0xFFFF0000 - 65534 - 7, 1)]
    for ln, blk_start, cuts in cases:
        end = sim.sim_parse_interior_end(ln, blk_start, cuts)
        assert end <= max(ln, 1), (ln, blk_start, cuts)
        lo = blk_start // TILE * TILE
        tiles = set(range(lo, min(ln, lo + 4 * TILE), TILE)) | {B for B in range(max(lo, end // TILE * TILE - 2 * TILE), min(ln, end + 3 * TILE), TILE)}
        for B in tiles:
            assert sim.sim_parse_tile_interior(B, ln, blk_start, cuts) == (B < end), (ln, blk_start, cuts, B, end)
