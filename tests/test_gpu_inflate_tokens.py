"""Every token of inflate by blocks on the MI355X against a serial decode, in both token forms.

The block path's second half -- inflate_tok_init, inflate_blocks_token, inflate_resolve, inflate_gather, the block-wise
Adler-32 -- hides its own failures (a stream it gives up on is decoded again by its one wave) and wrong tokens hide in right
bytes (out[i] = out[tok[i]] is right whenever the wrong source holds the same byte).  zipc_hip_debug_inflate_tokens lays
tok[] open behind the token run (raw) and behind the last resolve round (done), with a record per stream; here every word is
held to tests/token_ref.py over the catalogue of tests/token_cases.py:

  rows   form {0: a wave per interval; 1: follow} x hops {(256, 256), (16, 16), (3, 5)}, each ONE call over the
         whole catalogue side by side (ragged lengths, destination offsets 0, 1, 5, 15 mod 16, 64 guard bytes around every
         destination, both word arrays 0xFFFFFFFF beforehand); six streams also go alone, in the default row.
  per stream   the record says "taken" exactly where the catalogue says so and n_blocks is the reference's block count;
         token_bad == 0; more[] does not grow; form 0: more[r] <= the reference's count of bytes deeper than hops0 * hops1^r
         (a kernel may only shorten a chain); done in every row; raw meets the invariant (token_ref.word_failures; its exact
         clause tok[i] == src[i] is held on the host model only: on the device the wide turn's store and wave_match look the
         source's own word up in form 0 too, and a word does not say which code wrote it), done[i] ==
         root[i] for every byte; words outside [dst_off, dst_off + out_len) and those of refused streams stay 0xFFFFFFFF;
         status, length and bytes are the oracle's, guard bytes untouched.
  the (3, 5) rows   form 0: the stream "deep" must leave more[0] > 2048 * 256 bytes to the later rounds, whose grid is capped at
         2048 workgroups: their stride loop takes a second trip.  Form 1 follows that stream's chains in the token run itself and
         leaves the rounds nothing: no such assertion there (see the test).
  Adler-32   the streams of the Adler-32 group (blocks of 0, 1, 5551, 5552, 5553, 11104, 11105 bytes) through
         zipc_hip_inflate_batch with the reference's Adler-32 and RFC 1950's; last_inflate_blocks() is the exact block count.
"""
import os
import zlib

import numpy as np
import pytest

import token_cases as TC
import token_ref as TR

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(os.environ.get("ZIPC_HIP_INFLATE_BLOCKS") == "0", reason="the block path is turned off")]

POISON = 0xFFFFFFFF
GUARD, GUARD_BYTE = 64, 0xA5
OFFSETS = (0, 1, 5, 15)
ROWS = [(form, hops) for form in (0, 1) for hops in ((256, 256), (16, 16), (3, 5))]
SECOND_TRIP = 2048 * 256  # a later round's grid times its workgroup: more bytes than that and its stride loop goes round again


class World:
    """the catalogue, its reference and the oracle's verdicts, made once; batch(names): the device arenas of a call"""

    def __init__(self, oracle):
        self.cases = {c.name: c for c in TC.catalogue()}
        self.refs = {n: TR.decode(c.stream) for n, c in self.cases.items()}
        for n, c in self.cases.items():
            st, plain, _ = oracle.inflate(c.stream)
            assert st == 0 and plain == self.refs[n].plain, n

    def batch(self, names):
        import torch

        from zipc_amd import batch

        dev = torch.device("cuda", 0)
        streams = [self.cases[n].stream for n in names]
        lens = [len(self.refs[n].plain) for n in names]
        src_off = np.cumsum([0] + [(len(s) + 63) // 64 * 64 for s in streams[:-1]]).astype(np.uint64)
        src = np.zeros(int(src_off[-1]) + len(streams[-1]) + 64, dtype=np.uint8)
        for o, s in zip(src_off, streams):
            src[int(o):int(o) + len(s)] = np.frombuffer(s, dtype=np.uint8)
        dst_off, at = [], 0
        for k, n in enumerate(lens):  # 64 guard bytes, then the destination at 0, 1, 5, 15 mod 16 in turn
            at = (at + GUARD + 15) // 16 * 16 + OFFSETS[k % 4]
            dst_off.append(at)
            at += n
        B = type("Batch", (), {})()
        B.names, B.lens, B.dst_off, B.size = names, lens, dst_off, at + GUARD + 16
        B.descs = batch.to_device(batch.make_descs(src_off, [len(s) for s in streams], np.array(dst_off, dtype=np.uint64), lens), dev)
        B.src = torch.from_numpy(src).to(dev)
        B.dev = dev
        return B


@pytest.fixture(scope="module")
def world(oracle):
    return World(oracle)


@pytest.fixture(scope="module")
def whole(world):
    return world.batch(list(TC.NAMES))


def run_tokens(ctx, world, B, form, hops):
    """one zipc_hip_debug_inflate_tokens call over B, every assertion of a row -> the records"""
    import torch

    from zipc_amd import batch

    dst = torch.full((B.size,), GUARD_BYTE, dtype=torch.uint8, device=B.dev)
    raw = torch.full((B.size,), -1, dtype=torch.int32, device=B.dev)
    done = torch.full((B.size,), -1, dtype=torch.int32, device=B.dev)
    d_res = torch.zeros(len(B.names) * 16, dtype=torch.uint8, device=B.dev)
    rec = batch.debug_inflate_tokens(ctx, B.src, dst, B.descs, d_res, len(B.names), max(B.lens), raw, done, form, hops[0], hops[1])
    res = batch.results_from_device(d_res)
    out = dst.cpu().numpy()
    raw, done = raw.cpu().numpy().view(np.uint32), done.cpu().numpy().view(np.uint32)
    inside = np.zeros(B.size, dtype=bool)
    for k, name in enumerate(B.names):
        c, r, R, off, n = world.cases[name], world.refs[name], rec[k], B.dst_off[k], B.lens[k]
        what = (name, "form %d hops %s" % (form, hops))
        # status, length and bytes are the ordinary call's
        assert int(res["status"][k]) == 0 and int(res["out_len"][k]) == n, what
        got = out[off:off + n]
        if got.tobytes() != r.plain:
            i = int(np.nonzero(got != np.frombuffer(r.plain, dtype=np.uint8))[0][0])
            raise AssertionError("%s: bytes differ from %s" % (what, r.describe(i)))
        inside[off:off + n] = True
        # the record
        assert int(R["taken"]) == int(c.taken), (what, "taken %d" % R["taken"])
        if not c.taken:
            assert (raw[off:off + n] == POISON).all() and (done[off:off + n] == POISON).all(), (what, "words of a refused stream were written")
            assert R.tobytes() == bytes(R.nbytes), what
            continue
        assert int(R["n_blocks"]) == len(r.blocks), (what, int(R["n_blocks"]), len(r.blocks))
        assert int(R["n_intervals"]) >= len(r.blocks) and int(R["token_bad"]) == 0, (what, R)
        assert int(R["form"]) == form if form >= 0 else int(R["form"]) in (0, 1), (what, R)
        rounds = int(R["rounds"])
        more = [int(x) for x in R["more"][:rounds]]
        assert rounds == (6 if min(hops) >= 16 or hops == (0, 0) else 12), (what, rounds)
        assert all(a >= b for a, b in zip(more, more[1:])), (what, more)
        if int(R["form"]) == 0:  # no word is further from its literal than src[] puts it: a kernel may only shorten a chain
            h0, h1 = (hops[0] or 256), (hops[1] or 256)
            for rr, m in enumerate(more):
                ceiling = int((r.depth > h0 * h1 ** rr).sum()) if h0 * h1 ** rr <= int(r.depth.max()) else 0
                assert m <= ceiling, (what, "round %d left %d bytes open, the reference has %d that deep" % (rr, m, ceiling))
        assert more[-1] == 0 and int(R["blocks_done"]) == 1, (what, more, R)
        # the words
        bad = TR.word_failures(r, raw[off:off + n], False)
        if len(bad):
            i = int(bad[0])
            raise AssertionError("%s: %d raw words break the invariant, first at %s: tok %d" % (what, len(bad), r.describe(i), raw[off + i]))
        wrong = np.nonzero(done[off:off + n].astype(np.int64) != r.root)[0]
        if len(wrong):
            i = int(wrong[0])
            raise AssertionError("%s: %d resolved words are not the root, first at %s: tok %d" % (what, len(wrong), r.describe(i), done[off + i]))
    assert (raw[~inside] == POISON).all() and (done[~inside] == POISON).all(), "a word outside every stream's range was written"
    assert (out[~inside] == GUARD_BYTE).all(), "a guard byte was written"
    return {name: rec[k] for k, name in enumerate(B.names)}


@pytest.mark.parametrize("form,hops", ROWS, ids=["form%d-hops%d_%d" % (f, h[0], h[1]) for f, h in ROWS])
def test_every_token_of_the_catalogue(gpu_ctx, world, whole, form, hops):
    rec = run_tokens(gpu_ctx, world, whole, form, hops)
    if hops == (3, 5):
        deep = rec["deep"]
        more = [int(x) for x in deep["more"]]
        print("deep, form %d: more = %s (the reference has %d bytes deeper than 3)" % (form, more, int((world.refs["deep"].depth > 3).sum())))
        if form == 0:
            # the later rounds' second trip.  Measured on the MI355X: more = [1190976, 1568, 0, ...] of a ceiling of 1708032 --
            # round 0 resolves in place, and a thread that reads a word another has already moved gets further than its 3 hops
            assert more[0] > SECOND_TRIP, more
        # form 1 cannot be held to that: the body of "deep" is ONE block, so one wave writes all of it and looks every source up in
        # the words it wrote itself a tile or two earlier (inflate_span.h: "a source before the tile is looked up in tok[]") --
        # every byte arrives at its literal in the token run already and the rounds find nothing (measured: more[0] = 0).  That is
        # the form doing its work, not racing; whether a wave sees ANOTHER wave's words in time is a race no stream can pin.  The
        # row keeps every other assertion.


@pytest.mark.parametrize("name", TC.ALONE)
def test_a_stream_alone_in_the_default_row(gpu_ctx, world, name):
    rec = run_tokens(gpu_ctx, world, world.batch([name]), -1, (0, 0))
    assert int(rec[name]["form"]) == 0  # (follow is for calls of 32 MiB and more)


def test_arguments_no_launch_could_use(gpu_ctx, world):
    import torch

    from zipc_amd import batch

    from zipc_amd._lib import ERR_INVALID_ARG, ZipcHipError

    B = world.batch(["len_dist_grid"])
    dst = torch.zeros(B.size, dtype=torch.uint8, device=B.dev)
    words = torch.zeros(B.size, dtype=torch.int32, device=B.dev)
    d_res = torch.zeros(16, dtype=torch.uint8, device=B.dev)
    for form, h0, h1 in ((2, 0, 0), (-2, 0, 0), (0, -1, 0), (0, 0, -1), (0, 65537, 0), (0, 0, 65537)):
        with pytest.raises(ZipcHipError) as e:
            batch.debug_inflate_tokens(gpu_ctx, B.src, dst, B.descs, d_res, 1, B.lens[0], words, words, form, h0, h1)
        assert e.value.status == ERR_INVALID_ARG, (form, h0, h1, e.value.status)


@pytest.mark.parametrize("rfc", (False, True), ids=("reference", "rfc1950"))
def test_adler32_by_blocks(gpu_ctx, oracle, world, rfc):
    """the Adler-32 group, each stream alone (a call of several opens the block path at 256 KiB of room only): the checksum is
    the oracle's block-wise one, or zlib's; the block path decoded it: last_inflate_blocks() is the reference's block count"""
    import torch

    from zipc_amd import batch
    from zipc_amd._lib import CRC_ADLER32, CRC_ADLER32_RFC1950

    for name in ("adler_0", "adler_1", "adler_2"):
        c, r = world.cases[name], world.refs[name]
        B = world.batch([name])
        dst = torch.full((B.size,), GUARD_BYTE, dtype=torch.uint8, device=B.dev)
        d_res = torch.zeros(16, dtype=torch.uint8, device=B.dev)
        batch.inflate_batch(gpu_ctx, B.src, dst, B.descs, d_res, 1, B.lens[0], CRC_ADLER32_RFC1950 if rfc else CRC_ADLER32)
        res = batch.results_from_device(d_res)
        out = dst.cpu().numpy()
        off, n = B.dst_off[0], B.lens[0]
        assert int(res["status"][0]) == 0 and int(res["out_len"][0]) == n and out[off:off + n].tobytes() == r.plain, name
        assert (out[:off] == GUARD_BYTE).all() and (out[off + n:] == GUARD_BYTE).all(), name
        want = zlib.adler32(r.plain) if rfc else oracle.inflate(c.stream, None, CRC_ADLER32)[2]
        assert int(res["checksum"][0]) == want, (name, hex(int(res["checksum"][0])), hex(want))
        assert gpu_ctx.last_inflate_blocks() == len(r.blocks), (name, gpu_ctx.last_inflate_blocks(), len(r.blocks))
