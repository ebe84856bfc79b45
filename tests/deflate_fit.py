"""Deflate's destination-capacity rule, stated once, from the oracle's block trace alone (nothing here runs on the GPU or
imports the code under test).  include/zipc_hip.h states it in words at zipc_hip_deflate_batch.

A compressing level ('Fast, 'Default, 'Best): blocks are tested one by one, in order.  A block fits when the bits in front
of it plus its size, rounded up to bytes, do not exceed dst_cap.  The size is the block's real size for a fixed or a stored
block, and the reference's ESTIMATE dlen (zd.ml:1071-1079) for a dynamic block.  dlen counts the code-length symbols of
every block so far (their counts are never reset, Q1), so from the second block on it runs high: a capacity that holds the
whole output can be refused, and a block in the middle can be the one that decides.  The first block that does not fit
refuses the stream; of the stream at most the whole bytes in front of that block are written.

Level 'None: the stream fits iff len + 5 * nblocks <= dst_cap, nblocks = 1 for an empty input and ceil(len / 65534)
otherwise; nothing is written when it does not.

tests/test_deflate_fit.py holds the table below, a mutation table of `needs`, and the host simulator to this;
tests/test_gpu_deflate_fit.py every deflate form of the library."""
import collections
import functools

import util

ST_OK, ST_DST_TOO_SMALL = 0, 16
MAX_BLOCK_SRC_LEN = 65534
STORED, FIXED, DYNAMIC = 0, 1, 2

# what the rule reads of a block (oracle.BlockInfo's fields of the same names)
Block = collections.namedtuple("Block", "kind nlen flen dlen bit_start bit_end")


def blocks_of(trace):
    return [Block(b.kind, b.nlen, b.flen, b.dlen, b.bit_start, b.bit_end) for b in trace]


def needs(blocks):
    """per block: the bytes dst_cap must hold for the block to pass"""
    out = []
    for b in blocks:
        est = b.dlen if b.kind == DYNAMIC else b.bit_end - b.bit_start
        out.append((b.bit_start + est + 7) // 8)
    return out


def unfit(need, cap):
    return need > cap


def min_cap(blocks, needs=needs):
    return max(needs(blocks))


def first_unfit(blocks, cap, needs=needs, unfit=unfit):
    for i, n in enumerate(needs(blocks)):
        if unfit(n, cap):
            return i
    return None


def stored_nblocks(n):
    return 1 if n == 0 else (n + MAX_BLOCK_SRC_LEN - 1) // MAX_BLOCK_SRC_LEN


def stored_need(n, nblocks=stored_nblocks):
    return n + 5 * nblocks(n)


@functools.lru_cache(maxsize=None)
def trace(data, level):
    """(the oracle's output, its blocks)"""
    import oracle

    st, out, _, tr = oracle.deflate_trace(data, level=level)
    assert st == 0
    return out, tuple(blocks_of(tr))


def expect(data, level, cap):
    """-> (status, out, whole_bytes_in_front): what a deflate of `data` into `cap` bytes gives.  Status 0: out is the
    oracle's output.  Status 16: out is b"", and whole_bytes_in_front is where the first block that does not fit starts,
    in whole bytes: nothing is written at or behind it, and what is written in front of it is the oracle's."""
    out, blocks = trace(data, level)
    if level == 0:
        return (ST_OK, out, 0) if stored_need(len(data)) <= cap else (ST_DST_TOO_SMALL, b"", 0)
    i = first_unfit(blocks, cap)
    if i is None:
        assert len(out) <= cap
        return ST_OK, out, 0
    return ST_DST_TOO_SMALL, b"", blocks[i].bit_start // 8


def least_room(data, level):
    """the smallest dst_cap the rule takes"""
    return stored_need(len(data)) if level == 0 else min_cap(trace(data, level)[1])


def fits(data, level, cap):
    return expect(data, level, cap)[0] == ST_OK


# ---- the case table: the smallest inputs on which each clause of the rule matters
ZEROS196K = bytes(3 * 65534 + 10)


@functools.lru_cache(maxsize=None)
def inputs():
    d = util.deflate_cases()
    return {
        "empty": b"", "one": b"z", "fox": util.FOX, "text5000": util.text(5000, 7), "rand3000": util.rand_bytes(3000, 2),
        "zeros70k": d["zeros70k"], "zeros196k": ZEROS196K, "rand70k": d["rand70k"], "far_match": d["far_match"],
        "tie_nf_b2_loss8": d["tie_nf_b2_loss8"], "few70000": util.rand_bytes(70000, 9, bits=2),
        "text200k": util.text(200000, 3), "len65534": d["len65534"], "len65535": d["len65535"],
    }


STORED_LENGTHS = (0, 1, 65534, 65535)


@functools.lru_cache(maxsize=None)
def stored_inputs():
    return {"none%d" % n: util.rand_bytes(n, 60 + n % 5) for n in STORED_LENGTHS}


def levels_of(name):
    return (2,) if name in ("zeros196k", "text200k") else (1, 2, 3)


def caps_of(data, level):
    """the caps a (case, level) is run at, in order, deduplicated"""
    import oracle

    out, blocks = trace(data, level)
    clen = len(out)
    if level == 0:
        mc, front = stored_need(len(data)), 0
    else:
        mc = min_cap(blocks)
        n = needs(blocks)
        front = blocks[n.index(mc)].bit_start // 8  # whole_bytes_in_front of the binding block
    caps = [0, 1, front - 1, front, clen - 1, clen, mc - 1, mc, mc + 1, oracle.deflate_bound(len(data))]
    return sorted({c for c in caps if c >= 0})


@functools.lru_cache(maxsize=None)
def table():
    """[(name, level, cap)] of the whole table"""
    rows = []
    for name, data in inputs().items():
        for level in levels_of(name):
            rows += [(name, level, cap) for cap in caps_of(data, level)]
    for name, data in stored_inputs().items():
        rows += [(name, 0, cap) for cap in caps_of(data, 0)]
    return tuple(rows)


def data_of(name):
    return inputs()[name] if name in inputs() else stored_inputs()[name]
