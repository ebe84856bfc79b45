"""A serial reference for the tokens of inflate by blocks (tests/test_token_rules.py, tests/test_gpu_inflate_tokens.py).

A plain RFC 1951 decoder, written from the format and from the reference's read_block_symbols / Buf.recopy (zd.ml: a match
of `len` bytes at distance `dist` copies byte by byte, so byte i of it is byte i mod dist of its source) -- not from the
kernels and not from the host model.  Besides the plain bytes it says where every byte came from:

  src[i]    i for a literal or a stored byte, i - dist for a byte of a match
  root[i]   the literal (or stored byte) the chain i -> src[i] -> src[src[i]] ... ends in
  depth[i]  the links of that chain (0 for a literal)
  blocks    per block: first bit of its header, first bit behind it, output position, output length, kind
  matches   per match: output position, length, distance (numpy, in stream order)

and answers "is t on the chain of i" for whole arrays at once (is_ancestor: binary lifting over src[], n log(depth)).
Test only; the product never imports it.
"""
import collections

import numpy as np

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
         8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
STORED, FIXED, DYNAMIC = 0, 1, 2

Block = collections.namedtuple("Block", "start_bit end_bit out_pos out_len kind")


class FormatError(ValueError):
    pass


def _table(lengths):
    """(table, bits): table[next `bits` bits of the input, first bit lowest] = symbol << 4 | code length; 0: no code"""
    bits = max(lengths) if lengths else 0
    if bits == 0:
        return [0], 0
    table = [0] * (1 << bits)
    code = 0
    for ln in range(1, bits + 1):
        for sym, sl in enumerate(lengths):
            if sl != ln:
                continue
            if code >> ln:
                raise FormatError("over-subscribed code")
            rev = int(format(code, "0%db" % ln)[::-1], 2)  # (Huffman codes go into the stream from their top bit)
            table[rev::1 << ln] = [sym << 4 | ln] * (1 << (bits - ln))
            code += 1
        code <<= 1
    return table, bits


_FIXED = None


def _fixed_tables():
    global _FIXED
    if _FIXED is None:
        _FIXED = (_table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _table([5] * 30))
    return _FIXED


class Ref:
    """what decode() returns (see the module's docstring); root, depth and the ancestor levels are made when first asked for"""

    def __init__(self, plain, src, blocks, matches):
        self.plain, self.src, self.blocks = plain, src, blocks
        self.m_pos, self.m_len, self.m_dist = (np.array(c, dtype=np.int64) for c in (zip(*matches) if matches else ((), (), ())))
        self._root = self._depth = None
        self._up = None

    # ---- root and depth: one forward pass, a match at a time (its source is final when its turn comes)
    def _chains(self):
        n = len(self.src)
        root, depth = np.arange(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        for p, ln, d in zip(self.m_pos.tolist(), self.m_len.tolist(), self.m_dist.tolist()):
            if d >= ln:
                root[p:p + ln] = root[p - d:p - d + ln]
                depth[p:p + ln] = depth[p - d:p - d + ln] + 1
            else:  # byte i copies byte i - dist, which for i >= dist is a byte of this match: one link more each period
                k = np.arange(ln)
                root[p:p + ln] = root[p - d:p][k % d]
                depth[p:p + ln] = depth[p - d:p][k % d] + 1 + k // d
        self._root, self._depth = root, depth

    @property
    def root(self):
        if self._root is None:
            self._chains()
        return self._root

    @property
    def depth(self):
        if self._depth is None:
            self._chains()
        return self._depth

    def is_literal(self):
        return self.src == np.arange(len(self.src))

    def is_ancestor(self, t, i=None):
        """per byte i (default: every byte): t[i] lies on the chain of i, i itself included -- t[i] is the ancestor of i at
        depth[t[i]].  Walks depth[i] - depth[t[i]] links up from i by doubling: up_k = 2^k links."""
        i = np.arange(len(self.src), dtype=np.int64) if i is None else np.asarray(i, dtype=np.int64)
        t = np.asarray(t, dtype=np.int64)
        ok = (t >= 0) & (t <= i)
        ts = np.where(ok, t, 0)
        delta = self.depth[i] - self.depth[ts]
        ok &= delta >= 0
        delta = np.where(ok, delta, 0)
        cur, up = i.copy(), self.src
        k = 0
        top = int(delta.max()) if len(delta) else 0
        while top >> k:
            step = (delta >> k) & 1 == 1
            cur[step] = up[cur[step]]
            k += 1
            if top >> k:
                up = up[up]
        return ok & (cur == ts)

    def block_of(self, i):
        for k, b in enumerate(self.blocks):
            if b.out_pos <= i < b.out_pos + b.out_len:
                return k
        return -1

    def describe(self, i):
        """where byte i is: block and symbol, for a failure's message"""
        k = self.block_of(i)
        if self.src[i] == i:
            return "byte %d: block %d (kind %d), a literal %#04x" % (i, k, self.blocks[k].kind if k >= 0 else -1, self.plain[i])
        j = int(np.searchsorted(self.m_pos, i, side="right")) - 1
        return "byte %d: block %d (kind %d), byte %d of match %d (pos %d len %d dist %d), src %d root %d depth %d" % (
            i, k, self.blocks[k].kind if k >= 0 else -1, i - self.m_pos[j], j, self.m_pos[j], self.m_len[j], self.m_dist[j],
            self.src[i], self.root[i], self.depth[i])


def decode(data):
    """the whole stream -> Ref; FormatError where RFC 1951 says the stream is wrong"""
    data = bytes(data)
    n_in = len(data)
    out = bytearray()
    matches, blocks = [], []
    buf = cnt = pos = 0  # bit buffer: `cnt` bits of `buf`, the next input byte is data[pos]

    def bitpos():
        return pos * 8 - cnt

    final = False
    while not final:
        start_bit, out_pos = bitpos(), len(out)
        if cnt < 3:
            buf |= int.from_bytes(data[pos:pos + 4], "little") << cnt; pos += 4; cnt += 32
        final, kind = bool(buf & 1), (buf >> 1) & 3
        buf >>= 3; cnt -= 3
        if kind == 3:
            raise FormatError("block type 3")
        if kind == STORED:
            at = (bitpos() + 7) // 8
            if at + 4 > n_in:
                raise FormatError("stored header beyond the input")
            ln, nln = int.from_bytes(data[at:at + 2], "little"), int.from_bytes(data[at + 2:at + 4], "little")
            if ln != (~nln & 0xFFFF) or at + 4 + ln > n_in:
                raise FormatError("stored block")
            out += data[at + 4:at + 4 + ln]
            pos, buf, cnt = at + 4 + ln, 0, 0
            blocks.append(Block(start_bit, pos * 8, out_pos, ln, kind))
            continue
        if kind == FIXED:
            (lt, lb), (dt, db) = _fixed_tables()
        else:
            if cnt < 14:
                buf |= int.from_bytes(data[pos:pos + 4], "little") << cnt; pos += 4; cnt += 32
            hlit, hdist, hclen = (buf & 31) + 257, ((buf >> 5) & 31) + 1, ((buf >> 10) & 15) + 4
            buf >>= 14; cnt -= 14
            cl = [0] * 19
            for k in range(hclen):
                if cnt < 3:
                    buf |= int.from_bytes(data[pos:pos + 4], "little") << cnt; pos += 4; cnt += 32
                cl[CL_ORDER[k]] = buf & 7
                buf >>= 3; cnt -= 3
            ct, cb = _table(cl)
            lens = []
            while len(lens) < hlit + hdist:
                if cnt < 16:
                    buf |= int.from_bytes(data[pos:pos + 4], "little") << cnt; pos += 4; cnt += 32
                e = ct[buf & ((1 << cb) - 1)]
                if e == 0:
                    raise FormatError("code length code")
                buf >>= e & 15; cnt -= e & 15
                s = e >> 4
                if s < 16:
                    lens.append(s)
                elif s == 16:
                    if not lens:
                        raise FormatError("repeat without a length")
                    lens += [lens[-1]] * (3 + (buf & 3)); buf >>= 2; cnt -= 2
                elif s == 17:
                    lens += [0] * (3 + (buf & 7)); buf >>= 3; cnt -= 3
                else:
                    lens += [0] * (11 + (buf & 127)); buf >>= 7; cnt -= 7
            if len(lens) > hlit + hdist:
                raise FormatError("repeat past the end")
            lt, lb = _table(lens[:hlit])
            dt, db = _table(lens[hlit:])
        lmask, dmask = (1 << lb) - 1, (1 << db) - 1
        while True:
            if cnt < 48:
                buf |= int.from_bytes(data[pos:pos + 8], "little") << cnt; pos += 8; cnt += 64
            e = lt[buf & lmask]
            if e == 0:
                raise FormatError("literal/length code")
            buf >>= e & 15; cnt -= e & 15
            s = e >> 4
            if s < 256:
                out.append(s)
                continue
            if s == 256:
                break
            if s > 285:
                raise FormatError("length symbol")
            s -= 257
            x = LEXT[s]
            ln = LBASE[s] + (buf & ((1 << x) - 1)); buf >>= x; cnt -= x
            e = dt[buf & dmask]
            if e == 0:
                raise FormatError("distance code")
            buf >>= e & 15; cnt -= e & 15
            s = e >> 4
            if s > 29:
                raise FormatError("distance symbol")
            x = DEXT[s]
            dist = DBASE[s] + (buf & ((1 << x) - 1)); buf >>= x; cnt -= x
            p = len(out)
            if dist > p:
                raise FormatError("distance beyond the output")
            matches.append((p, ln, dist))
            if dist >= ln:
                out += out[p - dist:p - dist + ln]
            else:
                out += (bytes(out[p - dist:]) * (ln // dist + 1))[:ln]
        if bitpos() > n_in * 8:
            raise FormatError("input ends inside a block")
        blocks.append(Block(start_bit, bitpos(), out_pos, len(out) - out_pos, kind))
    n = len(out)
    src = np.arange(n, dtype=np.int64)
    for p, ln, d in matches:
        src[p:p + ln] -= d
    return Ref(bytes(out), src, blocks, matches)


def src_of_symbols(blocks):
    """src[] as a list of blocks of tests/golden/inflate_rules.py SAYS it (literals, ('m', len, dist) with dist a number or a
    function of the output so far, stored data): the other entry of the double entry -- nothing is decoded here"""
    src = []
    for blk in blocks:
        if blk.kind == "stored":
            src += range(len(src), len(src) + len(blk.syms))
            continue
        for s in blk.syms:
            if isinstance(s, int):
                src.append(len(src))
            else:
                assert s[0] == "m", s
                d = s[2](len(src)) if callable(s[2]) else s[2]
                for _ in range(s[1]):
                    src.append(len(src) - d)
    return np.array(src, dtype=np.int64)


def word_failures(ref, tok, exact):
    """THE INVARIANT of the block path's tokens, for a whole stream at once -> the bytes whose word breaks it:
         tok[i] == i  iff  byte i is a literal or a stored byte;
         else tok[i] < i and tok[i] lies on byte i's chain of copies (an ancestor);
         exact (sources written down plainly): tok[i] == src[i] itself."""
    n = len(ref.src)
    i = np.arange(n, dtype=np.int64)
    tok = np.asarray(tok[:n], dtype=np.int64)
    lit = ref.is_literal()
    bad = lit & (tok != i)
    bad |= ~lit & ~((tok < i) & ref.is_ancestor(tok))
    if exact:
        bad |= tok != ref.src
    return np.nonzero(bad)[0]
