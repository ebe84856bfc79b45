"""zipc_amd/csrc/recode_rules.h -- what stands before, between and behind inflate and deflate when a batch is recoded on
the device, one header for the kernels of recode.hip, the host form and this test -- compiled with g++
(tests/recode_sim/sim_recode.cpp, a program of its own) and held against a table of every rule, written down here from
include/zipc_hip.h's words.  No GPU; the kernels that apply the rules are checked in tests/test_gpu_recode_batch.py."""
import os
import subprocess

import pytest

import mutation
import util  # noqa: F401  (sets sys.path through conftest)

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "recode_sim", "sim_recode.cpp")
HAS_LIMIT, EXPECT_CRC32 = 1, 2
MAX_MID = 1000


def build(tmp, *flags):
    return mutation.gxx(tmp / ("sim_recode" + ("_san" if flags else "")), [SRC], shared=False, opt="-O1",
                        extra=["-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas", *flags])


@pytest.fixture(scope="module")
def sims(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("recode_sim")
    return build(tmp), build(tmp, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")


class Row:
    """one stream of the table: its descriptor, and what the codec says of it if it gets there"""

    def __init__(self, name, flags=0, expect=0, mid_cap=500, limit=0, inflate=(0, 0xC0FFEE, 300), deflate=(0, 120)):
        self.name, self.flags, self.expect, self.mid_cap, self.limit, self.inflate, self.deflate = name, flags, expect, mid_cap, limit, inflate, deflate

    def line(self, i):
        self.src_off, self.src_len, self.mid_off, self.dst_off, self.dst_cap = 1000 * i + 3, 77 + i, 2000 * i + 256, 3000 * i + 512, 400 + i
        return "%d %d %d %d %d %d %d %d %d %d %d %d %d %d" % (self.src_off, self.src_len, self.mid_off, self.mid_cap, self.dst_off, self.dst_cap,
                                                            self.limit, self.flags, self.expect, *self.inflate, *self.deflate)

    def expected(self, refused):
        """(verdict after open, inflate's descriptor, verdict after link, deflate's descriptor, result) by the header's words"""
        no_in, no_out = (self.src_off, 0, self.mid_off, 0, 0, 0, 0), (self.mid_off, 0, self.dst_off, 0, 0, 0, 0)
        if self.flags & ~(HAS_LIMIT | EXPECT_CRC32) or self.mid_cap > MAX_MID:
            return (18, 0, 0, 0), no_in, (18, 0, 0, 0), no_out, (18, 0, 0, 0, 0, 0)
        inflate_desc = (self.src_off, self.src_len, self.mid_off, self.mid_cap, self.limit, self.flags & HAS_LIMIT, 0)
        st, crc, mid_len = self.inflate
        if st != 0:
            return (0, 0, 0, 0), inflate_desc, (st, 1, 0, 0), no_out, (st, 0, 0, 0, 1, 0)
        if self.flags & EXPECT_CRC32 and crc != self.expect:
            return (0, 0, 0, 0), inflate_desc, (6, 2, crc, mid_len), no_out, (6, crc, 0, mid_len, 2, 0)
        deflate_desc = (self.mid_off, mid_len, self.dst_off, self.dst_cap, 0, 0, 0)
        dst, out_len = (18, 0) if refused else self.deflate
        result = (0, crc, out_len, mid_len, 0, 0) if dst == 0 else (dst, crc, 0, mid_len, 3, 0)
        return (0, 0, 0, 0), inflate_desc, (0, 0, crc, mid_len), deflate_desc, result


def table():
    rows = []
    for flags in range(4):  # every combination of the two flags anybody knows
        rows.append(Row("flags%d_ok" % flags, flags=flags, expect=0xC0FFEE, limit=300 if flags & HAS_LIMIT else 0))
    for bit in (2, 3, 7, 31):  # ... and a stray one beside each
        for flags in range(4):
            rows.append(Row("stray_bit%d_flags%d" % (bit, flags), flags=flags | 1 << bit, expect=0xC0FFEE))
    rows.append(Row("mid_cap_at_max", mid_cap=MAX_MID))
    rows.append(Row("mid_cap_over_max", mid_cap=MAX_MID + 1))
    rows.append(Row("mid_cap_over_max_and_stray_bit", mid_cap=MAX_MID + 1, flags=4))
    for st in (1, 2, 16, 17, 18):  # what inflate and its CRC-32 pass can say (a length that leaked into a failed result is dropped)
        rows.append(Row("inflate_status%d" % st, flags=3, expect=5, inflate=(st, 9, 33)))
        rows.append(Row("inflate_status%d_no_expect" % st, inflate=(st, 0, 0)))
    rows.append(Row("crc_equal_expected", flags=EXPECT_CRC32, expect=0xDEADBEEF, inflate=(0, 0xDEADBEEF, 450)))
    rows.append(Row("crc_differs_expected", flags=EXPECT_CRC32, expect=0xDEADBEEF, inflate=(0, 0xDEADBEEE, 450)))
    rows.append(Row("crc_differs_expected_with_limit", flags=3, expect=1, limit=450, inflate=(0, 0, 450)))
    rows.append(Row("crc_differs_not_expected", flags=0, expect=0xDEADBEEF, inflate=(0, 0xDEADBEEE, 450)))
    rows.append(Row("crc_zero_equal", flags=EXPECT_CRC32, expect=0, inflate=(0, 0, 0), deflate=(0, 2)))
    rows.append(Row("deflate_dst_too_small", flags=3, expect=0xC0FFEE, limit=300, deflate=(16, 0)))
    rows.append(Row("deflate_dst_too_small_no_flags", deflate=(16, 0)))
    rows.append(Row("empty_ok", inflate=(0, 0, 0), deflate=(0, 2)))
    rows.append(Row("ok", flags=3, expect=0xC0FFEE, limit=300))
    return rows


def run(exe, rows, refused):
    text = "%d %d %d\n" % (len(rows), MAX_MID, int(refused)) + "\n".join(r.line(i) for i, r in enumerate(rows)) + "\n"
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-2000:])
    out = []
    for line in p.stdout.splitlines():
        parts = [tuple(int(x) for x in f.split()) for f in line.split("|")]
        out.append(parts)
    assert [p[0] for p in out] == [(i,) for i in range(len(rows))]
    return out


@pytest.mark.parametrize("refused", [False, True], ids=["deflate_runs", "deflate_refuses_the_batch"])
def test_every_row_of_the_rule_table(sims, refused):
    rows = table()
    got = run(sims[0], rows, refused)
    seen = set()
    for r, g in zip(rows, got):
        opened, inflate_desc, linked, deflate_desc, result = r.expected(refused)
        assert g[1] == opened, (r.name, "open", g[1], opened)
        assert g[2] == inflate_desc, (r.name, "inflate's descriptor", g[2], inflate_desc)
        assert g[3] == linked, (r.name, "link", g[3], linked)
        assert g[4] == deflate_desc, (r.name, "deflate's descriptor", g[4], deflate_desc)
        assert g[5] == result, (r.name, "result", g[5], result)
        assert g[6] == (result[0], result[1], result[2]), (r.name, "the pipeline's view of the result")
        seen.add((result[0], result[4]))
    want = {(18, 0), (1, 1), (2, 1), (16, 1), (17, 1), (18, 1), (6, 2), (18, 3)} if refused else \
        {(0, 0), (18, 0), (1, 1), (2, 1), (16, 1), (17, 1), (18, 1), (6, 2), (16, 3)}
    assert seen == want, seen  # (on the expectation's side: every status at every stage it can have is in the table)


def test_refused_streams_get_the_no_stream_descriptor(sims):
    """a stream that does not go on is handed to the codec as one with nothing to read and no room to write (src_len 0,
    dst_cap 0, flags 0, and no limit), at its own offsets: zlib.hip's zlib_no_stream"""
    rows = table()
    got = run(sims[0], rows, False)
    n_in = n_out = 0
    for r, g in zip(rows, got):
        result = g[5]
        if result[0] == 18 and result[4] == 0:
            assert g[2] == (r.src_off, 0, r.mid_off, 0, 0, 0, 0), r.name
            n_in += 1
        else:
            assert g[2][1] == r.src_len and g[2][3] == r.mid_cap, r.name
        if result[4] in (1, 2) or (result[0] == 18 and result[4] == 0):
            assert g[4] == (r.mid_off, 0, r.dst_off, 0, 0, 0, 0), r.name
            n_out += 1
        else:
            assert g[4][1] == result[3] and g[4][3] == r.dst_cap, r.name  # deflate reads as many bytes as inflate said it wrote
    assert (n_in, n_out) == (18, 18 + 10 + 2), (n_in, n_out)  # refused; ... and the ten that did not inflate, the two whose CRC-32 differs


def test_sanitized_build_says_the_same_and_nothing_else(sims):
    """the same program under -fsanitize=address,undefined, as a process of its own (no preload, nothing loaded here)"""
    rows = table()
    for refused in (False, True):
        assert run(sims[1], rows, refused) == run(sims[0], rows, refused)
    assert run(sims[1], [], False) == []
