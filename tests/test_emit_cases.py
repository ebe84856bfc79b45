"""tests/emit_cases.py on the CPU: the walker against the oracle's own trace, and what the lists reach under the oracle."""
import pytest

import emit_cases as E


@pytest.mark.parametrize("level", E.LEVELS)
def test_walker_counts_what_the_oracle_traces(oracle, level):
    named = [("long_pairs", 60000, E.long_pairs_stream()), E.bench_shape()[0], E.bench_shape()[64]] + list(E.short_streams()[::97])
    for kind, ln, s in named:
        st, c, _, blocks = oracle.deflate_trace(s, level=level)
        walked = E.walk(c)
        assert st == 0 and [k for k, _ in walked] == [int(b.kind) for b in blocks], (kind, ln)
        assert [len(bits) + 1 for k, bits in walked if k] == [int(b.n_syms) for b in blocks if b.kind], (kind, ln)
        for (k, bits), b in zip(walked, blocks):  # type bits + header + symbols + end of block = the block's bits
            assert k == 0 or sum(bits) <= int(b.bit_end - b.bit_start) - 3 - 1, (kind, ln)


@pytest.mark.parametrize("level", E.LEVELS)
def test_lists_reach_the_edges_under_the_oracle(oracle, level):
    assert E.reaches_the_edges(oracle, E.short_streams(), level) == []
    by_count = E.streams_by_count(oracle)
    assert E.reaches_the_edges(oracle, by_count, level) == [] and len(by_count) + 139 <= 1024, len(by_count)
    st, c, _ = oracle.deflate(E.long_pairs_stream(), level=level)
    found = E.long_pairs(E.walk(c))
    assert {k & 1 for _, k in found} == {0, 1} and len(found) >= 8
    assert len(E.bench_shape()[0][2]) == 65536
    st, _, _, blocks = oracle.deflate_trace(E.bench_shape()[0][2], level=level)
    assert len(blocks) == 2 and 1 <= int(blocks[1].n_syms) - 1 <= 8, [int(b.n_syms) for b in blocks]
