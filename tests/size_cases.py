"""What the sizing tests (tests/test_inflate_size_sim.py, tests/test_gpu_inflate_size.py) expect, from the ORACLE and from
the rule cases as built: made once per process, shared, never changed.  Nothing here calls the code under test."""
import collections
import functools
import os
import sys

import util

sys.path.insert(0, util.GOLDEN)
import inflate_rules  # noqa: E402

# a stream to size with its ?decompressed_size or None, and the (status, out_len) the call is to report
Sized = collections.namedtuple("Sized", "name stream limit want")
# the cases that prove the distance check at the TRUE output position, and the limit
REQUIRED_NAMES = ("dist_eq_out/a", "dist_out_plus1/a", "dist_eq_out/c", "dist_out_plus1/c", "dist_32768_at_32767/a",
                  "dist_32768_at_32768/a", "dist_32768_at_32768/e", "limit_exact/a", "limit_one_short/a",
                  "limit_one_short_literal/c", "fixed_limit_exact/a", "fixed_limit_one_short/a", "far_match_over_limit/a",
                  "limit_exact_stored/a", "limit_one_short_stored/a", "corrupt_before_limit/a", "corrupt_after_limit/a")


@functools.lru_cache(maxsize=None)
def rule_cases():
    """all 486 cases of tests/golden/inflate_rules.wrapped_cases(), each with its own limit or none.  The oracle is held
    to every case first (as tests/test_gpu_inflate_rules.py _check does); what a sizing call is to say of it is the
    case's status and, when accepted, the length of its bytes as built."""
    import oracle

    out = []
    for name, c in inflate_rules.wrapped_cases().items():
        assert oracle.inflate(c.stream, decompressed_size=c.limit)[0] == c.status, (name, "the oracle left its case")
        out.append(Sized(name, c.stream, c.limit, (c.status, len(c.plain) if c.status == 0 else 0)))
    assert len(out) == 486 and all(n in {s.name for s in out} for n in REQUIRED_NAMES)
    return tuple(out)


def short_rule_cases():
    return tuple(s for s in rule_cases() if not s.name.endswith("/e"))


def long_rule_cases():
    return tuple(s for s in rule_cases() if s.name.endswith("/e"))


def expect_zlib_size(case):
    """What zipc_hip_zlib_size_batch is to say of a zlib_cases.Case, from the oracle: zlib_decompress's status where it
    is not 6, with the true length when OK; where the oracle says 6 (checksum mismatch) the stream is sized OK -- there
    are no bytes to take an Adler-32 of -- with the length of the oracle's inflate over the body range [2, len - 2).
    A descriptor with a stray flag bit is INVALID_ARG (the reference has no word for that)."""
    import oracle

    if case.flags:
        return 18, 0
    st, out, _, _, _ = oracle.zlib_decompress(case.stream, decompressed_size=case.limit)
    if st == 6:
        st_b, body, _ = oracle.inflate(case.stream[2:len(case.stream) - 2], decompressed_size=case.limit)
        assert st_b == 0
        return 0, len(body)
    return st, len(out) if st == 0 else 0


@functools.lru_cache(maxsize=None)
def zlib_expectations():
    """[(zlib_cases.Case, (status, out_len), the oracle's zlib_decompress status)]"""
    import oracle
    import zlib_cases

    out = []
    for c in zlib_cases.decompress_cases():
        st0 = 18 if c.flags else oracle.zlib_decompress(c.stream, decompressed_size=c.limit)[0]
        out.append((c, expect_zlib_size(c), st0))
    seen = {st0 for _, _, st0 in out}
    assert seen >= {0, 1, 2, 3, 4, 5, 6, 18}, seen  # (on the oracle's side: a checksum mismatch is among them)
    return tuple(out)
