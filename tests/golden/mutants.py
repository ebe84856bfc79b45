"""The mutation table of the two readings of the reference's encoder.

tests/golden/deflate_vectors.json holds what tests/golden/zd_second_reading.py makes of a list of named inputs, and
tests/test_oracle_pins.py holds oracle/zd_oracle.c to it.  That only means something if the vectors tell the
reference's rules from their "obvious" versions.  Each entry below is one such version, a one-line semantic mutant,
written twice: as a text patch of oracle/zd_oracle.c and as the same change to zd_second_reading.py.  With the vector
that is expected to kill it.  tests/test_mutants.py builds every oracle mutant with gcc and runs it over every
committed vector, and runs each second-reading mutant on its named killer: a mutant that changes no vector is a rule
the vectors do not pin.

Every patch must match its file exactly once, so that a refactor of either reading cannot quietly turn a mutant into
a no-op (the test fails instead).  Both readings are patched as text, in copies: the committed files are never touched.

`hclen`: a floor under HCLEN of 4 code-length codes (or of anything up to 12 codes) is an equivalent mutant.  The
distance code always has a code of length <= 4 (at most 30 symbols in a complete code, or the one length-1 code of the
empty-distance patch), so the last non-zero code-length code sits at index >= 11 of the order (zd.ml:312) and HCLEN is
never below 8.  The mutant here is the other way to get the trim wrong: all 19 lengths sent, HCLEN always 15.
"""
import collections
import os
import subprocess
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
from mutation import patched  # noqa: E402  (the exactly-once rule, tests/mutation.py)
ORACLE_C = os.path.join(ROOT, "oracle", "zd_oracle.c")
ORACLE_H = os.path.join(ROOT, "oracle", "zd_oracle.h")
SECOND_READING = os.path.join(HERE, "zd_second_reading.py")
# oracle/Makefile's CFLAGS
CFLAGS = ["-O2", "-g", "-std=c11", "-Wall", "-Wextra", "-fPIC", "-shared"]

Mutant = collections.namedtuple("Mutant", "name ref what c py killer")

MUTANTS = [
    Mutant("q1_codelen_counts_reset", "zd.ml:849-854", "the code-length symbol counts cleared with every block (Q1)",
           ("  memset(e->dist_sym_freqs, 0, sizeof e->dist_sym_freqs);\n}",
            "  memset(e->dist_sym_freqs, 0, sizeof e->dist_sym_freqs);\n"
            "  memset(e->codelen_sym_freqs, 0, sizeof e->codelen_sym_freqs);\n}"),
           ("    for i in range(len(e.dist_sym_freqs)):\n        e.dist_sym_freqs[i] = 0\n",
            "    for i in range(len(e.dist_sym_freqs)):\n        e.dist_sym_freqs[i] = 0\n"
            "    for i in range(len(e.codelen_sym_freqs)):\n        e.codelen_sym_freqs[i] = 0\n"),
           ("tie_fd_b2", "fast")),
    Mutant("q3_padding_mod_8", "zd.ml:1045-1047", "the stored estimate pads 0 bits, not 8, when the type bits end a byte (Q3)",
           ("int alignment_loss = 8 - ((e->dst_bits_len + 3) % 8);",
            "int alignment_loss = (8 - ((e->dst_bits_len + 3) % 8)) % 8;"),
           ("alignment_loss = 8 - ((e.dst_bits_len + 3) % 8)",
            "alignment_loss = (8 - ((e.dst_bits_len + 3) % 8)) % 8"),
           ("q3_b2_s6", "fast")),
    Mutant("chooser_stored_strict", "zd.ml:1102", "stored only when strictly shorter than both",
           ("if (nlen <= dlen && nlen <= flen) kind", "if (nlen < dlen && nlen < flen) kind"),
           ("if nlen <= dlen and nlen <= flen:", "if nlen < dlen and nlen < flen:"),
           ("tie_nf_b1", "default")),
    Mutant("chooser_fixed_strict", "zd.ml:1103", "fixed only when strictly shorter than dynamic",
           ("else if (flen <= dlen) kind", "else if (flen < dlen) kind"),
           ("elif flen <= dlen:", "elif flen < dlen:"),
           ("tie_fd_b1_s1062", "default")),
    Mutant("backref_k4_off", "zd.ml:1184-1187", "the chain never shortened to K/4 after a good match",
           ("  if (prev_match_len >= e->good_match) chain_steps = chain_steps / 4;\n", ""),
           ("chain_steps = e.max_chain_len // 4 if prev_match_len >= e.good_match else e.max_chain_len",
            "chain_steps = e.max_chain_len"),
           ("tie_fd_b1_s74", "fast")),
    Mutant("backref_farthest_on_tie", "zd.ml:1154-1174,1196-1199",
           "an equally long candidate further down the chain replaces the nearest",
           ("int len = find_match_length(e->src, i, pos, prev_match_len, max_match_len);",
            "int len = find_match_length(e->src, i, pos, prev_match_len - (match_pos != LZ77_NO_POS), max_match_len);"),
           ("        if s[i + prev_match_len] == s[pos + prev_match_len]:\n"
            "            ln = find_match_length(s, i, pos, prev_match_len, max_match_len)\n",
            "        q = prev_match_len - (match_pos != NO_POS)\n"
            "        if s[i + q] == s[pos + q]:\n"
            "            ln = find_match_length(s, i, pos, q, max_match_len)\n"),
           ("tie_fd_b1_s74", "default")),
    Mutant("window_ge", "zd.ml:1191", "a candidate exactly 32768 back is out of the window",
           ("pos - i > MAX_MATCH_DIST", "pos - i >= MAX_MATCH_DIST"),
           ("pos - i > MAX_DIST", "pos - i >= MAX_DIST"),
           ("far_match", "fast")),
    Mutant("rle_run_limit_7", "zd.ml:1015-1016", "a code-length run coded by 16 may repeat 7 times",
           ("int max = len_max < i + 6 ? len_max : i + 6;", "int max = len_max < i + 7 ? len_max : i + 7;"),
           ("mx = min(len_max, i + 6)", "mx = min(len_max, i + 7)"),
           ("palindrome", "fast")),
    Mutant("block_cut_65533", "zd.ml:747-750,1118-1123", "blocks cut at 65533 source bytes",
           ("MAX_BLOCK_SRC_LEN = 65534,", "MAX_BLOCK_SRC_LEN = 65533,"),
           ("MAX_BLOCK_SRC_LEN = 65534", "MAX_BLOCK_SRC_LEN = 65533"),
           ("rand70k", "none")),
    Mutant("hclen_no_trim", "zd.ml:1032-1036,1043", "all 19 code-length code lengths sent (HCLEN always 15)",
           ("while (o > 0 && SYM_CODE_LENGTH(", "while (o > 18 && SYM_CODE_LENGTH("),
           ("while o > 0 and (e.dyn_codelen", "while o > 18 and (e.dyn_codelen"),
           ("palindrome", "fast")),
    Mutant("no_empty_dist_patch", "zd.ml:974-979", "a block without matches gets no length-1 distance code",
           ("    e->dyn_dist.e[0] = SYM_INFO(0, 1);\n", ""),
           ("        e.dyn_dist[0] = (0 << 5) | 1\n", "        pass\n"),
           ("trip3", "default")),
    Mutant("len258_as_284", "zd.ml:260-267", "length 258 coded as symbol 284 with 5 extra bits, not as 285",
           ("if (len <= LENGTH_VALUE_MAX) length_value_to_sym[len] = 257 + i;",
            "if (len <= LENGTH_VALUE_MAX && !(len == 258 && i == 28)) length_value_to_sym[len] = 257 + i;"),
           ("LENGTH_VALUE_TO_SYM = _length_value_to_sym()\n",
            "LENGTH_VALUE_TO_SYM = _length_value_to_sym()\nLENGTH_VALUE_TO_SYM[258] = 284\n"),
           ("zeros5k", "fast")),
    Mutant("adler_unsigned_remainder", "zd.ml:196-197", "Adler-32 reduced by an unsigned remainder (Q6)",
           ("return (uint32_t)((int32_t)v % base);", "return v % (uint32_t)base;"),
           ("        s1 = i32_rem(s1, ADLER_BASE)\n        s2 = i32_rem(s2, ADLER_BASE)\n",
            "        s1 = (s1 & 0xFFFFFFFF) % ADLER_BASE\n        s2 = (s2 & 0xFFFFFFFF) % ADLER_BASE\n"),
           ("ff4200", "none")),
    Mutant("adler_once_per_stream", "zd.ml:1081-1086", "the fused Adler-32 updated once over the whole stream, not per block (Q7)",
           ("  e->crc = crc_op_update(e->crc_op, e->crc, e->src + e->block_src_start,\n"
            "                         (size_t)e->block_src_len);\n",
            "  if (e->block_src_start + e->block_src_len == e->src_len)\n"
            "    e->crc = crc_op_update(e->crc_op, e->crc, e->src, (size_t)e->src_len);\n"),
           ("        e.crc = adler_32_string_update(e.crc, e.src, e.block_src_start, e.block_src_len)\n",
            "        if e.block_src_start + e.block_src_len == e.src_len:\n"
            "            e.crc = adler_32_string_update(e.crc, e.src, 0, e.src_len)\n"),
           ("rand70k", "none")),
]


def build_oracle(m, out_dir, cc="gcc"):
    """oracle/zd_oracle.c with mutant `m` applied, built the way oracle/Makefile builds the oracle -> path of the .so"""
    return build_oracle_patched(m.name, [m.c], out_dir, cc)


def second_reading(m=None):
    """a fresh copy of zd_second_reading as a module, with mutant `m` applied to its text (None: unmutated)"""
    src = open(SECOND_READING).read()
    if m is not None:
        src = patched(src, m.py[0], m.py[1], "zd_second_reading.py " + m.name)
    mod = types.ModuleType("zd_second_reading_" + (m.name if m else "copy"))
    mod.__file__ = SECOND_READING
    exec(compile(src, SECOND_READING, "exec"), mod.__dict__)
    return mod


def second_reading_record(Z, data, level):
    """one "levels" entry of deflate_vectors.json as the reading `Z` makes it; the fused Adler-32 by the encoder's own
    per-block update (make_deflate_vectors.py replays it over the block cuts instead)"""
    sys.path.insert(0, HERE)
    import make_deflate_vectors

    return make_deflate_vectors.record(Z, data, level, adler_by_encoder=True)


# ---- inflate ------------------------------------------------------------------------------------------------------
# One-line mutants of the oracle's decoder, each a rule of zd.ml:355-391, 564-709 in its "obvious" other reading, and
# the case of tests/golden/inflate_rules.py that is expected to kill it ("name/wrapper").  `patches` are (old, new)
# text pairs of oracle/zd_oracle.c, each matching once.  A relaxed mutant (one that accepts more) clamps where the
# real decoder would have refused before indexing a table, so that it stays well-defined.
#
# `killer` None: an equivalent mutant, which no input can tell from the oracle -- the test requires it to change
# nothing, so that the claim is checked too.  empty_codelen_code_ok: with no code-length code every code-length
# symbol is undecodable, so read_symbol refuses the block at its first code-length symbol (hlit + hdist >= 258 of them
# follow), with the same status the missing check gives.
InflateMutant = collections.namedtuple("InflateMutant", "name ref what patches killer")

_RAISE = "ZD_RAISE(d->x, ZD_ERR_CORRUPTED);"
INFLATE_MUTANTS = [
    # -- what the deflate-side inputs and the header fuzz left standing
    InflateMutant("hlit_287_ok", "zd.ml:641", "HLIT 287 accepted",
                  [("if (hlit > MAX_LITLEN_SYM_COUNT ||", "if (hlit > MAX_LITLEN_SYM_COUNT + 1 ||")], "hlit_287/a"),
    InflateMutant("hdist_31_ok", "zd.ml:641", "HDIST 31 accepted",
                  [("|| hdist > MAX_DIST_SYM_COUNT)", "|| hdist > MAX_DIST_SYM_COUNT + 1)")], "hdist_31/a"),
    InflateMutant("cl16_first_ok", "zd.ml:653", "code-length symbol 16 accepted as the first item (it copies a 0)",
                  [("      if (num == 0) " + _RAISE + "\n      repeat = (int)read_int(d, 3, 2);\n      sym = lengths[num - 1];",
                    "      repeat = (int)read_int(d, 3, 2);\n      sym = num ? lengths[num - 1] : 0;")], "cl16_first/a"),
    InflateMutant("eob_length_zero_ok", "zd.ml:662", "lengths[256] == 0 accepted",
                  [("  if (lengths[256] == 0) " + _RAISE + "\n", "")], "lengths256_zero_over_limit/a"),
    InflateMutant("dist_out_plus_1_ok", "zd.ml:614", "a distance of out_len + 1 accepted (it copies zeros)",
                  [("    if (dist > (int64_t)d->dst.len) " + _RAISE + "\n",
                    "    if (dist > (int64_t)d->dst.len + 1) " + _RAISE + "\n"
                    "    if (dist > (int64_t)d->dst.len) { for (int64_t k = 0; k < length; k++) buf_add_uint8(&d->dst, 0); continue; }\n")],
                  "match_first/a"),
    InflateMutant("no_phantom", "zd.ml:389-390", "a single code's second code decodes the same symbol (no phantom)",
                  [("t->symbols[1] = t->max_sym + 1; }", "t->symbols[1] = t->max_sym; }")], "litlen_eob_only_phantom/a"),
    InflateMutant("phantom_is_0", "zd.ml:389-390", "the phantom symbol is 0",
                  [("t->symbols[1] = t->max_sym + 1; }", "t->symbols[1] = 0; }")], "litlen_eob_only_phantom/a"),
    InflateMutant("codelen_phantom_unchecked", "zd.ml:646", "the code-length symbol's sym > max_sym check removed",
                  [("    if (sym > huff->max_sym) " + _RAISE, "    if (sym > CODELEN_SYM_MAX) " + _RAISE)],
                  "codelen_single_phantom/a"),
    InflateMutant("empty_codelen_code_ok", "zd.ml:635", "an empty code-length code accepted",
                  [("  if (huff->max_sym == -1) " + _RAISE + "\n", "")], None),
    InflateMutant("fixed_litlen_286_ok", "zd.ml:603", "fixed litlen symbols 286/287 accepted (as 285)",
                  [("t->max_sym = LITLEN_SYM_MAX; /* 286 and 287 are unused */", "t->max_sym = LITLEN_SYM_FIXED_MAX;"),
                   ("if (sym > hlitlen->max_sym || sym > LITLEN_SYM_MAX ||", "if (sym > hlitlen->max_sym ||"),
                   ("length_value_of_sym_table[sym - LITLEN_FIRST_LEN_SYM]",
                    "length_value_of_sym_table[(sym > LITLEN_SYM_MAX ? LITLEN_SYM_MAX : sym) - LITLEN_FIRST_LEN_SYM]")],
                  "fixed_litlen_286/a"),
    InflateMutant("fixed_dist_30_ok", "zd.ml:608", "fixed distance symbols 30/31 accepted (as 0)",
                  [("t->max_sym = DIST_SYM_MAX; /* 30 and 31 are unused */", "t->max_sym = DIST_SYM_FIXED_MAX;"),
                   ("if (dsym > hdist->max_sym || dsym > DIST_SYM_MAX)", "if (dsym > hdist->max_sym)"),
                   ("dist_value_of_sym[dsym];", "dist_value_of_sym[dsym > DIST_SYM_MAX ? 0 : dsym];")],
                  "fixed_dist_30/a"),
    InflateMutant("btype3_as_fixed", "zd.ml:701", "BTYPE 3 decoded as a fixed block",
                  [("    case 1: read_fixed_block(d); break;", "    case 1: case 3: read_fixed_block(d); break;")],
                  "btype3_first/a"),
    InflateMutant("size_before_distance", "zd.ml:612-616", "the size limit tested before the distance check",
                  [("    if (dist > (int64_t)d->dst.len) ",
                    "    if (d->dst.fixed && d->dst.len + (size_t)length > d->dst.cap) ZD_RAISE(d->x, ZD_ERR_SIZE_EXCEEDED);\n"
                    "    if (dist > (int64_t)d->dst.len) ")], "far_match_over_limit/a"),
    InflateMutant("size_before_stored_input", "zd.ml:677", "the size limit tested before a stored block's input check",
                  [("  if (d->src_max - d->src_pos + 1 < length) ",
                    "  if (d->dst.fixed && d->dst.len + (size_t)length > d->dst.cap) ZD_RAISE(d->x, ZD_ERR_SIZE_EXCEEDED);\n"
                    "  if (d->src_max - d->src_pos + 1 < length) ")], "stored_short_of_input_and_limit/a"),
    # -- what the earlier inputs already killed
    InflateMutant("hlit_286_refused", "zd.ml:641", "HLIT 286 refused",
                  [("if (hlit > MAX_LITLEN_SYM_COUNT ||", "if (hlit >= MAX_LITLEN_SYM_COUNT ||")], "hlit_286/a"),
    InflateMutant("hdist_30_refused", "zd.ml:641", "HDIST 30 refused",
                  [("|| hdist > MAX_DIST_SYM_COUNT)", "|| hdist >= MAX_DIST_SYM_COUNT)")], "hdist_30/a"),
    InflateMutant("repeat_to_end_refused", "zd.ml:659", "a repeat that ends at hlit + hdist refused",
                  [("if (repeat > hlit + hdist - num)", "if (repeat >= hlit + hdist - num)")], "cl18_ends_at_hlit_hdist/a"),
    InflateMutant("repeat_one_past_ok", "zd.ml:659", "a repeat one past hlit + hdist accepted",
                  [("if (repeat > hlit + hdist - num)", "if (repeat > hlit + hdist - num + 1)")], "cl18_one_past/a"),
    InflateMutant("dist_eq_out_refused", "zd.ml:614", "a distance equal to the output so far refused",
                  [("if (dist > (int64_t)d->dst.len)", "if (dist >= (int64_t)d->dst.len)")], "dist_eq_out/a"),
    InflateMutant("stored_len_eq_input_refused", "zd.ml:677", "a stored LEN equal to the input left refused",
                  [("if (d->src_max - d->src_pos + 1 < length)", "if (d->src_max - d->src_pos + 1 <= length)")],
                  "stored_len_eq_input_left/a"),
    InflateMutant("stored_header_5", "zd.ml:672", "a stored header wants 5 bytes left, not 4",
                  [("if (d->src_max - d->src_pos + 1 < 4)", "if (d->src_max - d->src_pos + 1 < 5)")],
                  "stored_len_zero_final/a"),
    InflateMutant("single_code_refused", "zd.ml:377-378", "a single code refused",
                  [("(num_codes == 1 && counts[1] != 1)", "(num_codes == 1)")], "litlen_eob_only/a"),
    InflateMutant("single_code_any_length", "zd.ml:377-378", "a single code of any length accepted",
                  [("if ((num_codes > 1 && available > 0) || (num_codes == 1 && counts[1] != 1))",
                    "if (num_codes > 1 && available > 0)")], "litlen_single_len2/a"),
    InflateMutant("oversubscribed_ok", "zd.ml:370", "an over-subscribed code accepted",
                  [("    if (used > available) ZD_RAISE(x, ZD_ERR_CORRUPTED); /* over-subscribed */\n", "")],
                  "litlen_oversubscribed/a"),
    InflateMutant("incomplete_ok", "zd.ml:377", "an incomplete code of two or more codes accepted",
                  [("if ((num_codes > 1 && available > 0) || (num_codes == 1 && counts[1] != 1))",
                    "if (num_codes == 1 && counts[1] != 1)")], "litlen_incomplete/a"),
    InflateMutant("nlen_unchecked", "zd.ml:675", "a stored block's NLEN not checked",
                  [("if (length != ((~inv_length) & 0xFFFF))", "if (0 && length != ((~inv_length) & 0xFFFF))")],
                  "stored_nlen_byte2_bit0/a"),
    InflateMutant("litlen_285_refused", "zd.ml:603", "litlen symbol 285 refused",
                  [("|| sym > LITLEN_SYM_MAX ||", "|| sym >= LITLEN_SYM_MAX ||")], "fixed_litlen_285/a"),
    InflateMutant("dist_29_refused", "zd.ml:608", "distance symbol 29 refused",
                  [("|| dsym > DIST_SYM_MAX)", "|| dsym >= DIST_SYM_MAX)")], "fixed_dist_29/a"),
]


def build_oracle_patched(name, patches, out_dir, cc="gcc"):
    """oracle/zd_oracle.c with every (old, new) of `patches` applied, built as oracle/Makefile builds it -> the .so"""
    src = open(ORACLE_C).read()
    for old, new in patches:
        src = patched(src, old, new, "oracle/zd_oracle.c " + name)
    d = os.path.join(out_dir, name)
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "zd_oracle.c"), "w") as f:
        f.write(src)
    with open(os.path.join(d, "zd_oracle.h"), "w") as f:
        f.write(open(ORACLE_H).read())
    so = os.path.join(d, "libzd_oracle.so")
    subprocess.run([cc] + CFLAGS + ["-o", so, os.path.join(d, "zd_oracle.c")], check=True, capture_output=True)
    return so
