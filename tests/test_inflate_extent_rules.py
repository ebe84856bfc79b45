"""The extent forms on the CPU (include/zipc_hip.h at zipc_hip_inflate_extent_batch): where a stream of unknown compressed
length ends.  The host model is tests/extent_sim/sim_extent.cpp -- inflate_lane.h's plain lane step run serially, the rule
of inflate_extent.h and zlib_container.h's zlib_close_extent over what it ends with.  What is expected comes from the
catalogue (tests/extent_cases.py): status, length and bytes from the oracle, the extent from two references that know
nothing of the project's decoder -- tests/token_ref.py's last block end and Python's zlib's unused_data.  This file holds

  - the two references against each other and against len(stream) on the whole catalogue, with the coverage the catalogue
    claims (every residue of end_bit mod 8, ends on 32-bit word boundaries) asserted;
  - the model in its four forms (raw / zlib x decode / size) at two budgets of turns against those expectations, and the
    invariant src_used <= src_len;
  - extent_with_crc as a table (a refusal of the CRC-32 pass is the stream's status);
  - EXTENT_MUTANTS, each built into a model of its own and run in a child process;
  - the model as a stand-alone program under the address sanitizer, every source a heap block of exactly src_len bytes;
  - the ABI: every new symbol exported, the C struct's layout equal to EXTENT_RESULT_DTYPE."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import extent_cases as EC
import mutation
import token_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SIM_CPP = os.path.join(HERE, "extent_sim", "sim_extent.cpp")
FORMS = {"raw": 0, "raw-size": 1, "zlib": 2, "zlib-size": 3}
BUDGETS = (512, 7)
GUARD, POISON = 64, 0xA5


def bind(so):
    L = C.CDLL(so)
    L.sim_extent.restype = None
    L.sim_extent.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, C.c_int,
                             C.POINTER(C.c_uint64)]
    L.sim_extent_bytes.restype = C.c_ulonglong
    L.sim_extent_bytes.argtypes = [C.c_ulonglong]
    L.sim_extent_with_crc.restype = None
    L.sim_extent_with_crc.argtypes = [C.c_uint, C.c_uint, C.c_ulonglong, C.c_ulonglong, C.c_uint, C.c_uint, C.POINTER(C.c_ulonglong)]
    L.sim_size_blocks_end_bit.restype = C.c_ulonglong
    L.sim_size_blocks_end_bit.argtypes = [C.c_uint, C.c_ulonglong, C.c_ulonglong]
    return L


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return bind(mutation.gxx(tmp_path_factory.mktemp("extent_sim") / "libextent_sim.so", [SIM_CPP], extra=["-Wall", "-Wno-unknown-pragmas"]))


def extent_by_tokens(src):
    """the first CPU reference: the serial decoder's end of the last block, in bytes"""
    return (token_ref.decode(src).blocks[-1].end_bit + 7) // 8


def run(sim, c, form, budget, adler):
    """the model over one case, its room between guard bytes -> ((status, checksum, out_len, src_used, reserved), the room's
    first out_len bytes, the guards untouched)"""
    size = form.endswith("size")
    cap = 0 if size else c.cap
    buf = (C.c_ubyte * (GUARD + cap + GUARD))()
    C.memset(buf, POISON, len(buf))
    out = (C.c_uint64 * 5)(*[0xEE] * 5)
    sim.sim_extent(c.src, len(c.src), None if size else C.byref(buf, GUARD), cap, int(c.limit is not None), c.limit or 0, c.flags, FORMS[form],
                   adler, budget, out)
    got = np.frombuffer(buf, np.uint8)
    rec = tuple(int(x) for x in out)
    clean = bool((got[:GUARD] == POISON).all() and (got[GUARD + cap:] == POISON).all())
    return rec, got[GUARD:GUARD + min(rec[2], cap)].tobytes(), clean


def failures(sim, oracle, cases, forms, budgets=BUDGETS):
    """-> [(case, form, budget, what)]: every case of a form's kind against what the catalogue says of it"""
    bad = []
    for c in cases:
        for form in forms:
            if c.zlib != form.startswith("zlib"):
                continue
            size = form.endswith("size")
            st, ck, n, used, data = EC.want(oracle, c, size=size)
            # (a raw form's checksum is the crc_op's, which the model is handed: 0 here)
            want = (st, ck or 0, n, used, 0)
            for budget in budgets:
                # (the model is handed the Adler-32 of the body's bytes, which is the oracle's: `ck` of an OK stream and of a mismatch)
                rec, got, clean = run(sim, c, form, budget, (ck or 0) if c.zlib and not size else 0)
                what = []
                if rec != want:
                    what.append("%r, not %r" % (rec, want))
                elif got != data:
                    what.append("bytes")
                if not clean:
                    what.append("wrote outside its room")
                if rec[3] > len(c.src):
                    what.append("src_used beyond src_len")
                if what:
                    bad.append((c.name, form, budget, "; ".join(what)))
    return bad


# ---- the references and the catalogue -------------------------------------------------------------------------------

def test_the_two_references_agree_and_the_catalogue_covers_what_it_claims():
    residues, word_ends = {}, {"fixed": [], "dynamic": []}
    for s in EC.short_streams() + EC.span() + EC.long_streams()[:1]:
        ref = token_ref.decode(s.raw)
        end = ref.blocks[-1].end_bit
        assert ref.plain == s.plain, s.name
        if s.name.startswith("span/"):  # (one dynamic block each, the first with more than the span decoder's 1 KiB of input)
            assert [b.kind for b in ref.blocks] == [token_ref.DYNAMIC], s.name
        assert (end + 7) // 8 == len(s.raw) == EC.extent_by_zlib(s.raw), (s.name, end, len(s.raw))
        if s.name.startswith("basic/"):
            residues[end % 8] = residues.get(end % 8, 0) + 1
            if end % 32 == 0:
                word_ends["fixed" if "fixed" in s.name else "dynamic"].append((len(s.plain), end))
    assert EC.extent_by_zlib(EC.long_streams()[1].raw) == len(EC.long_streams()[1].raw)
    assert sorted(residues) == list(range(8)) and min(residues.values()) >= 20, residues
    assert word_ends["fixed"] and word_ends["dynamic"], word_ends
    # every OK case: both references, whatever trails the stream
    n_ok = 0
    for c in EC.raw_cases():
        u = EC.extent_by_zlib(c.src)
        if u is not None and not c.name.startswith("span/"):
            assert extent_by_tokens(c.src) == u <= len(c.src), c.name
            n_ok += 1
    for c in EC.zlib_cases():
        u = EC.extent_by_zlib(c.src, wrapped=True)
        if u is not None and "/span/" not in c.name:
            assert extent_by_tokens(c.src[2:len(c.src) - 2]) + 6 == u <= len(c.src), c.name
            n_ok += 1
    assert n_ok > 1500, n_ok
    lens = {len(c.src) - EC.extent_by_zlib(c.src) for c in EC.raw_cases() if c.name.startswith("hand/") and EC.extent_by_zlib(c.src)}
    assert lens == set(EC.TRAIL_LENS), lens


def test_the_catalogue_has_every_refusal_and_every_header_failure(oracle):
    got = {c.name: EC.want(oracle, c)[0] for c in EC.raw_cases() if c.name.startswith("refuse/")}
    assert got == {"refuse/btype3": 1, "refuse/far_distance": 1, "refuse/limit_exceeded": 2, "refuse/limit_exact": 0, "refuse/room_too_small": 16,
                   "refuse/empty_source": 1, "refuse/bad_flag": 18, "refuse/done_flag": 18}, got
    z = {c.name: EC.want(oracle, c)[0] for c in EC.zlib_cases() if c.name.count("/") == 1}
    assert z == {"zlib/wrong_adler": 6, "zlib/wrong_adler_right_one_at_the_end": 6, "zlib/trailer_cut1": 1, "zlib/trailer_cut2": 1,
                 "zlib/trailer_cut3": 1, "zlib/trailer_cut4": 1,  # (the body itself is cut there: the oracle's verdict of it)
                 "zlib/src_len0": 1, "zlib/src_len1": 1, "zlib/src_len2": 1, "zlib/src_len3": 1, "zlib/src_len4": 1, "zlib/src_len5": 1,
                 "zlib/header_fcheck": 1, "zlib/header_method": 3, "zlib/header_window": 4, "zlib/header_dict": 5, "zlib/limit_exceeded": 2,
                 "zlib/bad_flag": 18}, z
    # the stated Adler-32 of every wrapped body is the project's own value (the reference's flavour and RFC 1950's agree on them)
    import zlib
    for c in EC.zlib_cases():
        st, ck, n, used, data = EC.want(oracle, c)
        if st == 0:
            assert ck == zlib.adler32(data) and used <= len(c.src), c.name
    # src_len := src_used - 1: whatever the oracle says of the cut stream -- mostly corrupted, not always
    cut = [EC.want(oracle, c)[0] for c in EC.raw_cases() if c.name.endswith("/cut1")]
    assert len(cut) > 400 and set(cut) <= {0, 1} and cut.count(1) > 400, (len(cut), set(cut))


def test_extent_bytes_and_the_blocks_end_bit_as_tables(sim):
    for bit, want in ((0, 0), (1, 1), (7, 1), (8, 1), (9, 2), (10, 2), (16, 2), (224, 28), (225, 29), (448, 56), ((1 << 35) + 1, (1 << 32) + 1)):
        assert sim.sim_extent_bytes(bit) == want, bit
    assert sim.sim_size_blocks_end_bit(1, 100, 999) == 100 and sim.sim_size_blocks_end_bit(0, 100, 999) == 999


# extent_with_crc (the decode form with CRC-32, behind the checksum pass): name -> ((the kernel's record), the pass's status
# and CRC-32, the record that must come of them).  zipc_hip_inflate_batch refuses a stream whose output is longer than the
# call's max_dst_cap with INVALID_ARG when a CRC-32 is asked for; the extent form must, and a refusal has no extent.
CRC_TABLE = {
    "crc/ok": ((0, 0, 500, 123), 0, 0xCAFEF00D, (0, 0xCAFEF00D, 500, 123, 0)),
    "crc/ok_empty": ((0, 0, 0, 2), 0, 0, (0, 0, 0, 2, 0)),
    "crc/longer_than_max_dst_cap": ((0, 0, 70000, 123), 18, 0, (18, 0, 0, 0, 0)),
    "crc/stream_refused": ((1, 0, 0, 0), 1, 0, (1, 0, 0, 0, 0)),
    "crc/stream_refused_pass_untouched": ((16, 0, 0, 0), 16, 0xEEEEEEEE, (16, 0, 0, 0, 0)),
}


def crc_table_failures(sim, names=None):
    bad = []
    for name, (rec, pass_status, crc, want) in CRC_TABLE.items():
        out = (C.c_ulonglong * 5)(*[0xEE] * 5)
        sim.sim_extent_with_crc(rec[0], rec[1], rec[2], rec[3], pass_status, crc, out)
        if tuple(int(x) for x in out) != want and (names is None or name in names):
            bad.append((name, "table", 0, "%r, not %r" % (tuple(int(x) for x in out), want)))
    return bad


def test_the_checksum_pass_refusal_is_the_streams_status(sim):
    assert not crc_table_failures(sim)


# ---- the model ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", sorted(FORMS))
def test_the_model_gives_what_the_references_say(sim, oracle, form):
    cases = EC.zlib_cases() if form.startswith("zlib") else EC.raw_cases()
    bad = failures(sim, oracle, cases, [form])
    assert not bad, (len(bad), bad[:5])


def test_back_to_back_streams_are_walked_by_the_recipe(sim, oracle):
    """bound, extent, next stream: each zlib stream is found from the one before's src_used"""
    arena, plains = EC.back_to_back()
    at, got = 0, []
    while at < len(arena):
        c = EC.Case("walk@%d" % at, arena[at:], 1 << 17, None, 0, True)
        data = oracle.zlib_decompress(arena[at:at + EC.extent_by_zlib(arena[at:], wrapped=True)])[1]
        rec, out, clean = run(sim, c, "zlib", 512, oracle.adler32(data))
        assert rec[0] == 0 and rec[3] > 0 and clean, (at, rec)
        got.append(out)
        at += rec[3]
    assert got == plains and at == len(arena)


# ---- the mutants ----------------------------------------------------------------------------------------------------
# (name, file, text, replacement, (form, the case that must fail)): one-line mutants of inflate_extent.h, of zlib_container.h's
# close rule and of the two places of inflate_lane.h the extent rests on.  Host-model mutants: built with g++ and run in
# child processes, never built into a GPU library.
EXTENT_MUTANTS = [
    ("extent_rounds_down", "inflate_extent.h", "return (end_bit + 7u) / 8u; }", "return end_bit / 8u; }", ("raw", "hand/empty_fixed/exact")),
    ("extent_one_byte_more", "inflate_extent.h", "return (end_bit + 7u) / 8u; }", "return (end_bit + 8u) / 8u; }", ("raw", "hand/stored_len1/ff5")),
    ("extent_kept_on_an_error", "inflate_extent.h", "r.status = status; r.checksum = 0; r.out_len = 0; r.src_used = 0; r.reserved = 0;",
     "r.status = status; r.checksum = 0; r.out_len = 0; r.src_used = extent_bytes(end_bit); r.reserved = 0;", ("raw", "refuse/far_distance")),
    ("length_kept_on_an_error", "inflate_extent.h", "r.status = status; r.checksum = 0; r.out_len = 0; r.src_used = 0; r.reserved = 0;",
     "r.status = status; r.checksum = 0; r.out_len = out_len; r.src_used = 0; r.reserved = 0;", ("raw", "refuse/far_distance")),
    ("zlib_trailer_at_src_len_minus_4", "zlib_container.h", "zlib_expect(stream + 2u + u)", "zlib_expect(stream + src_len - 4u)",
     ("zlib", "zlib/hand/stored_len1/ff5")),
    ("zlib_trailer_at_src_len_minus_4_passes_a_wrong_one", "zlib_container.h", "zlib_expect(stream + 2u + u)", "zlib_expect(stream + src_len - 4u)",
     ("zlib", "zlib/wrong_adler_right_one_at_the_end")),
    ("zlib_used_without_the_trailer", "zlib_container.h", "inner.src_used = u + 6u;", "inner.src_used = u + 2u;", ("zlib", "zlib/hand/empty_fixed/exact")),
    ("zlib_trailer_bound_refuses_the_exact_fit", "zlib_container.h", "if (2u + u + 4u > src_len) return", "if (2u + u + 4u >= src_len) return",
     ("zlib", "zlib/hand/empty_fixed/exact")),
    ("zlib_trailer_bound_one_byte_late", "zlib_container.h", "if (2u + u + 4u > src_len) return", "if (2u + u + 3u > src_len) return",
     ("zlib-size", "zlib/trailer_cut1")),
    ("zlib_size_form_without_the_bound", "zlib_container.h", "if (2u + u + 4u > src_len) return", "if (compare && 2u + u + 4u > src_len) return",
     ("zlib-size", "zlib/trailer_cut2")),
    ("zlib_mismatch_keeps_its_extent", "zlib_container.h", "inner.status = ST_CHECKSUM; inner.out_len = 0; inner.src_used = 0;",
     "inner.status = ST_CHECKSUM; inner.out_len = 0;", ("zlib", "zlib/wrong_adler")),
    ("crc_pass_refusal_dropped", "inflate_extent.h", "  if (pass_status != ST_OK) return extent_result(pass_status, 0, 0, 0);\n", "",
     ("table", "crc/longer_than_max_dst_cap")),
    ("crc_pass_refusal_keeps_its_extent", "inflate_extent.h", "  if (pass_status != ST_OK) return extent_result(pass_status, 0, 0, 0);\n",
     "  if (pass_status != ST_OK) { r.status = pass_status; return r; }\n", ("table", "crc/longer_than_max_dst_cap")),
    ("stored_final_block_ends_in_front_of_its_data", "inflate_lane.h", "    const uint32_t next = pos + length;\n",
     "    const uint32_t next = d.final_block ? pos : pos + length;\n", ("raw", "hand/stored_len1/ff5")),
    ("word_carry_dropped_when_boff_wraps_to_0", "inflate_lane.h", "    in_word += p >> 5;\n", "    in_word += (p & 31u) ? p >> 5 : 0u;\n",
     ("raw", "basic/dynamic35/ff5")),
]

_CHILD = r"""
import json, os, sys
root, so, form, name = sys.argv[1:5]
sys.path.insert(0, os.path.join(root, "tests")); sys.path.insert(0, root)
import extent_cases as EC
import oracle
import test_inflate_extent_rules as T
oracle.lib()
bad = T.crc_table_failures(T.bind(so), [name]) if form == "table" else T.failures(T.bind(so), oracle, [EC.by_name(name)], [form])
print(json.dumps(sorted({b[0] for b in bad})))
"""


def mutant_model(m, into):
    """the model over a copy of zipc_amd/csrc with one text changed -> its shared library"""
    name, fname, old, new = m[:4]
    csrc, sim_dir = os.path.join(str(into), "zipc_amd", "csrc"), os.path.join(str(into), "tests", "extent_sim")
    shutil.copytree(os.path.join(ROOT, "zipc_amd", "csrc"), csrc, ignore=shutil.ignore_patterns("build", "*.hip"))
    os.makedirs(sim_dir)
    shutil.copy(SIM_CPP, sim_dir)
    path = os.path.join(csrc, fname)
    text = mutation.patched(open(path).read(), old, new, name)
    with open(path, "w") as f:
        f.write(text)
    return mutation.gxx(os.path.join(sim_dir, "libextent_sim.so"), [os.path.join(sim_dir, "sim_extent.cpp")], extra=["-Wno-unknown-pragmas"])


def test_a_word_boundary_end_is_among_the_killers():
    """the killer of the dropped word carry is a stream whose final block ends exactly on a 32-bit word boundary"""
    c = EC.by_name("basic/dynamic35/ff5")
    assert token_ref.decode(c.src).blocks[-1].end_bit % 32 == 0


def test_extent_mutants_are_killed(tmp_path, capsys):
    import concurrent.futures

    sos = mutation.build_all(lambda m: mutant_model(m, tmp_path / m[0]), EXTENT_MUTANTS)
    with concurrent.futures.ThreadPoolExecutor(max_workers=mutation.workers()) as ex:
        jobs = [ex.submit(mutation.run_child, _CHILD, ROOT, so, m[4][0], m[4][1]) for m, so in zip(EXTENT_MUTANTS, sos)]
        rows = []
        for m, job in zip(EXTENT_MUTANTS, jobs):
            rc, failed, err = job.result()
            crashed = rc != 0 or failed is None
            rows.append((m[0], m[4][1], crashed, mutation.verdict(m[4][1], failed or [], crashed), err[-300:] if crashed else ""))
    with capsys.disabled():
        print("\nextent mutants in the host model")
        for name, killer, crashed, ok, _ in rows:
            print("  %-52s %s%s %s" % (name, killer, " (child crashed)" if crashed else "", "" if ok else "-- NOT AS EXPECTED"))
    assert all(r[3] and not r[2] for r in rows), [r for r in rows if not r[3] or r[2]]


def test_the_unmutated_model_fails_none_of_the_killers(sim, oracle):
    for m in EXTENT_MUTANTS:
        if m[4][0] == "table":
            assert m[4][1] in CRC_TABLE and not crc_table_failures(sim, [m[4][1]]), m[0]
        else:
            assert not failures(sim, oracle, [EC.by_name(m[4][1])], [m[4][0]]), m[0]


# ---- the audit program ----------------------------------------------------------------------------------------------

def test_audit_program_under_the_address_sanitizer(tmp_path, oracle):
    """the model as a stand-alone program with its own main, built with -fsanitize=address,undefined and run as a process
    over the catalogue: every source a heap block of exactly src_len bytes and every room one of exactly dst_cap, so a load
    behind the declared source (the zlib trailer's among them) or a store behind the room trips the sanitizer; it aborts on
    any record that differs from what is expected"""
    rows = []
    for c in EC.raw_cases() + EC.zlib_cases():
        for form in ("zlib", "zlib-size") if c.zlib else ("raw", "raw-size"):
            size = form.endswith("size")
            st, ck, n, used, data = EC.want(oracle, c, size=size)
            adler = ck or 0
            rows.append(struct.pack("<10I", len(c.src), 0 if size else c.cap, int(c.limit is not None), c.limit or 0, c.flags, FORMS[form], adler,
                                    st, n, used) + c.src)
    path = tmp_path / "cases.bin"
    path.write_bytes(struct.pack("<I", len(rows)) + b"".join(rows))
    exe = str(tmp_path / "extent_audit")
    mutation.gxx(exe, [os.path.join(HERE, "extent_sim", "audit_main.cpp")], shared=False,
                 extra=["-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert b"nothing outside a source or a room" in r.stdout and ("%d cases" % len(rows)).encode() in r.stdout


# ---- the ABI --------------------------------------------------------------------------------------------------------

NEW_SYMBOLS = ("zipc_hip_inflate_extent_batch", "zipc_hip_zlib_decompress_extent_batch", "zipc_hip_inflate_size_extent_batch",
               "zipc_hip_zlib_size_extent_batch", "zipc_hip_inflate_size_extent_blocks_batch", "zipc_hip_zlib_size_extent_blocks_batch",
               "zipc_hip_inflate_extent", "zipc_hip_zlib_decompress_extent")


def test_every_new_symbol_is_exported_and_bound():
    from zipc_amd import _lib

    L = _lib.lib()
    bound = {s[0] for s in _lib.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert name in bound and getattr(L, name) is not None, name
    assert L.zipc_hip_abi_version() == 1


def test_the_result_record_is_the_dtype(tmp_path):
    from zipc_amd.batch import EXTENT_RESULT_DTYPE as D

    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "zipc_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(zipc_hip_extent_result), offsetof(zipc_hip_extent_result, status), offsetof(zipc_hip_extent_result, checksum), "
                   "offsetof(zipc_hip_extent_result, out_len), offsetof(zipc_hip_extent_result, src_used), "
                   "offsetof(zipc_hip_extent_result, reserved)); return 0; }\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    got = [int(x) for x in subprocess.run([exe], stdout=subprocess.PIPE, check=True).stdout.split()]
    assert got == [D.itemsize] + [D.fields[f][1] for f in ("status", "checksum", "out_len", "src_used", "reserved")] == [32, 0, 4, 8, 16, 24]
