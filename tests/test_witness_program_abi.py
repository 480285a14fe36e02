"""CPU: the witness seam is declared - include/p3r.h carries p3r_witness_program_info and p3r_witness_program_dmat with
their argument lists and the four enumerators INV = 23, BITS = 24, ROW = 25, STORE = 26 in an enum of their own (the ops
of the older seams end at 22, as before); the built library exports both symbols; the ctypes bindings have the declared
arguments; the ABI version stays 8; the host entry validates and counts; every older host entry still takes the four ops
for unknown ops; include/p3r.hpp, the Python layer, the example and the documents reach the entry."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import witness_ref
from test_fri_seam_abi import arguments, header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P3R_EINVAL, P3R_EUNSUPPORTED = -1, -5
INFO, DMAT = "p3r_witness_program_info", "p3r_witness_program_dmat"
INFO_ARGS = ["const p3r_config* cfg", "const p3r_air_insn* prog", "size_t n_insns", "const size_t* widths", "size_t n_mats",
             "p3r_witness_info* out"]
DMAT_ARGS = ["p3r_ctx* ctx", "const p3r_air_insn* prog", "size_t n_insns", "const p3r_dmat* const* mats", "size_t n_mats", "size_t height",
             "const uint32_t* public_values", "size_t n_public", "const uint32_t* challenges", "size_t n_challenges", "p3r_dmat** out"]
OPS = {"P3R_AIR_INV": 23, "P3R_AIR_BITS": 24, "P3R_AIR_ROW": 25, "P3R_AIR_STORE": 26}


def test_header_declares_both_entries_and_the_library_exports_them():
    from test_abi import header_symbols
    from plonky3_recursion_amd import _lib
    assert INFO in header_symbols() and DMAT in header_symbols()
    assert arguments(INFO) == INFO_ARGS and arguments(DMAT) == DMAT_ARGS
    src = header()
    assert int(re.search(r"#define\s+P3R_ABI_VERSION\s+(\d+)", src).group(1)) == 8 == _lib.P3R_ABI_VERSION
    # what the section must state: the zero convention, the canonical word, and what is out of scope and where it stays
    for item in ("0 for 0", "CANONICAL word", "recurrences", "prefix sums", "stay with the caller", "running sum of p3r_logup_program_dmat",
                 "n_mats == 0 is legal", "only enqueues"):
        assert item in src, item
    lib = _lib.load()   # raises if a declared symbol is not exported
    assert getattr(lib, INFO) and getattr(lib, DMAT)


def test_the_four_enumerators_and_their_values():
    from plonky3_recursion_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name, value in OPS.items():
        assert int(re.search(r"\b%s\s*=\s*(\d+)" % name, code).group(1)) == value == getattr(_lib, name)
    # the ops of the older seams are as they were
    body = re.search(r"enum \{\s*P3R_AIR_CHALLENGE = 8,(.*?)\};", header(), flags=re.S).group(1)
    assert max(int(v) for v in re.findall(r"\bP3R_AIR_[A-Z_]+\s*=\s*(\d+)", body)) == 22
    assert (witness_ref.INV, witness_ref.BITS, witness_ref.ROW, witness_ref.STORE) == (23, 24, 25, 26)


def test_binding_table_carries_the_signatures():
    from plonky3_recursion_amd import _lib
    vp, u32p, insn = C.c_void_p, _lib.u32p, C.POINTER(_lib.P3rAirInsn)
    res, args = _lib.SIGNATURES[INFO]
    assert res is C.c_int and args == [C.POINTER(_lib.P3rConfig), insn, C.c_size_t, C.POINTER(C.c_size_t), C.c_size_t,
                                       C.POINTER(_lib.P3rWitnessInfo)]
    res, args = _lib.SIGNATURES[DMAT]
    assert res is C.c_int and len(args) == len(DMAT_ARGS)
    assert args == [vp, insn, C.c_size_t, C.POINTER(vp), C.c_size_t, C.c_size_t, u32p, C.c_size_t, u32p, C.c_size_t, C.POINTER(vp)]
    assert [n for n, _ in _lib.P3rWitnessInfo._fields_] == ["n_stores", "n_out_columns", "n_inversions", "peak_live"]


@pytest.mark.parametrize("field,dc", [("koala-bear", 4), ("koala-bear", 5), ("baby-bear", 4)])
def test_the_host_entry_counts_and_refuses(field, dc):
    import plonky3_recursion_amd as p3r
    cfg, keep = p3r.make_config(field=field, challenge_degree=dc)
    b = p3r.AirBuilder(field)
    x, c = b.local(0, 1), b.challenge(0)
    w = b.inv(x)
    b.store(b.bits(x, 8, 8), 0)
    b.store(b.inv(c * x), 1)
    b.store(1 - x * w, 1 + dc)
    b.store(b.row() + b.next(1, 0), 2 + dc)
    info = p3r.witness_program_info(cfg, b, [2, 1])
    want = witness_ref.info(field, dc, b.program(), [2, 1])
    assert want == {"n_stores": 4, "n_out_columns": 3 + dc, "n_inversions": 2}
    assert {k: info[k] for k in want} == want and 1 <= info["peak_live"] <= 6
    # a table of the row index needs no matrix
    t = p3r.AirBuilder(field)
    t.store(t.row(), 0)
    assert p3r.witness_program_info(cfg, t, []) == {"n_stores": 1, "n_out_columns": 1, "n_inversions": 0, "peak_live": 1}
    for text, prog in (("no STORE", [(witness_ref.ROW, 0, 0)]),
                       ("stored twice", [(witness_ref.ROW, 0, 0), (witness_ref.STORE, 0, 0), (witness_ref.STORE, 0, 0)]),
                       ("stored by no instruction", [(witness_ref.ROW, 0, 0), (witness_ref.STORE, 0, 1)]),
                       ("ASSERT_ZERO in a witness program", [(witness_ref.ROW, 0, 0), (witness_ref.STORE, 0, 0), (20, 0, 0)]),
                       ("BITS of an extension value", [(witness_ref.CHALLENGE, 0, 0), (witness_ref.BITS, 0, 8 << 8), (witness_ref.STORE, 1, 0)]),
                       ("unknown op 27", [(27, 0, 0)])):
        with pytest.raises(p3r.P3rError) as err:
            p3r.witness_program_info(cfg, np.array(prog, dtype=np.uint32), [])
        assert err.value.code == P3R_EINVAL and text in str(err.value), (text, str(err.value))


def test_the_older_host_entries_take_the_four_ops_for_unknown_ops():
    import plonky3_recursion_amd as p3r
    from plonky3_recursion_amd import _lib as L
    cfg, keep = p3r.make_config(field="koala-bear")
    for op in OPS.values():
        b = (8 << 8) if op == L.P3R_AIR_BITS else 0
        with pytest.raises(p3r.P3rError) as err:
            p3r.air_program_info(cfg, [(L.P3R_AIR_LOCAL, 0, 0), (op, 0, b), (L.P3R_AIR_ASSERT_ZERO, 0, 0)], [1])
        assert err.value.code == P3R_EINVAL and "unknown op %d" % op in str(err.value)
        with pytest.raises(p3r.P3rError) as err:
            p3r.lookup_program_info(cfg, [(L.P3R_AIR_LOCAL, 0, 0), (op, 0, b), (L.P3R_AIR_LOOKUP, 0, 0), (L.P3R_AIR_LOOKUP_END, 0, 0)], [1])
        assert err.value.code == P3R_EINVAL and "unknown op %d" % op in str(err.value)


def test_mirrors_example_and_documents_reach_the_entry():
    from plonky3_recursion_amd import device
    assert callable(device.Context.witness_device) and callable(device.witness_program_info)
    for method in ("inv", "bits", "row", "store"):
        assert callable(getattr(device.AirBuilder, method))
    hpp = open(os.path.join(ROOT, "include/p3r.hpp")).read()
    assert re.search(r"\bwitness_columns\s*\(.*?%s\s*\(" % DMAT, hpp, flags=re.S)
    for method in ("inv", "bits", "row", "store"):
        assert re.search(r"\b(Value|void) %s\(" % method, hpp), method
    mk = open(os.path.join(ROOT, "examples/Makefile")).read()
    assert re.search(r"^all:.*\bwitness_program\b", mk, flags=re.M)
    example = open(os.path.join(ROOT, "examples/witness_program.cpp")).read()
    assert "p3r::witness_columns" in example and "p3r::lookup_multiplicities" in example and "p3r::check_constraints" in example
    assert "examples/witness_program" in open(os.path.join(ROOT, ".gitignore")).read().split()
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert DMAT in open(os.path.join(ROOT, doc)).read(), doc
