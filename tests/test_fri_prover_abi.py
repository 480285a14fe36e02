"""CPU: the rest of prove_fri is declared at the seam - include/p3r.h carries the challenger entries,
p3r_fri_leaf_view_dmat, p3r_fri_final_poly_dmat and p3r_fri_log_arity, the ctypes table binds them with the header's
argument lists, the library exports them, and include/p3r.hpp and the Python layer reach them.  Functions are only
added, so the ABI version stays where the other ABI tests pin it.  p3r_fri_log_arity needs a context (the schedule is the
context's), so it is called in tests/test_gpu_prove_fri.py."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = {
    "p3r_challenger_create": ["p3r_ctx* ctx"],
    "p3r_challenger_clone": ["const p3r_challenger* ch"],
    "p3r_challenger_free": ["p3r_challenger* ch"],
    "p3r_challenger_observe": ["p3r_challenger* ch", "const uint32_t* words", "size_t n"],
    "p3r_challenger_sample": ["p3r_challenger* ch", "uint32_t* out", "size_t n"],
    "p3r_challenger_sample_ext": ["p3r_challenger* ch", "uint32_t* out"],
    "p3r_challenger_sample_bits": ["p3r_challenger* ch", "uint32_t bits", "uint32_t* out"],
    "p3r_challenger_check_witness": ["p3r_challenger* ch", "uint32_t bits", "uint32_t witness", "int* ok_out"],
    "p3r_challenger_grind": ["p3r_ctx* ctx", "p3r_challenger* ch", "uint32_t bits", "uint32_t* witness_out"],
    "p3r_fri_leaf_view_dmat": ["p3r_ctx* ctx", "const p3r_dmat* vec", "uint32_t log_arity", "p3r_dmat** out"],
    "p3r_fri_final_poly_dmat": ["p3r_ctx* ctx", "const p3r_dmat* vec", "uint32_t log_final_poly_len", "uint32_t* coeffs_out"],
    "p3r_fri_log_arity": ["const p3r_ctx* ctx", "size_t phase", "int log_cur", "int log_final", "int log_next_input"],
}


def header():
    return open(os.path.join(ROOT, "include/p3r.h")).read()


def arguments(name):
    """The argument list of the declaration of `name` in include/p3r.h, comments removed."""
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, code, flags=re.S)
    assert m, f"{name} is not declared in include/p3r.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(NEW))
def test_declared_bound_and_exported(name):
    from plonky3_recursion_amd import _lib
    from test_abi import header_symbols   # the suite's one list of the header's symbols
    assert name in header_symbols()
    assert arguments(name) == NEW[name]
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(NEW[name])
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    assert hasattr(C.CDLL(_lib.LIB_PATH), name), f"{name} declared in include/p3r.h but not exported"


def test_header_names_what_the_entries_stand_for():
    src = header()
    assert "typedef struct p3r_challenger p3r_challenger;" in src
    for item in ("DuplexChallenger<F, Perm16, 16, 8>", "ExtensionMmcs::commit_matrix", "check_witness", "prove_fri"):
        assert item in src, item
    # the paragraph that listed what a caller still owns of the PCS now says: nothing but its AIR
    assert "what a caller still owns of the PCS is the challenger" not in src
    assert re.search(r"a caller owns nothing of the PCS any more: what it brings is its AIR", src)
    # functions are only added: the version the other ABI tests pin
    from plonky3_recursion_amd import _lib
    assert int(re.search(r"#define\s+P3R_ABI_VERSION\s+(\d+)", src).group(1)) == _lib.P3R_ABI_VERSION


def test_binding_table_carries_the_signatures():
    from plonky3_recursion_amd import _lib
    vp, u32p = C.c_void_p, _lib.u32p
    assert _lib.SIGNATURES["p3r_challenger_create"] == (vp, [vp])
    assert _lib.SIGNATURES["p3r_challenger_clone"] == (vp, [vp])
    assert _lib.SIGNATURES["p3r_challenger_free"] == (None, [vp])
    assert _lib.SIGNATURES["p3r_challenger_observe"] == (C.c_int, [vp, u32p, C.c_size_t])
    assert _lib.SIGNATURES["p3r_challenger_grind"] == (C.c_int, [vp, vp, C.c_uint32, u32p])
    assert _lib.SIGNATURES["p3r_fri_leaf_view_dmat"] == (C.c_int, [vp, vp, C.c_uint32, C.POINTER(vp)])
    assert _lib.SIGNATURES["p3r_fri_final_poly_dmat"] == (C.c_int, [vp, vp, C.c_uint32, u32p])
    assert _lib.SIGNATURES["p3r_fri_log_arity"] == (C.c_int, [vp, C.c_size_t, C.c_int, C.c_int, C.c_int])


def test_calls_that_need_no_device():
    """A NULL handle is refused with a message before any context is touched; a NULL context has no schedule."""
    from plonky3_recursion_amd import _lib
    lib = _lib.load()
    assert lib.p3r_fri_log_arity(None, 0, 8, 3, -1) == -1
    assert lib.p3r_challenger_clone(None) is None
    assert b"NULL" in lib.p3r_last_error(None)
    w = C.c_uint32()
    assert lib.p3r_challenger_sample_bits(None, 3, C.byref(w)) == -1
    lib.p3r_challenger_free(None)


def test_mirrors_reach_the_entries():
    import plonky3_recursion_amd as p3r
    from plonky3_recursion_amd import device
    for attr in ("challenger", "fri_leaf_view_device", "fri_final_poly_device", "fri_log_arity", "prove_fri"):
        assert callable(getattr(device.Context, attr)), attr
    for attr in ("observe", "sample", "sample_ext", "sample_bits", "grind", "check_witness", "clone"):
        assert callable(getattr(p3r.Challenger, attr)), attr
    hpp = open(os.path.join(ROOT, "include/p3r.hpp")).read()
    assert re.search(r"class\s+DuplexChallenger\b.*?p3r_challenger_grind\s*\(", hpp, flags=re.S)
    assert re.search(r"class\s+TwoAdicFriFolding\b.*?\bleaf_view\s*\(.*?p3r_fri_leaf_view_dmat\s*\(", hpp, flags=re.S)
    assert re.search(r"inline\s+FriProof\s+prove_fri\s*\(.*?p3r_fri_final_poly_dmat\s*\(", hpp, flags=re.S)
    mk = open(os.path.join(ROOT, "examples/Makefile")).read()
    assert re.search(r"^all:.*\bprove_fri\b", mk, flags=re.M) and os.path.exists(os.path.join(ROOT, "examples/prove_fri.cpp"))
