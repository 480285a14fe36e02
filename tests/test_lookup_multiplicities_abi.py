"""CPU: the multiplicity join is declared - include/p3r.h carries p3r_lookup_multiplicities_dmat with its argument list
and the rule on which challenges a caller passes; the built library exports the symbol; the ctypes binding has the
declared number of arguments; the ABI version stays 8 (functions are only added, no op is); include/p3r.hpp, the Python
layer, the example and INTEGRATION.md reach the entry."""
import ctypes as C
import os
import re

from test_fri_seam_abi import arguments, header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "p3r_lookup_multiplicities_dmat"
ARGS = ["p3r_ctx* ctx", "const p3r_lookup_instance* table", "const p3r_lookup_instance* queries", "size_t n_queries",
        "const uint32_t* challenges", "size_t n_challenges", "p3r_dmat** out", "p3r_lookup_imbalance* missing", "size_t cap",
        "uint64_t* n_missing_out"]


def test_header_declares_the_entry_and_the_library_exports_it():
    from test_abi import header_symbols
    from plonky3_recursion_amd import _lib
    assert NAME in header_symbols()
    assert arguments(NAME) == ARGS
    src = header()
    assert int(re.search(r"#define\s+P3R_ABI_VERSION\s+(\d+)", src).group(1)) == 8 == _lib.P3R_ABI_VERSION
    # the one thing a caller must know, and the bound on a false join as a formula
    for item in ("CALLER'S OWN", "1, X, .., X^(DC-1)", "c - v", "(k - 1) / p^DC", "enable flag", "first offering"):
        assert item in src, item
    lib = _lib.load()   # raises if a declared symbol is not exported
    assert getattr(lib, NAME)


def test_binding_table_carries_the_signature():
    from plonky3_recursion_amd import _lib
    vp, u32p, inst = C.c_void_p, _lib.u32p, C.POINTER(_lib.P3rLookupInstance)
    res, args = _lib.SIGNATURES[NAME]
    assert res is C.c_int and len(args) == len(ARGS)
    assert args == [vp, inst, inst, C.c_size_t, u32p, C.c_size_t, C.POINTER(vp), C.POINTER(_lib.P3rLookupImbalance), C.c_size_t,
                    C.POINTER(C.c_uint64)]


def test_no_op_was_added():
    from plonky3_recursion_amd import _lib
    body = re.search(r"enum \{\s*P3R_AIR_CHALLENGE = 8,(.*?)\};", header(), flags=re.S).group(1)   # the ops of a program
    ops = [int(v) for v in re.findall(r"\bP3R_AIR_[A-Z_]+\s*=\s*(\d+)", body)]
    assert max(ops) == 22 == _lib.P3R_AIR_LOOKUP_END


def test_mirrors_example_and_documents_reach_the_entry():
    from plonky3_recursion_amd import device
    assert callable(device.Context.lookup_multiplicities_device)
    hpp = open(os.path.join(ROOT, "include/p3r.hpp")).read()
    assert re.search(r"\blookup_multiplicities\s*\(.*?%s\s*\(" % NAME, hpp, flags=re.S)
    mk = open(os.path.join(ROOT, "examples/Makefile")).read()
    assert re.search(r"^all:.*\blookup_table\b", mk, flags=re.M)
    example = open(os.path.join(ROOT, "examples/lookup_table.cpp")).read()
    assert "p3r::lookup_multiplicities" in example and "p3r::check_lookups" in example
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert NAME in guide and "3b" in guide and "p^DC" in guide
    for doc in ("README.md", "DESIGN.md"):
        assert NAME in open(os.path.join(ROOT, doc)).read(), doc
