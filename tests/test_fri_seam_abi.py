"""CPU: the public FRI seam is declared - include/p3r.h carries p3r_fri_reduce_dmat (ten arguments) and p3r_fri_fold_dmat
(six), the ctypes table binds both with the header's argument lists, the ABI version stays 8 (functions are only added),
and include/p3r.hpp and the Python layer reach both entries."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include/p3r.h")).read()


def arguments(name):
    """The argument list of the declaration `int <name>(...)` in include/p3r.h, comments removed."""
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, code, flags=re.S)
    assert m, f"{name} is not declared in include/p3r.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_both_entry_points():
    from test_abi import header_symbols   # the suite's one list of the header's symbols
    syms = header_symbols()
    assert "p3r_fri_reduce_dmat" in syms and "p3r_fri_fold_dmat" in syms
    assert arguments("p3r_fri_reduce_dmat") == [
        "p3r_ctx* ctx", "const p3r_dmat* const* mats", "size_t n_mats", "uint32_t shift", "const size_t* point_offsets",
        "const uint32_t* points", "const uint32_t* values", "const uint32_t* alpha", "p3r_dmat** outs", "size_t* n_outs"]
    assert arguments("p3r_fri_fold_dmat") == [
        "p3r_ctx* ctx", "const p3r_dmat* in", "uint32_t log_arity", "const uint32_t* beta", "const p3r_dmat* roll_in", "p3r_dmat** out"]
    src = header()
    assert int(re.search(r"#define\s+P3R_ABI_VERSION\s+(\d+)", src).group(1)) == 8
    # the Rust items the entries stand for are named next to them
    for item in ("TwoAdicFriPcs::open", "FriFoldingStrategy::fold_matrix", "TwoAdicFriFolding"):
        assert item in src, item


def test_binding_table_carries_both_signatures():
    from plonky3_recursion_amd import _lib
    vp, u32p, szp = C.c_void_p, _lib.u32p, C.POINTER(C.c_size_t)
    res, args = _lib.SIGNATURES["p3r_fri_reduce_dmat"]
    assert res is C.c_int
    assert args == [vp, C.POINTER(vp), C.c_size_t, C.c_uint32, szp, u32p, u32p, u32p, C.POINTER(vp), szp]
    res, args = _lib.SIGNATURES["p3r_fri_fold_dmat"]
    assert res is C.c_int
    assert args == [vp, vp, C.c_uint32, u32p, vp, C.POINTER(vp)]
    assert _lib.P3R_ABI_VERSION == 8


def test_wrappers_reach_both_entries():
    from plonky3_recursion_amd import device
    assert callable(device.Context.fri_reduce_device) and callable(device.Context.fri_fold_device)
    hpp = open(os.path.join(ROOT, "include/p3r.hpp")).read()
    assert re.search(r"\breduced_openings\s*\(.*?p3r_fri_reduce_dmat\s*\(", hpp, flags=re.S)
    assert re.search(r"class\s+TwoAdicFriFolding\b.*?\bfold_matrix\s*\(.*?p3r_fri_fold_dmat\s*\(", hpp, flags=re.S)
    # the compiled caller of tests/test_gpu_fri_seam_cpp.py is one of the examples the build makes
    mk = open(os.path.join(ROOT, "examples/Makefile")).read()
    assert re.search(r"^all:.*\bfri_seam\b", mk, flags=re.M) and os.path.exists(os.path.join(ROOT, "examples/fri_seam.cpp"))


def test_the_unit_is_built_into_both_libraries():
    import __graft_entry__ as g
    assert "tu_fri.hip" in g.HIP_SOURCES and os.path.exists(os.path.join(g.CSRC, "tu_fri.hip"))
