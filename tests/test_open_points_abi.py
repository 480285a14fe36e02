"""CPU: the value half of Pcs::open is declared - include/p3r.h carries p3r_open_points / p3r_open_points_dmat with
nine arguments each and P3R_OPEN_POINTS_PER_PASS, the ctypes table binds both with the header's argument lists and the
same constant, and the ABI version stays 8 (functions are only added)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include/p3r.h")).read()


def arity(name):
    """Number of arguments of the declaration `int <name>(...)` in include/p3r.h, comments removed."""
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, code, flags=re.S)
    assert m, f"{name} is not declared in include/p3r.h"
    return len(m.group(1).split(","))


def test_header_declares_both_entry_points_and_the_cap():
    from test_abi import header_symbols   # the suite's one list of the header's symbols
    syms = header_symbols()
    for name in ("p3r_open_points", "p3r_open_points_dmat"):
        assert name in syms
        assert arity(name) == 9
    src = header()
    assert int(re.search(r"#define\s+P3R_ABI_VERSION\s+(\d+)", src).group(1)) == 8
    assert re.search(r"#define\s+P3R_OPEN_POINTS_PER_PASS\s+(\d+)", src)
    # the Rust items the entries stand for are named next to them
    for item in ("TwoAdicFriPcs::open", "interpolate_coset", "Pcs::open"):
        assert item in src, item


def test_binding_table_carries_both_signatures_and_the_same_cap():
    from plonky3_recursion_amd import _lib
    vp, u32p, szp = C.c_void_p, _lib.u32p, C.POINTER(C.c_size_t)
    res, args = _lib.SIGNATURES["p3r_open_points_dmat"]
    assert res is C.c_int
    assert args == [vp, C.POINTER(vp), C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, szp, u32p, u32p]
    res, args = _lib.SIGNATURES["p3r_open_points"]
    assert res is C.c_int
    assert args == [vp, C.POINTER(_lib.P3rMatrix), C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, szp, u32p, u32p]
    cap = int(re.search(r"#define\s+P3R_OPEN_POINTS_PER_PASS\s+(\d+)", header()).group(1))
    assert _lib.P3R_OPEN_POINTS_PER_PASS == cap >= 2
    assert _lib.P3R_ABI_VERSION == 8


def test_wrappers_exist():
    from plonky3_recursion_amd import device
    assert callable(device.Context.open_points) and callable(device.Context.open_points_device)
    hpp = open(os.path.join(ROOT, "include/p3r.hpp")).read()
    # a member named open_points that goes through the C entry (the compiled caller of tests/test_gpu_open_points_cpp.py
    # runs it; here only that it is declared)
    assert re.search(r"class\s+CosetInterpolation\b.*?\bopen_points\s*\(.*?p3r_open_points_dmat\s*\(", hpp, flags=re.S)
