"""CPU: the public DFT seam is declared - include/p3r.h carries p3r_dft / p3r_dft_batch_dmat and the four
P3R_DFT_* constants, the ctypes table binds both with the header's argument lists, and the ABI version stays where
tests/test_abi_mmcs_open.py pins it (functions are only added)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include/p3r.h")).read()


def test_header_declares_the_dft_entry_points_and_constants():
    src = header()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in (("p3r_dft", 8), ("p3r_dft_batch_dmat", 7)):
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, code, flags=re.S)
        assert m, f"{name} is not declared in include/p3r.h"
        assert len(m.group(1).split(",")) == nargs
    want = {"P3R_DFT_FORWARD": 0, "P3R_DFT_INVERSE": 1, "P3R_DFT_NATURAL": 0, "P3R_DFT_BITREV": 1}
    for name, value in want.items():
        m = re.search(r"#define\s+%s\s+(\d+)" % name, src)
        assert m and int(m.group(1)) == value, name
    assert int(re.search(r"#define\s+P3R_ABI_VERSION\s+(\d+)", src).group(1)) == 8
    # each derived method of the trait is named next to the entry points that replace it
    for item in ("dft_batch", "idft_batch", "coset_dft_batch", "coset_idft_batch", "dft_algebra_batch"):
        assert "TwoAdicSubgroupDft::" + item in src, item


def test_binding_table_carries_both_signatures():
    from plonky3_recursion_amd import _lib
    vp, u32p = C.c_void_p, _lib.u32p
    res, args = _lib.SIGNATURES["p3r_dft"]
    assert res is C.c_int
    assert args == [vp, u32p, C.c_size_t, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, u32p]
    res, args = _lib.SIGNATURES["p3r_dft_batch_dmat"]
    assert res is C.c_int
    assert args == [vp, C.POINTER(vp), C.c_size_t, C.c_uint32, u32p, C.c_uint32, C.POINTER(vp)]
    assert (_lib.P3R_DFT_FORWARD, _lib.P3R_DFT_INVERSE, _lib.P3R_DFT_NATURAL, _lib.P3R_DFT_BITREV) == (0, 1, 0, 1)


def test_wrappers_exist():
    from plonky3_recursion_amd import device
    assert callable(device.Context.dft_batch) and callable(device.Context.dft_batch_device)
