"""CPU: the recurrence seam is declared - include/p3r.h carries p3r_affine_scan_info and p3r_affine_scan_dmat with their
argument lists, the struct p3r_recurrence and the flags; the built library exports both symbols; the ctypes bindings have
the declared arguments; the ABI version stays 8 and no P3R_AIR_* op is added; the host entry accepts a valid set, counts
it, and gives every refusal of the header's list with its message; include/p3r.hpp, the Python layer, the example and the
documents reach the entry."""
import ctypes as C
import os
import re

import pytest

from test_fri_seam_abi import arguments, header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P3R_EINVAL, P3R_EUNSUPPORTED = -1, -5
INFO, DMAT = "p3r_affine_scan_info", "p3r_affine_scan_dmat"
INFO_ARGS = ["const p3r_config* cfg", "const p3r_recurrence* recs", "size_t n_recs", "const size_t* widths", "size_t n_mats",
             "p3r_scan_info* out"]
DMAT_ARGS = ["p3r_ctx* ctx", "const p3r_recurrence* recs", "size_t n_recs", "const p3r_dmat* const* mats", "size_t n_mats",
             "p3r_dmat** out", "uint32_t* last_out"]
CASES = [("koala-bear", 4), ("koala-bear", 5), ("baby-bear", 4)]


def test_header_declares_both_entries_and_the_library_exports_them():
    from test_abi import header_symbols
    from plonky3_recursion_amd import _lib
    assert INFO in header_symbols() and DMAT in header_symbols()
    assert arguments(INFO) == INFO_ARGS and arguments(DMAT) == DMAT_ARGS
    src = header()
    assert int(re.search(r"#define\s+P3R_ABI_VERSION\s+(\d+)", src).group(1)) == 8 == _lib.P3R_ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"enum\s*\{\s*P3R_SCAN_EXT\s*=\s*1\s*,\s*P3R_SCAN_INCLUSIVE\s*=\s*2\s*\}", code)
    assert re.search(r"#define\s+P3R_SCAN_NONE\s+0xffffffffu", code)
    body = re.search(r"typedef struct p3r_recurrence \{(.*?)\} p3r_recurrence;", code, flags=re.S).group(1)
    assert [" ".join(f.split()) for f in body.split(";") if f.strip()] == [
        "uint32_t flags", "uint32_t mul_mat, mul_col", "uint32_t add_mat, add_col", "uint32_t out_col", "uint32_t init[5]"]
    assert re.search(r"typedef struct p3r_scan_info \{\s*uint32_t n_out_columns, n_products, n_sums, n_affine;\s*\} p3r_scan_info;", code)
    # the witness section still says what it said, and the new one says where such columns now go and what the caller writes
    for item in ("Out of scope: recurrences - a column that reads its own previous row - and prefix sums.",
                 "Such columns stay with the caller, or with the running sum of p3r_logup_program_dmat.",
                 "now go to\n * p3r_affine_scan_dmat", "is_first_row  * (s - init)", "is_transition * (s' - a * s - b)",
                 "is_last_row   * (a * s + b - T)", "resets the accumulator", "Nothing is inverted", "no error depends on the data",
                 "coupled or vector-state recurrences", "non-linear recurrences", "not powers of two", "only enqueues"):
        assert item in src, item
    assert src.index("p3r_witness_program_dmat(p3r_ctx*") < src.index("first-order affine recurrences") < src.index("batch-STARK proving (the chosen")
    lib = _lib.load()   # raises if a declared symbol is not exported
    assert getattr(lib, INFO) and getattr(lib, DMAT)


def test_no_air_op_is_added():
    from plonky3_recursion_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    ops = {name: int(value) for name, value in re.findall(r"\b(P3R_AIR_[A-Z0-9_]+)\s*=\s*(\d+)", code)}
    # the instruction ops 8 .. 26 of the three program seams, and the table kinds 0 .. 5 (CONST and PUBLIC are both): as before
    assert len(ops) == 25 and sorted(ops.values()) == list(range(6)) + list(range(8, 27))
    assert (ops["P3R_AIR_CHALLENGE"], ops["P3R_AIR_ASSERT_ZERO"], ops["P3R_AIR_LOOKUP_END"], ops["P3R_AIR_INV"], ops["P3R_AIR_STORE"]) == (8, 20, 22, 23, 26)
    assert all(getattr(_lib, name) == value for name, value in ops.items() if value >= 8)


def test_binding_table_carries_the_signatures():
    from plonky3_recursion_amd import _lib
    vp, u32p, rec = C.c_void_p, _lib.u32p, C.POINTER(_lib.P3rRecurrence)
    res, args = _lib.SIGNATURES[INFO]
    assert res is C.c_int and args == [C.POINTER(_lib.P3rConfig), rec, C.c_size_t, C.POINTER(C.c_size_t), C.c_size_t, C.POINTER(_lib.P3rScanInfo)]
    res, args = _lib.SIGNATURES[DMAT]
    assert res is C.c_int and len(args) == len(DMAT_ARGS)
    assert args == [vp, rec, C.c_size_t, C.POINTER(vp), C.c_size_t, C.POINTER(vp), u32p]
    assert [n for n, _ in _lib.P3rRecurrence._fields_] == ["flags", "mul_mat", "mul_col", "add_mat", "add_col", "out_col", "init"]
    assert C.sizeof(_lib.P3rRecurrence) == 44 and _lib.P3rRecurrence.init.offset == 24
    assert [n for n, _ in _lib.P3rScanInfo._fields_] == ["n_out_columns", "n_products", "n_sums", "n_affine"]
    assert (_lib.P3R_SCAN_EXT, _lib.P3R_SCAN_INCLUSIVE, _lib.P3R_SCAN_NONE) == (1, 2, 0xFFFFFFFF)


def valid_set(dc):
    """Matrix 0: three base columns; matrix 1: two flattened extension columns.  Interleaved outputs, every form."""
    return [dict(out_col=dc, add=(0, 0)),                                                  # base sum
            dict(out_col=0, mul=(1, 0), add=(1, dc), ext=True, init=[1, 2, 3, 4, 5][:dc]),  # extension affine
            dict(out_col=dc + 1, mul=(0, 1), init=1, inclusive=True),                       # base product
            dict(out_col=dc + 2, mul=(1, dc), ext=True, init=1),                            # extension product
            dict(out_col=2 * dc + 2, mul=(0, 2), add=(0, 0), init=7),                       # base affine
            dict(out_col=2 * dc + 3, add=(1, 0), ext=True, inclusive=True)]                 # extension sum


@pytest.mark.parametrize("field,dc", CASES)
def test_the_host_entry_counts_and_refuses(field, dc):
    import plonky3_recursion_amd as p3r
    from plonky3_recursion_amd import _lib
    cfg, keep = p3r.make_config(field=field, challenge_degree=dc)
    p = {"koala-bear": 0x7f000001, "baby-bear": 0x78000001}[field]
    widths = [3, 2 * dc]
    good = valid_set(dc)
    assert p3r.affine_scan_info(cfg, good, widths) == {"n_out_columns": 3 * dc + 3, "n_products": 2, "n_sums": 2, "n_affine": 2}
    assert p3r.affine_scan_info(cfg, [p3r.Recurrence(0, add=(0, 2), init=p - 1)], widths) == {
        "n_out_columns": 1, "n_products": 0, "n_sums": 1, "n_affine": 0}

    def but(i, **kw):
        return good[:i] + [dict(good[i], **kw)] + good[i + 1:]
    unknown_flag = p3r.Recurrence(0, add=(0, 0)).raw()
    unknown_flag.flags = 4
    padded = [1, 0, 0, 0, 0]
    padded[dc if dc < 5 else 4] = 1 if dc < 5 else p
    refusals = [
        ("n_recs == 0", [], widths),
        ("n_mats == 0", good, []),
        ("reads matrix 2 of 2", but(0, add=(2, 0)), widths),
        ("reads column 3 of matrix 0", but(0, add=(0, 3)), widths),
        ("+ DC of matrix 1", but(1, mul=(1, dc + 1)), widths),
        ("+ DC of matrix 0", but(3, mul=(0, 0)), widths),
        ("unknown flag bits 0x4", [unknown_flag], widths),
        ("non-canonical word 0 of init", but(4, init=p), widths),
        ("non-canonical word %d of init" % (dc - 1), but(1, init=[0] * (dc - 1) + [p]), widths),
        ("of init is not zero", but(4, init=[7, 1]), widths),
        ("of init is not zero" if dc < 5 else "non-canonical word 4 of init", but(1, init=padded), widths),
        ("recurrences 0 and 1 overlap at column %d" % (dc - 1), but(0, out_col=dc - 1), widths),
        ("recurrences 2 and 3 overlap at column %d" % (dc + 1), but(3, out_col=dc + 1), widths),
        ("output column %d, below W = %d, is written by no recurrence" % (3 * dc + 3, 3 * dc + 5), good + [dict(out_col=3 * dc + 4, add=(0, 0))], widths),
        ("output column 0, below W = 2, is written by no recurrence", [dict(out_col=1, add=(0, 0))], widths),
        ("neither mul nor add", but(2, mul=None), widths),
    ]
    for text, recs, ws in refusals:
        with pytest.raises(p3r.P3rError) as err:
            p3r.affine_scan_info(cfg, recs, ws)
        assert err.value.code == P3R_EINVAL and text in str(err.value), (text, str(err.value))
    assert "witness program" in str(err.value)   # where a constant column belongs
    # NULL arguments, through the entry itself
    lib = _lib.load()
    arr, n = p3r.device._recurrences(good)
    ws = (C.c_size_t * 2)(*widths)
    info = _lib.P3rScanInfo()
    for args, text in (((C.byref(cfg), None, n, ws, 2, C.byref(info)), "recs is NULL"),
                       ((C.byref(cfg), arr, n, None, 2, C.byref(info)), "widths is NULL"),
                       ((C.byref(cfg), arr, n, ws, 2, None), "NULL argument"),
                       ((None, arr, n, ws, 2, C.byref(info)), "NULL argument")):
        assert lib.p3r_affine_scan_info(*args) == P3R_EINVAL and text in lib.p3r_last_error(None).decode()
    assert lib.p3r_affine_scan_info(C.byref(cfg), arr, n, ws, 2, C.byref(info)) == 0 and info.n_out_columns == 3 * dc + 3


def test_mirrors_example_and_documents_reach_the_entry():
    import plonky3_recursion_amd as p3r
    from plonky3_recursion_amd import device
    assert callable(device.Context.affine_scan_device) and callable(device.affine_scan_info) and p3r.Recurrence is device.Recurrence
    raw = p3r.Recurrence(3, mul=(1, 2), init=[5, 6], ext=True, inclusive=True).raw()
    assert (raw.flags, raw.mul_mat, raw.mul_col, raw.add_mat, raw.out_col, list(raw.init)) == (3, 1, 2, 0xFFFFFFFF, 3, [5, 6, 0, 0, 0])
    hpp = open(os.path.join(ROOT, "include/p3r.hpp")).read()
    assert re.search(r"\baffine_scan\s*\(.*?%s\s*\(" % DMAT, hpp, flags=re.S)
    mk = open(os.path.join(ROOT, "examples/Makefile")).read()
    assert re.search(r"^all:.*\brunning_product\b", mk, flags=re.M)
    example = open(os.path.join(ROOT, "examples/running_product.cpp")).read()
    assert "p3r::affine_scan" in example and "p3r::witness_columns" in example and "p3r::check_constraints" in example
    assert "examples/running_product" in open(os.path.join(ROOT, ".gitignore")).read().split()
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert DMAT in open(os.path.join(ROOT, doc)).read(), doc
    tool = open(os.path.join(ROOT, "tools/time_affine_scan.py")).read()
    assert "affine_scan_device" in tool
    csrc = os.path.join(ROOT, "plonky3_recursion_amd", "csrc")
    assert "hip" not in re.sub(r"//.*", "", open(os.path.join(csrc, "scan_plan.h")).read()).lower()   # a pure host header
    assert '#include "kernels_scan.hip.h"' in open(os.path.join(csrc, "tu_air.hip")).read()
