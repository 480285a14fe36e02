"""CPU: the lookup-program seam is declared - include/p3r.h carries p3r_lookup_program_info and p3r_logup_program_dmat
with their argument lists, the two new op numbers and the p3r_lookup_info layout, the ctypes table binds both, the ABI
version stays 8 (functions are only added), and include/p3r.hpp, the Python layer and the examples reach the entries.
p3r_lookup_program_info needs no GPU: AirBuilder.lookup / end_lookup_column are checked through it, and
p3r_air_program_info still takes the two ops for unknown."""
import ctypes as C
import os
import re

import pytest

from test_fri_seam_abi import arguments, header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTXS = [("koala-bear", 4), ("koala-bear", 5), ("baby-bear", 4)]
P3R_EINVAL, P3R_EUNSUPPORTED = -1, -5


def test_header_declares_both_entry_points_and_the_library_exports_them():
    from test_abi import header_symbols
    from plonky3_recursion_amd import _lib
    syms = header_symbols()
    assert "p3r_lookup_program_info" in syms and "p3r_logup_program_dmat" in syms
    assert arguments("p3r_lookup_program_info") == [
        "const p3r_config* cfg", "const p3r_air_insn* prog", "size_t n_insns", "const size_t* widths", "size_t n_mats", "p3r_lookup_info* out"]
    assert arguments("p3r_logup_program_dmat") == [
        "p3r_ctx* ctx", "const p3r_air_insn* prog", "size_t n_insns", "const p3r_dmat* const* mats", "size_t n_mats",
        "const uint32_t* public_values", "size_t n_public", "const uint32_t* challenges", "size_t n_challenges", "p3r_dmat** out",
        "uint32_t* sum_out"]
    src = header()
    assert int(re.search(r"#define\s+P3R_ABI_VERSION\s+(\d+)", src).group(1)) == 8 == _lib.P3R_ABI_VERSION
    for item in ("p3_lookup", "LogUp", "batch_stark.rs:1086-1110", "zero denominator", "is_transition * (s' - s - sum_g f_g)"):
        assert item in src, item
    lib = _lib.load()   # raises if a declared symbol is not exported
    assert lib.p3r_lookup_program_info and lib.p3r_logup_program_dmat


def test_op_numbers_and_the_struct_layout_agree_with_the_header():
    from plonky3_recursion_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name, value in (("LOOKUP", 21), ("LOOKUP_END", 22)):
        m = re.search(r"\bP3R_AIR_%s\s*=\s*(\d+)" % name, code)
        assert m and int(m.group(1)) == value == getattr(_lib, "P3R_AIR_" + name), name
    body = re.search(r"typedef struct p3r_lookup_info \{(.*?)\} p3r_lookup_info;", code, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            assert decl.split()[0] == "uint32_t", decl
            fields += [f.strip() for f in decl.strip()[len("uint32_t"):].split(",")]
    assert fields == ["n_terms", "n_columns", "max_terms_per_column", "max_constraint_degree", "peak_live"]
    assert [(n, t) for n, t in _lib.P3rLookupInfo._fields_] == [(f, C.c_uint32) for f in fields]
    assert C.sizeof(_lib.P3rLookupInfo) == 20


def test_binding_table_carries_both_signatures():
    from plonky3_recursion_amd import _lib
    vp, u32p = C.c_void_p, _lib.u32p
    res, args = _lib.SIGNATURES["p3r_lookup_program_info"]
    assert res is C.c_int
    assert args == [C.POINTER(_lib.P3rConfig), C.POINTER(_lib.P3rAirInsn), C.c_size_t, C.POINTER(C.c_size_t), C.c_size_t,
                    C.POINTER(_lib.P3rLookupInfo)]
    res, args = _lib.SIGNATURES["p3r_logup_program_dmat"]
    assert res is C.c_int
    assert args == [vp, C.POINTER(_lib.P3rAirInsn), C.c_size_t, C.POINTER(vp), C.c_size_t, u32p, C.c_size_t, u32p, C.c_size_t, C.POINTER(vp), u32p]


def test_mirrors_reach_the_entries():
    import plonky3_recursion_amd as p3r
    from plonky3_recursion_amd import device
    assert callable(device.Context.logup_device) and callable(device.Context.lookup_program_info) and callable(p3r.lookup_program_info)
    assert callable(device.AirBuilder.lookup) and callable(device.AirBuilder.end_lookup_column)
    hpp = open(os.path.join(ROOT, "include/p3r.hpp")).read()
    assert re.search(r"class\s+AirProgram\b.*?void\s+lookup\s*\(.*?void\s+end_lookup_column\s*\(.*?p3r_lookup_program_info\s*\(", hpp, flags=re.S)
    assert re.search(r"\blogup_trace\s*\(.*?p3r_logup_program_dmat\s*\(", hpp, flags=re.S)
    mk = open(os.path.join(ROOT, "examples/Makefile")).read()
    assert re.search(r"^all:.*\blogup_program\b", mk, flags=re.M) and os.path.exists(os.path.join(ROOT, "examples/logup_program.cpp"))


def bus_program(p3r, field, n_fields=2):
    """One column of two terms on a bus: denominators bus_prefix + sum_j beta^j * field_j (challenges [bus_prefix, beta]),
    the first with multiplicity 1, the second with the cell next to its tuple."""
    b = p3r.AirBuilder(field)
    prefix, beta = b.challenge(0), b.challenge(1)
    for first, mult in ((0, 1), (n_fields, None)):
        d, bp = prefix, None
        for j in range(n_fields):
            cell = b.local(0, first + j)
            d = d + (cell if bp is None else bp * cell)
            bp = beta if bp is None else bp * beta
        b.lookup(mult if mult is not None else b.local(0, 2 * n_fields), d)
    b.end_lookup_column()
    return b


@pytest.mark.parametrize("field,dc", CTXS)
def test_lookup_program_info_through_the_library(field, dc):
    import plonky3_recursion_amd as p3r
    from plonky3_recursion_amd import _lib as L
    cfg, keep = p3r.make_config(field=field, challenge_degree=dc)
    info = p3r.lookup_program_info(cfg, bus_program(p3r, field), [5])
    # two denominators of degree 1, multiplicities of degree 0 and 1: max(1 + 2, max(0 + 1, 1 + 1)) = 3
    assert info["n_terms"] == 2 and info["n_columns"] == 1 and info["max_terms_per_column"] == 2 and info["max_constraint_degree"] == 3
    assert 0 < info["peak_live"] <= 8
    # an extension read needs DC columns
    e = p3r.AirBuilder(field)
    e.lookup(e.local_ext(1, 1), e.challenge(0) - e.next(0, 0))
    e.end_lookup_column()
    assert p3r.lookup_program_info(cfg, e, [1, dc + 1]) == dict(n_terms=1, n_columns=1, max_terms_per_column=1, max_constraint_degree=2, peak_live=3)
    with pytest.raises(p3r.P3rError) as err:
        p3r.lookup_program_info(cfg, e, [1, dc])
    assert err.value.code == P3R_EINVAL and "column" in str(err.value)
    LOC, LK, END = L.P3R_AIR_LOCAL, L.P3R_AIR_LOOKUP, L.P3R_AIR_LOOKUP_END
    refusals = [
        ("ASSERT_ZERO", [(LOC, 0, 0), (LK, 0, 0), (END, 0, 0), (L.P3R_AIR_ASSERT_ZERO, 0, 0)]),
        ("selector", [(L.P3R_AIR_IS_FIRST_ROW, 0, 0), (LOC, 0, 0), (LK, 0, 1), (END, 0, 0)]),
        ("selector", [(L.P3R_AIR_IS_LAST_ROW, 0, 0), (LOC, 0, 0), (LK, 0, 1), (END, 0, 0)]),
        ("selector", [(L.P3R_AIR_IS_TRANSITION, 0, 0), (LOC, 0, 0), (LK, 0, 1), (END, 0, 0)]),
        ("earlier", [(LOC, 0, 0), (LK, 0, 1), (END, 0, 0)]),
        ("no value", [(LOC, 0, 0), (LK, 0, 0), (LK, 0, 1), (END, 0, 0)]),
        ("no value", [(LOC, 0, 0), (LK, 0, 0), (END, 0, 0), (LK, 2, 0), (END, 0, 0)]),
        ("no open column", [(LOC, 0, 0), (END, 0, 0), (LK, 0, 0), (END, 0, 0)]),
        ("still open", [(LOC, 0, 0), (LK, 0, 0)]),
        ("no LOOKUP", [(LOC, 0, 0), (L.P3R_AIR_NEG, 0, 0)]),
        ("unknown op", [(23, 0, 0), (LK, 0, 0), (END, 0, 0)]),
    ]
    for word, prog in refusals:
        with pytest.raises(p3r.P3rError) as err:
            p3r.lookup_program_info(cfg, prog, [5])
        assert err.value.code == P3R_EINVAL and word in str(err.value), (word, str(err.value))
    too_many = p3r.AirBuilder(field)
    cells = [too_many.local(0, k % 5) for k in range(L.P3R_AIR_MAX_LIVE + 1)]
    acc = cells[0]
    for c in cells[1:]:
        acc = acc + c
    too_many.lookup(1, acc)
    too_many.end_lookup_column()
    with pytest.raises(p3r.P3rError) as err:
        p3r.lookup_program_info(cfg, too_many, [5])
    assert err.value.code == P3R_EUNSUPPORTED and "P3R_AIR_MAX_LIVE" in str(err.value)


@pytest.mark.parametrize("field,dc", CTXS)
def test_the_constraint_entry_still_takes_both_ops_for_unknown(field, dc):
    import plonky3_recursion_amd as p3r
    from plonky3_recursion_amd import _lib as L
    cfg, keep = p3r.make_config(field=field, challenge_degree=dc)
    for op in (L.P3R_AIR_LOOKUP, L.P3R_AIR_LOOKUP_END):
        with pytest.raises(p3r.P3rError) as err:
            p3r.air_program_info(cfg, [(L.P3R_AIR_LOCAL, 0, 0), (op, 0, 0), (L.P3R_AIR_ASSERT_ZERO, 0, 0)], [1])
        assert err.value.code == P3R_EINVAL and "unknown op %d" % op in str(err.value)
    with pytest.raises(p3r.P3rError) as err:
        p3r.air_program_info(cfg, bus_program(p3r, field), [5])
    assert err.value.code == P3R_EINVAL and "unknown op 21" in str(err.value)
