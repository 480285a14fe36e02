"""CPU: the two trace checks are declared - include/p3r.h carries p3r_check_program_dmat and p3r_lookup_check_dmat with
their argument lists, the three structs and P3R_LOOKUP_CHECK_MAX_RECORDS; the ctypes mirrors have the header's layouts
(p3r_check_report 16 bytes, p3r_lookup_imbalance 56); the ABI version stays 8 (functions are only added, no op is); the
Python layer, include/p3r.hpp and the example reach the entries; and p3r_lookup_program_info still refuses selectors and
ASSERT_ZERO, as p3r_air_program_info still takes ops 21 and 22 for unknown."""
import ctypes as C
import os
import re

import pytest

from test_fri_seam_abi import arguments, header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTXS = [("koala-bear", 4), ("koala-bear", 5), ("baby-bear", 4)]
P3R_EINVAL = -1


def test_header_declares_both_entry_points_and_the_library_exports_them():
    from test_abi import header_symbols
    from plonky3_recursion_amd import _lib
    syms = header_symbols()
    assert "p3r_check_program_dmat" in syms and "p3r_lookup_check_dmat" in syms
    assert arguments("p3r_check_program_dmat") == [
        "p3r_ctx* ctx", "const p3r_air_insn* prog", "size_t n_insns", "const p3r_dmat* const* mats", "size_t n_mats",
        "const uint32_t* public_values", "size_t n_public", "const uint32_t* challenges", "size_t n_challenges", "p3r_check_report* report",
        "uint32_t* first_row_out", "uint64_t* n_failed_out"]
    assert arguments("p3r_lookup_check_dmat") == [
        "p3r_ctx* ctx", "const p3r_lookup_instance* inst", "size_t n_inst", "const uint32_t* challenges", "size_t n_challenges",
        "p3r_lookup_imbalance* out", "size_t cap", "uint64_t* n_unbalanced_out"]
    src = header()
    assert int(re.search(r"#define\s+P3R_ABI_VERSION\s+(\d+)", src).group(1)) == 8 == _lib.P3R_ABI_VERSION
    m = re.search(r"#define\s+P3R_LOOKUP_CHECK_MAX_RECORDS\s+\(1u\s*<<\s*(\d+)\)", src)
    assert m and 1 << int(m.group(1)) == 1 << 28 == _lib.P3R_LOOKUP_CHECK_MAX_RECORDS
    for item in ("DebugConstraintBuilder", "test-utils/src/lib.rs:165-260", "check_air_satisfies", "check_lookups",
                 "batch_stark_prover.rs:1546-1593", "is_transition =", "0xffffffff"):
        assert item in src, item
    lib = _lib.load()   # raises if a declared symbol is not exported
    assert lib.p3r_check_program_dmat and lib.p3r_lookup_check_dmat


def struct_fields(name):
    """[(C type, field name, array length or None)] of `typedef struct <name> {...} <name>;` in the header."""
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), code, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        first, *more = decl.split(",")   # "<type> <name>", then further names of the type
        ctype, name0 = first.rsplit(" ", 1)
        for n in [name0] + more:
            m = re.fullmatch(r"\s*(\w+)(?:\[(\d+)\])?\s*", n)
            assert m, decl
            fields.append((ctype.strip(), m.group(1), int(m.group(2)) if m.group(2) else None))
    return fields


CTYPE = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "size_t": C.c_size_t, "const uint32_t*": C.POINTER(C.c_uint32),
         "const p3r_dmat_cptr*": C.POINTER(C.c_void_p)}   # p3r_dmat_cptr = const p3r_dmat*: the member is const p3r_dmat* const*


def test_struct_layouts_agree_with_the_header():
    from plonky3_recursion_amd import _lib
    CTYPE["const p3r_air_insn*"] = C.POINTER(_lib.P3rAirInsn)
    assert re.search(r"typedef\s+const\s+p3r_dmat\s*\*\s*p3r_dmat_cptr\s*;", header())
    for name, mirror, size in (("p3r_check_report", _lib.P3rCheckReport, 16), ("p3r_lookup_instance", _lib.P3rLookupInstance, 6 * C.sizeof(C.c_void_p)),
                               ("p3r_lookup_imbalance", _lib.P3rLookupImbalance, 56)):
        want = [(n, CTYPE[t] * k if k else CTYPE[t]) for t, n, k in struct_fields(name)]
        assert [(n, t) for n, t in mirror._fields_] == want, name
        assert C.sizeof(mirror) == size, name
    assert [n for _, n, _ in struct_fields("p3r_check_report")] == ["n_failures", "first_row", "first_constraint"]
    assert [n for _, n, _ in struct_fields("p3r_lookup_imbalance")] == ["instance", "row", "term", "n_records", "denominator", "net"]
    assert _lib.P3rLookupImbalance.denominator.offset == 16 and _lib.P3rLookupImbalance.net.offset == 36


def test_binding_table_carries_both_signatures():
    from plonky3_recursion_amd import _lib
    vp, u32p = C.c_void_p, _lib.u32p
    res, args = _lib.SIGNATURES["p3r_check_program_dmat"]
    assert res is C.c_int
    assert args == [vp, C.POINTER(_lib.P3rAirInsn), C.c_size_t, C.POINTER(vp), C.c_size_t, u32p, C.c_size_t, u32p, C.c_size_t,
                    C.POINTER(_lib.P3rCheckReport), u32p, C.POINTER(C.c_uint64)]
    res, args = _lib.SIGNATURES["p3r_lookup_check_dmat"]
    assert res is C.c_int
    assert args == [vp, C.POINTER(_lib.P3rLookupInstance), C.c_size_t, u32p, C.c_size_t, C.POINTER(_lib.P3rLookupImbalance), C.c_size_t,
                    C.POINTER(C.c_uint64)]


def test_mirrors_and_the_example_reach_the_entries():
    from plonky3_recursion_amd import device
    assert callable(device.Context.check_device) and callable(device.Context.lookup_check_device)
    hpp = open(os.path.join(ROOT, "include/p3r.hpp")).read()
    assert re.search(r"\bcheck_constraints\s*\(.*?p3r_check_program_dmat\s*\(", hpp, flags=re.S)
    assert re.search(r"\bcheck_lookups\s*\(.*?p3r_lookup_check_dmat\s*\(", hpp, flags=re.S)
    mk = open(os.path.join(ROOT, "examples/Makefile")).read()
    assert re.search(r"^all:.*\bcheck_program\b", mk, flags=re.M)
    example = open(os.path.join(ROOT, "examples/check_program.cpp")).read()
    assert "p3r::check_constraints" in example and "p3r::check_lookups" in example


@pytest.mark.parametrize("field,dc", CTXS)
def test_no_op_was_added_and_the_program_infos_refuse_what_they_refused(field, dc):
    import plonky3_recursion_amd as p3r
    from plonky3_recursion_amd import _lib as L
    cfg, keep = p3r.make_config(field=field, challenge_degree=dc)
    LOC, LK, END = L.P3R_AIR_LOCAL, L.P3R_AIR_LOOKUP, L.P3R_AIR_LOOKUP_END
    for sel in (L.P3R_AIR_IS_FIRST_ROW, L.P3R_AIR_IS_LAST_ROW, L.P3R_AIR_IS_TRANSITION):
        with pytest.raises(p3r.P3rError) as err:
            p3r.lookup_program_info(cfg, [(sel, 0, 0), (LOC, 0, 0), (LK, 0, 1), (END, 0, 0)], [1])
        assert err.value.code == P3R_EINVAL and "selector" in str(err.value)
    with pytest.raises(p3r.P3rError) as err:
        p3r.lookup_program_info(cfg, [(LOC, 0, 0), (LK, 0, 0), (END, 0, 0), (L.P3R_AIR_ASSERT_ZERO, 0, 0)], [1])
    assert err.value.code == P3R_EINVAL and "ASSERT_ZERO" in str(err.value)
    for op in (LK, END, 23):
        with pytest.raises(p3r.P3rError) as err:
            p3r.air_program_info(cfg, [(LOC, 0, 0), (op, 0, 0), (L.P3R_AIR_ASSERT_ZERO, 0, 0)], [1])
        assert err.value.code == P3R_EINVAL and "unknown op %d" % op in str(err.value)
    with pytest.raises(p3r.P3rError) as err:
        p3r.lookup_program_info(cfg, [(23, 0, 0), (LK, 0, 0), (END, 0, 0)], [1])
    assert err.value.code == P3R_EINVAL and "unknown op 23" in str(err.value)
