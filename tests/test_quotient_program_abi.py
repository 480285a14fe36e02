"""CPU: the constraint-program seam is declared - include/p3r.h carries p3r_air_program_info and
p3r_quotient_program_dmat with their argument lists and the op numbers, the ctypes table binds both, the ABI version stays
8 (functions are only added), the unit is built into both libraries, and include/p3r.hpp, the Python layer and the
examples reach the entries.  p3r_air_program_info needs no GPU: the AirBuilder mirror is checked through it."""
import ctypes as C
import os
import re

import pytest

from test_fri_seam_abi import arguments, header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ["CONST", "PUBLIC", "CHALLENGE", "LOCAL", "NEXT", "LOCAL_EXT", "NEXT_EXT", "IS_FIRST_ROW", "IS_LAST_ROW", "IS_TRANSITION", "ADD",
       "SUB", "MUL", "NEG", "ASSERT_ZERO"]


def test_header_declares_both_entry_points():
    from test_abi import header_symbols
    syms = header_symbols()
    assert "p3r_air_program_info" in syms and "p3r_quotient_program_dmat" in syms
    assert arguments("p3r_air_program_info") == [
        "const p3r_config* cfg", "const p3r_air_insn* prog", "size_t n_insns", "const size_t* widths", "size_t n_mats", "p3r_air_info* out"]
    assert arguments("p3r_quotient_program_dmat") == [
        "p3r_ctx* ctx", "const p3r_air_insn* prog", "size_t n_insns", "const p3r_dmat* const* mats", "size_t n_mats", "uint32_t added_bits",
        "uint32_t shift", "uint32_t log_quotient_degree", "const uint32_t* public_values", "size_t n_public", "const uint32_t* challenges",
        "size_t n_challenges", "const uint32_t* alpha", "p3r_dmat** outs"]
    src = header()
    assert int(re.search(r"#define\s+P3R_ABI_VERSION\s+(\d+)", src).group(1)) == 8
    assert re.search(r"typedef struct p3r_air_insn \{\s*uint32_t op, a, b;\s*\} p3r_air_insn;", src)
    for item in ("quotient_values", "split_evals", "ProverConstraintFolder", "SymbolicAirBuilder"):
        assert item in src, item


def test_op_numbers_and_the_live_limit_agree_with_the_header():
    from plonky3_recursion_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in OPS:
        m = re.search(r"\bP3R_AIR_%s\s*=\s*(\d+)" % name, code)
        assert m and int(m.group(1)) == getattr(_lib, "P3R_AIR_" + name), name
    assert len({getattr(_lib, "P3R_AIR_" + n) for n in OPS}) == len(OPS)
    live = int(re.search(r"#define\s+P3R_AIR_MAX_LIVE\s+(\d+)", code).group(1))
    assert live == _lib.P3R_AIR_MAX_LIVE and live >= 40


def test_binding_table_carries_both_signatures():
    from plonky3_recursion_amd import _lib
    vp, u32p = C.c_void_p, _lib.u32p
    res, args = _lib.SIGNATURES["p3r_air_program_info"]
    assert res is C.c_int
    assert args == [C.POINTER(_lib.P3rConfig), C.POINTER(_lib.P3rAirInsn), C.c_size_t, C.POINTER(C.c_size_t), C.c_size_t,
                    C.POINTER(_lib.P3rAirInfo)]
    res, args = _lib.SIGNATURES["p3r_quotient_program_dmat"]
    assert res is C.c_int
    assert args == [vp, C.POINTER(_lib.P3rAirInsn), C.c_size_t, C.POINTER(vp), C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, u32p,
                    C.c_size_t, u32p, C.c_size_t, u32p, C.POINTER(vp)]
    assert C.sizeof(_lib.P3rAirInsn) == 12 and C.sizeof(_lib.P3rAirInfo) == 16
    assert _lib.P3R_ABI_VERSION == 8


def test_mirrors_reach_the_entries():
    from plonky3_recursion_amd import device
    assert callable(device.Context.quotient_device) and callable(device.Context.air_program_info) and callable(device.AirBuilder)
    hpp = open(os.path.join(ROOT, "include/p3r.hpp")).read()
    assert re.search(r"class\s+AirProgram\b.*?p3r_air_program_info\s*\(", hpp, flags=re.S)
    assert re.search(r"\bquotient_values\s*\(.*?p3r_quotient_program_dmat\s*\(", hpp, flags=re.S)
    mk = open(os.path.join(ROOT, "examples/Makefile")).read()
    assert re.search(r"^all:.*\bquotient_program\b", mk, flags=re.M) and os.path.exists(os.path.join(ROOT, "examples/quotient_program.cpp"))


def test_the_unit_is_built_into_both_libraries():
    import __graft_entry__ as g
    assert "tu_air.hip" in g.HIP_SOURCES and os.path.exists(os.path.join(g.CSRC, "tu_air.hip"))
    src = open(g.__file__).read()
    assert re.search(r"shared\s*=\s*\[[^\]]*\"tu_air\.hip\"", src)
    api = open(os.path.join(g.CSRC, "tu_api.h")).read()
    assert "quotient_program(" in api and "tu_air.hip" in api


def fib_cube(p3r, field):
    """The three-column AIR of the composition test: c = a^3 + b, the next row starts from (b, c)."""
    b = p3r.AirBuilder(field)
    x, y, z = b.local(0, 0), b.local(0, 1), b.local(0, 2)
    b.assert_zero(z - (x * x * x + y))
    t = b.is_transition()
    b.assert_zero(t * (b.next(0, 0) - y))
    b.assert_zero(t * (b.next(0, 1) - z))
    b.assert_zero(b.is_first_row() * (x - b.public(0)))
    b.assert_zero(b.is_last_row() * (z - b.public(1)))
    return b


@pytest.mark.parametrize("field,dc", [("koala-bear", 4), ("koala-bear", 5), ("baby-bear", 4)])
def test_builder_programs_through_the_host_entry(field, dc):
    import plonky3_recursion_amd as p3r
    cfg, keep = p3r.make_config(field=field, challenge_degree=dc)
    b = fib_cube(p3r, field)
    info = p3r.air_program_info(cfg, b, [3])
    assert info["n_constraints"] == 5 and info["max_degree"] == 3 and info["log_quotient_degree"] == 1
    assert 0 < info["peak_live"] <= 8
    # python ints become constants; an extension read needs DC columns
    e = p3r.AirBuilder(field)
    e.assert_zero((e.local_ext(1, 1) * e.challenge(0) + 1) * (2 - e.next(0, 0)) * -e.local(0, 0))
    assert p3r.air_program_info(cfg, e, [1, dc + 1])["max_degree"] == 3
    for widths in ([1, dc], [0, dc + 1]):
        with pytest.raises(p3r.P3rError) as err:
            p3r.air_program_info(cfg, e, widths)
        assert err.value.code == -1 and "column" in str(err.value)
    with pytest.raises(p3r.P3rError) as err:
        p3r.air_program_info(cfg, [(16, 0, 0)], [1])
    assert err.value.code == -1 and "earlier" in str(err.value)
