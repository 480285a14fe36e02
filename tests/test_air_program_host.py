"""CPU: the host half of the constraint-program seam (csrc/air_program.h: validation, typing, the degree walk, liveness,
the slot assignment, the compiled instruction stream, the per-chunk domain constants) walked by
tests/air_program_host_main.cpp, compiled with g++ alone - and, being a program with its own main, with the address and
undefined-behaviour sanitizers.  The program checks every case itself; what it prints is pinned here."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "plonky3_recursion_amd", "csrc")
P3R_EINVAL, P3R_EUNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("air_program_host")), "air_program_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "air_program_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return [l.split() for l in r.stdout.splitlines()]


def test_every_host_refusal_has_its_code(lines):
    got = {}
    for kind, name, code in (l for l in lines if l[0] == "refused"):
        got.setdefault(name, set()).add(int(code))
    einval = ["operand_not_earlier", "operand_later", "operand_is_assert", "assert_of_assert", "unknown_op", "matrix_out_of_range",
              "column_out_of_range", "ext_columns_out_of_range", "ext_columns_narrow_matrix", "column_wraps", "public_out_of_range",
              "challenge_out_of_range", "non_canonical_constant", "no_assert", "empty", "shift_h_is_one", "shift_in_trace_domain",
              "shift_h_is_chunk_root", "non_canonical_shift", "domain_above_two_adicity"]
    assert got == {**{n: {P3R_EINVAL} for n in einval}, "log_quotient_degree_5": {P3R_EUNSUPPORTED}}


def test_degrees_and_the_quotient_degree_they_need(lines):
    # log2_ceil(max(d, 2) - 1)
    assert [(int(d), int(q)) for kind, d, q in (l for l in lines if l[0] == "degree")] == [(1, 0), (2, 0), (3, 1), (5, 2), (9, 3)]


def test_the_live_limit_from_both_sides(lines):
    from plonky3_recursion_amd import _lib
    assert [l[1:] for l in lines if l[0] == "live"] == [[str(_lib.P3R_AIR_MAX_LIVE), "accepted"], [str(_lib.P3R_AIR_MAX_LIVE + 1), "refused"]]
    assert _lib.P3R_AIR_MAX_LIVE >= 40


def test_slots_never_hold_two_live_values(lines):
    (kind, programs, constraints), = [l for l in lines if l[0] == "replay"]
    assert int(programs) >= 100 and int(constraints) >= int(programs)
