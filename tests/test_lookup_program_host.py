"""CPU: the host half of the lookup-program seam (csrc/air_program.h in its lookup mode: validation, typing, liveness and
slots of lookup programs, the degree of each auxiliary column's constraint, the compiled term and end-of-column ops)
walked by tests/lookup_program_host_main.cpp, compiled with g++ alone - and, being a program with its own main, with the
address and undefined-behaviour sanitizers.  The program checks every case itself; what it prints is pinned here."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "plonky3_recursion_amd", "csrc")
P3R_EINVAL, P3R_EUNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("lookup_program_host")), "lookup_program_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "lookup_program_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return [l.split() for l in r.stdout.splitlines()]


def test_every_refusal_of_a_lookup_program_has_its_code(lines):
    got = {}
    for kind, name, code in (l for l in lines if l[0] == "refused"):
        got.setdefault(name, []).append(int(code))
    einval = {"assert_zero": 1, "selector": 3, "operand_not_earlier": 1, "operand_later": 1, "operand_is_lookup": 1, "operand_is_lookup_end": 1,
              "value_of_a_sink": 1, "end_with_no_open_column": 1, "end_twice": 1, "column_still_open": 1, "no_lookup": 1, "empty": 1,
              "unknown_op": 1, "matrix_out_of_range": 1, "column_out_of_range": 1, "ext_columns_out_of_range": 1, "public_out_of_range": 1,
              "challenge_out_of_range": 1, "non_canonical_constant": 1,
              # the traces' height: 0, 3, 6, 12, 1000 and 2^20 + 1 rows; 2^25 under KoalaBear, 2^28 under BabyBear
              "height_not_a_power_of_two": 6, "height_above_two_adicity": 2,
              # ops 21 and 22 under the constraint mode, named and by default
              "constraint_mode_unknown_op": 2, "default_mode_unknown_op": 2}
    assert got == {n: [P3R_EINVAL] * k for n, k in einval.items()}


def test_the_degree_of_a_column_constraint_on_hand_computed_cases(lines):
    # max(1 + sum_k deg d_k, max_k(deg m_k + sum_{l != k} deg d_l))
    assert [(name, int(d)) for kind, name, d in (l for l in lines if l[0] == "degree")] == [
        ("one_term", 2), ("one_term_base_multiplicity", 2), ("one_term_ext_multiplicity", 2), ("one_term_cubic_multiplicity", 3),
        ("one_term_quadratic_denominator", 3), ("two_terms", 3), ("two_terms_mixed", 4), ("two_terms_numerator_decides", 5),
        ("three_terms", 4), ("three_terms_mixed", 5), ("three_columns", 4), ("constant_denominator", 1)]


def test_typing_slots_and_the_compiled_sinks(lines):
    # n_terms, n_columns, max_terms_per_column, max_constraint_degree, peak_live of the typed program; its stream's sinks
    assert [l[1:] for l in lines if l[0] == "info"] == [["3", "2", "2", "3", "4"]]
    assert [l[1:] for l in lines if l[0] == "stream"] == [["3", "2"]]


def test_the_live_limit_from_both_sides(lines):
    from plonky3_recursion_amd import _lib
    assert [l[1:] for l in lines if l[0] == "live"] == [[str(_lib.P3R_AIR_MAX_LIVE), "accepted"], [str(_lib.P3R_AIR_MAX_LIVE + 1), "refused"]]
