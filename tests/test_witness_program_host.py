"""CPU: the host half of the witness seam (csrc/air_program.h in its witness mode: validation and typing of witness
programs, STORE as a sink that takes no slot, the output columns stored exactly once, the compiled INV / BITS / ROW / STORE
ops) walked by tests/witness_program_host_main.cpp, compiled with g++ alone - once plainly and once, being a program with
its own main, with the address and undefined-behaviour sanitizers.  The program checks every case and every message
itself; what it prints is pinned here, for both builds."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "plonky3_recursion_amd", "csrc")
P3R_EINVAL, P3R_EUNSUPPORTED = -1, -5
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def lines(request, tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("witness_program_host_" + request.param)), "witness_program_host")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + BUILDS[request.param] +
                   ["-I", CSRC, os.path.join(ROOT, "tests", "witness_program_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return [l.split() for l in r.stdout.splitlines()]


def test_every_refusal_of_a_witness_program_has_its_code_and_message(lines):
    got = {}
    for kind, name, code in (l for l in lines if l[0] == "refused"):
        got.setdefault(name, []).append(int(code))
    einval = {"assert_zero": 1, "lookup": 1, "lookup_end": 1,
              "bits_of_extension": 1, "bits_none": 1, "bits_1_31": 1, "bits_31_1": 1, "bits_huge_count": 1,
              "inv_operand_not_earlier": 1, "bits_operand_not_earlier": 1, "store_operand_not_earlier": 1, "store_of_store": 1,
              "inv_of_store": 1, "add_of_store": 1,
              "no_store": 1, "empty": 1, "stored_twice": 1, "ext_store_overlaps_later": 1, "ext_store_overlaps_earlier": 1,
              "column_not_stored": 1, "column_0_not_stored": 1, "gap_before_ext_store": 1, "too_many_columns": 1, "ext_store_wraps": 1,
              "unknown_op": 1, "unknown_op_low": 1, "matrix_out_of_range": 1, "column_out_of_range": 1, "ext_columns_out_of_range": 1,
              "public_out_of_range": 1, "challenge_out_of_range": 1, "non_canonical_constant": 1, "input_with_no_matrix": 1,
              # the height of a program with no input: 0, 3 and 100 rows; 2^25 under KoalaBear
              "height_not_a_power_of_two": 3, "height_above_two_adicity": 1,
              # ops 23 .. 26 under the two other modes, named and by default
              "constraint_mode_unknown_op": 4, "lookup_mode_unknown_op": 4, "default_mode_unknown_op": 4}
    assert got == {n: [P3R_EINVAL] * k for n, k in einval.items()}


def test_the_edges_a_witness_program_may_stand_on(lines):
    assert [l[1] for l in lines if l[0] == "accepted"] == [
        "bits_0_31", "bits_30_1", "ext_store_at_w_minus_dc", "ext_store_between_base_stores", "row_with_no_matrix", "selectors"]


def test_typing_counts_and_the_compiled_ops(lines):
    # n_stores, n_out_columns (2 base and 2 quartic stores), n_inversions, peak_live of the typed program; its stream's new ops
    assert [l[1:] for l in lines if l[0] == "info"] == [["4", "10", "2", "5"]]
    assert [l[1:] for l in lines if l[0] == "stream"] == [["2", "1", "1", "4"]]


def test_the_live_limit_from_both_sides(lines):
    from plonky3_recursion_amd import _lib
    assert [l[1:] for l in lines if l[0] == "live"] == [[str(_lib.P3R_AIR_MAX_LIVE), "accepted"], [str(_lib.P3R_AIR_MAX_LIVE + 1), "refused"]]
