"""CPU: the host half of the recurrence seam (csrc/scan_plan.h: validation of p3r_recurrence descriptors, the form each
runs in, the output width and the counts, the heights, the geometry of the passes) walked by tests/scan_plan_host_main.cpp,
compiled with g++ alone - once plainly and once, being a program with its own main, with the address and
undefined-behaviour sanitizers.  The program checks every case and every message itself; what it prints is pinned here,
for both builds."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "plonky3_recursion_amd", "csrc")
P3R_EINVAL = -1
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def lines(request, tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("scan_plan_host_" + request.param)), "scan_plan_host")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + BUILDS[request.param] +
                   ["-I", CSRC, os.path.join(ROOT, "tests", "scan_plan_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return [l.split() for l in r.stdout.splitlines()]


def test_every_refusal_of_a_descriptor_set_has_its_code_and_message(lines):
    got = [(name, int(code)) for kind, name, code in (l for l in lines if l[0] == "refused")]
    names = ["no_recurrences", "null_recs", "too_many_recurrences", "no_matrices", "null_widths", "unknown_flag", "unknown_flag_high",
             "neither_mul_nor_add", "mul_matrix_out_of_range", "add_matrix_out_of_range", "matrix_just_below_none", "column_out_of_range",
             "column_wraps", "ext_columns_out_of_range", "ext_columns_of_a_narrow_matrix", "ext_columns_wrap", "init_not_canonical",
             "ext_init_not_canonical", "base_init_not_padded", "ext_init_not_padded", "same_output_column", "base_inside_ext_output",
             "ext_outputs_overlap", "gap_below_w", "column_0_not_written", "gap_before_ext_output", "output_column_out_of_range",
             "ext_output_column_out_of_range", "height_0", "height_3", "height_above_two_adicity"]
    assert got == [(n, P3R_EINVAL) for n in names]


def test_the_edges_a_descriptor_set_may_stand_on(lines):
    assert [l[1:] for l in lines if l[0] == "accepted"] == [
        ["one_base_sum", "1"], ["last_columns_read", "5"], ["outputs_in_any_order", "6"], ["same_input_for_a_and_b", "3"],
        ["quintic_init_of_five_words", "5"]]


def test_counts_forms_and_geometry(lines):
    # ext affine at 0, base sum at 4, base product at 5, ext product at 6, base affine at 10, ext sum at 11: W = 15
    assert [l[1:] for l in lines if l[0] == "info"] == [["15", "2", "2", "2"]]
    # EXT = 1, MUL = 2, ADD = 4, in the order the recurrences were given
    assert [l[1:] for l in lines if l[0] == "forms"] == [["4", "7", "2", "3", "6", "5"]]
    # items per thread, threads, rows per tile, and the height tests/test_gpu_affine_scan.py takes for its largest
    import test_gpu_affine_scan as gpu
    assert [l[1:] for l in lines if l[0] == "geometry"] == [[str(gpu.ITEMS), str(gpu.BLOCK), str(gpu.TILE), str(gpu.HEIGHTS[-1])]]
    assert (gpu.ITEMS, gpu.BLOCK, gpu.TILE, gpu.HEIGHTS[-1]) == (4, 256, 1024, 1 << 19)
