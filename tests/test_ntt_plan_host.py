"""CPU: the geometry of the NTT passes (csrc/ntt_plan.h: the split of a transform, lean or generic kernels, tile sizes,
workgroup counts) walked by tests/ntt_plan_host_main.cpp for both fields - every height up to the two-adicity, added_bits
0..3, widths 1 and 33, the default tuning values and P3R_NTT_LINE_LOG_TILE = 13.  The program checks the properties the
launches rely on for every case; the plans it prints are pinned here at the points read off the rules."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "plonky3_recursion_amd", "csrc")
TWO_ADICITY = {"koala-bear": 24, "baby-bear": 27}


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("ntt_plan_host")), "ntt_plan_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "ntt_plan_host_main.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = {}
    for line in r.stdout.splitlines():
        field, direction, line_tile, log_n, kind, *nums = line.split()
        key = (field, direction, int(line_tile), int(log_n))
        assert key not in out
        out[key] = (kind, *map(int, nums))
    return out


def test_every_height_of_both_fields_is_walked(plans):
    for field, top in TWO_ADICITY.items():
        for log_n in range(top + 1):
            assert (field, "inv", 12, log_n) in plans
            assert (field, "fwd", 12, log_n) in plans and (field, "fwd", 13, log_n) in plans
    assert len(plans) == 3 * sum(top + 1 for top in TWO_ADICITY.values())


# (kind, la, lb, log2 of the tile of pass 1, of pass 2); heights above 2^24 exist for BabyBear only
INVERSE = {11: ("single", 0, 11, 0, 0), 12: ("generic", 6, 6, 0, 0), 13: ("lean", 6, 7, 13, 13), 20: ("lean", 10, 10, 14, 14),
           24: ("lean", 12, 12, 14, 14), 25: ("generic", 12, 13, 0, 0)}
FORWARD = {11: ("single", 0, 11, 0, 0), 12: ("generic", 6, 6, 0, 0), 13: ("lean", 6, 7, 13, 12), 20: ("lean", 8, 12, 13, 12),
           22: ("lean", 9, 13, 14, 13), 25: ("lean", 12, 13, 14, 13), 26: ("generic", 13, 13, 0, 0)}


@pytest.mark.parametrize("field", sorted(TWO_ADICITY))
def test_pinned_plans(plans, field):
    for log_n, want in INVERSE.items():
        if log_n <= TWO_ADICITY[field]:
            assert plans[field, "inv", 12, log_n] == want, ("inverse", log_n)
    for log_n, want in FORWARD.items():
        if log_n <= TWO_ADICITY[field]:
            assert plans[field, "fwd", 12, log_n] == want, ("forward", log_n)
            # P3R_NTT_LINE_LOG_TILE = 13 moves the line tile and nothing else
            assert plans[field, "fwd", 13, log_n] == want[:4] + (13 if want[0] == "lean" else 0,), ("forward, line tile 13", log_n)


def test_the_fields_share_one_rule(plans):
    for (field, direction, line_tile, log_n), plan in plans.items():
        if field == "koala-bear":
            assert plans["baby-bear", direction, line_tile, log_n] == plan
