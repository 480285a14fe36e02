"""GPU: p3r::affine_scan of include/p3r.hpp from compiled code (examples/running_product.cpp), in the manner of
tests/test_gpu_witness_program_cpp.py: from two uploaded columns, one a permutation of the other, the example derives the
factor (gamma - x) / (gamma - y) with p3r::witness_columns and the running product with p3r::affine_scan, checks the four
constraints with p3r::check_constraints, and finds the total one - and not one after a cell of y is changed.  What it
must print is worked out here from the example's own description of its inputs."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "running_product")
CTXS = [("koala-bear", 4), ("koala-bear", 5), ("baby-bear", 4)]


@pytest.mark.parametrize("field,dc", CTXS)
def test_the_example_multiplies_checks_and_tells_a_permutation(field, dc):
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "running_product"], check=True)
    r = subprocess.run([EXE, field, str(dc)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    x = [(1021 * row + 7) % 65536 for row in range(64)]
    y = [x[(5 * row + 3) % 64] for row in range(64)]
    assert sorted(x) == sorted(y) and x != y and len(set(x)) == 64   # a permutation, and one changed cell breaks it
    assert r.stdout.strip().split("\n") == [
        "columns %d rows 64" % (2 * dc),
        "total one",
        "spoiled total not one",
        "ok"]
