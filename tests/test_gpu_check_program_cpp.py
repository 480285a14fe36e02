"""GPU: p3r::check_constraints and p3r::check_lookups of include/p3r.hpp from compiled code (examples/check_program.cpp),
in the manner of tests/test_gpu_quotient_program_cpp.py: the example passes a Fibonacci table and a balanced bus of two
tables, then plants one wrong cell (b of row 37) and drops one send (the sender's row 11) and prints what the two checks
find.  The findings are worked out here from the example's own description of its inputs."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "check_program")
CTXS = [("koala-bear", 4), ("koala-bear", 5), ("baby-bear", 4)]
MODULUS = {"koala-bear": 0x7F000001, "baby-bear": 0x78000001}


@pytest.mark.parametrize("field,dc", CTXS)
def test_the_example_prints_both_findings(field, dc):
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "check_program"], check=True)
    r = subprocess.run([EXE, field, str(dc)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    # b of row 37: next.b = a + b (constraint 1) fails into the row and out of it, next.a = b (constraint 0) out of it.
    # The send of row 11 is tuple 11 * 5 mod 8 = 7, which row 3 sends too: the key's first record is the sender's row 3,
    # one send and the receive of -2 are left, the net is -1.
    net = " ".join([str(MODULUS[field] - 1)] + ["0"] * (dc - 1))
    assert r.stdout.strip().split("\n") == [
        "constraints ok",
        "constraint 0 fails first in row 37 (1 rows)",
        "constraint 1 fails first in row 36 (2 rows)",
        "first failure: row 36 constraint 1",
        "bus ok",
        "unbalanced 1",
        "key first at instance 0 row 3 term 0, 2 records, net " + net,
        "ok"]
