"""GPU: p3r::witness_columns of include/p3r.hpp from compiled code (examples/witness_program.cpp), in the manner of
tests/test_gpu_lookup_multiplicities_cpp.py: from one uploaded column of 16-bit values the example derives the byte limbs,
the is-zero flag with its inverse witness and the byte table on the device, counts the limbs with
p3r::lookup_multiplicities and checks the gadgets with p3r::check_constraints.  What it must print is worked out here
from the example's own description of its inputs."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "witness_program")
CTXS = [("koala-bear", 4), ("koala-bear", 5), ("baby-bear", 4)]


@pytest.mark.parametrize("field,dc", CTXS)
def test_the_example_derives_counts_and_checks(field, dc):
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "witness_program"], check=True)
    r = subprocess.run([EXE, field, str(dc)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    v = [0 if row % 8 == 0 else 1021 * row % 65536 for row in range(64)]   # every eighth row zeroed
    limbs = [x & 0xFF for x in v] + [x >> 8 for x in v]
    assert v.count(0) == 8 and len(limbs) == 128
    assert r.stdout.strip().split("\n") == [
        "derived 4 columns, table 256 rows",
        "zeros 8",
        "bytes 128 %d" % len(set(limbs)),
        "ok"]
