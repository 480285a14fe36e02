"""GPU: the integer field arithmetic of csrc/field.h (Fp, Fp4, Fp5, Fp1) as the DEVICE build computes it, one operation at
a time through the p3r_test_field_op seam that only the knobs build of the library exports, against Python integers and
against the host build of the same header: edge Montgomery words (0, 1, P - 1, one, minus one, the halves), dot2 with all
four factors at P - 1, every extension element with coefficients from {0, one, P - 1} and the full square of that set
through the products, inverses compared word for word with a^(p^D - 2), the inverse of zero pinned, and 2^14 random cases
per operation (tests/field_cases.py, tests/field_device_cases.py).  tests/test_field_host.py runs the same cases on the
host; this is the check that the device branch of reduce64 and the range arguments that lean on it hold at the edges."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = os.path.join(ROOT, "plonky3_recursion_amd", "knobs", "libp3r_hip.so")


@pytest.mark.gpu
def test_device_field_arithmetic_against_integers():
    if not os.path.exists(KNOBS):
        pytest.skip("knobs build of the library is absent (__graft_entry__.build() makes it)")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "field_device_cases.py")], capture_output=True, text=True,
                       env=dict(os.environ, P3R_LIB_PATH=KNOBS), timeout=600)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "field_device ok" in r.stdout
    for field in ("koala-bear", "baby-bear"):
        assert "%s: " % field in r.stdout and "equal the integer reference" in r.stdout
