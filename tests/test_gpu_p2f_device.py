"""GPU: the FP64 Poseidon2 permutations of the hashing kernels (csrc/poseidon2_f64.hip.h, csrc/poseidon2_w32_f64.hip.h) and
p2f_store as the DEVICE build computes them, against integer arithmetic, through the p3r_test_p2f_* seam that only the
knobs build of the library exports: both fields, both widths, every carried-lane mask the kernels instantiate, the
built-in diagonal's forms and the general path, edge states with the carried lanes at their stated maxima and 2^12 random
states a case (tests/p2f_device_cases.py).  tests/test_host_fp64_permutation.py runs the same arithmetic on the host; this
is the check that the two builds agree."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = os.path.join(ROOT, "plonky3_recursion_amd", "knobs", "libp3r_hip.so")


@pytest.mark.gpu
def test_device_fp64_permutations_against_integers():
    if not os.path.exists(KNOBS):
        pytest.skip("knobs build of the library is absent (__graft_entry__.build() makes it)")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "p2f_device_cases.py")], capture_output=True, text=True,
                       env=dict(os.environ, P3R_LIB_PATH=KNOBS), timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "p2f_device ok" in r.stdout
