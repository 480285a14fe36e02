"""GPU: p3r::lookup_multiplicities of include/p3r.hpp from compiled code (examples/lookup_table.cpp), in the manner of
tests/test_gpu_check_program_cpp.py: the example range-checks a column of 64 values against the table 0 .. 15, builds the
table's counts on the device, shows with p3r::check_lookups that they balance the bus, then puts one value out of range
and prints the miss.  What it must print is worked out here from the example's own description of its inputs."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "lookup_table")
CTXS = [("koala-bear", 4), ("koala-bear", 5), ("baby-bear", 4)]


@pytest.mark.parametrize("field,dc", CTXS)
def test_the_example_prints_the_counts_and_the_miss(field, dc):
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "lookup_table"], check=True)
    r = subprocess.run([EXE, field, str(dc)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    counts = [0] * 16
    for row in range(64):   # v[r] = floor(r^2 / 3) mod 16
        counts[row * row // 3 % 16] += 1
    assert sum(counts) == 64 and 0 in counts
    # v[37] = 16 is in no table row: one record, asked for once
    assert r.stdout.strip().split("\n") == [
        "counts " + " ".join(str(c) for c in counts),
        "bus ok",
        "missing 1",
        "key first at query 0 row 37 term 0, 1 records, net " + " ".join(["1"] + ["0"] * (dc - 1)),
        "ok"]
