"""Run by tests/test_gpu_mmcs_geometry.py in a fresh process with P3R_LIB_PATH = the knobs build of the library and one
setting of the Merkle tuning knobs in the environment (they are read once per process): groups a and b of
tests/mmcs_cases.py on the device against tests/mmcs_ref.py, both fields.  Prints one JSON line: the list of mismatches."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import plonky3_recursion_amd as p3r  # noqa: E402
import mmcs_cases  # noqa: E402
import oracle_lib  # noqa: E402


def main():
    oracle = oracle_lib.Oracle()
    cases = mmcs_cases.GROUPS["a"] + mmcs_cases.GROUPS["b"]
    bad = []
    for field in mmcs_cases.FIELDS:
        bad += ["%s: %s" % (field, m) for m in mmcs_cases.walk_device(p3r, oracle, field, cases)]
    print(json.dumps({"mismatches": bad, "trees": sum(len(c.caps) for c in cases) * len(mmcs_cases.FIELDS)}))


if __name__ == "__main__":
    main()
