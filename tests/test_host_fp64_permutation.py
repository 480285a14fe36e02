"""CPU: the FP64 Poseidon2 permutation of the hashing kernels (csrc/poseidon2_f64.hip.h: p2f_permute, deferred 2^-k
fix-ups in the partial rounds) computes the integer permutation of csrc/poseidon2.h on the host: both fields, every
carried-lane mask the kernels use, 2^20 random states and the edge states, zero mismatches.  The header's static_asserts
(the bound walker over the partial-round schedule) are compiled on the way."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fp64_permutation_equals_integer(tmp_path):
    exe = str(tmp_path / "hp2f")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "plonky3_recursion_amd", "csrc"),
                    os.path.join(ROOT, "tools", "microbench", "host_p2f_check.cpp"), "-o", exe], check=True)
    # 2^17 random states per field and mask: 2^20 in all
    r = subprocess.run([exe, str(1 << 17)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if "mismatches" in ln]
    assert len(lines) == 8, r.stdout
    for ln in lines:
        assert "mismatches 0 of %d" % ((1 << 17) + 7) in ln, ln
