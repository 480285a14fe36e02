"""CPU: the FP64 Poseidon2 permutation of the hashing kernels (csrc/poseidon2_f64.hip.h: p2f_permute, deferred 2^-k
fix-ups in the partial rounds) computes the integer permutation of csrc/poseidon2.h on the host: both fields, every
carried-lane mask the kernels use, 2^20 random states and the edge states, zero mismatches.  The header's static_asserts
(the bound walker over the partial-round schedule) are compiled on the way.  The same for the width-32 form of the arity-4
MMCS (csrc/poseidon2_w32_f64.hip.h: p2wf_permute): the built-in diagonal's compile-time forms and the general path with
the built-in, a random and three adversarial diagonals."""
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


def test_fp64_w32_permutation_equals_integer(tmp_path):
    exe = str(tmp_path / "hp2wf")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "plonky3_recursion_amd", "csrc"),
                    os.path.join(ROOT, "tools", "microbench", "host_p2wf_check.cpp"), "-o", exe], check=True)
    # 2^13 random states per field, mask and diagonal (2 x 4 x 6 lines): a width-32 permutation costs about three width-16
    # ones, so this runs as long as the width-16 test above
    r = subprocess.run([exe, str(1 << 13)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if "mismatches" in ln]
    assert len(lines) == 48, r.stdout
    for ln in lines:
        assert "mismatches 0 of %d" % ((1 << 13) + 7) in ln, ln
