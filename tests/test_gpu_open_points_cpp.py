"""GPU: p3r::CosetInterpolation::open_points of include/p3r.hpp from compiled code (examples/open_points.cpp), in the
manner of tests/test_gpu_cpp_host.py: one mixed batch - heights 2^3, 2^6, 2^6 with a shared point, committed layout
with added_bits = 1 - written to a case file; the caller's values equal sum_k c_k z^k computed here with Python integers."""
import os
import subprocess

import numpy as np
import pytest

import test_gpu_open_points as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "open_points")


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_cpp_member_opens_a_mixed_batch(tmp_path, field, dc):
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "open_points"], check=True)
    p, g, added_bits = ref.P(field), ref.GEN(field), 1
    rng = np.random.default_rng(77 + dc)
    shared = ref.random_points(field, dc, 1, rng)
    shapes = [(8, 5), (64, 9), (64, 1)]
    points = [np.concatenate([shared, ref.random_points(field, dc, ref.cap(), rng)]), shared,
              np.concatenate([ref.random_points(field, dc, 1, rng), shared])]
    coefs = [rng.integers(0, p, size=s, dtype=np.uint32) for s in shapes]
    words = [added_bits, 0, 1, len(shapes)]
    for c, q in zip(coefs, points):
        m = ref.committed_layout(ref.evals_dense(field, c.shape[0], g, c).astype(np.uint32), added_bits, True, rng, p)
        words += [m.shape[0], m.shape[1], len(q)] + m.reshape(-1).tolist() + q.reshape(-1).tolist()
    case = tmp_path / "case.txt"
    case.write_text(" ".join(str(int(v)) for v in words))
    r = subprocess.run([EXE, field, str(dc), str(case)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok" and len(lines) == len(shapes) + 1
    for line, c, q in zip(lines, coefs, points):
        got = np.array(line.split(), dtype=np.uint64).reshape(len(q), c.shape[1], dc)
        for j, z in enumerate(q):
            assert np.array_equal(got[j], ref.want_dense(field, dc, c, z))
