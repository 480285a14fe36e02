"""GPU: p3r::CosetInterpolation::reduced_openings and p3r::TwoAdicFriFolding::fold_matrix of include/p3r.hpp from compiled
code (examples/fri_seam.cpp), in the manner of tests/test_gpu_open_points_cpp.py: the two 2^6-row traces (widths 9 and 2)
of the composition test go through commit -> open_points -> reduced openings -> folds -> p3r_dft in the example, with the
points, alpha, schedule and betas of a case file; the printed final coefficients equal those the Python layer gets from
the same steps, and the high ones are zero."""
import os
import subprocess

import numpy as np
import pytest

import field_ref
import test_gpu_fri_seam as seam
import test_gpu_open_points as ref

pytestmark = pytest.mark.gpu
ctxs = ref.ctxs
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "fri_seam")


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_cpp_members_reduce_and_fold_to_the_final_polynomial(ctxs, tmp_path, field, dc):
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "fri_seam"], check=True)
    ctx, p, g, log_blowup, h = ctxs(field, dc), ref.P(field), ref.GEN(field), 1, 1 << 6
    E = ref.ext(field, dc)
    rng = np.random.default_rng(88 + dc)
    traces = [ref.evals_dense(field, h, 1, rng.integers(0, p, size=(h, w), dtype=np.uint32)).astype(np.uint32) for w in (9, 2)]
    z = [int(v) for v in seam.rand_ext(field, dc, rng)]
    pts = np.array([z, E.scale(z, field_ref.two_adic_generator(field, 6))], dtype=np.uint32)
    alpha = seam.rand_ext(field, dc, rng)
    phases = [(2, seam.rand_ext(field, dc, rng)), (1, seam.rand_ext(field, dc, rng)), (1, seam.rand_ext(field, dc, rng))]   # 2^7 -> 2^3
    words = [log_blowup, g, len(traces)]
    for t in traces:
        words += [t.shape[0], t.shape[1], len(pts)] + t.reshape(-1).tolist() + pts.reshape(-1).tolist()
    words += alpha.tolist() + [len(phases)]
    for la, beta in phases:
        words += [la] + beta.tolist()
    case = tmp_path / "case.txt"
    case.write_text(" ".join(str(int(v)) for v in words))
    r = subprocess.run([EXE, field, str(dc), str(case)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok" and len(lines) == 1 + 8 + 1
    got = np.array([l.split() for l in lines[1:-1]], dtype=np.uint64).astype(np.uint32)
    # the same steps through the Python layer
    dts = [ctx.upload(t) for t in traces]
    ldes = [ctx.coset_lde_batch_device(t, log_blowup, g) for t in dts]
    cap, tree = ctx.commit_device(ldes)
    assert np.array_equal(np.array(lines[0].split(), dtype=np.uint64), cap.reshape(-1))
    vals = ctx.open_points_device(ldes, [pts, pts], added_bits=log_blowup)
    cur, = ctx.fri_reduce_device(ldes, [pts, pts], vals, alpha)
    for la, beta in phases:
        nxt = ctx.fri_fold_device(cur, la, beta)
        cur.free()
        cur = nxt
    coef, = ctx.dft_batch_device([cur], inverse=True, bit_reversed=True, shifts=[1])
    want = coef.download()
    tree.free()
    for d in dts + ldes + [cur, coef]:
        d.free()
    assert want.shape == (8, dc) and np.array_equal(got, want)
    assert not got[4:].any() and got[:4].any(), "degree < 4: the high coefficients are zero"
