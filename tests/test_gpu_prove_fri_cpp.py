"""GPU: p3r::DuplexChallenger, p3r::TwoAdicFriFolding::leaf_view and p3r::prove_fri of include/p3r.hpp from compiled code
(examples/prove_fri.cpp), in the manner of tests/test_gpu_fri_seam_cpp.py: two traces of different heights go through
LDE, commit, open_points, reduced openings and prove_fri in the example, with the library's challenger throughout; every
printed word equals what the Python mirror gets from the same steps."""
import os
import subprocess

import numpy as np
import pytest

import field_ref
import test_gpu_fri_seam as seam
import test_gpu_open_points as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "prove_fri")
FRI = dict(log_blowup=1, max_log_arity=2, log_final_poly_len=2, commit_pow_bits=2, query_pow_bits=4, num_queries=3)


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_cpp_prove_fri_prints_the_python_mirrors_words(tmp_path, field, dc):
    import plonky3_recursion_amd as p3r
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "prove_fri"], check=True)
    p, g = ref.P(field), ref.GEN(field)
    rng = np.random.default_rng(21 + dc)
    traces = [rng.integers(0, p, size=(h, w), dtype=np.uint32) for h, w in ((1 << 6, 3), (1 << 4, 2))]
    pts = [seam.rand_ext(field, dc, rng, 2), seam.rand_ext(field, dc, rng, 1)]
    words = [FRI[k] for k in ("log_blowup", "max_log_arity", "log_final_poly_len", "commit_pow_bits", "query_pow_bits", "num_queries")]
    words += [g, len(traces)]
    for t, q in zip(traces, pts):
        words += [t.shape[0], t.shape[1], len(q)] + t.reshape(-1).tolist() + q.reshape(-1).tolist()
    case = tmp_path / "case.txt"
    case.write_text(" ".join(str(int(v)) for v in words))
    r = subprocess.run([EXE, field, str(dc), str(case)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l.split() for l in r.stdout.strip().split("\n")]
    assert lines[-1] == ["ok"]

    # the same steps through the Python layer
    ctx = p3r.Context(field=field, challenge_degree=dc, cap_height=0, **FRI)
    dts = [ctx.upload(t) for t in traces]
    ldes = [ctx.coset_lde_batch_device(t, FRI["log_blowup"], g) for t in dts]
    cap, tree = ctx.commit_device(ldes)
    ch = ctx.challenger()
    ch.observe(cap.reshape(-1))
    vals = ctx.open_points_device(ldes, pts, added_bits=FRI["log_blowup"])
    for v in vals:
        ch.observe(v.reshape(-1))
    alpha = ch.sample_ext()
    ros = ctx.fri_reduce_device(ldes, pts, vals, alpha)
    assert [d.shape[0] for d in ros] == [1 << 7, 1 << 5]
    proof = ctx.prove_fri(ch, ros)
    want = [["commit"] + cap.reshape(-1).tolist(), ["alpha"] + alpha.tolist(), ["caps", len(proof.commit_phase_caps)]]
    want += [["cap"] + c.reshape(-1).tolist() for c in proof.commit_phase_caps]
    want += [["pow"] + proof.commit_pow_witnesses, ["arities"] + proof.log_arities, ["final", len(proof.final_poly)]]
    want += [["coeff"] + row.tolist() for row in proof.final_poly]
    want += [["query_pow", proof.query_pow_witness], ["indices"] + proof.query_indices]
    want += [["row"] + o.row.tolist() for q in proof.query_openings for o in q]
    want += [["ok"]]
    assert lines == [[str(v) for v in l] for l in want]
    assert len(proof.log_arities) >= 2 and proof.final_poly.shape == (4, dc)
    tree.free()
    for d in dts + ldes + ros:
        d.free()
    ctx.close()
