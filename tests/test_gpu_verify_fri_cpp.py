"""GPU: p3r::HostChallenger, p3r::verify_fri_transcript and p3r::verify_fri of include/p3r.hpp from compiled code
(examples/verify_fri.cpp), in the manner of tests/test_gpu_prove_fri_cpp.py: two traces of different heights are proved
on the device with p3r::prove_fri and verified on the host; the example exits 0, prints the query indices the Python
mirror gets from the same steps, "accepted", and the refusal of a proof with one flipped sibling word."""
import os
import subprocess

import numpy as np
import pytest

import test_gpu_fri_seam as seam
import test_gpu_open_points as ref
from test_gpu_prove_fri_cpp import FRI

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "verify_fri")
P3R_EVERIFY = -7


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_cpp_verify_fri_accepts_and_shows_the_refusal(tmp_path, field, dc):
    import plonky3_recursion_amd as p3r
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "verify_fri"], check=True)
    p, g = ref.P(field), ref.GEN(field)
    rng = np.random.default_rng(31 + dc)
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
    lines = r.stdout.strip().split("\n")
    assert lines[1] == "accepted" and lines[-1] == "ok" and len(lines) == 4
    assert lines[2].startswith("refused %d: " % P3R_EVERIFY) and "FRI commit phase 0 of query 0: Merkle root mismatch" in lines[2], lines[2]

    # the same steps through the Python layer: the verifier's indices are the prover's
    ctx = p3r.Context(field=field, challenge_degree=dc, cap_height=0, **FRI)
    dts = [ctx.upload(t) for t in traces]
    ldes = [ctx.coset_lde_batch_device(t, FRI["log_blowup"], g) for t in dts]
    cap, tree = ctx.commit_device(ldes)
    ch = ctx.challenger()
    ch.observe(cap.reshape(-1))
    values, proof, openings = ctx.pcs_open(ch, [(tree, ldes, pts)])
    assert lines[0].split() == ["indices"] + [str(i) for i in proof.query_indices]
    tree.free()
    for d in dts + ldes:
        d.free()
    ctx.close()
