"""GPU: the plain bench.py run - headline only, --steps timed steps, and --dump-outputs writing the last timed proof,
the same bytes from run to run (the inputs are fixed by the arguments); and the bytes the bench's own path proves at
2^14 rows are the CPU oracle's (tests/golden/proof_digests_large.json)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_dumps_the_timed_proof(tmp_path):
    dumps = []
    for run in ("a", "b"):
        out_dir = tmp_path / run
        cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--log-height", "12",
               "--dump-outputs", str(out_dir), "--detail-out", str(tmp_path / f"detail_{run}.json")]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-3000:]
        line = json.loads(out.stdout.strip().splitlines()[-1])
        assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
        assert line["ms_per_step"] > 0 and line["value"] == line["ms_per_step"] and line["unit"] == "ms"
        assert line["roofline"] is None and line["cpu_baseline"] is None   # measurements of --full
        proof = np.load(out_dir / "proof.npy")
        assert proof.dtype == np.float32 and proof.size == line["config"]["proof_bytes"]
        assert hashlib.sha256(proof.astype(np.uint8).tobytes()).hexdigest() == line["proof_sha256"]
        dumps.append(proof)
    assert np.array_equal(dumps[0], dumps[1])


@pytest.mark.gpu
def test_plain_run_proves_the_oracles_bytes(tmp_path):
    """The bench builds its workload, context and packing itself: this ties that path - not a test's restatement of
    it - to the oracle's proof of the same layer (kb_headline_14 of tools/gen_proof_digests.py --large)."""
    pin = json.load(open(os.path.join(ROOT, "tests", "golden", "proof_digests_large.json")))["cases"]["kb_headline_14"]
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "1", "--warmup", "1", "--log-height", "14",
           "--detail-out", str(tmp_path / "detail.json")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["steps"] == 1 and line["warmup"] == 1 and line["config"]["log_height"] == 14
    # (the plain run does not verify its proof - `proof_verified` is None, --full does -: equality with the oracle's bytes,
    # which the oracle's verifier accepted when the pin was made, is the stronger statement)
    assert line["config"]["proof_bytes"] == pin["proof_bytes"]
    assert line["proof_sha256"] == pin["proof"]
