"""GPU: byte parity with the CPU oracle at the sizes the metric and the bench legs are quoted on.  For every entry of
tests/golden/proof_digests_large.json (tools/gen_proof_digests.py --large; 2^14 to 2^20 rows, the reference examples' FRI
defaults) the device prover must give the oracle's preprocessed commitment, proof length and proof bytes - through BOTH
seams where the layer exists as a circuit: `prove_next_layer` from the circuit and its inputs (device preparation, device
runner), and `prove_all_tables` from the generator's traces over a preparation made from its arrays.  A proof that
merely verifies is not enough here: another valid ALU lane schedule, a non-minimal proof-of-work witness or another legal
FRI arity schedule changes the bytes.  On a mismatch the proof is decoded and the first differing `sections` entry, in
protocol order, is reported.  Reads the fixture and the tree only; every case is a single prove per seam."""
import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("gen_proof_digests", os.path.join(ROOT, "tools", "gen_proof_digests.py"))
gpd = importlib.util.module_from_spec(spec)
spec.loader.exec_module(gpd)
PINS = json.load(open(gpd.LARGE_PATH))["cases"]

pytestmark = pytest.mark.gpu


def sha(b):
    return hashlib.sha256(b).hexdigest()


def make_ctx(case):
    """The device twin of gpd.large_params(case): under ZK / salts the deterministic mode with the case's key, so that
    proof number 0 is the oracle's (the mechanism of tests/test_gpu_zk.py::make_ctx)."""
    import plonky3_recursion_amd as p3r
    kw = dict(gpd.FRI, **case["prm"])
    if "zk_key" in kw:
        kw.update(zk_key=list(kw["zk_key"]), zk_deterministic=True)
    return p3r.Context(field=case["field"], ext_degree=case["d"], allow_unpinned_w32_defaults=True, **kw)


def assert_pinned(pin, case, commitment, proof, seam):
    assert sha(np.ascontiguousarray(commitment, dtype=np.uint32).tobytes()) == pin["prep_commit"], \
        f"{case['name']} ({seam}): the preprocessed commitment differs from the oracle's"
    if len(proof) != pin["proof_bytes"] or sha(proof) != pin["proof"]:
        pytest.fail(f"({seam}) " + gpd.describe_mismatch(pin, proof, case), pytrace=False)


@pytest.mark.parametrize("case", gpd.LARGE_CASES, ids=[c["name"] for c in gpd.LARGE_CASES])
def test_device_reproduces_the_large_digests(case):
    import harness_adapters as wl
    import plonky3_recursion_amd as p3r
    pin = PINS[case["name"]]
    d = case["d"]
    arrs = gpd.large_arrays(case)
    assert gpd.workload_digest(arrs) == pin["workload"]
    tp = p3r.TablePacking().with_fri_params(gpd.FRI["log_final_poly_len"], gpd.FRI["log_blowup"])
    params = p3r.ProveNextLayerParams(table_packing=tp)
    backend = p3r.FriRecursionBackendD5() if d == 5 else p3r.FriRecursionBackend()
    zk = bool(case["prm"].get("zk"))
    if case["circuit"]:
        # seam 1: the circuit and its inputs - device preparation, device runner, prover
        ctx = make_ctx(case)
        cache = p3r.build_next_layer_prep(ctx, wl.circuit_from_arrays(arrs), backend, params)
        assert cache.prepared_circuit.prepared_on_device
        out = p3r.prove_next_layer(p3r.RecursionInput(circuit_inputs=wl.circuit_inputs_from_arrays(arrs)), ctx, backend,
                                   params, prep=cache)
        assert_pinned(pin, case, cache.circuit_prover_data.preprocessed_commitment, out.proof.proof, "prove_next_layer from the circuit")
        cache.prepared_circuit.free()
        ctx.close()
    # seam 2: the generator's traces, over a preparation made from its arrays
    ctx = make_ctx(case)
    cache = p3r.build_next_layer_prep(ctx, wl.circuit_prep_from_arrays(arrs, ext_degree=d), backend, params)
    cpd = cache.circuit_prover_data
    traces = wl.traces_from_arrays(arrs, ext_degree=d)
    proof = cache.prover.prove_all_tables(traces, cpd).proof
    assert_pinned(pin, case, cpd.preprocessed_commitment, proof, "prove_all_tables from traces")
    if zk:
        assert ctx.zk_nonce == 1
        second = cache.prover.prove_all_tables(traces, cpd).proof     # proof number 1: other masks, other bytes
        assert ctx.zk_nonce == 2 and second != proof and sha(second) != pin["proof"]
    cpd.free()
    ctx.close()
