"""GPU: byte parity with the CPU oracle under `max_log_arity = 4` at the bench's sizes.  For every entry of
tests/golden/proof_digests_arity16.json (tools/gen_proof_digests.py --arity16: the bench workload at 2^14, 2^16 and 2^20
KoalaBear rows and the arity-4-MMCS recursion layer at 2^16, each with a 16-ary FRI commit phase) the device prover must
give the oracle's preprocessed commitment, proof length and proof bytes through BOTH seams: `prove_next_layer` from the
circuit and its inputs, and `prove_all_tables` from the generator's traces.  On a mismatch the proof is decoded and the
first differing `sections` entry, in protocol order, is reported (as tests/test_gpu_large_digests.py does).  Reads the
fixture and the tree only; every case is a single prove per seam."""
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
PINS = json.load(open(gpd.ARITY16_PATH))["cases"]

pytestmark = pytest.mark.gpu


def sha(b):
    return hashlib.sha256(b).hexdigest()


def make_ctx(case):
    import plonky3_recursion_amd as p3r
    return p3r.Context(field=case["field"], ext_degree=case["d"], allow_unpinned_w32_defaults=True, **dict(gpd.FRI, **case["prm"]))


def assert_pinned(pin, case, commitment, proof, seam):
    assert sha(np.ascontiguousarray(commitment, dtype=np.uint32).tobytes()) == pin["prep_commit"], \
        f"{case['name']} ({seam}): the preprocessed commitment differs from the oracle's"
    if len(proof) != pin["proof_bytes"] or sha(proof) != pin["proof"]:
        pytest.fail(f"({seam}) " + gpd.describe_mismatch(pin, proof, case), pytrace=False)
    assert 4 in gpd.fri_log_arities(proof, case), f"{case['name']} ({seam}): no commit phase folds by 16"


@pytest.mark.parametrize("case", gpd.ARITY16_CASES, ids=[c["name"] for c in gpd.ARITY16_CASES])
def test_device_reproduces_the_arity16_digests(case):
    import harness_adapters as wl
    import plonky3_recursion_amd as p3r
    assert case["prm"]["max_log_arity"] == 4 and case["circuit"] and case["d"] == 4
    pin = PINS[case["name"]]
    arrs = gpd.large_arrays(case)
    assert gpd.workload_digest(arrs) == pin["workload"]
    tp = p3r.TablePacking().with_fri_params(gpd.FRI["log_final_poly_len"], gpd.FRI["log_blowup"])
    params = p3r.ProveNextLayerParams(table_packing=tp)
    backend = p3r.FriRecursionBackend()
    # seam 1: the circuit and its inputs - device preparation, device runner, prover
    ctx = make_ctx(case)
    cache = p3r.build_next_layer_prep(ctx, wl.circuit_from_arrays(arrs), backend, params)
    assert cache.prepared_circuit.prepared_on_device
    out = p3r.prove_next_layer(p3r.RecursionInput(circuit_inputs=wl.circuit_inputs_from_arrays(arrs)), ctx, backend, params,
                               prep=cache)
    assert_pinned(pin, case, cache.circuit_prover_data.preprocessed_commitment, out.proof.proof, "prove_next_layer from the circuit")
    cache.prover.verify_all_tables(out.proof)
    cache.prepared_circuit.free()
    ctx.close()
    # seam 2: the generator's traces, over a preparation made from its arrays
    ctx = make_ctx(case)
    cache = p3r.build_next_layer_prep(ctx, wl.circuit_prep_from_arrays(arrs), backend, params)
    cpd = cache.circuit_prover_data
    proof = cache.prover.prove_all_tables(wl.traces_from_arrays(arrs), cpd).proof
    assert_pinned(pin, case, cpd.preprocessed_commitment, proof, "prove_all_tables from traces")
    cpd.free()
    ctx.close()
