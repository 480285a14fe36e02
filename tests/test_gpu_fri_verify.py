"""GPU: Context.prove_fri on the device, p3r_fri_verify on the host with a challenger made from the configuration alone.
Inputs as in tests/test_fri_verify_host.py: heights 2^8 / 2^6 / 2^5 of low-degree polynomials, log_blowup 2, 3 queries.
Accepted for both fields, max_log_arity 1 / 2 / 4, both MMCS arities, the plain and the hiding MMCS, both challenge
degrees; every negative of the CPU list on a device-made proof; a proof of one configuration under another."""
import numpy as np
import pytest

import fri_verify_ref as fv
import test_fri_verify_host as host
from fri_verify_ref import P3R_EINVAL, P3R_EVERIFY

pytestmark = pytest.mark.gpu


def make_ctx(field, dc, prm):
    import plonky3_recursion_amd as p3r
    prm = dict(prm)
    extra = dict(allow_unpinned_w32_defaults=True) if prm["mmcs_arity"] == 4 else {}
    if prm.get("mmcs_salt_elems"):
        extra.update(zk_key=[1, 2, 3, 4, 5, 6, 7, 8], zk_deterministic=True)
    return p3r.Context(field=field, challenge_degree=dc, **prm, **extra)


def prove_on_device(ctx, ins):
    dev = [ctx.upload(a) for a in ins]
    ch = ctx.challenger()
    ch.observe([1, 2, 3])
    proof = ctx.prove_fri(ch, dev)
    for d in dev:
        d.free()
    for openings in proof.query_openings:   # an opened row as its 2^log_arity elements, as the CPU-made proofs carry it
        for o in openings:
            o.row = o.row.reshape(-1, ctx.challenge_degree)
    return proof, ch.sample()


CASES = [(f, la, ma, s, 4) for f in host.FIELDS for la in (1, 2, 4) for ma in (2, 4) for s in (0, 4)] + \
        [("koala-bear", la, ma, s, 5) for la, ma, s in ((2, 2, 0), (4, 4, 4))]


@pytest.mark.parametrize("field,max_log_arity,mmcs_arity,salt,dc", CASES)
def test_device_proofs_verify_on_the_host(field, max_log_arity, mmcs_arity, salt, dc):
    import plonky3_recursion_amd as p3r
    prm = host.params(max_log_arity=max_log_arity, mmcs_arity=mmcs_arity, mmcs_salt_elems=salt,
                      log_final_poly_len=0 if max_log_arity == 4 else 3, commit_pow_bits=2, query_pow_bits=3)
    ctx = make_ctx(field, dc, prm)
    ins = host.inputs_of(field, dc)
    proof, after = prove_on_device(ctx, ins)
    ch, betas, indices = host.verify(ctx.cfg, proof, ins)   # a host challenger from ctx.cfg: no device call in here
    assert indices == proof.query_indices
    probe = host.fresh(ctx.cfg)
    p3r.fri_verify(ctx.cfg, probe, proof, fv.input_values(ins, indices))
    assert probe.sample() == after, "the verifier's challenger is left where the prover's is"
    if salt:
        bad = fv.clone_proof(proof)
        bad.query_openings[0][0].salts = fv.bump(bad.query_openings[0][0].salts, 1, ctx.p)
        err = host.rejected(ctx.cfg, bad, fv.input_values(ins, indices))
        assert err.code == P3R_EVERIFY and "FRI commit phase 0 of query 0: Merkle root mismatch" in str(err)
    ctx.close()


@pytest.fixture(scope="module", params=host.FIELDS)
def proved(request):
    field = request.param
    prm = host.params(max_log_arity=2, log_final_poly_len=3, cap_height=2, commit_pow_bits=3, query_pow_bits=3)
    ctx = make_ctx(field, 4, prm)
    ins = host.inputs_of(field, 4)
    proof, _ = prove_on_device(ctx, ins)
    ctx.close()
    assert proof.commit_pow_witnesses[-1] > 0 and proof.query_pow_witness > 0, "pick another seed: a witness is 0"
    return field, prm, proof, ins


# the negatives are the CPU file's, on the device-made proof
test_each_rule_has_its_rejection = host.test_each_rule_has_its_rejection
test_schedule_phases_and_queries = host.test_schedule_phases_and_queries
test_a_proof_of_another_configuration_is_rejected = host.test_a_proof_of_another_configuration_is_rejected
test_malformed_views_are_refused = host.test_malformed_views_are_refused
