"""CPU: p3r_fri_verify and p3r_fri_verify_transcript on proofs made without the library - fri_ref.prove_fri_ref, the CPU
oracle's trees for the siblings (tests/fri_verify_ref.py) - with a host challenger made from the configuration alone.
Inputs: heights 2^8 / 2^6 / 2^5 of low-degree polynomials (log_blowup 2), so that every folded sum stays of low degree
and the final polynomial has 2^0 or 2^3 coefficients.  Every accepted case must leave the challenger where the prover's
is; every rule has one negative, rejected with P3R_EVERIFY and a message that names a rule; malformed views are refused
with P3R_EINVAL."""
import itertools
import re

import numpy as np
import pytest

import fri_ref
import fri_verify_ref as fv
from fri_verify_ref import P3R_EINVAL, P3R_EUNSUPPORTED, P3R_EVERIFY

FIELDS = ["koala-bear", "baby-bear"]
LOG_BLOWUP = 2
RULE = re.compile(r"proof of work|proof-of-work|Merkle root mismatch|final polynomial mismatch|log arity|commit phases|queries, expected")


def params(**over):
    prm = dict(log_blowup=LOG_BLOWUP, log_final_poly_len=3, max_log_arity=2, cap_height=0, commit_pow_bits=0, query_pow_bits=0,
               num_queries=3, mmcs_arity=2, fri_log_arities=None)
    prm.update(over)
    return prm


def config(field, dc, prm):
    import plonky3_recursion_amd as p3r
    extra = dict(allow_unpinned_w32_defaults=True) if prm["mmcs_arity"] == 4 else {}
    return p3r.make_config(field=field, challenge_degree=dc, **prm, **extra)


_inputs = {}


def inputs_of(field, dc):
    if (field, dc) not in _inputs:
        _inputs[field, dc] = fv.low_degree_inputs(field, dc, LOG_BLOWUP, np.random.default_rng(len(field) + dc))
    return _inputs[field, dc]


def prove(oracle, field, dc, prm):
    """(proof, inputs, the prover-side challenger after the proof)"""
    rch = fri_ref.ScriptChallenger(oracle, field, dc)
    rch.observe([1, 2, 3])
    ins = inputs_of(field, dc)
    return fv.prove_on_cpu(oracle, field, dc, prm, ins, rch), ins, rch


def fresh(cfg):
    import plonky3_recursion_amd as p3r
    ch = p3r.host_challenger(cfg)
    ch.observe([1, 2, 3])
    return ch


def verify(cfg, proof, ins):
    """The caller's two steps: the transcript on a clone gives the indices, then the inputs at them and the check."""
    import plonky3_recursion_amd as p3r
    ch = fresh(cfg)
    probe = ch.clone()
    betas, indices = p3r.fri_verify_transcript(cfg, probe, proof)
    p3r.fri_verify(cfg, ch, proof, fv.input_values(ins, indices))
    assert ch.sample() == probe.sample(), "both entries leave the challenger in one place"
    return ch, betas, indices


@pytest.mark.parametrize("field,max_log_arity,lf,cap_height,pow_bits",
                         list(itertools.product(FIELDS, [1, 2, 4], [0, 3], [0, 2], [0, 3])))
def test_cpu_made_proofs_are_accepted(oracle, field, max_log_arity, lf, cap_height, pow_bits):
    prm = params(max_log_arity=max_log_arity, log_final_poly_len=lf, cap_height=cap_height, commit_pow_bits=pow_bits, query_pow_bits=pow_bits)
    cfg, keep = config(field, 4, prm)
    proof, ins, rch = prove(oracle, field, 4, prm)
    want = {(1, 3): [1, 1, 1], (2, 3): [2, 1], (4, 3): [2, 1], (1, 0): [1] * 6, (2, 0): [2, 1, 2, 1], (4, 0): [2, 1, 3]}[max_log_arity, lf]
    assert proof.log_arities == want
    ch, betas, indices = verify(cfg, proof, ins)
    assert indices == proof.query_indices and betas.shape == (len(want), 4)
    # ch was sampled once in verify(); the prover-side challenger must agree from the same place
    probe = fresh(cfg)
    import plonky3_recursion_amd as p3r
    p3r.fri_verify(cfg, probe, proof, fv.input_values(ins, indices))
    assert probe.sample() == rch.sample(), "the challenger is left where the prover's is"


@pytest.mark.parametrize("name,field,dc,over", [
    ("quintic", "koala-bear", 5, dict()),
    ("arity4_mmcs", "baby-bear", 4, dict(mmcs_arity=4, max_log_arity=4, log_final_poly_len=0)),
    ("schedule", "koala-bear", 4, dict(fri_log_arities=[1, 1, 1], max_log_arity=3)),
])
def test_variations_are_accepted(oracle, name, field, dc, over):
    prm = params(**over)
    cfg, keep = config(field, dc, prm)
    proof, ins, rch = prove(oracle, field, dc, prm)
    ch, betas, indices = verify(cfg, proof, ins)
    assert betas.shape[1] == dc


@pytest.fixture(scope="module", params=FIELDS)
def proved(request, oracle):
    field = request.param
    prm = params(max_log_arity=2, log_final_poly_len=3, cap_height=2, commit_pow_bits=3, query_pow_bits=3)
    proof, ins, rch = prove(oracle, field, 4, prm)
    # the prover's witnesses are the smallest the check accepts: the one below is certainly refused
    assert proof.commit_pow_witnesses[-1] > 0 and proof.query_pow_witness > 0, "pick another seed: a witness is 0"
    return field, prm, proof, ins


def rejected(cfg, proof, views):
    import plonky3_recursion_amd as p3r
    ch, twin = fresh(cfg), fresh(cfg)
    with pytest.raises(p3r.P3rError) as e:
        p3r.fri_verify(cfg, ch, proof, views)
    assert ch.sample() == twin.sample(), "a refused call leaves the challenger as it was"
    return e.value


@pytest.mark.parametrize("name", ["cap_word", "commit_pow", "query_pow", "final_coeff", "row_word", "sibling", "input_value"])
def test_each_rule_has_its_rejection(proved, name):
    field, prm, proof, ins = proved
    cfg, keep = config(field, 4, prm)
    p = fv.seam.P(field)
    bad, views = fv.clone_proof(proof), fv.input_values(ins, proof.query_indices)
    if name == "commit_pow":
        bad.commit_pow_witnesses[-1] -= 1
        want = "commit proof-of-work of phase %d" % (len(bad.log_arities) - 1)
    elif name == "query_pow":
        bad.query_pow_witness -= 1
        want = "query proof of work"
    else:
        mutate, want = fv.mutations(p)[name]
        mutate(bad, views)
    err = rejected(cfg, bad, views)
    assert err.code == P3R_EVERIFY, str(err)
    assert RULE.search(str(err)) and (want is None or want in str(err)), str(err)
    if name == "input_value":
        assert "final polynomial mismatch" in str(err) or "Merkle root mismatch" in str(err)


@pytest.mark.parametrize("field", FIELDS)
def test_the_final_polynomial_rule_names_itself(oracle, field):
    """A changed coefficient moves the query indices (the final polynomial is observed before they are sampled).  An honest
    prover's openings at the NEW indices, and the inputs there, pass every Merkle check and every fold: what is left is the
    final polynomial, which no longer is the end of the chain."""
    import plonky3_recursion_amd as p3r
    prm = params(max_log_arity=2, log_final_poly_len=3, cap_height=1)   # no proof of work: nothing else can reject
    cfg, keep = config(field, 4, prm)
    rch = fri_ref.ScriptChallenger(oracle, field, 4)
    rch.observe([1, 2, 3])
    ins, kept = inputs_of(field, 4), []
    proof = fv.prove_on_cpu(oracle, field, 4, prm, ins, rch, keep=kept)
    bad = fv.clone_proof(proof)
    bad.final_poly = fv.bump(bad.final_poly, 4 + 1, fv.seam.P(field))   # coefficient 1, word 1
    _, indices = p3r.fri_verify_transcript(cfg, fresh(cfg), bad)
    assert indices != proof.query_indices
    bad.query_indices = indices
    bad.query_openings = fv.open_at(*kept[0], indices, 4)
    err = rejected(cfg, bad, fv.input_values(ins, indices))
    assert err.code == P3R_EVERIFY and "query 0: final polynomial mismatch" in str(err), str(err)
    # the same openings under the unchanged polynomial at its own indices are accepted
    verify(cfg, proof, ins)


def test_schedule_phases_and_queries(proved):
    import plonky3_recursion_amd as p3r
    field, prm, proof, ins = proved
    cfg, keep = config(field, 4, prm)
    views = fv.input_values(ins, proof.query_indices)
    # an arity the schedule does not allow: 2^8 -> 2^6 by two folds of 2 where the rule folds by 4 (well-formed: the
    # phases still end at the final height)
    bad = fv.clone_proof(proof)
    assert bad.log_arities == [2, 1]
    bad.log_arities = [1, 1, 1]
    bad.commit_phase_caps.append(bad.commit_phase_caps[-1])
    bad.commit_pow_witnesses.append(0)
    for o in bad.query_openings:
        o.append(o[-1])
    # judged without proofs of work, whose checks come first in the replay: the schedule rule names itself
    cfg0, keep0 = config(field, 4, dict(prm, commit_pow_bits=0, query_pow_bits=0))
    err = rejected(cfg0, bad, views)
    assert err.code == P3R_EVERIFY and "3 commit phases, expected 2" in str(err), str(err)
    # above max_log_arity: the transcript entry already says so
    bad = fv.clone_proof(proof)
    bad.log_arities = [3]
    fv.drop_phase(bad)
    bad.log_arities = [3]
    with pytest.raises(p3r.P3rError) as e:
        p3r.fri_verify_transcript(cfg, fresh(cfg), bad)
    assert e.value.code == P3R_EVERIFY and "log arity 3 of phase 0" in str(e.value)
    # a phase dropped
    bad = fv.clone_proof(proof)
    fv.drop_phase(bad)
    err = rejected(cfg, bad, views)
    assert err.code == P3R_EVERIFY and "commit phases" in str(err), str(err)
    # a query dropped
    bad = fv.clone_proof(proof)
    fv.drop_query(bad)
    err = rejected(cfg, bad, [(l, v[:2]) for l, v in views])
    assert err.code == P3R_EVERIFY and "2 queries, expected 3" in str(err), str(err)
    # and the proof itself is still fine
    verify(cfg, proof, ins)


def test_a_proof_of_another_configuration_is_rejected(proved):
    field, prm, proof, ins = proved
    views = fv.input_values(ins, proof.query_indices)
    for over in (dict(cap_height=0), dict(max_log_arity=1), dict(log_final_poly_len=2), dict(query_pow_bits=20)):
        cfg, keep = config(field, 4, dict(prm, **over))
        err = rejected(cfg, proof, views)
        assert err.code in (P3R_EVERIFY, P3R_EINVAL), (over, str(err))
        if "cap_height" not in over and "log_final_poly_len" not in over:   # those two change a length: malformed
            assert err.code == P3R_EVERIFY, (over, str(err))


def test_malformed_views_are_refused(proved):
    import plonky3_recursion_amd as p3r
    field, prm, proof, ins = proved
    cfg, keep = config(field, 4, prm)
    p = fv.seam.P(field)
    views = fv.input_values(ins, proof.query_indices)

    def refused(bad, bad_views=None, text=None):
        err = rejected(cfg, bad, views if bad_views is None else bad_views)
        assert err.code == P3R_EINVAL and (text is None or text in str(err)), str(err)

    for where in ("cap", "final", "row", "sibling", "pow", "input"):
        bad, bv = fv.clone_proof(proof), list(views)
        if where == "cap":
            bad.commit_phase_caps[1][0, 0] = p
        elif where == "final":
            bad.final_poly[0, 0] = 0xFFFFFFFF
        elif where == "row":
            o = bad.query_openings[0][0]
            pos = bad.query_indices[0] & (o.row.shape[0] - 1)
            o.row[(pos + 1) % o.row.shape[0], 0] = p
        elif where == "sibling":
            bad.query_openings[2][1].siblings[0, 7] = p
        elif where == "pow":
            bad.query_pow_witness = p
        else:
            a = bv[2][1].copy()
            a[0, 0] = p
            bv[2] = (bv[2][0], a)
        refused(bad, bv, "non-canonical")
    # short arrays
    bad = fv.clone_proof(proof)
    bad.final_poly = bad.final_poly[:-1]
    refused(bad, text="final_poly holds")
    bad = fv.clone_proof(proof)
    bad.commit_phase_caps[0] = bad.commit_phase_caps[0][:-1]
    refused(bad, text="commit_caps holds")
    bad = fv.clone_proof(proof)
    bad.commit_pow_witnesses.pop()
    refused(bad, text="commit_pow holds")
    bad = fv.clone_proof(proof)
    bad.query_openings[1][0].siblings = bad.query_openings[1][0].siblings[:-1]
    refused(bad, text="sibling words")
    bad = fv.clone_proof(proof)
    bad.query_openings[1][1].row = bad.query_openings[1][1].row[:0]
    refused(bad)
    bad = fv.clone_proof(proof)
    bad.query_openings[2].pop()
    refused(bad, text="openings holds")
    # inputs: short, a height above log_max_height, repeated, out of order, none at the top
    refused(proof, [views[0], (views[1][0], views[1][1][:2]), views[2]], "input 1 holds")
    refused(proof, [(9, views[0][1])] + views[1:], "above log_max_height")
    refused(proof, [views[0], views[1], views[1]], "one input per height")
    refused(proof, [views[0], views[2], views[1]], "one input per height")
    refused(proof, views[1:], "tallest input comes first")
    refused(proof, [], "no input")
    # a challenger of another field or challenge degree
    other, keep2 = config("baby-bear" if field == "koala-bear" else "koala-bear", 4, prm)
    ch = p3r.host_challenger(other)
    with pytest.raises(p3r.P3rError) as e:
        p3r.fri_verify(cfg, ch, proof, views)
    assert e.value.code == P3R_EINVAL and "another field" in str(e.value)
    # zk configurations are out of scope; the hiding MMCS is not
    zk, keep3 = p3r.make_config(field=field, zk=1, **{k: v for k, v in prm.items()})
    with pytest.raises(p3r.P3rError) as e:
        p3r.fri_verify(zk, fresh(cfg), proof, views)
    assert e.value.code == P3R_EUNSUPPORTED
    # NULL arguments
    from plonky3_recursion_amd import _lib
    lib = _lib.load()
    assert lib.p3r_fri_verify(None, None, None, None, 0) == P3R_EINVAL
    assert lib.p3r_fri_verify_transcript(_lib.C.byref(cfg), fresh(cfg).h, None, None, None) == P3R_EINVAL
