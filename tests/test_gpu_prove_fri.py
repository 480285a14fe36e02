"""GPU: Context.prove_fri - p3_fri::prover::prove_fri composed from the public calls - against the independent restatement
of tests/fri_ref.py (fold2 on Python integers, the schedule rule, the CPU oracle's MMCS on reshaped host matrices and the
CPU oracle's challenger).  Caps, proof-of-work witnesses, log arities, query indices and opened leaf rows are compared
for equality; the final polynomial is checked by evaluating it at the last vector's points (and against known
coefficients where the input is a low-degree polynomial); the siblings are checked with p3r_mmcs_verify.

Also here, because it needs a context: p3r_fri_log_arity over all (log_cur, log_final, log_next, max_log_arity) with
log_cur <= 10 against the three-line rule."""
import numpy as np
import pytest

import field_ref
import fri_ref
import test_gpu_fri_seam as seam
import test_gpu_open_points as ref

pytestmark = pytest.mark.gpu
P3R_EINVAL = -1
FIELDS = ["koala-bear", "baby-bear"]
BASE = dict(log_blowup=0, log_final_poly_len=5, max_log_arity=2, cap_height=0, commit_pow_bits=0, query_pow_bits=0,
            num_queries=3, mmcs_arity=2, fri_log_arities=None)


def make_ctx(field, dc=4, **over):
    import plonky3_recursion_amd as p3r
    prm = dict(BASE, **over)
    extra = dict(allow_unpinned_w32_defaults=True) if prm["mmcs_arity"] == 4 else {}
    for k in ("mmcs_salt_elems", "zk_key", "zk_deterministic"):
        if k in prm:
            extra[k] = prm.pop(k)
    return p3r.Context(field=field, challenge_degree=dc, **prm, **extra), prm


def random_inputs(field, dc, logs, rng):
    return [rng.integers(0, ref.P(field), size=(1 << l, dc), dtype=np.uint32) for l in logs]


def run_and_compare(ctx, orc, field, dc, prm, host_inputs, hiding=False):
    import plonky3_recursion_amd as p3r
    dev = [ctx.upload(a) for a in host_inputs]
    ch = ctx.challenger()
    ch.observe([1, 2, 3])
    proof = ctx.prove_fri(ch, dev)
    after = ch.sample()
    for d, a in zip(dev, host_inputs):
        assert np.array_equal(d.download(), a), "the inputs are left as they are"
        d.free()
    rch = fri_ref.ScriptChallenger(orc, field, dc)
    rch.observe([1, 2, 3])
    want = fri_ref.prove_fri_ref(orc, field, dc, prm, host_inputs, rch, proof.final_poly,
                                 given_caps=proof.commit_phase_caps if hiding else None)
    assert proof.log_arities == want.arities
    assert len(proof.commit_phase_caps) == len(want.caps)
    for got, exp in zip(proof.commit_phase_caps, want.caps):
        assert np.array_equal(got, exp)
    assert proof.commit_pow_witnesses == want.pow
    assert want.final_ok, "the final polynomial does not evaluate to the last folded vector"
    assert proof.query_pow_witness == want.query_pow
    assert proof.query_indices == want.indices
    assert after == rch.sample(), "the challenger is left where the restatement's is"
    S = prm.get("mmcs_salt_elems", 0)
    assert len(proof.query_openings) == prm["num_queries"]
    for q, (index, openings) in enumerate(zip(proof.query_indices, proof.query_openings)):
        shift = 0
        assert len(openings) == len(want.arities)
        for ph, o in enumerate(openings):
            shift += want.arities[ph]
            assert np.array_equal(o.row, want.rows[q][ph]), (q, ph)
            dims = [want.leaves[ph].shape]
            if S:
                assert o.salts.shape == (1, S)
                p3r.mmcs_verify(ctx.cfg, proof.commit_phase_caps[ph], dims, index >> shift, o.row, o.siblings, salts=o.salts)
                with pytest.raises(p3r.P3rError):
                    p3r.mmcs_verify(ctx.cfg, proof.commit_phase_caps[ph], dims, index >> shift, o.row, o.siblings,
                                    salts=(o.salts + 1) % ref.P(field))
            else:
                assert o.salts is None
                p3r.mmcs_verify(ctx.cfg, proof.commit_phase_caps[ph], dims, index >> shift, o.row, o.siblings)
    return proof, want


# ---- case 1: the backbone.  Random words are no low-degree polynomial, so the final length is the last height
# (log_final_poly_len = 5, log_blowup = 0): no coefficient lies above it and the degree check cannot fire
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("max_log_arity", [1, 2, 4])
def test_backbone_three_heights(oracle, field, max_log_arity):
    ctx, prm = make_ctx(field, max_log_arity=max_log_arity)
    inputs = random_inputs(field, 4, (8, 6, 5), np.random.default_rng(40 + max_log_arity))
    proof, want = run_and_compare(ctx, oracle, field, 4, prm, inputs)
    # 2^8 -> 2^6 -> 2^5, never passing an input height
    assert proof.log_arities == {1: [1, 1, 1], 2: [2, 1], 4: [2, 1]}[max_log_arity]
    assert proof.final_poly.shape == (32, 4) and want.last.shape == (32, 4)
    ctx.close()


# ---- case 2: a low-degree input: the final polynomial is the polynomial
@pytest.mark.parametrize("field", FIELDS)
def test_low_degree_input_gives_its_coefficients(oracle, field):
    import plonky3_recursion_amd as p3r
    dc, p = 4, ref.P(field)
    ctx, prm = make_ctx(field, log_blowup=2, log_final_poly_len=3, max_log_arity=2)
    rng = np.random.default_rng(7)
    coef = rng.integers(0, p, size=(8, dc), dtype=np.uint32)
    evals = fri_ref.eval_at_rows(field, coef, 1 << 7)   # over <w_2^7>, bit-reversed
    # final height 2^5: one fold by 4.  fold(f)(y) at arity 4 of f = sum_j x^j f_j(x^4) is sum_j beta^j f_j(y): degree < 2
    proof, want = run_and_compare(ctx, oracle, field, dc, prm, [evals])
    assert proof.log_arities == [2]
    E = ref.ext(field, dc)
    rch = fri_ref.ScriptChallenger(oracle, field, dc)
    rch.observe([1, 2, 3])
    rch.observe(proof.commit_phase_caps[0].reshape(-1))
    beta = [int(v) for v in rch.sample_ext()]
    bp = [E.one(0), beta, E.mul(beta, beta), E.mul(E.mul(beta, beta), beta)]
    folded = []
    for i in range(8):
        acc = E.zero(0)
        for j in range(4):
            k = 4 * i + j
            if k < 8:
                acc = E.add(acc, E.mul(bp[j], [int(v) for v in coef[k]]))
        folded.append([int(v) for v in acc])
    assert np.array_equal(proof.final_poly, np.array(folded, dtype=np.uint32)), "the final polynomial is the folded polynomial"
    assert proof.final_poly[2:].any() == False and proof.final_poly[:2].any()   # noqa: E712
    # the identity fold at no phase: a context whose final height is the input's returns the coefficients themselves
    ctx0, prm0 = make_ctx(field, log_blowup=4, log_final_poly_len=3)
    proof0, _ = run_and_compare(ctx0, oracle, field, dc, prm0, [evals])
    assert proof0.log_arities == [] and np.array_equal(proof0.final_poly, coef)
    # one flipped word: the vector is no longer of low degree
    bad = evals.copy()
    bad[5, 1] = (int(bad[5, 1]) + 1) % p
    d = ctx0.upload(bad)
    with pytest.raises(p3r.P3rError) as e:
        ctx0.prove_fri(ctx0.challenger(), [d])
    assert e.value.code == P3R_EINVAL and "FRI final polynomial has degree >= 2^3" in str(e.value)
    with pytest.raises(p3r.P3rError):
        ctx0.fri_final_poly_device(d)
    d.free()
    ctx.close()
    ctx0.close()


# ---- case 3: each variation once
VARIATIONS = {
    "pow": ("koala-bear", 4, dict(commit_pow_bits=3, query_pow_bits=5)),
    "cap_height": ("baby-bear", 4, dict(cap_height=1)),
    "schedule": ("koala-bear", 4, dict(fri_log_arities=[1, 1, 1], max_log_arity=3)),
    "quintic": ("koala-bear", 5, dict()),
    "arity4": ("baby-bear", 4, dict(mmcs_arity=4)),
}


@pytest.mark.parametrize("name", sorted(VARIATIONS))
def test_variations(oracle, name):
    field, dc, over = VARIATIONS[name]
    ctx, prm = make_ctx(field, dc, **over)
    inputs = random_inputs(field, dc, (8, 6, 5), np.random.default_rng(len(name)))
    proof, _ = run_and_compare(ctx, oracle, field, dc, prm, inputs)
    if name == "schedule":
        assert proof.log_arities == [1, 1, 1]
    if name == "pow":
        assert len(proof.commit_pow_witnesses) == len(proof.log_arities)
    ctx.close()


def test_hiding_context(oracle):
    field, dc = "koala-bear", 4
    ctx, prm = make_ctx(field, dc, mmcs_salt_elems=4, zk_key=[1, 2, 3, 4, 5, 6, 7, 8], zk_deterministic=True)
    prm["mmcs_salt_elems"] = 4
    inputs = random_inputs(field, dc, (8, 6, 5), np.random.default_rng(99))
    ctx.zk_nonce = 7
    first, _ = run_and_compare(ctx, oracle, field, dc, prm, inputs, hiding=True)
    assert ctx.zk_nonce == 7 + len(first.log_arities), "every commit phase is a public commit on a hiding context"
    ctx.zk_nonce = 7
    again, _ = run_and_compare(ctx, oracle, field, dc, prm, inputs, hiding=True)
    for a, b in zip(first.commit_phase_caps, again.commit_phase_caps):
        assert np.array_equal(a, b)
    assert first.query_indices == again.query_indices
    other, _ = run_and_compare(ctx, oracle, field, dc, prm, inputs, hiding=True)   # the nonce moved on: other salts
    assert not np.array_equal(other.commit_phase_caps[0], first.commit_phase_caps[0])
    ctx.close()


# ---- case 4: what raises
def test_schedules_that_do_not_fit_raise(oracle):
    import plonky3_recursion_amd as p3r
    field, dc = "koala-bear", 4
    rng = np.random.default_rng(4)

    def raises(ctx, logs, text):
        dev = [ctx.upload(a) for a in random_inputs(field, dc, logs, rng)]
        with pytest.raises(p3r.P3rError) as e:
            ctx.prove_fri(ctx.challenger(), dev)
        assert e.value.code == P3R_EINVAL and text in str(e.value), str(e.value)
        for d in dev:
            d.free()

    # an explicit schedule that would pass the input height 2^6 on the way from 2^8: never reached
    ctx, _ = make_ctx(field, dc, fri_log_arities=[3], max_log_arity=3)
    raises(ctx, (8, 6), "fri_log_arities does not fit the proof: phase 0 at height 2^8")
    ctx.close()
    # a schedule that ends before the final height
    ctx, _ = make_ctx(field, dc, fri_log_arities=[2], max_log_arity=3)
    raises(ctx, (8, 6), "fri_log_arities does not fit the proof: phase 1 at height 2^6")
    ctx.close()
    # an input below the final height is never rolled in; inputs out of order are refused
    ctx, prm = make_ctx(field, dc)
    raises(ctx, (8, 4), "FRI: an input height was never rolled in")
    raises(ctx, (6, 8), "tallest first")
    raises(ctx, (6, 6), "tallest first")
    run_and_compare(ctx, oracle, field, dc, prm, random_inputs(field, dc, (7, 5), rng))   # and the context still proves
    ctx.close()


def test_final_poly_refusals(oracle):
    import plonky3_recursion_amd as p3r
    ctx, _ = make_ctx("baby-bear", 4)
    rng = np.random.default_rng(8)
    p = ref.P("baby-bear")
    small = ctx.upload(np.zeros((4, 4), dtype=np.uint32))
    wide = ctx.upload(rng.integers(0, p, size=(8, 5), dtype=np.uint32))
    big = ctx.upload(np.zeros((1 << 17, 4), dtype=np.uint32))
    for d, lf in ((small, 3), (wide, 3), (big, 3)):
        with pytest.raises(p3r.P3rError) as e:
            ctx.fri_final_poly_device(d, lf)
        assert e.value.code == P3R_EINVAL
    assert np.array_equal(ctx.fri_final_poly_device(small, 2), np.zeros((4, 4), dtype=np.uint32))
    for d in (small, wide, big):
        d.free()
    ctx.close()


@pytest.mark.parametrize("schedule", [None, [1, 2, 3, 4, 1, 2]])
def test_log_arity_is_the_rule(schedule):
    import plonky3_recursion_amd as p3r
    for max_la in (1, 2, 3, 4):
        ctx = p3r.Context(field="koala-bear", max_log_arity=max_la, fri_log_arities=schedule)
        for log_cur in range(1, 11):
            for log_final in range(0, log_cur):
                for log_next in range(-1, log_cur + 2):
                    for phase in (0, 1, 3, 5, 6):
                        want = fri_ref.log_arity_rule(schedule or [], phase, max_la, log_cur, log_final, log_next)
                        assert ctx.fri_log_arity(phase, log_cur, log_final, log_next) == want, (max_la, log_cur, log_final, log_next, phase)
        ctx.close()
