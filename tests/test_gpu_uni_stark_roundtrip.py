"""GPU: a caller's AIR proved on the device and verified on the host - the loop p3_uni_stark's tests close.

Prover, all resident: trace LDE, commit -> (LogUp trace through logup_device, LDE, commit) -> quotient_device -> every
chunk extended onto the commit coset, commit -> zeta -> Context.pcs_open.  Verifier, host only, a fresh host challenger
made from ctx.cfg: the same transcript, pcs_verify, then folded * inv_zh from air_program_eval against the quotient
recombined from the chunk openings (the recombination of tests/test_gpu_quotient_program_composition.py).

  fibonacci   2^4 x 2, next.a = b, next.b = a + b, first.a and last.b public: degree 2, one chunk
  lookup      2^5 x 2, column t a permutation of column v; one LogUp column 1 / (gamma - v) - 1 / (gamma - t) and its four
              constraints: degree 3, two chunks

Negatives: a trace cell changed before commit (the openings stay true openings of low-degree LDEs, so FRI accepts: the
identity at zeta fails, or for the lookup AIR the table's sum is no longer zero), a
claimed opened value changed after proving (pcs_verify rejects), an opened input row changed (its batch no longer opens its
cap), a wrong public value (observed: the transcript moves and pcs_verify rejects; handed over on the side: the opening
proof verifies and the identity fails)."""
import numpy as np
import pytest

import field_ref
import test_gpu_open_points as ref

pytestmark = pytest.mark.gpu
P3R_EINVAL, P3R_EVERIFY = -1, -7
LB = 2
CASES = [("koala-bear", 4), ("baby-bear", 4), ("koala-bear", 5)]


def make_ctx(field, dc):
    import plonky3_recursion_amd as p3r
    return p3r.Context(field=field, challenge_degree=dc, log_blowup=LB, log_final_poly_len=0, max_log_arity=2, cap_height=1,
                       commit_pow_bits=2, query_pow_bits=3, num_queries=3)


def fibonacci(field, rng, log_h=4):
    import plonky3_recursion_amd as p3r
    p = ref.P(field)
    b = p3r.AirBuilder(field)
    a0, a1 = b.local(0, 0), b.local(0, 1)
    t = b.is_transition()
    b.assert_zero(b.is_first_row() * (a0 - b.public(0)))
    b.assert_zero(t * (b.next(0, 0) - a1))
    b.assert_zero(t * (b.next(0, 1) - a0 - a1))
    b.assert_zero(b.is_last_row() * (a1 - b.public(1)))
    x, y, rows = int(rng.integers(0, p)), int(rng.integers(0, p)), []
    for _ in range(1 << log_h):
        rows.append([x, y])
        x, y = y, (x + y) % p
    trace = np.array(rows, dtype=np.uint32)
    return dict(program=b, trace=trace, log_h=log_h, publics=[int(trace[0, 0]), int(trace[-1, 1])], lookups=None, log_q=0)


def lookup_air(field, dc, rng, log_h=5):
    import plonky3_recursion_amd as p3r
    p = ref.P(field)
    lk = p3r.AirBuilder(field)
    gamma = lk.challenge(0)
    lk.lookup(1, gamma - lk.local(0, 0))
    lk.lookup(p - 1, gamma - lk.local(0, 1))
    lk.end_lookup_column()
    b = p3r.AirBuilder(field)
    gamma = b.challenge(0)
    d_v, d_t = gamma - b.local(0, 0), gamma - b.local(0, 1)
    s, s_next, f = b.local_ext(1, 0), b.next_ext(1, 0), b.local_ext(1, dc)
    b.assert_zero(f * d_v * d_t - (d_t - d_v))
    b.assert_zero(b.is_first_row() * s)
    b.assert_zero(b.is_transition() * (s_next - s - f))
    b.assert_zero(b.is_last_row() * (s + f - b.challenge(1)))
    v = rng.integers(0, p, size=1 << log_h, dtype=np.uint32)
    trace = np.stack([v, rng.permutation(v)], axis=1).astype(np.uint32)
    return dict(program=b, trace=trace, log_h=log_h, publics=[], lookups=lk, log_q=1)


def chunk_shifts(field, log_h, log_q):
    p, g = ref.P(field), ref.GEN(field)
    w_n = field_ref.two_adic_generator(field, log_h + log_q)
    return [g * pow(w_n, c, p) % p for c in range(1 << log_q)]


def prove(ctx, field, air, trace=None):
    """Returns what travels to the verifier: caps, the LogUp table sum, opened values, the FRI proof, input openings."""
    p, g, dc = ref.P(field), ref.GEN(field), ctx.challenge_degree
    E = ref.ext(field, dc)
    keep, trees = [], []
    try:
        ch = ctx.challenger()
        d_trace = ctx.upload(air["trace"] if trace is None else trace)
        lde = ctx.coset_lde_batch_device(d_trace, LB, g)
        keep += [d_trace, lde]
        cap_t, tree_t = ctx.commit_device([lde])
        trees.append(tree_t)
        ch.observe(cap_t.reshape(-1))
        if air.get("observe_publics", True):
            ch.observe(air["publics"])
        msg = dict(cap_trace=cap_t, cap_aux=None, table_sum=None)
        ldes, challenges = [lde], np.zeros((0, dc), dtype=np.uint32)
        if air["lookups"] is not None:
            gamma = ch.sample_ext()
            aux, total = ctx.logup_device(air["lookups"], [d_trace], challenges=[gamma])
            aux_lde = ctx.coset_lde_batch_device(aux, LB, g)
            keep += [aux, aux_lde]
            cap_a, tree_a = ctx.commit_device([aux_lde])
            trees.append(tree_a)
            ch.observe(cap_a.reshape(-1))
            ch.observe(total)
            msg.update(cap_aux=cap_a, table_sum=total)
            ldes.append(aux_lde)
            challenges = np.array([gamma, total], dtype=np.uint32)
        alpha = ch.sample_ext()
        chunks = ctx.quotient_device(air["program"], ldes, LB, air["log_q"], alpha, public_values=air["publics"], challenges=challenges)
        exts = [ctx.coset_lde_batch_device(c, LB, g * field_ref.inv(s, p) % p) for c, s in zip(chunks, chunk_shifts(field, air["log_h"], air["log_q"]))]
        keep += chunks + exts
        cap_q, tree_q = ctx.commit_device(exts)
        trees.append(tree_q)
        ch.observe(cap_q.reshape(-1))
        zeta = [int(v) for v in ch.sample_ext()]
        z_next = E.scale(zeta, field_ref.two_adic_generator(field, air["log_h"]))
        two = np.array([zeta, z_next], dtype=np.uint32)
        rounds = [(tree_t, [lde], [two])]
        if air["lookups"] is not None:
            rounds.append((trees[1], [ldes[1]], [two]))
        rounds.append((tree_q, exts, [np.array([zeta], dtype=np.uint32)] * len(exts)))
        values, proof, openings = ctx.pcs_open(ch, rounds)
        msg.update(cap_quotient=cap_q, values=values, proof=proof, openings=openings, dims=[[d.shape for d in r[1]] for r in rounds],
                   after=ch.sample())
        return msg
    finally:
        for t in trees:
            t.free()
        for d in keep:
            d.free()


def verify(cfg, field, dc, air, msg, publics=None):
    """Host only.  Returns (folded * inv_zh, the quotient at zeta recombined from the chunk openings)."""
    import plonky3_recursion_amd as p3r
    p, E = ref.P(field), ref.ext(field, dc)
    publics = air["publics"] if publics is None else publics
    h = 1 << air["log_h"]
    ch = p3r.host_challenger(cfg)
    ch.observe(msg["cap_trace"].reshape(-1))
    if air.get("observe_publics", True):
        ch.observe(publics)
    caps, challenges = [msg["cap_trace"]], np.zeros((0, dc), dtype=np.uint32)
    if air["lookups"] is not None:
        gamma = ch.sample_ext()
        ch.observe(msg["cap_aux"].reshape(-1))
        ch.observe(msg["table_sum"])
        caps.append(msg["cap_aux"])
        challenges = np.array([gamma, msg["table_sum"]], dtype=np.uint32)
    alpha = ch.sample_ext()
    ch.observe(msg["cap_quotient"].reshape(-1))
    caps.append(msg["cap_quotient"])
    zeta = [int(v) for v in ch.sample_ext()]
    z_next = E.scale(zeta, field_ref.two_adic_generator(field, air["log_h"]))
    two, one = np.array([zeta, z_next], dtype=np.uint32), np.array([zeta], dtype=np.uint32)
    values = msg["values"]
    points = [[two]] * (len(caps) - 1) + [[one] * len(values[-1])]
    p3r.observe_opened_values(ch, values)
    rounds = [(cap, dims, pts, vals) for cap, dims, pts, vals in zip(caps, msg["dims"], points, values)]
    p3r.pcs_verify(cfg, ch, rounds, msg["proof"], msg["openings"])
    assert ch.sample() == msg["after"], "the verifier's challenger is left where the prover's is"
    # the constraint check at zeta
    traces = values[:-1]
    widths = [v[0].shape[1] for v in traces]
    local = np.concatenate([v[0][0] for v in traces])
    nxt = np.concatenate([v[0][1] for v in traces])
    folded, inv_zh = p3r.air_program_eval(cfg, air["program"], widths, local, nxt, air["log_h"], zeta, publics, challenges, alpha)
    lhs = E.mul([int(v) for v in folded], [int(v) for v in inv_zh])
    shifts = chunk_shifts(field, air["log_h"], air["log_q"])
    one_e, q_zeta = E.one(0), E.zero(0)
    for c, sc in enumerate(shifts):
        num, den = one_e, 1
        for j, sj in enumerate(shifts):
            if j != c:
                num = E.mul(num, E.sub(E.pow(E.scale(zeta, field_ref.inv(sj, p)), h), one_e))
                den = den * ((pow(sc * field_ref.inv(sj, p) % p, h, p) - 1) % p) % p
        q_c = E.zero(0)
        for k in range(dc):   # the chunk's DC columns are the coefficients of one extension element
            q_c = E.add(q_c, E.mul([int(v) for v in values[-1][c][0][k]], [1 if i == k else 0 for i in range(dc)]))
        q_zeta = E.add(q_zeta, E.mul(E.scale(num, field_ref.inv(den, p)), q_c))
    return [int(v) for v in lhs], [int(v) for v in q_zeta]


def make_air(kind, field, dc):
    rng = np.random.default_rng(len(kind) + dc)
    return fibonacci(field, rng) if kind == "fibonacci" else lookup_air(field, dc, rng)


@pytest.mark.parametrize("field,dc", CASES)
@pytest.mark.parametrize("kind", ["fibonacci", "lookup"])
def test_device_proof_host_verification(kind, field, dc):
    import plonky3_recursion_amd as p3r
    ctx = make_ctx(field, dc)
    p = ref.P(field)
    air = make_air(kind, field, dc)
    msg = prove(ctx, field, air)
    cfg = ctx.cfg
    lhs, q_zeta = verify(cfg, field, dc, air, msg)
    assert lhs == q_zeta and any(lhs)

    # a claimed opened value changed after proving: pcs_verify rejects (the transcript moves, or the reduced opening does)
    bad = dict(msg, values=[[v.copy() for v in r] for r in msg["values"]])
    bad["values"][0][0][1, 0, 0] = (int(bad["values"][0][0][1, 0, 0]) + 1) % p
    with pytest.raises(p3r.P3rError) as e:
        verify(cfg, field, dc, air, bad)
    assert e.value.code == P3R_EVERIFY, str(e.value)

    # one opened input row changed: the input batch no longer opens its cap
    opened, salts, sib = msg["openings"][0]
    spoiled = opened.copy()
    spoiled[1, 0] = (int(spoiled[1, 0]) + 1) % p
    with pytest.raises(p3r.P3rError) as e:
        verify(cfg, field, dc, air, dict(msg, openings=[(spoiled, salts, sib)] + msg["openings"][1:]))
    assert e.value.code == P3R_EVERIFY and "input batch 0 of query 1" in str(e.value), str(e.value)

    # a wrong public value: the opening proof does not depend on what the verifier believes the public values are beyond
    # the transcript, so it is the transcript that moves first
    if air["publics"]:
        wrong = [air["publics"][0], (air["publics"][1] + 1) % p]
        with pytest.raises(p3r.P3rError) as e:
            verify(cfg, field, dc, air, msg, publics=wrong)
        assert e.value.code == P3R_EVERIFY

    # one trace cell changed before commit.  Every committed matrix is still an LDE of its h values and every claimed value a
    # true opening, so the reduced openings stay of low degree: the prover does not refuse and pcs_verify accepts.  What
    # fails, deterministically, is the identity at zeta (fibonacci: a transition no longer holds on the trace domain) or
    # the bus (lookup: the LogUp constraints hold for any trace, but the table's sum is no longer zero).
    spoiled_trace = air["trace"].copy()
    spoiled_trace[5, 1] = (int(spoiled_trace[5, 1]) + 1) % p
    bad = prove(ctx, field, air, trace=spoiled_trace)
    lhs, q_zeta = verify(cfg, field, dc, air, bad)
    if kind == "fibonacci":
        assert lhs != q_zeta
    else:
        assert lhs == q_zeta and bad["table_sum"].any() and not msg["table_sum"].any()
    ctx.close()


@pytest.mark.parametrize("field,dc", CASES)
def test_a_wrong_public_value_breaks_the_identity(field, dc):
    """The public values kept out of the transcript (a verifier that is handed them on the side): the opening proof
    verifies whatever the verifier believes them to be, and the constraint check at zeta is what fails."""
    ctx = make_ctx(field, dc)
    p = ref.P(field)
    air = dict(make_air("fibonacci", field, dc), observe_publics=False)
    msg = prove(ctx, field, air)
    lhs, q_zeta = verify(ctx.cfg, field, dc, air, msg)
    assert lhs == q_zeta and any(lhs)
    for k in (0, 1):   # the first-row and the last-row boundary value
        wrong = list(air["publics"])
        wrong[k] = (wrong[k] + 1) % p
        lhs, q_zeta = verify(ctx.cfg, field, dc, air, msg, publics=wrong)
        assert lhs != q_zeta, "the identity fails under a wrong public value"
    ctx.close()
