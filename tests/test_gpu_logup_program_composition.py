"""GPU: the lookup-program seam composed with the LDE, the constraint-program, the opening and the DFT seams into the
prover half of a STARK with a lookup argument, checked by the verifier's identity.

The AIR: a main trace (a, b, c, m0, m1) of 16 rows with the degree-2 constraint c = a * b, and two auxiliary columns of two
terms each on denominators gamma + (a tuple of cells): 1 / (gamma + a) - m0 / (gamma + b), and m1 / (gamma + beta c + a)
+ 1 / (gamma + c).  logup_device builds the permutation trace (s, f_0, f_1) from the resident main trace; nothing of it is
computed on the host.  The constraint program then holds, written through AirBuilder, the main constraint and the four
families of include/p3r.h: f_g prod d - sum m prod d for both columns (degree 3: log_quotient_degree 1, two chunks),
is_first * s, is_transition * (s' - s - f_0 - f_1), is_last * (s + f_0 + f_1 - T) with the table's sum T as a challenge.

coset_lde_batch_device of both traces -> quotient_device -> every chunk extended onto the commit coset ->
open_points_device at a random zeta.  Then, on Python integers, as tests/test_gpu_quotient_program_composition.py has it:
the folded constraints at zeta equal Z_H(zeta) * Q(zeta), and the coefficients of the whole quotient vanish from the
degree bound 2h - 2 on.  With one main-trace cell changed after the LogUp trace was built, both checks fail."""
import numpy as np
import pytest

import air_ref
import field_ref
import logup_ref
import test_gpu_open_points as ref

pytestmark = pytest.mark.gpu
ctxs = ref.ctxs
H, ADDED_BITS, LOG_Q = 16, 2, 1


def terms(b):
    """[(multiplicity, denominator)] of the four terms, over matrix 0 and the challenges gamma, beta."""
    a, bb, c, m0, m1 = [b.local(0, k) for k in range(5)]
    gamma, beta = b.challenge(0), b.challenge(1)
    return [(b.const(1), gamma + a), (-m0, gamma + bb), (m1, gamma + beta * c + a), (b.const(1), gamma + c)]


def lookups(field):
    import plonky3_recursion_amd as p3r
    b = p3r.AirBuilder(field)
    t = terms(b)
    for column in (t[:2], t[2:]):
        for m, d in column:
            b.lookup(m, d)
        b.end_lookup_column()
    return b


def air(field, dc):
    import plonky3_recursion_amd as p3r
    b = p3r.AirBuilder(field)
    b.assert_zero(b.local(0, 2) - b.local(0, 0) * b.local(0, 1))
    t = terms(b)
    s, s_next, fs = b.local_ext(1, 0), b.next_ext(1, 0), [b.local_ext(1, dc), b.local_ext(1, 2 * dc)]
    for f, ((m_x, d_x), (m_y, d_y)) in zip(fs, (t[:2], t[2:])):
        b.assert_zero(f * d_x * d_y - (m_x * d_y + m_y * d_x))
    b.assert_zero(b.is_first_row() * s)
    b.assert_zero(b.is_transition() * (s_next - s - (fs[0] + fs[1])))
    b.assert_zero(b.is_last_row() * (s + fs[0] + fs[1] - b.challenge(2)))
    return b


def main_trace(field, rng):
    p = ref.P(field)
    t = rng.integers(0, p, size=(H, 5), dtype=np.uint32)
    t[:, 2] = (t[:, 0].astype(np.uint64) * t[:, 1].astype(np.uint64) % np.uint64(p)).astype(np.uint32)
    t[:, 3] = rng.integers(0, 4, size=H)   # multiplicities as a table has them: small counts
    t[:, 4] = rng.integers(0, 4, size=H)
    return t


def prove_half(ctx, field, dc, main_for_logup, main, gamma_beta, alpha, zeta):
    """The permutation trace of `main_for_logup`, then the quotient of (`main`, that trace).  Returns (folded constraints at
    zeta, Z_H(zeta) * Q(zeta), coefficients of the whole quotient, the permutation trace, the table's sum)."""
    p, g, E, prog = ref.P(field), ref.GEN(field), ref.ext(field, dc), air(field, dc)
    assert ctx.lookup_program_info(lookups(field), [5])["max_constraint_degree"] == 3
    assert ctx.air_program_info(prog, [5, 3 * dc])["log_quotient_degree"] == LOG_Q
    w_h, w_n = field_ref.two_adic_generator(field, 4), field_ref.two_adic_generator(field, 5)
    d_logup = ctx.upload(main_for_logup)
    aux, table_sum = ctx.logup_device(lookups(field), [d_logup], challenges=gamma_beta)
    aux_host = aux.download()
    challenges = np.concatenate([np.asarray(gamma_beta, dtype=np.uint32), np.asarray(table_sum, dtype=np.uint32)[None, :]])
    dts = [ctx.upload(main), aux]   # the permutation trace goes on as it is
    ldes = [ctx.coset_lde_batch_device(t, ADDED_BITS, g) for t in dts]
    chunks = ctx.quotient_device(prog, ldes, ADDED_BITS, LOG_Q, alpha, challenges=challenges)
    assert len(chunks) == 2
    shifts = [g * pow(w_n, c, p) % p for c in range(2)]               # chunk c lives on shifts[c] * <w_h>
    ext = [ctx.coset_lde_batch_device(ch, ADDED_BITS, g * field_ref.inv(s, p) % p) for ch, s in zip(chunks, shifts)]
    z_next = E.scale(zeta, w_h)
    opened = ctx.open_points_device(ldes + ext, [np.array([zeta, z_next], dtype=np.uint32)] * 2 + [np.array([zeta], dtype=np.uint32)] * 2,
                                    added_bits=ADDED_BITS)
    local = [[[int(v) for v in col] for col in opened[m][0]] for m in range(2)]
    nxt = [[[int(v) for v in col] for col in opened[m][1]] for m in range(2)]
    folded = air_ref.fold_at_point(field, dc, prog.program(), local, nxt, zeta, H, (), challenges, alpha)
    # Q(zeta) = sum_c zps[c] * Q_c(zeta),  zps[c] = prod_{j != c} Z_j(zeta) / Z_j(shifts[c]),  Z_j(x) = (x / shifts[j])^h - 1
    one, q_zeta = E.one(0), E.zero(0)
    for c in range(2):
        j = 1 - c
        num = E.sub(E.pow(E.scale(zeta, field_ref.inv(shifts[j], p)), H), one)
        den = (pow(shifts[c] * field_ref.inv(shifts[j], p) % p, H, p) - 1) % p
        q_c = [0] * dc
        for k in range(dc):   # the chunk's DC columns are the coefficients of one extension element
            mono = [1 if i == k else 0 for i in range(dc)]
            q_c = E.add(q_c, E.mul([int(v) for v in opened[2 + c][0][k]], mono))
        q_zeta = E.add(q_zeta, E.mul(E.scale(num, field_ref.inv(den, p)), q_c))
    rhs = E.mul(E.sub(E.pow(list(zeta), H), one), q_zeta)
    # the whole quotient over g * <w_N>, natural order: row i = chunk (i mod 2), row i // 2
    whole = np.empty((2 * H, dc), dtype=np.uint32)
    for c, ch in enumerate(chunks):
        whole[c::2] = ch.download()
    dw = ctx.upload(whole)
    coef, = ctx.dft_batch_device([dw], inverse=True, shifts=[g])
    coeffs = coef.download()
    for d in [d_logup] + dts + ldes + chunks + ext + [dw, coef]:
        d.free()
    return folded, rhs, coeffs, aux_host, [int(v) for v in table_sum]


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_the_verifier_identity_holds_and_breaks_with_the_trace(ctxs, field, dc):
    ctx, p = ctxs(field, dc), ref.P(field)
    rng = np.random.default_rng(1560 + dc)
    main = main_trace(field, rng)
    gamma_beta = rng.integers(0, p, size=(2, dc), dtype=np.uint32)
    alpha = [int(v) for v in rng.integers(0, p, size=dc)]
    zeta = [int(v) for v in rng.integers(0, p, size=dc)]
    assert logup_ref.zero_rows(field, dc, lookups(field).program(), [main], (), gamma_beta) == []
    folded, rhs, coeffs, aux, table_sum = prove_half(ctx, field, dc, main, main, gamma_beta, alpha, zeta)
    want_aux, want_sum = logup_ref.logup_trace(field, dc, lookups(field).program(), [main], (), gamma_beta)
    assert np.array_equal(aux, want_aux) and table_sum == want_sum and aux.shape == (H, 3 * dc)
    assert folded == rhs and any(folded)
    bound = 3 * (H - 1) - H + 1   # deg Q <= 3 (h - 1) - h
    assert not coeffs[bound:].any() and coeffs[:bound].any()
    # one cell changed after the LogUp trace was built: neither c = a * b nor the first column's constraint vanishes on
    # the trace domain any more, the "quotient" is no polynomial of that degree
    spoiled = main.copy()
    spoiled[5, 1] = (int(spoiled[5, 1]) + 1) % p
    folded, rhs, coeffs, _, _ = prove_half(ctx, field, dc, main, spoiled, gamma_beta, alpha, zeta)
    assert folded != rhs
    assert coeffs[bound:].any()
