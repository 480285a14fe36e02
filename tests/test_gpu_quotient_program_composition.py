"""GPU: the constraint-program seam composed with the LDE, the opening and the DFT seams into the prover half of
p3_uni_stark::prove, checked by the verifier's identity.

The AIR: a main trace (a, b, c) with the degree-3 constraint c = a^3 + b, the transitions next.a = b and next.b = c, the
boundary values first.a and last.c as public values, and a second matrix holding one challenge-field running sum s
flattened into DC columns: s = gamma * a on the first row, next.s = s + gamma * next.a on transitions, s = the total on the
last row (gamma and the total are challenges 0 and 1).  The largest degree is 3: log_quotient_degree 1, two chunks.

coset_lde_batch_device -> quotient_device -> every chunk extended onto the commit coset -> open_points_device at a random
zeta (the trace at zeta and zeta * w_h).  Then, on Python integers: the folded constraints at zeta (air_ref.fold_at_point)
equal Z_H(zeta) * Q(zeta), Q(zeta) recombined from the chunk openings with the `zps` of p3_uni_stark::verify; and the
inverse coset DFT of the whole quotient has zero coefficients from 2h - 2 on (deg Q <= 3 (h - 1) - h).  With one trace cell
changed the identity fails and those coefficients are not zero: the mathematics on a wrong input, nothing faults."""
import numpy as np
import pytest

import air_ref
import field_ref
import test_gpu_open_points as ref

pytestmark = pytest.mark.gpu
ctxs = ref.ctxs
H, ADDED_BITS, LOG_Q = 16, 2, 1


def air(field):
    import plonky3_recursion_amd as p3r
    b = p3r.AirBuilder(field)
    x, y, z = b.local(0, 0), b.local(0, 1), b.local(0, 2)
    b.assert_zero(z - (x * x * x + y))
    t = b.is_transition()
    b.assert_zero(t * (b.next(0, 0) - y))
    b.assert_zero(t * (b.next(0, 1) - z))
    b.assert_zero(b.is_first_row() * (x - b.public(0)))
    b.assert_zero(b.is_last_row() * (z - b.public(1)))
    s, gamma = b.local_ext(1, 0), b.challenge(0)
    b.assert_zero(b.is_first_row() * (s - gamma * x))
    b.assert_zero(t * (b.next_ext(1, 0) - s - gamma * b.next(0, 0)))
    b.assert_zero(b.is_last_row() * (s - b.challenge(1)))
    return b


def traces(field, dc, rng):
    p, E = ref.P(field), ref.ext(field, dc)
    gamma = [int(v) for v in rng.integers(0, p, size=dc)]
    a, b = int(rng.integers(0, p)), int(rng.integers(0, p))
    main, run, s = [], [], E.zero(0)
    for _ in range(H):
        c = (pow(a, 3, p) + b) % p
        s = E.add(s, E.scale(gamma, a))
        main.append([a, b, c])
        run.append(s)
        a, b = b, c
    main, run = np.array(main, dtype=np.uint32), np.array(run, dtype=np.uint32)
    return main, run, [int(main[0, 0]), int(main[-1, 2])], np.array([gamma, run[-1]], dtype=np.uint32)


def prove_half(ctx, field, dc, main, run, publics, challenges, alpha, zeta):
    """Returns (folded constraints at zeta, Z_H(zeta) * Q(zeta), coefficients of the whole quotient)."""
    p, g, E, prog = ref.P(field), ref.GEN(field), ref.ext(field, dc), air(field)
    assert ctx.air_program_info(prog, [3, dc])["log_quotient_degree"] == LOG_Q
    w_h, w_n = field_ref.two_adic_generator(field, 4), field_ref.two_adic_generator(field, 5)
    dts = [ctx.upload(main), ctx.upload(run)]
    ldes = [ctx.coset_lde_batch_device(t, ADDED_BITS, g) for t in dts]
    chunks = ctx.quotient_device(prog, ldes, ADDED_BITS, LOG_Q, alpha, public_values=publics, challenges=challenges)
    assert len(chunks) == 2
    shifts = [g * pow(w_n, c, p) % p for c in range(2)]               # chunk c lives on shifts[c] * <w_h>
    ext = [ctx.coset_lde_batch_device(ch, ADDED_BITS, g * field_ref.inv(s, p) % p) for ch, s in zip(chunks, shifts)]
    z_next = E.scale(zeta, w_h)
    opened = ctx.open_points_device(ldes + ext, [np.array([zeta, z_next], dtype=np.uint32)] * 2 + [np.array([zeta], dtype=np.uint32)] * 2,
                                    added_bits=ADDED_BITS)
    local = [[[int(v) for v in col] for col in opened[m][0]] for m in range(2)]
    nxt = [[[int(v) for v in col] for col in opened[m][1]] for m in range(2)]
    folded = air_ref.fold_at_point(field, dc, prog.program(), local, nxt, zeta, H, publics, challenges, alpha)
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
    for d in dts + ldes + chunks + ext + [dw, coef]:
        d.free()
    return folded, rhs, coeffs


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_the_verifier_identity_holds_and_breaks_with_the_trace(ctxs, field, dc):
    ctx, p = ctxs(field, dc), ref.P(field)
    rng = np.random.default_rng(1460 + dc)
    main, run, publics, challenges = traces(field, dc, rng)
    alpha = [int(v) for v in rng.integers(0, p, size=dc)]
    zeta = [int(v) for v in rng.integers(0, p, size=dc)]
    folded, rhs, coeffs = prove_half(ctx, field, dc, main, run, publics, challenges, alpha, zeta)
    assert folded == rhs and any(folded)
    bound = 3 * (H - 1) - H + 1   # deg Q <= 3 (h - 1) - h
    assert not coeffs[bound:].any() and coeffs[:bound].any()
    # one cell changed: the constraints no longer vanish on the trace domain, the "quotient" is no polynomial of that degree
    spoiled = main.copy()
    spoiled[5, 1] = (int(spoiled[5, 1]) + 1) % p
    folded, rhs, coeffs = prove_half(ctx, field, dc, spoiled, run, publics, challenges, alpha, zeta)
    assert folded != rhs
    assert coeffs[bound:].any()
