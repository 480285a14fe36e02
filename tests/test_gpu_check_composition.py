"""GPU: the constraint check composed with the seams it stands in front of.  For the AIR of tests/test_gpu_check_program.py
(largest constraint degree 2) on 2^6 rows: a trace the check passes gives, through coset_lde_batch_device and
quotient_device (two chunks) and the inverse coset DFT of the whole quotient, a polynomial with no coefficient at or above
h (deg Q <= 2 (h - 1) - h); a trace in which the check names a row gives one that has such coefficients - what
p3r_fri_final_poly_dmat would much later refuse as "not of low degree", without a row.

The inputs and alpha are fixed.  Both outcomes are confirmed on the CPU beforehand: the LDE by naive DFTs on Python
integers, the chunks by air_ref.quotient_chunks, the coefficients by a naive inverse DFT; the device's chunks and
coefficients are then compared with those word for word."""
import numpy as np
import pytest

import air_ref
import check_ref
import field_ref
import test_gpu_check_program as cp
import test_gpu_open_points as ref

pytestmark = pytest.mark.gpu
ctxs = ref.ctxs
H, ADDED_BITS, LOG_Q = 64, 1, 1
FIELDS = [("koala-bear", 4), ("baby-bear", 4)]   # one context per field


def dft_matrix(field, n, sign):
    """M[i, k] = w_n^(sign * i * k)."""
    wt, idx = ref.omega_table(field, n), np.arange(n, dtype=np.int64)
    return wt[(sign * idx[:, None] * idx[None, :]) % n]


def times(field, m, cols):
    """m (a x n) times cols (n x w) over the field: every product is reduced before the n of them are added."""
    p = np.uint64(ref.P(field))
    return np.stack([(m * cols[:, c].astype(np.uint64)[None, :] % p).sum(axis=1) % p for c in range(cols.shape[1])], axis=1)


def coefficients(field, evals, shift):
    """Coefficients of the columns from their evaluations over shift * <w_n>, natural order."""
    p, n = ref.P(field), evals.shape[0]
    c = times(field, dft_matrix(field, n, -1), evals)
    scale = np.array([field_ref.inv(n * pow(shift, k, p) % p, p) for k in range(n)], dtype=np.uint64)
    return (c * scale[:, None] % np.uint64(p)).astype(np.uint32)


def lde(field, trace, added_bits, shift):
    """The committed LDE: evaluations over shift * <w_N>, N = h << added_bits, rows in bit-reversed order."""
    p, h = ref.P(field), trace.shape[0]
    n = h << added_bits
    coef = coefficients(field, trace, 1).astype(np.uint64)
    scaled = coef * np.array([pow(shift, k, p) for k in range(h)], dtype=np.uint64)[:, None] % np.uint64(p)
    wt, i, k = ref.omega_table(field, n), np.arange(n, dtype=np.int64), np.arange(h, dtype=np.int64)
    evals = times(field, wt[(i[:, None] * k[None, :]) % n], scaled)
    return evals[ref.bitrev_indices(n)].astype(np.uint32)


def cpu_quotient(field, dc, prog, mats, publics, chal, alpha):
    g = ref.GEN(field)
    ldes = [lde(field, m, ADDED_BITS, g) for m in mats]
    chunks = air_ref.quotient_chunks(field, dc, prog.program(), ldes, ADDED_BITS, LOG_Q, None, publics, chal, alpha)
    whole = np.empty((2 * H, dc), dtype=np.uint32)
    for c, ch in enumerate(chunks):
        whole[c::2] = ch
    return ldes, chunks, coefficients(field, whole, g)


def device_quotient(ctx, field, dc, prog, mats, publics, chal, alpha):
    g = ref.GEN(field)
    dts = [ctx.upload(m) for m in mats]
    report = ctx.check_device(prog, dts, public_values=publics, challenges=chal)
    ldes = [ctx.coset_lde_batch_device(t, ADDED_BITS, g) for t in dts]
    chunks = ctx.quotient_device(prog, ldes, ADDED_BITS, LOG_Q, alpha, public_values=publics, challenges=chal)
    got_ldes, got_chunks = [m.download() for m in ldes], [c.download() for c in chunks]
    whole = np.empty((2 * H, dc), dtype=np.uint32)
    for c, ch in enumerate(got_chunks):
        whole[c::2] = ch
    dw = ctx.upload(whole)
    coef, = ctx.dft_batch_device([dw], inverse=True, shifts=[g])
    coeffs = coef.download()
    for d in dts + ldes + chunks + [dw, coef]:
        d.free()
    return report, got_ldes, got_chunks, coeffs


@pytest.mark.parametrize("field,dc", FIELDS)
def test_what_the_check_says_is_what_the_quotient_shows(ctxs, field, dc):
    ctx, p, prog = ctxs(field, dc), ref.P(field), cp.build(field, dc)
    rng = np.random.default_rng(1900)
    mats, publics, chal = cp.traces(field, dc, H, rng)
    alpha = [int(v) for v in rng.integers(1, p, size=dc)]
    assert ctx.air_program_info(prog, [2, dc + 1])["max_degree"] == 2
    broken = [mats[0].copy(), mats[1]]
    broken[0][41, 0] = (int(broken[0][41, 0]) + 1) % p   # a of row 41: next.a = b fails in row 40, next.b = a + b in row 41
    for traces, right in ((mats, True), (broken, False)):
        # ---- on the CPU first
        want_report = check_ref.check(field, dc, prog.program(), traces, publics, chal)
        want_ldes, want_chunks, want_coeffs = cpu_quotient(field, dc, prog, traces, publics, chal, alpha)
        assert (want_report["first_row"] == cp.NONE) == right
        assert want_coeffs[H:].any() != right and want_coeffs[:H - 1].any()
        # ---- the device
        report, ldes, chunks, coeffs = device_quotient(ctx, field, dc, prog, traces, publics, chal, alpha)
        cp.same(report, want_report)
        if right:
            assert report["first_row"] == cp.NONE and report["n_failures"] == 0
        else:
            assert (report["first_row"], report["first_constraint"], report["n_failures"]) == (40, 0, 2)
        assert all(np.array_equal(a, b) for a, b in zip(ldes, want_ldes)) and all(np.array_equal(a, b) for a, b in zip(chunks, want_chunks))
        assert np.array_equal(coeffs, want_coeffs)
        assert coeffs[H:].any() != right
