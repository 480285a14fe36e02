"""GPU: two AIRs at 2^5 rows whose accumulator columns come from the device (affine_scan_device), with the three
constraints include/p3r.h states for such a column: is_first_row (s - init), is_transition (s' - a s - b),
is_last_row (a s + b - T).

  ledger          base field: bal' = keep * bal + delta, keep in {0, 1} (a closed account restarts), init and T public.
                  check_device reports nothing; then the AIR is carried to a verified proof through the public seams by
                  the prove and verify of tests/test_gpu_uni_stark_roundtrip.py - LDE, commit, quotient program, openings,
                  prove_fri, verify_fri and the constraint check at zeta.
  grand product   challenge field: y a permutation of x, gamma fixed, the factor (gamma - x) / (gamma - y) from
                  witness_device, z from affine_scan_device; the total is one and check_device is clean.  With one cell of
                  y changed the total is not one and check_device names the row and constraint tests/check_ref.py predicts."""
import numpy as np
import pytest

import check_ref
import scan_ref
import test_gpu_open_points as ref
import test_gpu_uni_stark_roundtrip as roundtrip

pytestmark = pytest.mark.gpu
ctxs = ref.ctxs
LOG_H = 5


def ledger_air(field, bal):
    """keep and delta are columns 0 and 1 of matrix 0; `bal` = (matrix, column) of the balance; publics: init, total."""
    import plonky3_recursion_amd as p3r
    b = p3r.AirBuilder(field)
    keep, delta, s, s_next = b.local(0, 0), b.local(0, 1), b.local(*bal), b.next(*bal)
    b.assert_zero(b.is_first_row() * (s - b.public(0)))
    b.assert_zero(b.is_transition() * (s_next - keep * s - delta))
    b.assert_zero(b.is_last_row() * (keep * s + delta - b.public(1)))
    return b


@pytest.mark.parametrize("field,dc", roundtrip.CASES)
def test_ledger_from_the_device_to_a_verified_proof(field, dc):
    ctx = roundtrip.make_ctx(field, dc)
    p, h = ref.P(field), 1 << LOG_H
    rng = np.random.default_rng(2140 + dc)
    keep = np.ones(h, dtype=np.uint32)
    keep[[0, 7, 8, 20, h - 1]] = 0
    moves = np.stack([keep, rng.integers(0, p, size=h, dtype=np.uint32)], axis=1)
    init = 12345
    rec = dict(out_col=0, mul=(0, 0), add=(0, 1), init=init)
    want, want_last = scan_ref.columns(field, dc, [rec], [moves])

    d_moves = ctx.upload(moves)
    d_bal, last = ctx.affine_scan_device([rec], [d_moves], want_last=True)
    bal = d_bal.download()
    assert np.array_equal(bal, want) and np.array_equal(last, want_last) and bal[8, 0] == moves[7, 1]   # a restart
    publics = [init, int(last[0, 0])]
    report = ctx.check_device(ledger_air(field, (1, 0)), [d_moves, d_bal], public_values=publics)
    assert report["n_failures"] == 0 and report["first_row"] == 0xFFFFFFFF
    d_bal.free()
    d_moves.free()

    # ---- to a verified proof: one committed trace keep | delta | bal; the transition has degree 3, two quotient chunks
    air = dict(program=ledger_air(field, (0, 2)), trace=np.concatenate([moves, bal], axis=1), log_h=LOG_H, publics=publics, lookups=None, log_q=1)
    msg = roundtrip.prove(ctx, field, air)
    lhs, q_zeta = roundtrip.verify(ctx.cfg, field, dc, air, msg)
    assert lhs == q_zeta and any(lhs)
    # a verifier that believes another total: the transcript moves first
    import plonky3_recursion_amd as p3r
    with pytest.raises(p3r.P3rError) as e:
        roundtrip.verify(ctx.cfg, field, dc, air, msg, publics=[init, (publics[1] + 1) % p])
    assert e.value.code == roundtrip.P3R_EVERIFY
    # a balance that is not the recurrence's: the identity at zeta fails
    spoiled = air["trace"].copy()
    spoiled[11, 2] = (int(spoiled[11, 2]) + 1) % p
    lhs, q_zeta = roundtrip.verify(ctx.cfg, field, dc, air, roundtrip.prove(ctx, field, air, trace=spoiled))
    assert lhs != q_zeta
    ctx.close()


def product_programs(field):
    """(the witness program of the factor, the AIR): matrix 0 = x | y, matrix 1 = f, matrix 2 = z; challenge 0 = gamma."""
    import plonky3_recursion_amd as p3r
    w = p3r.AirBuilder(field)
    g = w.challenge(0)
    w.store((g - w.local(0, 0)) * w.inv(g - w.local(0, 1)), 0)
    b = p3r.AirBuilder(field)
    g = b.challenge(0)
    f, z, z_next = b.local_ext(1, 0), b.local_ext(2, 0), b.next_ext(2, 0)
    b.assert_zero(f * (g - b.local(0, 1)) - (g - b.local(0, 0)))
    b.assert_zero(b.is_first_row() * (z - 1))
    b.assert_zero(b.is_transition() * (z_next - f * z))
    b.assert_zero(b.is_last_row() * (f * z - 1))   # T = 1: the two columns hold the same multiset
    return w, b


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_grand_product_of_two_permuted_columns(ctxs, field, dc):
    ctx, p, E, h = ctxs(field, dc), ref.P(field), ref.ext(field, dc), 1 << LOG_H
    rng = np.random.default_rng(2150 + dc)
    x = rng.integers(0, p, size=h, dtype=np.uint32)
    xy = np.stack([x, rng.permutation(x)], axis=1)
    gamma = rng.integers(1, p, size=(1, dc), dtype=np.uint32)
    one = [1] + [0] * (dc - 1)
    witness, air = product_programs(field)
    rec = dict(out_col=0, mul=(0, 0), ext=True, init=one)

    def on_device(cells):
        d_xy = ctx.upload(cells)
        d_f = ctx.witness_device(witness, [d_xy], challenges=gamma)
        d_z, last = ctx.affine_scan_device([rec], [d_f], want_last=True)
        report = ctx.check_device(air, [d_xy, d_f, d_z], challenges=gamma)
        f, z = d_f.download(), d_z.download()
        for d in (d_xy, d_f, d_z):
            d.free()
        return f, z, last, report

    f, z, last, report = on_device(xy)
    # f against integers, z against the integer loop over f
    g = [int(v) for v in gamma[0]]
    for r in (0, 13, h - 1):
        num, den = E.sub(g, [int(xy[r, 0])] + [0] * (dc - 1)), E.sub(g, [int(xy[r, 1])] + [0] * (dc - 1))
        assert [int(v) for v in f[r]] == E.mul(num, E.inv(den))
    want, want_last = scan_ref.columns(field, dc, [rec], [f])
    assert np.array_equal(z, want) and np.array_equal(last, want_last)
    assert last[0].tolist() == one + [0] * (5 - dc) and z[0].tolist() == one
    assert report["n_failures"] == 0 and report["first_row"] == 0xFFFFFFFF

    # ---- one cell of y changed: the recurrence still holds, the total is not one, and the last row says so
    bad = xy.copy()
    bad[9, 1] = (int(bad[9, 1]) + 1) % p
    f, z, last, report = on_device(bad)
    assert last[0].tolist() != one + [0] * (5 - dc)
    want_report = check_ref.check(field, dc, air.program(), [bad, f, z], challenges=gamma)
    assert (want_report["first_row"], want_report["first_constraint"], want_report["n_failures"]) == (h - 1, 3, 1)
    assert (report["first_row"], report["first_constraint"], report["n_failures"]) == (h - 1, 3, 1)
    assert report["first_row_of"].tolist() == [0xFFFFFFFF] * 3 + [h - 1] == list(want_report["first_row_of"])

