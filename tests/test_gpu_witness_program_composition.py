"""GPU: a 16-bit range check whose every derived column is built on the device - the AIR of examples/witness_program.cpp,
at 2^5 values against the 2^8 rows of the byte table.

From the one uploaded column v a witness program derives lo = bits [0, 8), hi = bits [8, 16), the inverse witness w and
the is-zero flag z = 1 - v w; a second one, with no input, the table t = 0 .. 255.  lookup_multiplicities_device counts the
limbs, check_device finds v = lo + 256 hi, v z = 0 and z = 1 - v w satisfied and lookup_check_device the bus balanced.
Then hi is derived with the wrong lo, bits [9, 17): both checks name the row tests/witness_ref.py predicts."""
import numpy as np
import pytest

import check_ref
import test_gpu_open_points as ref
import witness_ref

pytestmark = pytest.mark.gpu
ctxs = ref.ctxs
LOG_H, LOG_T = 5, 8
SHIFT = 1000003   # the constant c of the key c - x


def derive_program(field, hi_lo=8):
    import plonky3_recursion_amd as p3r
    b = p3r.AirBuilder(field)
    x = b.local(0, 0)
    w = b.inv(x)
    b.store(b.bits(x, 0, 8), 0)
    b.store(b.bits(x, hi_lo, 8), 1)
    b.store(w, 2)
    b.store(1 - x * w, 3)
    return b


def table_program(field):
    import plonky3_recursion_amd as p3r
    b = p3r.AirBuilder(field)
    b.store(b.row(), 0)
    return b


def gadget_air(field):
    """Matrix 0 is v, matrix 1 the derived columns lo, hi, w, z."""
    import plonky3_recursion_amd as p3r
    b = p3r.AirBuilder(field)
    x, lo, hi, w, z = b.local(0, 0), b.local(1, 0), b.local(1, 1), b.local(1, 2), b.local(1, 3)
    b.assert_zero(x - lo - 256 * hi)
    b.assert_zero(x * z)
    b.assert_zero(z + x * w - 1)
    return b


def bus_programs(field):
    """asks: both limbs of a row, once each; offers: the table in the join; receives: the table on the bus, minus its count."""
    import plonky3_recursion_amd as p3r
    asks, offers, receives = p3r.AirBuilder(field), p3r.AirBuilder(field), p3r.AirBuilder(field)
    for limb in (0, 1):
        asks.lookup(1, asks.const(SHIFT) - asks.local(0, limb))
    asks.end_lookup_column()
    offers.lookup(1, offers.const(SHIFT) - offers.local(0, 0))
    offers.end_lookup_column()
    receives.lookup(-receives.local(1, 0), receives.const(SHIFT) - receives.local(0, 0))
    receives.end_lookup_column()
    return asks, offers, receives


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_range_check_with_every_derived_column_from_the_device(ctxs, field, dc):
    ctx, p = ctxs(field, dc), ref.P(field)
    h, ht = 1 << LOG_H, 1 << LOG_T
    rng = np.random.default_rng(2050 + dc)
    v = rng.integers(1, 1 << 16, size=(h, 1), dtype=np.uint32)
    v[[3, 17]] = 0
    asks, offers, receives = bus_programs(field)
    air = gadget_air(field)

    # ---- 1. the limbs, the is-zero columns and the table
    want_w = witness_ref.columns(field, dc, derive_program(field).program(), [v])
    want_t = witness_ref.columns(field, dc, table_program(field).program(), [], ht)
    assert np.array_equal(want_w[:, 0] + 256 * want_w[:, 1], v[:, 0]) and want_w[:, 3].tolist() == [int(r in (3, 17)) for r in range(h)]
    assert all(int(a) * int(b) % p == 1 for a, b in zip(v[:, 0], want_w[:, 2]) if a) and want_t[:, 0].tolist() == list(range(ht))
    d_v = ctx.upload(v)
    d_w = ctx.witness_device(derive_program(field), [d_v])
    d_t = ctx.witness_device(table_program(field), [], height=ht)
    assert np.array_equal(d_w.download(), want_w) and np.array_equal(d_t.download(), want_t)

    # ---- 2. the counts
    d_m, n_missing, entries = ctx.lookup_multiplicities_device((offers, [d_t]), [(asks, [d_w])])
    m = d_m.download()
    assert n_missing == 0 and entries == []
    assert np.array_equal(m[:, 0], np.bincount(want_w[:, :2].reshape(-1), minlength=ht)) and m.sum() == 2 * h

    # ---- 3. nothing to report
    report = ctx.check_device(air, [d_v, d_w])
    assert report["n_failures"] == 0 and report["first_row"] == 0xFFFFFFFF
    n, unbalanced = ctx.lookup_check_device([(asks, [d_w]), (receives, [d_t, d_m])], cap=2 * h)
    assert n == 0 and unbalanced == []

    # ---- 4. hi from the wrong bits
    bad = derive_program(field, hi_lo=9)
    want_bad = witness_ref.columns(field, dc, bad.program(), [v])
    d_bad = ctx.witness_device(bad, [d_v])
    assert np.array_equal(d_bad.download(), want_bad)

    # ---- 5. both checks name the row the reference predicts
    wrong = want_bad[:, 0].astype(np.int64) + 256 * want_bad[:, 1].astype(np.int64) != v[:, 0]
    assert wrong.any() and not wrong.all()   # the zero rows still decompose
    report = ctx.check_device(air, [d_v, d_bad])
    want_report = check_ref.check(field, dc, air.program(), [v, want_bad])
    assert (report["first_row"], report["first_constraint"], report["n_failures"]) == (int(np.argmax(wrong)), 0, int(wrong.sum()))
    assert (want_report["first_row"], want_report["n_failures"]) == (report["first_row"], report["n_failures"])
    assert report["first_row_of"].tolist() == [int(np.argmax(wrong)), 0xFFFFFFFF, 0xFFFFFFFF]
    n, unbalanced = ctx.lookup_check_device([(asks, [d_bad]), (receives, [d_t, d_m])], cap=4 * h)
    want_n, want_unbalanced = check_ref.lookup_balance(field, dc, [(asks.program(), [want_bad], ()), (receives.program(), [want_t, m], ())])
    assert n == want_n >= 1 and unbalanced == want_unbalanced
    assert (unbalanced[0]["instance"], unbalanced[0]["row"]) == (want_unbalanced[0]["instance"], want_unbalanced[0]["row"])
    for d in (d_v, d_w, d_t, d_m, d_bad):
        d.free()
