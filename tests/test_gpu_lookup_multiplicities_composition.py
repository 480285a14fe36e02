"""GPU: a range check end to end, with the table's multiplicity column built on the device.

One trace of 2^5 rows: v holds values in [0, 32), t = row is the table, and m comes from lookup_multiplicities_device
under the key c - x, which is exact for a single field.  The LogUp column is 1 / (gamma - v) - m / (gamma - t) with its
four constraints, as the lookup AIR of tests/test_gpu_uni_stark_roundtrip.py has them; that module's prove and verify
carry the AIR from trace to a proof verified on the host.

  balanced     lookup_check_device finds no unbalanced key, check_device passes, the table's sum is zero, the proof
               verifies and folded * inv_zh equals the recombined quotient
  m = 0        lookup_check_device names every value of v as an unbalanced key and the table's sum is not zero
  v[r] = 32    the join reports exactly that miss, with its row"""
import numpy as np
import pytest

import test_gpu_open_points as ref
import test_gpu_uni_stark_roundtrip as roundtrip

pytestmark = pytest.mark.gpu
LOG_H = 5
SHIFT = 1000003   # the constant c of the key c - x


def join_programs(field):
    """The query (column 0) and the table (column 1) of the join: every row asks once, every row offers."""
    import plonky3_recursion_amd as p3r
    progs = []
    for col in (0, 1):
        b = p3r.AirBuilder(field)
        b.lookup(1, b.const(SHIFT) - b.local(0, col))
        b.end_lookup_column()
        progs.append(b)
    return progs


def range_air(field, dc, trace):
    """Columns v, t, m of matrix 0; the auxiliary trace is matrix 1."""
    import plonky3_recursion_amd as p3r
    lk = p3r.AirBuilder(field)
    gamma = lk.challenge(0)
    lk.lookup(1, gamma - lk.local(0, 0))
    lk.lookup(-lk.local(0, 2), gamma - lk.local(0, 1))
    lk.end_lookup_column()
    b = p3r.AirBuilder(field)
    gamma = b.challenge(0)
    d_v, d_t, m = gamma - b.local(0, 0), gamma - b.local(0, 1), b.local(0, 2)
    s, s_next, f = b.local_ext(1, 0), b.next_ext(1, 0), b.local_ext(1, dc)
    b.assert_zero(f * d_v * d_t - (d_t - m * d_v))
    b.assert_zero(b.is_first_row() * s)
    b.assert_zero(b.is_transition() * (s_next - s - f))
    b.assert_zero(b.is_last_row() * (s + f - b.challenge(1)))
    return dict(program=b, trace=trace, log_h=LOG_H, publics=[], lookups=lk, log_q=1)


def counts_on_device(ctx, field, v):
    """(m as an array, n_missing, entries) for the column v against t = 0 .. 2^LOG_H - 1."""
    h = 1 << LOG_H
    query, table = join_programs(field)
    d = ctx.upload(np.stack([v, np.arange(h, dtype=np.uint32)], axis=1))
    col, n_missing, entries = ctx.lookup_multiplicities_device((table, [d]), [(query, [d])])
    m = col.download()
    col.free()
    d.free()
    return m, n_missing, entries


@pytest.mark.parametrize("field,dc", roundtrip.CASES)
def test_range_check_from_counts_to_verified_proof(field, dc):
    ctx = roundtrip.make_ctx(field, dc)
    p, h = ref.P(field), 1 << LOG_H
    rng = np.random.default_rng(1970 + dc)
    v = rng.integers(0, h, size=h, dtype=np.uint32)
    t = np.arange(h, dtype=np.uint32)
    m, n_missing, entries = counts_on_device(ctx, field, v)
    assert m.shape == (h, 1) and n_missing == 0 and entries == []
    assert np.array_equal(m[:, 0], np.bincount(v, minlength=h)) and (m == 0).any() and (m > 1).any()
    air = range_air(field, dc, np.stack([v, t, m[:, 0]], axis=1).astype(np.uint32))
    gamma = rng.integers(1, p, size=dc, dtype=np.uint32)

    def bus_of(trace):
        """(unbalanced keys, check_device's report, the table's sum) of a trace under gamma."""
        d = ctx.upload(trace)
        n, unbalanced = ctx.lookup_check_device([(air["lookups"], [d])], challenges=[gamma], cap=h)
        aux, total = ctx.logup_device(air["lookups"], [d], challenges=[gamma])
        report = ctx.check_device(air["program"], [d, aux], challenges=np.array([gamma, total], dtype=np.uint32))
        aux.free()
        d.free()
        return n, unbalanced, report, total

    # ---- balanced
    n, _, report, total = bus_of(air["trace"])
    assert n == 0 and report["n_failures"] == 0 and report["first_row"] == 0xFFFFFFFF and not total.any()
    msg = roundtrip.prove(ctx, field, air)
    assert not msg["table_sum"].any()
    lhs, q_zeta = roundtrip.verify(ctx.cfg, field, dc, air, msg)
    assert lhs == q_zeta and any(lhs)

    # ---- without the counts: every value of v is an unbalanced key, by first row, and the sum does not vanish.  The LogUp
    # constraints hold for any trace: it is the sum that tells
    empty = air["trace"].copy()
    empty[:, 2] = 0
    n, unbalanced, report, total = bus_of(empty)
    firsts = sorted(int(np.argmax(v == x)) for x in np.unique(v))
    assert n == len(np.unique(v)) and [e["row"] for e in unbalanced] == firsts and total.any() and report["n_failures"] == 0
    assert all(e["net"][0] == np.count_nonzero(v == v[e["row"]]) for e in unbalanced)

    # ---- one value out of range
    row = 21
    spoiled = v.copy()
    spoiled[row] = h
    m_bad, n_missing, entries = counts_on_device(ctx, field, spoiled)
    assert n_missing == 1 and len(entries) == 1
    e = entries[0]
    assert (e["instance"], e["row"], e["term"], e["n_records"]) == (0, row, 0, 1)
    assert e["denominator"] == [SHIFT - h] + [0] * (dc - 1) and e["net"] == [1] + [0] * (dc - 1)
    want = np.bincount(np.delete(v, row), minlength=h)
    assert np.array_equal(m_bad[:, 0], want)
    ctx.close()
