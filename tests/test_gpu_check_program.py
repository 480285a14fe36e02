"""GPU: the constraint check (p3r_check_program_dmat, k_trace_program<CheckProgSink>) word for word against the integer reference
tests/check_ref.py: the report, every first failing row and every count.  No tolerance.

The AIR: a Fibonacci table (a, b) - next.a = b and next.b = a + b on transitions, a = public 0 and b = 1 in the first row,
b = public 1 in the last - beside a second matrix with one challenge-field running sum s flattened into DC columns and a
value column v: s = 0 in the first row, next.s = s + gamma * v on transitions (gamma is challenge 0).  Base and extension
constraints, all three selectors, publics and a challenge.

Heights 1 and 2 (the next row wraps onto the row itself / the other row), 64 and 128 (one and two waves), 1024 (sixteen
workgroups)."""
import numpy as np
import pytest

import check_ref
import test_gpu_open_points as ref

pytestmark = pytest.mark.gpu
ctxs = ref.ctxs
P3R_EINVAL, P3R_EUNSUPPORTED = -1, -5
HEIGHTS = (1, 2, 64, 128, 1024)
NONE = 0xFFFFFFFF


def build(field, dc):
    """The AIR above; the matrices have the widths (2, DC + 1)."""
    import plonky3_recursion_amd as p3r
    b = p3r.AirBuilder(field)
    x, y, t = b.local(0, 0), b.local(0, 1), b.is_transition()
    b.assert_zero(t * (b.next(0, 0) - y))                                # 0
    b.assert_zero(t * (b.next(0, 1) - (x + y)))                          # 1
    b.assert_zero(b.is_first_row() * (x - b.public(0)))                  # 2
    b.assert_zero(b.is_first_row() * (y - 1))                            # 3
    b.assert_zero(b.is_last_row() * (y - b.public(1)))                   # 4
    s, gamma = b.local_ext(1, 0), b.challenge(0)
    b.assert_zero(t * (b.next_ext(1, 0) - s - gamma * b.local(1, dc)))   # 5, extension
    b.assert_zero(b.is_first_row() * s)                                  # 6, extension
    return b


def traces(field, dc, h, rng):
    """A satisfying pair of traces, its publics and its challenge."""
    p, E = ref.P(field), ref.ext(field, dc)
    gamma = [int(v) for v in rng.integers(1, p, size=dc)]
    a, b, s = int(rng.integers(0, p)), 1, E.zero(0)
    main, side = [], []
    for _ in range(h):
        v = int(rng.integers(0, p))
        main.append([a, b])
        side.append(list(s) + [v])
        s = E.add(s, E.scale(gamma, v))
        a, b = b, (a + b) % p
    main, side = np.array(main, dtype=np.uint32), np.array(side, dtype=np.uint32)
    return [main, side], [int(main[0, 0]), int(main[-1, 1])], np.array([gamma], dtype=np.uint32)


def run(ctx, prog, mats, publics=(), challenges=()):
    dm = [ctx.upload(m) for m in mats]
    try:
        return ctx.check_device(prog, dm, public_values=publics, challenges=challenges)
    finally:
        for d in dm:
            d.free()


def same(got, want):
    for k in ("n_failures", "first_row", "first_constraint"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert got["first_row_of"].dtype == np.uint32 and got["n_failed_of"].dtype == np.uint64
    assert np.array_equal(got["first_row_of"], want["first_row_of"]), (got["first_row_of"], want["first_row_of"])
    assert np.array_equal(got["n_failed_of"], want["n_failed_of"]), (got["n_failed_of"], want["n_failed_of"])


def check(ctx, field, dc, prog, mats, publics=(), challenges=()):
    want = check_ref.check(field, dc, prog.program(), mats, publics, challenges)
    got = run(ctx, prog, mats, publics, challenges)
    same(got, want)
    return got


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_a_satisfying_trace_passes_at_every_height(ctxs, field, dc):
    ctx, prog = ctxs(field, dc), build(field, dc)
    rng = np.random.default_rng(1700 + dc)
    for h in HEIGHTS:
        mats, publics, chal = traces(field, dc, h, rng)
        got = check(ctx, field, dc, prog, mats, publics, chal)
        assert got["first_row"] == NONE and got["first_constraint"] == NONE and got["n_failures"] == 0
        assert len(got["n_failed_of"]) == 7 and not got["n_failed_of"].any() and (got["first_row_of"] == NONE).all()


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_one_broken_cell_is_located(ctxs, field, dc):
    """b of one row changed, at both wave edges and both selector edges.  The transition into the row fails in the row
    BEFORE it, the transitions out of it in its own; in row 0 the first-row constraint, in row h - 1 the last-row one."""
    ctx, p, prog = ctxs(field, dc), ref.P(field), build(field, dc)
    rng = np.random.default_rng(1710 + dc)
    seen = set()
    for h in (2, 64, 128, 1024):
        mats, publics, chal = traces(field, dc, h, rng)
        for row in sorted({0, 63, 64, h - 1}):
            if row >= h:
                continue
            bad = mats[0].copy()
            bad[row, 1] = (int(bad[row, 1]) + 1) % p
            got = check(ctx, field, dc, prog, [bad, mats[1]], publics, chal)
            want_first = max(row - 1, 0)
            assert got["first_row"] == want_first, (h, row)
            if row > 0:
                assert got["first_constraint"] == 1 and got["first_row_of"][1] == row - 1
            else:
                assert got["first_constraint"] == 0 and got["first_row_of"][3] == 0 and got["n_failed_of"][3] == 1
            if row == h - 1:
                assert got["first_row_of"][4] == h - 1 and got["n_failed_of"][0] == 0
            else:
                assert got["first_row_of"][0] == row and got["n_failed_of"][1] == (2 if row else 1)
            seen.add((h, row))
    assert {(128, 63), (128, 64), (128, 127), (1024, 1023), (2, 1)} <= seen


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_a_non_leading_coefficient_alone_fails_an_extension_constraint(ctxs, field, dc):
    ctx, p, prog = ctxs(field, dc), ref.P(field), build(field, dc)
    rng = np.random.default_rng(1720 + dc)
    mats, publics, chal = traces(field, dc, 128, rng)
    for k in (1, dc - 1):
        bad = mats[1].copy()
        bad[70, k] = (int(bad[70, k]) + 1) % p   # coefficient k of s in row 70; coefficient 0 is as it was
        got = check(ctx, field, dc, prog, [mats[0], bad], publics, chal)
        assert got["first_row"] == 69 and got["first_constraint"] == 5
        assert got["n_failed_of"].tolist() == [0, 0, 0, 0, 0, 2, 0] and got["n_failures"] == 2
    bad = mats[1].copy()
    bad[0, dc - 1] = 1                           # the first-row constraint on s: only its top coefficient
    got = check(ctx, field, dc, prog, [mats[0], bad], publics, chal)
    assert got["first_row"] == 0 and got["first_constraint"] == 5 and got["first_row_of"][6] == 0 and got["n_failed_of"][6] == 1


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_constraints_that_fail_in_every_row(ctxs, field, dc):
    """A base and an extension constraint that hold nowhere, and one that holds everywhere between them: the counts are h,
    every wave votes and adds."""
    import plonky3_recursion_amd as p3r
    ctx, p = ctxs(field, dc), ref.P(field)
    rng = np.random.default_rng(1730 + dc)
    b = p3r.AirBuilder(field)
    x = b.local(0, 0)
    b.assert_zero(x - x + 1)
    b.assert_zero(x - x)
    b.assert_zero(b.challenge(0) * (x - x + 1))
    chal = np.zeros((1, dc), dtype=np.uint32)
    chal[0, dc - 1] = p - 1
    for h in HEIGHTS:
        got = check(ctx, field, dc, b, [rng.integers(0, p, size=(h, 1), dtype=np.uint32)], challenges=chal)
        assert got["n_failed_of"].tolist() == [h, 0, h] and got["first_row_of"].tolist() == [0, NONE, 0]
        assert got["n_failures"] == 2 * h and got["first_row"] == 0 and got["first_constraint"] == 0


def full_house(field, dc, n_live, all_ext=False):
    """n_live values alive at one point (half of them extension values, or all): loaded first, then summed; the sum has to
    be the extension value of the third matrix.  Widths (3, 2 DC, DC)."""
    import plonky3_recursion_amd as p3r
    b = p3r.AirBuilder(field)
    vals = [(b.local_ext(1, k % (dc + 1)) if all_ext or k % 2 else b.next(0, k % 3)) for k in range(n_live)]
    acc = vals[0]
    for v in vals[1:]:
        acc = acc + v
    b.assert_zero(acc - b.local_ext(2, 0))
    return b


def full_house_traces(field, dc, h, n_live, all_ext, rng):
    """Two random matrices and the third that satisfies full_house: the sums, taken over the integers here."""
    p = ref.P(field)
    m0, m1 = (rng.integers(0, p, size=(h, w), dtype=np.uint32) for w in (3, 2 * dc))
    nxt = np.roll(m0, -1, axis=0).astype(np.int64)   # the row after the last is row 0
    total = np.zeros((h, dc), dtype=np.int64)
    for k in range(n_live):
        if all_ext or k % 2:
            total += m1[:, k % (dc + 1):k % (dc + 1) + dc]
        else:
            total[:, 0] += nxt[:, k % 3]
    return [m0, m1, (total % p).astype(np.uint32)]


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_a_slot_file_of_extension_values_only(ctxs, field, dc):
    """P3R_AIR_MAX_LIVE extension values alive at once: a slot file of 48 x DC words for each of the 64 lanes.  In the
    KoalaBear quintic context that is 60 KiB, above the 48 KiB a kernel gets without asking, so the launch has to ask for
    it; at degree 4 it is exactly 48 KiB and does not cross the line.  Heights 64 and 128: one workgroup and two.  The
    satisfying trace passes; with one cell broken the wave that holds it votes and its two atomics run."""
    from plonky3_recursion_amd import _lib
    ctx, p = ctxs(field, dc), ref.P(field)
    rng = np.random.default_rng(1750 + dc)
    n_live = _lib.P3R_AIR_MAX_LIVE
    prog = full_house(field, dc, n_live, all_ext=True)
    assert ctx.air_program_info(prog, (3, 2 * dc, dc))["peak_live"] == n_live
    for h in (64, 128):
        mats = full_house_traces(field, dc, h, n_live, True, rng)
        got = check(ctx, field, dc, prog, mats)
        assert got["n_failures"] == 0 and got["first_row"] == NONE
        row = h - 3
        mats[1][row, 2 * dc - 1] = (int(mats[1][row, 2 * dc - 1]) + 1) % p   # the top word of the last window only
        got = check(ctx, field, dc, prog, mats)
        assert got["n_failures"] == 1 and got["first_row"] == row and got["first_constraint"] == 0
        assert got["n_failed_of"].tolist() == [1] and got["first_row_of"].tolist() == [row]


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_refusals_leave_the_context_usable(ctxs, field, dc):
    import plonky3_recursion_amd as p3r
    from plonky3_recursion_amd import _lib as L
    ctx, p, prog = ctxs(field, dc), ref.P(field), build(field, dc)
    rng = np.random.default_rng(1740 + dc)
    mats, publics, chal = traces(field, dc, 64, rng)
    mats[0][10, 0] = (int(mats[0][10, 0]) + 1) % p
    want = check_ref.check(field, dc, prog.program(), mats, publics, chal)
    assert want["n_failures"] == 2
    dm = [ctx.upload(m) for m in mats]
    short = ctx.upload(mats[1][:32])
    bad_chal = chal.copy()
    bad_chal[0, 1] = p
    LOC = L.P3R_AIR_LOCAL
    cases = [
        ("matrices of different heights", P3R_EINVAL, dict(mats_=[dm[0], short])),
        ("a non-canonical public value", P3R_EINVAL, dict(publics_=[publics[0], p])),
        ("a non-canonical challenge word", P3R_EINVAL, dict(chal_=bad_chal)),
        ("a lookup op", P3R_EINVAL, dict(prog_=[(LOC, 0, 0), (L.P3R_AIR_LOOKUP, 0, 0), (L.P3R_AIR_LOOKUP_END, 0, 0), (L.P3R_AIR_ASSERT_ZERO, 0, 0)])),
        ("no ASSERT_ZERO", P3R_EINVAL, dict(prog_=[(LOC, 0, 0)])),
        ("a column out of range", P3R_EINVAL, dict(prog_=[(LOC, 0, 2), (L.P3R_AIR_ASSERT_ZERO, 0, 0)])),
        ("a public index out of range", P3R_EINVAL, dict(prog_=[(L.P3R_AIR_PUBLIC, 2, 0), (L.P3R_AIR_ASSERT_ZERO, 0, 0)])),
        ("n_mats == 0", P3R_EINVAL, dict(mats_=[])),
    ]
    for name, code, kw in cases:
        with pytest.raises(p3r.P3rError) as e:
            ctx.check_device(kw.get("prog_", prog), kw.get("mats_", dm), public_values=kw.get("publics_", publics), challenges=kw.get("chal_", chal))
        assert e.value.code == code and len(str(e.value)) > 15, (name, str(e.value))
        same(ctx.check_device(prog, dm, public_values=publics, challenges=chal), want)
    for d in dm + [short]:
        d.free()


def test_zk_contexts_are_refused():
    import plonky3_recursion_amd as p3r
    ctx = p3r.Context(field="koala-bear", zk=1, zk_seed=1, log_blowup=1, max_log_arity=1, log_final_poly_len=0, query_pow_bits=3, num_queries=4)
    try:
        d = ctx.upload(np.ones((8, 1), dtype=np.uint32))
        b = p3r.AirBuilder("koala-bear")
        b.assert_zero(b.local(0, 0) - 1)
        with pytest.raises(p3r.P3rError) as e:
            ctx.check_device(b, [d])
        assert e.value.code == P3R_EUNSUPPORTED and "zk" in str(e.value)
        d.free()
    finally:
        ctx.close()
