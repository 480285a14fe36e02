"""GPU: the public FRI seam (p3r_fri_reduce_dmat, p3r_fri_fold_dmat) against Python integers.  Every expected word comes
from tests/field_ref.py (Ext.inv, Ext.mul, two_adic_generator, bit_reverse; its functions take numpy uint64 arrays, one
entry per row) or from a closed form, and every comparison is equality of canonical words.

The reduced openings are computed here from the definition, row by row:
    walk the matrices in call order and each matrix's points in order; one running factor a_H per height H, 1 at first;
    ro_H[r] += a_H * sum_c alpha^c * (V[i][p][c] - M_i[r][c]) / (z[i][p] - x_r),  x_r = shift * w_H^bitrev(r);  a_H *= alpha^w_i.
One arity-2 fold is fold2(e0, e1, beta, x0) = (e0 + e1) / 2 + beta * (e0 - e1) / (2 * x0) with x0 the point of e0."""
import itertools

import numpy as np
import pytest

import field_ref
import harness_lib
import layer_lib
import test_gpu_open_points as ref

pytestmark = pytest.mark.gpu

CTXS = ref.CTXS
P3R_EINVAL, P3R_EUNSUPPORTED = -1, -5
WIDTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9)
COUNTS = (0, 1, 2, 3, 5)
ctxs = ref.ctxs
P, GEN, ext = ref.P, ref.GEN, ref.ext
U = np.uint64


# ---------------------------------------------------------------- the definitions
def row_points(field, h, shift):
    """x_r = shift * w_h^bitrev(r), uint64."""
    p, bits = P(field), h.bit_length() - 1
    w = field_ref.two_adic_generator(field, bits)
    return np.array([shift * pow(w, field_ref.bit_reverse(r, bits), p) % p for r in range(h)], dtype=U)


def bc(e, n):
    """An extension element (dc integers) as dc arrays of n equal entries."""
    return [np.full(n, int(v), dtype=U) for v in e]


def cols(a):
    """(n, dc) words -> dc uint64 arrays."""
    return [np.ascontiguousarray(a[:, k]).astype(U) for k in range(a.shape[1])]


def rows(e):
    """dc arrays -> (n, dc) uint32 words."""
    return np.stack([np.asarray(c, dtype=U) for c in e], axis=1).astype(np.uint32)


_INV = {}


def inverse_vectors(field, dc, shift, need):
    """1 / (z - x_r) for every (h, z) of `need`, one Ext.inv over all of them; remembered, since many calls of a test share
    their points and the vector does not depend on anything else."""
    E, p = ext(field, dc), P(field)
    todo = [k for k in dict.fromkeys(need) if (field, dc, shift) + k not in _INV]
    if todo:
        den = [[] for _ in range(dc)]
        for h, z in todo:
            x = row_points(field, h, shift)
            d = bc(z, h)
            d[0] = (d[0] + (U(p) - x)) % U(p)
            for k in range(dc):
                den[k].append(d[k])
        inv = E.inv([np.concatenate(c) for c in den])
        at = 0
        for h, z in todo:
            _INV[(field, dc, shift) + (h, z)] = [c[at:at + h] for c in inv]
            at += h
    return {k: _INV[(field, dc, shift) + k] for k in need}


def reduce_ref(field, dc, mats, pts, vals, alpha, shift=None):
    """{height: (height, dc) uint32} from the definition.  mats[i]: (h, w) words, pts[i]: (k, dc), vals[i]: (k, w, dc)."""
    E, p = ext(field, dc), P(field)
    shift = GEN(field) if shift is None else shift
    alpha = [int(v) for v in alpha]
    inv = inverse_vectors(field, dc, shift, [(m.shape[0], tuple(int(v) for v in z)) for m, q in zip(mats, pts) for z in q])
    ro, a = {}, {}
    for m, q, v in zip(mats, pts, vals):
        h, w = m.shape
        for j, z in enumerate(q):
            acc = ro.setdefault(h, E.zero(np.zeros(h, dtype=U)))
            a_h = a.setdefault(h, E.one(0))
            num, ap = E.zero(np.zeros(h, dtype=U)), E.one(0)
            for c in range(w):
                diff = bc(v[j][c], h)
                diff[0] = (diff[0] + (U(p) - m[:, c].astype(U))) % U(p)
                num = E.add(num, E.mul(bc(ap, h), diff))
                ap = E.mul(ap, alpha)
            ro[h] = E.add(acc, E.mul(bc(a_h, h), E.mul(num, inv[(h, tuple(int(x) for x in z))])))
            a[h] = E.mul(a_h, ap)          # ap is alpha^w here
    return {h: rows(e) for h, e in ro.items()}


def fold_ref(field, dc, vec, la, beta, roll=None):
    """la arity-2 folds of the (n, dc) vector over <w_n> in bit-reversed order, from fold2, then the roll-in."""
    E, p = ext(field, dc), P(field)
    e, b = cols(vec), [int(v) for v in beta]
    for _ in range(la):
        n = len(e[0])
        x0 = row_points(field, n, 1)[0::2]
        e0, e1 = [c[0::2] for c in e], [c[1::2] for c in e]
        inv_2x0 = field_ref.inv(2 * x0 % U(p), p)
        e = E.add(E.halve(E.add(e0, e1)), E.mul(bc(b, n // 2), [c * inv_2x0 % U(p) for c in E.sub(e0, e1)]))
        b = E.mul(b, b)
    if roll is not None:
        e = E.add(e, E.mul(bc(b, len(e[0])), cols(roll)))
    return rows(e)


def rand_ext(field, dc, rng, n=None):
    """Random extension elements with a non-zero second coefficient: outside the base field, so in no coset."""
    z = rng.integers(0, P(field), size=(1 if n is None else n, dc), dtype=np.uint32)
    z[:, 1] = rng.integers(1, P(field), size=len(z), dtype=np.uint32)
    return z[0] if n is None else z


def dmat(ctx, m):
    import plonky3_recursion_amd as p3r
    if m.shape[1] == 0:
        return p3r.device.DeviceMatrix(ctx, ctx.ptr(ctx.lib.p3r_dmat_alloc(ctx.h, m.shape[0], 0)))
    return ctx.upload(m)


def run_reduce(ctx, mats, pts, vals, alpha, shift=None, dms=None):
    """fri_reduce_device on uploads of `mats`: [(height, (height, dc) words)], tallest first as the call returned them."""
    own = dms is None
    dms = [dmat(ctx, m) for m in mats] if own else dms
    outs = ctx.fri_reduce_device(dms, pts, vals, alpha, shift=shift)
    got = [(o.shape, o.download()) for o in outs]
    for o in outs:
        o.free()
    if own:
        for d in dms:
            d.free()
    return got


def assert_reduce(got, want, what):
    assert [s for s, _ in got] == [(h, want[h].shape[1]) for h in sorted(want, reverse=True)], what
    for (h, _), g in got:
        assert np.array_equal(g, want[h]), what + (h,)


# ---------------------------------------------------------------- 1. reduce from the definition
@pytest.mark.parametrize("h", [1, 2, 4, 8, 1 << 8, 1 << 9])
@pytest.mark.parametrize("field,dc", CTXS)
def test_reduce_from_the_definition(ctxs, field, dc, h):
    """h = 1, 2: below a lane's four rows of the inverse vector; 4, 8: at and above; 2^8: one block; 2^9: two.  All widths
    (around the column loop's groups of four and two) go in ONE call, so the running a_H crosses every matrix, with 0, 1,
    2, 3 and 5 points per matrix and once with a different count per matrix.  Matrix and value words are random: the
    entry does not ask for values that belong to the matrices, nor does the definition."""
    ctx, p = ctxs(field, dc), P(field)
    rng = np.random.default_rng(h * 37 + dc)
    mats = [rng.integers(0, p, size=(h, w), dtype=np.uint32) for w in WIDTHS]
    dms = [dmat(ctx, m) for m in mats]
    for counts in [(k,) * len(WIDTHS) for k in COUNTS] + [tuple(COUNTS[(i + 2) % len(COUNTS)] for i in range(len(WIDTHS)))]:
        pts = [rand_ext(field, dc, rng, k) for k in counts]
        vals = [rng.integers(0, p, size=(k, w, dc), dtype=np.uint32) for k, w in zip(counts, WIDTHS)]
        alpha = rand_ext(field, dc, rng)
        got = run_reduce(ctx, mats, pts, vals, alpha, dms=dms)
        if not any(counts):
            assert got == [], "no matrix has a point: no height has a vector"
            continue
        assert_reduce(got, reduce_ref(field, dc, mats, pts, vals, alpha), (h, counts))
    for m, d in zip(mats, dms):
        if m.shape[1]:
            assert np.array_equal(d.download(), m), "an input matrix was modified"
        d.free()


# ---------------------------------------------------------------- 2. one call for a mixed batch
@pytest.mark.parametrize("field,dc", CTXS)
def test_mixed_batch(ctxs, field, dc):
    ctx, p = ctxs(field, dc), P(field)
    rng = np.random.default_rng(2000 + dc)
    shapes = [(1 << 3, 5), (1 << 6, 9), (1 << 6, 2), (1 << 10, 3)]
    mats = [rng.integers(0, p, size=s, dtype=np.uint32) for s in shapes]
    shared = rand_ext(field, dc, rng, 1)
    # `shared` at all three heights and in both 2^6 matrices: one inverse vector per height serves every use
    pts = [np.concatenate([shared, rand_ext(field, dc, rng, 1)]), np.concatenate([rand_ext(field, dc, rng, 2), shared]),
           np.concatenate([shared, rand_ext(field, dc, rng, 1)]), np.concatenate([rand_ext(field, dc, rng, 1), shared, shared])]
    vals = [rng.integers(0, p, size=(len(q), s[1], dc), dtype=np.uint32) for q, s in zip(pts, shapes)]
    alpha = rand_ext(field, dc, rng)
    got = run_reduce(ctx, mats, pts, vals, alpha)
    assert [s for s, _ in got] == [(1 << 10, dc), (1 << 6, dc), (1 << 3, dc)], "tallest first, n_outs == 3"
    want = reduce_ref(field, dc, mats, pts, vals, alpha)
    assert_reduce(got, want, ("mixed",))
    by_h = {s[0]: g for s, g in got}
    single = [run_reduce(ctx, [m], [q], [v], alpha) for m, q, v in zip(mats, pts, vals)]
    assert np.array_equal(single[0][0][1], by_h[1 << 3]) and np.array_equal(single[3][0][1], by_h[1 << 10])
    # the 2^6 vector carries the running offset across its two matrices: it is NOT the sum of the two single calls
    summed = (single[1][0][1].astype(U) + single[2][0][1].astype(U)) % U(p)
    assert not np.array_equal(summed, by_h[1 << 6].astype(U))
    # the 2^6 matrices in the other order: another vector (the offsets follow the call order)
    swapped = run_reduce(ctx, [mats[2], mats[1]], [pts[2], pts[1]], [vals[2], vals[1]], alpha)
    assert np.array_equal(swapped[0][1], reduce_ref(field, dc, [mats[2], mats[1]], [pts[2], pts[1]], [vals[2], vals[1]], alpha)[1 << 6])
    assert not np.array_equal(swapped[0][1], by_h[1 << 6])
    # a matrix without points among matrices with points changes nothing and does not advance a_H; nor does a height
    # whose only matrix has no point get a vector
    none = np.empty((0, dc), dtype=np.uint32)
    extra, lone = rng.integers(0, p, size=(1 << 6, 4), dtype=np.uint32), rng.integers(0, p, size=(1 << 4, 3), dtype=np.uint32)
    again = run_reduce(ctx, [mats[0], mats[1], extra, mats[2], lone, mats[3]], [pts[0], pts[1], none, pts[2], none, pts[3]],
                       [vals[0], vals[1], np.empty((0, 4, dc), dtype=np.uint32), vals[2], np.empty((0, 3, dc), dtype=np.uint32), vals[3]], alpha)
    assert len(again) == 3
    for (s, g), (s2, g2) in zip(got, again):
        assert s == s2 and np.array_equal(g, g2)
    # another shift: another coset under the same rows
    shift = int(rng.integers(2, p))
    assert_reduce(run_reduce(ctx, mats[:3], pts[:3], vals[:3], alpha, shift=shift),
                  reduce_ref(field, dc, mats[:3], pts[:3], vals[:3], alpha, shift=shift), ("shift",))


# ---------------------------------------------------------------- 3. fold from the closed form
def fold_closed_form(field, dc, coef, la, beta):
    """coef: (n, dc) coefficients c_k.  Folding the bit-reversed evaluations over <w_n> by 2^la with beta gives the
    bit-reversed evaluations over <w_(n >> la)> of d_j = sum_{t < 2^la} beta^t * c_(j * 2^la + t)."""
    E, n = ext(field, dc), coef.shape[0]
    m = n >> la
    d, bt = E.zero(np.zeros(m, dtype=U)), E.one(0)
    for t in range(1 << la):
        d = E.add(d, E.mul(bc(bt, m), cols(coef[t::1 << la])))
        bt = E.mul(bt, [int(v) for v in beta])
    return ref.evals_dense(field, m, 1, rows(d))[ref.bitrev_indices(m)].astype(np.uint32), bt   # bt = beta^(2^la)


@pytest.mark.parametrize("la", [1, 2, 3, 4])
@pytest.mark.parametrize("field,dc", CTXS)
def test_fold_from_the_closed_form(ctxs, field, dc, la):
    """n = 2^la (one output row) .. 2^9 (2^8 -> 2^9 input rows: output rows below and above one block at la = 1).  The
    evaluations come from the definition (a Vandermonde product, no FFT on this side)."""
    ctx, p, E = ctxs(field, dc), P(field), ext(field, dc)
    rng = np.random.default_rng(3000 + 10 * la + dc)
    for log_n in range(la, 10):
        n = 1 << log_n
        coef = rng.integers(0, p, size=(n, dc), dtype=np.uint32)
        vec = ref.evals_dense(field, n, 1, coef)[ref.bitrev_indices(n)].astype(np.uint32)
        beta = rand_ext(field, dc, rng)
        roll = rng.integers(0, p, size=(n >> la, dc), dtype=np.uint32)
        want, b_top = fold_closed_form(field, dc, coef, la, beta)
        d_in, d_roll = ctx.upload(vec), ctx.upload(roll)
        out = ctx.fri_fold_device(d_in, la, beta)
        assert out.shape == (n >> la, dc)
        assert np.array_equal(out.download(), want), (log_n, "fold")
        out_r = ctx.fri_fold_device(d_in, la, beta, roll_in=d_roll)
        want_r = rows(E.add(cols(want), E.mul(bc(b_top, n >> la), cols(roll))))
        assert np.array_equal(out_r.download(), want_r), (log_n, "roll-in")
        assert np.array_equal(d_in.download(), vec) and np.array_equal(d_roll.download(), roll), "an input was modified"
        if log_n == 9:   # folding by 2^la == la folds by 2 with beta, beta^2, beta^4, ..
            cur, b = d_in, [int(v) for v in beta]
            for _ in range(la):
                nxt = ctx.fri_fold_device(cur, 1, np.array(b, dtype=np.uint32))
                if cur is not d_in:
                    cur.free()
                cur, b = nxt, E.mul(b, b)
            assert np.array_equal(cur.download(), want), "sequential arity-2 folds"
            cur.free()
        for d in (d_in, d_roll, out, out_r):
            d.free()


# ---------------------------------------------------------------- 4. edge operands
@pytest.mark.parametrize("field,dc", CTXS)
def test_edge_operands(ctxs, field, dc):
    """alpha, beta and the points from {0, 1, P - 1}^DC (every pattern of alpha and beta, every point pattern outside the
    coset); matrix, value and roll-in words from {0, 1, P - 1} with one all-zero and one all-(P - 1) column; h = 8 (and
    16 rows for the fold by 16, which 8 rows are too few for), against the definitions."""
    ctx, p, g, h = ctxs(field, dc), P(field), GEN(field), 8
    rng = np.random.default_rng(4000 + dc)
    edge = np.array([0, 1, p - 1], dtype=np.uint32)
    patterns = np.array(list(itertools.product((0, 1, p - 1), repeat=dc)), dtype=np.uint32)
    pts_all = np.array([z for z in patterns.tolist() if not ref.in_coset(field, dc, z, h, g)], dtype=np.uint32)
    assert len(pts_all) >= 3 ** dc - 2 and [0] * dc in pts_all.tolist()
    mats = [rng.choice(edge, size=(h, 6)), rng.choice(edge, size=(h, 3))]
    mats[0][:, 2], mats[0][:, 3] = 0, p - 1
    dms = [ctx.upload(m) for m in mats]
    # every point pattern, all of them the points of ONE matrix, under three alphas
    vals_all = [rng.choice(edge, size=(len(pts_all), 6, dc)), rng.choice(edge, size=(3, 3, dc))]
    vals_all[0][:, 2], vals_all[0][:, 3] = 0, p - 1
    for alpha in (rand_ext(field, dc, rng), [0] * dc, [p - 1] * dc):
        q = [pts_all, pts_all[[0, 1, len(pts_all) - 1]]]
        assert_reduce(run_reduce(ctx, mats, q, vals_all, alpha, dms=dms), reduce_ref(field, dc, mats, q, vals_all, alpha), ("points", tuple(alpha)))
    # every alpha pattern, at three edge points per matrix
    q = [pts_all[[0, 1, 2]], pts_all[[len(pts_all) - 1, 0, len(pts_all) // 2]]]
    vals = [vals_all[0][:3], vals_all[1]]
    for alpha in patterns:
        got = run_reduce(ctx, mats, q, vals, alpha, dms=dms)
        assert_reduce(got, reduce_ref(field, dc, mats, q, vals, alpha), ("alpha", tuple(alpha.tolist())))
        if not alpha.any():
            # alpha = 0 keeps column 0 only, and of the walk only its first (matrix, point): a_H is 0 after it
            E = ext(field, dc)
            z = tuple(int(v) for v in q[0][0])
            inv = inverse_vectors(field, dc, g, [(h, z)])[(h, z)]
            diff = bc(vals[0][0][0], h)
            diff[0] = (diff[0] + (U(p) - mats[0][:, 0].astype(U))) % U(p)
            assert np.array_equal(got[0][1], rows(E.mul(diff, inv)))
    for d in dms:
        d.free()
    # the fold: every beta pattern at every arity
    E = ext(field, dc)
    for la, n in ((1, 8), (2, 8), (3, 8), (4, 16)):
        vec, roll = rng.choice(edge, size=(n, dc)), rng.choice(edge, size=(n >> la, dc))
        vec[:, 1], vec[:, 2] = 0, p - 1
        d_in, d_roll = ctx.upload(vec), ctx.upload(roll)
        for beta in patterns:
            for r_np, r_d in ((None, None), (roll, d_roll)):
                out = ctx.fri_fold_device(d_in, la, beta, roll_in=r_d)
                got = out.download()
                out.free()
                assert np.array_equal(got, fold_ref(field, dc, vec, la, beta, r_np)), (la, tuple(beta.tolist()), r_np is not None)
                if not beta.any() and r_np is None and la == 1:   # beta = 0 keeps the even part: (e0 + e1) / 2
                    assert np.array_equal(got, rows(E.halve(E.add(cols(vec[0::2]), cols(vec[1::2])))))
        d_in.free()
        d_roll.free()


# ---------------------------------------------------------------- 5. the seams compose into a low-degree test
def compose(ctx, field, dc, log_blowup, traces, rng, spoil=False):
    """coset_lde_batch_device -> open_points_device at (z, z * g_h) -> fri_reduce_device -> fri_fold_device down to
    2^(log_blowup + 2) rows, rolling every lower height in -> the coefficients of the last vector, (rows, dc)."""
    p, g = P(field), GEN(field)
    E = ext(field, dc)
    ldes = [ctx.coset_lde_batch_device(t, log_blowup, g) for t in traces]
    z = [int(v) for v in rand_ext(field, dc, rng)]
    pts = [np.array([z, E.scale(z, field_ref.two_adic_generator(field, t.shape[0].bit_length() - 1))], dtype=np.uint32) for t in traces]
    vals = ctx.open_points_device(ldes, pts, added_bits=log_blowup)
    if spoil:
        vals = [v.copy() for v in vals]
        vals[1][1, 3, dc - 1] = (int(vals[1][1, 3, dc - 1]) + 1) % p
    ros = ctx.fri_reduce_device(ldes, pts, vals, rand_ext(field, dc, rng))
    heights = [r.shape[0] for r in ros]
    assert heights == sorted(set(t.shape[0] << log_blowup for t in traces), reverse=True)
    cur, nxt, schedule = ros[0], 1, []
    while cur.shape[0] > 1 << (log_blowup + 2):
        # by 4 when that lands on the next input height or on the final one, else by 2 - both arities occur
        target = heights[nxt] if nxt < len(heights) else 1 << (log_blowup + 2)
        la = 2 if len(schedule) % 2 == 0 and (cur.shape[0] >> 2) >= target else 1
        rolls = nxt < len(heights) and heights[nxt] == cur.shape[0] >> la
        out = ctx.fri_fold_device(cur, la, rand_ext(field, dc, rng), roll_in=ros[nxt] if rolls else None)
        cur.free()
        if rolls:
            ros[nxt].free()
            nxt += 1
        cur = out
        schedule.append(la)
    assert nxt == len(heights) and {1, 2} <= set(schedule), schedule
    coef, = ctx.dft_batch_device([cur], inverse=True, bit_reversed=True, shifts=[1])
    res = coef.download()
    for d in ldes + [cur, coef]:
        d.free()
    return res


@pytest.mark.parametrize("log_blowup", [1, 2])
@pytest.mark.parametrize("field,dc", CTXS)
def test_the_seams_compose_into_a_low_degree_test(ctxs, field, dc, log_blowup):
    """Reduced openings of polynomials of degree < h at consistent values are codewords of rate 2^-log_blowup, folding
    keeps the rate and the roll-ins add codewords of the same rate: the last vector, 2^(log_blowup + 2) evaluations, has
    degree < 4.  One opened value off by one and the quotient is no polynomial any more."""
    ctx, p = ctxs(field, dc), P(field)
    rng = np.random.default_rng(5000 + 10 * log_blowup + dc)
    shapes = [(1 << 4, 5), (1 << 6, 9), (1 << 6, 2), (1 << 8, 3)]
    traces = [ctx.upload(ref.evals_dense(field, h, 1, rng.integers(0, p, size=(h, w), dtype=np.uint32)).astype(np.uint32)) for h, w in shapes]
    good = compose(ctx, field, dc, log_blowup, traces, np.random.default_rng(77))
    assert good.shape == (1 << (log_blowup + 2), dc)
    assert not good[4:].any(), "every coefficient from 2^2 up is zero"
    assert good[:4].any(), "the low coefficients are not all zero"
    bad = compose(ctx, field, dc, log_blowup, traces, np.random.default_rng(77), spoil=True)
    assert bad[4:].any(), "a wrong opened value leaves high coefficients"
    for t in traces:
        t.free()


# ---------------------------------------------------------------- 6. refusals, and the context still proves
@pytest.mark.parametrize("field,dc", CTXS)
def test_refusals_and_the_context_still_proves(ctxs, oracle, field, dc):
    import ctypes as C
    import plonky3_recursion_amd as p3r
    from plonky3_recursion_amd import _lib
    ctx, p, g, h = ctxs(field, dc), P(field), GEN(field), 8
    rng = np.random.default_rng(6000 + dc)
    m = rng.integers(0, p, size=(h, 2), dtype=np.uint32)
    dm = ctx.upload(m)
    ok, alpha = rand_ext(field, dc, rng, 1), rand_ext(field, dc, rng)
    val = rng.integers(0, p, size=(1, 2, dc), dtype=np.uint32)
    u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32).ctypes.data_as(_lib.u32p)

    def refused(fn, code=P3R_EINVAL):
        with pytest.raises(p3r.P3rError) as e:
            fn()
        assert e.value.code == code, e.value
        assert str(e.value).split(":", 1)[1].strip(), "a refusal carries a message"

    def raw_reduce(handles, offs, points=ok, values=val, al=alpha, shift=0, n=None):
        """The C entry itself; whatever it answers, it must have handed out nothing the caller would have to free."""
        n = len(handles) if n is None else n
        arr = (C.c_void_p * max(1, len(handles)))(*handles)
        outs = (C.c_void_p * max(1, len(handles)))()
        n_outs = C.c_size_t(99)
        rc = ctx.lib.p3r_fri_reduce_dmat(ctx.h, arr, n, shift, (C.c_size_t * len(offs))(*offs), u32(points),
                                         None if values is None else u32(values), u32(al), outs, C.byref(n_outs))
        if rc != 0:
            assert n_outs.value == 0 and not any(outs), "a refused call allocates nothing the caller must free"
        else:
            for i in range(n_outs.value):
                p3r.device.DeviceMatrix(ctx, outs[i]).free()
        ctx.check(rc)
        return n_outs.value

    assert raw_reduce([dm.h], (0, 1)) == 1                                        # the accepted call
    refused(lambda: raw_reduce([dm.h], (0, 1), n=0))                              # n_mats == 0
    too_tall = 1 << (field_ref.PARAMS[field]["two_adicity"] + 1)
    tall = p3r.device.DeviceMatrix(ctx, ctx.ptr(ctx.lib.p3r_dmat_alloc(ctx.h, too_tall, 0)))   # width 0: no storage
    refused(lambda: raw_reduce([tall.h], (0, 0)))                                 # a height above the two-adicity
    refused(lambda: raw_reduce([dm.h, tall.h], (0, 1, 1)))
    tall.free()
    # (a height that is not a power of two cannot reach the entry: no handle of such a height can be made)
    assert not ctx.lib.p3r_dmat_alloc(ctx.h, 12, 2)
    refused(lambda: raw_reduce([dm.h, dm.h], (0, 1, 0), points=np.concatenate([ok, ok]), values=np.concatenate([val, val])))   # decreasing offsets
    refused(lambda: raw_reduce([dm.h, dm.h], (1, 0, 0)))
    for where in ("points", "values", "al"):                                       # a non-canonical word
        bad = {"points": ok, "values": val, "al": alpha}[where].copy()
        bad.reshape(-1)[-1] = p
        refused(lambda: raw_reduce([dm.h], (0, 1), **{where: bad}))
    refused(lambda: raw_reduce([dm.h], (0, 1), shift=p))
    refused(lambda: raw_reduce([dm.h], (0, 1), values=None))                       # values NULL, points and columns present
    w_h = field_ref.two_adic_generator(field, 3)
    base = lambda x: np.array([[x] + [0] * (dc - 1)], dtype=np.uint32)
    for shift in (0, 1, 4321):                                                     # a point IN the evaluation coset
        for j in (0, h - 1):
            z = base((shift or g) * pow(w_h, j, p) % p)
            refused(lambda: raw_reduce([dm.h], (0, 1), points=z, shift=shift))
            refused(lambda: raw_reduce([dm.h, dm.h], (0, 1, 3), points=np.concatenate([ok, ok, z]), values=np.concatenate([val] * 3), shift=shift))
    assert raw_reduce([dm.h], (0, 1)) == 1

    # ---- the fold
    vec = ctx.upload(rng.integers(0, p, size=(16, dc), dtype=np.uint32))
    beta = rand_ext(field, dc, rng)

    def raw_fold(in_h, la, b=beta, roll=None):
        out = C.c_void_p(12345)
        rc = ctx.lib.p3r_fri_fold_dmat(ctx.h, in_h, la, u32(b), roll, C.byref(out))
        if rc != 0:
            assert not out.value, "a refused call allocates nothing the caller must free"
        else:
            p3r.device.DeviceMatrix(ctx, out.value).free()
        ctx.check(rc)

    raw_fold(vec.h, 4)
    refused(lambda: raw_fold(vec.h, 0))                                            # la == 0
    refused(lambda: raw_fold(vec.h, 5), P3R_EUNSUPPORTED)                          # la > 4, as in the prover
    small = ctx.upload(rng.integers(0, p, size=(4, dc), dtype=np.uint32))
    refused(lambda: raw_fold(small.h, 3))                                          # n < 2^la
    wide = ctx.upload(rng.integers(0, p, size=(16, dc + 1), dtype=np.uint32))
    refused(lambda: raw_fold(wide.h, 1))                                           # width of `in` != DC
    wide_roll = ctx.upload(rng.integers(0, p, size=(4, dc + 1), dtype=np.uint32))
    refused(lambda: raw_fold(vec.h, 2, roll=wide_roll.h))                          # width of roll_in != DC
    refused(lambda: raw_fold(vec.h, 1, roll=small.h))                              # roll_in of another height
    raw_fold(vec.h, 2, roll=small.h)
    bad = beta.copy()
    bad[0] = p
    refused(lambda: raw_fold(vec.h, 1, b=bad))                                     # a non-canonical beta word
    # (n not a power of two: no such handle can be made, as above)
    for d in (dm, vec, small, wide, wide_roll):
        d.free()
    # the context proves the smallest layer of tests/test_gpu_prove.py, bytes equal to the oracle
    log_h, kw = ref.PROVE[field]
    kw = dict(kw, challenge_degree=dc) if dc != 4 else kw
    arrs = harness_lib.generate(field, log_h, seed=100 + log_h, horner_chain_len=20, sponge_chain_len=3, merkle_depth=5)
    L = layer_lib.OracleLayer(oracle, field, arrs, layer_lib.params(**kw))
    tables = L.tables()
    airs = [dict(kind=t["kind_id"], lanes=t["lanes"], horner_packed_steps=t["horner_k"], coeff_lookups=0) for t in tables]
    cap_, pd = ctx.prep_create(airs, [t["prep"] for t in tables])
    assert np.array_equal(cap_, L.prep_commit())
    proof = ctx.prove_batch(pd, [t["main"] for t in tables])
    L.verify(proof)
    assert proof == L.prove()
    pd.free()
