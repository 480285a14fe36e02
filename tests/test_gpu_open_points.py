"""GPU: the value half of Pcs::open (p3r_open_points / p3r_open_points_dmat) against Python integers.  Every expected
value is f(z) = sum_k c_k z^k of KNOWN coefficients in the challenge field (tests/field_ref.py); the matrices handed to
the library hold the evaluations of those polynomials, computed here from the definition (no FFT on this side), laid out
as a committed LDE keeps them.  Every comparison is exact equality of canonical words.

The dot kernel groups columns by eight for one or two points and by FOUR for three or four (kernels_open.hip.h::pts_cols), so
the widths below go around both group widths: 3, 4, 5 and 7, 8, 9, plus 0, 1 and 17."""
import functools
import itertools

import numpy as np
import pytest

import field_ref
import harness_lib
import layer_lib
import oracle_lib

pytestmark = pytest.mark.gpu

CTXS = [("koala-bear", 4), ("koala-bear", 5), ("baby-bear", 4)]
P3R_EINVAL = -1
PROVE = {"koala-bear": (5, dict(log_blowup=1, max_log_arity=1, log_final_poly_len=0, query_pow_bits=3, num_queries=4)),
         "baby-bear": (6, dict(log_blowup=2, max_log_arity=2, log_final_poly_len=1, query_pow_bits=4, num_queries=5))}
WIDTHS = (0, 1, 3, 4, 5, 7, 8, 9, 17)


def cap():
    from plonky3_recursion_amd import _lib
    return _lib.P3R_OPEN_POINTS_PER_PASS


@pytest.fixture(scope="module")
def ctxs():
    import plonky3_recursion_amd as p3r
    made = {}

    def get(field, dc):
        if (field, dc) not in made:
            made[(field, dc)] = p3r.Context(field=field, cap_height=0, commit_pow_bits=0, challenge_degree=dc, **PROVE[field][1])
        return made[(field, dc)]
    yield get
    for c in made.values():
        c.close()


def P(field):
    return field_ref.PARAMS[field]["p"]


def GEN(field):
    return field_ref.PARAMS[field]["gen"]


def ext(field, dc):
    return field_ref.quartic(field) if dc == 4 else field_ref.quintic(field)


def omega_table(field, h):
    """w_h^0 .. w_h^(h-1) as uint64."""
    p, w = P(field), field_ref.two_adic_generator(field, h.bit_length() - 1)
    t = np.ones(1, dtype=np.uint64)
    while t.size < h:
        t = np.concatenate([t, t * np.uint64(pow(w, t.size, p)) % np.uint64(p)])
    return t


def bitrev_indices(h):
    bits = h.bit_length() - 1
    return np.array([field_ref.bit_reverse(i, bits) for i in range(h)], dtype=np.int64)


def evals_of_terms(field, h, shift, terms):
    """One column in natural order: sum over (k, c) of c * x_i^k at x_i = shift * w_h^i."""
    p, wt, idx = P(field), omega_table(field, h), np.arange(h, dtype=np.int64)
    col = np.zeros(h, dtype=np.uint64)
    for k, c in terms:
        col = (col + wt[(idx * k) % h] * np.uint64(c * pow(shift, k, p) % p)) % np.uint64(p)
    return col


def evals_dense(field, h, shift, coef):
    """coef: h x w canonical coefficients -> h x w evaluations over shift * <w_h> in natural order, from the definition."""
    p, wt, idx = P(field), omega_table(field, h), np.arange(h, dtype=np.int64)
    spow = np.array([pow(shift, k, p) for k in range(h)], dtype=np.uint64)
    V = wt[(idx[:, None] * idx[None, :]) % h] * spow[None, :] % np.uint64(p)           # V[i, k] = x_i^k
    c64 = coef.astype(np.uint64)
    if coef.shape[1] == 0:
        return np.zeros((h, 0), dtype=np.uint64)
    return np.stack([(V * c64[:, c][None, :] % np.uint64(p)).sum(axis=1) % np.uint64(p) for c in range(coef.shape[1])], axis=1).reshape(h, coef.shape[1])


def committed_layout(evals_nat, added_bits, bit_reversed, rng, p):
    """The matrix a caller holds: (h << added_bits) rows; the interpolant's evaluations are rows 0 .. h in bit-reversed
    order, or rows k << added_bits in natural order.  Every other row is noise that must not be read."""
    h, w = evals_nat.shape
    m = rng.integers(0, p, size=(h << added_bits, w), dtype=np.uint32)
    if bit_reversed:
        m[:h] = evals_nat[bitrev_indices(h)]
    else:
        m[::1 << added_bits] = evals_nat
    return m


def want_dense(field, dc, coef, z):
    """sum_k coef[k, c] z^k for every column: (w, dc) canonical words."""
    E, p = ext(field, dc), P(field)
    zp, cur = [], E.one(0)
    for _ in range(coef.shape[0]):
        zp.append(cur)
        cur = E.mul(cur, [int(v) for v in z])
    zp = np.array(zp, dtype=np.uint64)                                                   # [k][dc]
    return ((coef.astype(np.uint64)[:, :, None] * zp[:, None, :]) % np.uint64(p)).sum(axis=0) % np.uint64(p)


def want_terms(field, dc, terms, z):
    E = ext(field, dc)
    acc = E.zero(0)
    for k, c in terms:
        acc = E.add(acc, E.scale(E.pow([int(v) for v in z], k), c))
    return acc


def in_coset(field, dc, z, h, shift):
    E = ext(field, dc)
    return E.pow([int(v) for v in z], h) == [pow(shift, h, P(field))] + [0] * (dc - 1)


def random_points(field, dc, k, rng):
    return rng.integers(0, P(field), size=(k, dc), dtype=np.uint32)


def check(got, coef, pts, field, dc, what):
    assert got.shape == (len(pts), coef.shape[1], dc), what
    for j, z in enumerate(pts):
        assert np.array_equal(got[j].astype(np.uint64).reshape(coef.shape[1], dc), want_dense(field, dc, coef, z).reshape(coef.shape[1], dc)), what + (j,)


# ---------------------------------------------------------------- 1. heights x widths x points per matrix
@pytest.mark.parametrize("h", [1, 2, 4, 8, 1 << 8, 1 << 9])
@pytest.mark.parametrize("field,dc", CTXS)
def test_heights_widths_and_point_counts(ctxs, field, dc, h):
    """h = 1 .. 8: below and at a lane's four-row share of the weights; 2^8: one block's rows; 2^9: two chunks.  Every
    width goes with 0, 1, 2, cap and cap + 1 points (cap + 1: a second pass over the matrix), all widths in one call."""
    import plonky3_recursion_amd as p3r
    ctx, p, g = ctxs(field, dc), P(field), GEN(field)
    rng = np.random.default_rng(h * 31 + dc)
    coefs = [rng.integers(0, p, size=(h, w), dtype=np.uint32) for w in WIDTHS]
    mats = [evals_dense(field, h, g, c)[bitrev_indices(h)].astype(np.uint32) for c in coefs]
    dms = [p3r.device.DeviceMatrix(ctx, ctx.ptr(ctx.lib.p3r_dmat_alloc(ctx.h, h, 0))) if m.shape[1] == 0 else ctx.upload(m) for m in mats]
    for k in (0, 1, 2, cap(), cap() + 1):
        pts = [random_points(field, dc, k, rng) for _ in WIDTHS]
        got = ctx.open_points_device(dms, pts)
        for w, c, q, v in zip(WIDTHS, coefs, pts, got):
            check(v, c, q, field, dc, (h, w, k))
    for d in dms:
        d.free()


# ---------------------------------------------------------------- 2. many chunks, the serial reduce
@pytest.mark.parametrize("field,dc", CTXS)
def test_many_chunks_of_a_single_column(ctxs, field, dc):
    ctx, p, g, h = ctxs(field, dc), P(field), GEN(field), 1 << 14
    rng = np.random.default_rng(14 + dc)
    terms = [(0, 5), (1, p - 1), (h // 2, 7), (h - 1, int(rng.integers(1, p))), (1234, int(rng.integers(1, p)))]
    nat = evals_of_terms(field, h, g, terms).astype(np.uint32)[:, None]
    for bit_reversed in (True, False):
        dm = ctx.upload(nat[bitrev_indices(h)] if bit_reversed else nat)
        for k in (1, cap() + 1):
            pts = random_points(field, dc, k, rng)
            got, = ctx.open_points_device([dm], [pts], bit_reversed=bit_reversed)
            for j, z in enumerate(pts):
                assert [int(v) for v in got[j, 0]] == want_terms(field, dc, terms, z), (bit_reversed, k, j)
        dm.free()


# ---------------------------------------------------------------- 3. orders, blow-ups, shifts
@pytest.mark.parametrize("field,dc", CTXS)
def test_orders_blowups_and_shifts(ctxs, field, dc):
    ctx, p, h, w = ctxs(field, dc), P(field), 16, 3
    rng = np.random.default_rng(300 + dc)
    coef = rng.integers(0, p, size=(h, w), dtype=np.uint32)
    pts = random_points(field, dc, 3, rng)
    for shift in (None, 1, int(rng.integers(2, p))):
        nat = evals_dense(field, h, GEN(field) if shift is None else shift, coef).astype(np.uint32)
        for added_bits in (0, 1, 2, 3):
            for bit_reversed in (True, False):
                m = committed_layout(nat, added_bits, bit_reversed, rng, p)
                dm = ctx.upload(m)
                got, = ctx.open_points_device([dm], [pts], added_bits=added_bits, shift=shift, bit_reversed=bit_reversed)
                check(got, coef, pts, field, dc, (shift, added_bits, bit_reversed))
                assert np.array_equal(dm.download(), m), "the input matrix was modified"
                dm.free()


# ---------------------------------------------------------------- 4. commit-shaped input in, interpolant values out
@pytest.mark.parametrize("field,dc", CTXS)
def test_from_the_lde_of_coset_lde_batch_device(ctxs, field, dc):
    """A trace with known coefficients -> coset_lde_batch_device (what commit_device commits) -> the values of Pcs::open."""
    ctx, p, g = ctxs(field, dc), P(field), GEN(field)
    rng = np.random.default_rng(400 + dc)
    for h, w in ((8, 5), (64, 9)):
        coef = rng.integers(0, p, size=(h, w), dtype=np.uint32)
        trace = ctx.upload(evals_dense(field, h, 1, coef).astype(np.uint32))     # evaluations over the subgroup, natural order
        pts = random_points(field, dc, cap() + 1, rng)
        for added_bits in (0, 1, 2, 3):
            lde = ctx.coset_lde_batch_device(trace, added_bits, g)
            assert lde.shape == (h << added_bits, w)
            got, = ctx.open_points_device([lde], [pts], added_bits=added_bits)
            check(got, coef, pts, field, dc, (h, added_bits))
            lde.free()
        trace.free()


# ---------------------------------------------------------------- 5. one call for a mixed batch
@pytest.mark.parametrize("field,dc", CTXS)
def test_mixed_batch_equals_single_calls(ctxs, field, dc):
    ctx, p, g = ctxs(field, dc), P(field), GEN(field)
    rng = np.random.default_rng(500 + dc)
    shapes = [(1 << 3, 5), (1 << 6, 9), (1 << 6, 2), (1 << 10, 3)]
    coefs, dms = [], []
    for h, w in shapes:
        if h <= 64:
            c = rng.integers(0, p, size=(h, w), dtype=np.uint32)
            nat = evals_dense(field, h, g, c)
        else:   # closed forms: X^k, a constant, a sparse polynomial
            terms = [[(777, 1)], [(0, p - 1)], [(k, int(rng.integers(1, p))) for k in (0, 1, 511, 512, 1023)]]
            c = np.zeros((h, w), dtype=np.uint32)
            for col, ts in enumerate(terms):
                for k, v in ts:
                    c[k, col] = v
            nat = np.stack([evals_of_terms(field, h, g, ts) for ts in terms], axis=1)
        coefs.append(c)
        dms.append(ctx.upload(committed_layout(nat.astype(np.uint32), 2, True, rng, p)))
    shared = random_points(field, dc, 1, rng)
    # matrices 1 and 2 (both 2^6) share `shared`; `shared` is also used at heights 2^3 and 2^10
    pts = [np.concatenate([shared, random_points(field, dc, 1, rng)]), np.concatenate([random_points(field, dc, cap(), rng), shared]),
           shared, np.concatenate([random_points(field, dc, 2, rng), shared])]
    got = ctx.open_points_device(dms, pts, added_bits=2)
    for i, (dm, q) in enumerate(zip(dms, pts)):
        one, = ctx.open_points_device([dm], [q], added_bits=2)
        assert np.array_equal(got[i], one), i
        check(got[i], coefs[i], q, field, dc, (i,))
    for d in dms:
        d.free()


# ---------------------------------------------------------------- 6. edge operands
@pytest.mark.parametrize("field,dc", CTXS)
def test_edge_operands(ctxs, field, dc):
    """Coefficients from {0, 1, P - 1}; every point pattern from {0, 1, P - 1}^DC outside the coset (z = 0 and the
    base-field points 1 and P - 1 among them); an all-zero column."""
    ctx, p, g, h = ctxs(field, dc), P(field), GEN(field), 8
    rng = np.random.default_rng(600 + dc)
    coef = rng.choice(np.array([0, 1, p - 1], dtype=np.uint32), size=(h, 6))
    coef[:, 2] = 0
    coef[:, 3] = p - 1
    coef[:, 4] = 1
    pts = np.array([z for z in itertools.product((0, 1, p - 1), repeat=dc) if not in_coset(field, dc, z, h, g)], dtype=np.uint32)
    assert len(pts) >= 3 ** dc - 2 and [0] * dc in pts.tolist() and [1] + [0] * (dc - 1) in pts.tolist()
    dm = ctx.upload(evals_dense(field, h, g, coef)[bitrev_indices(h)].astype(np.uint32))
    got, = ctx.open_points_device([dm], [pts])
    check(got, coef, pts, field, dc, ("edge",))
    zero = pts.tolist().index([0] * dc)
    assert np.array_equal(got[zero][:, 0], coef[0]) and not got[zero][:, 1:].any(), "f(0) is the constant coefficient"
    assert not got[:, 2].any(), "the all-zero column"
    dm.free()


# ---------------------------------------------------------------- 7. host form
@pytest.mark.parametrize("field,dc", CTXS)
def test_host_form_equals_device_form(ctxs, field, dc):
    ctx, p = ctxs(field, dc), P(field)
    rng = np.random.default_rng(700 + dc)
    mats = [rng.integers(0, p, size=(h, w), dtype=np.uint32) for h, w in ((32, 5), (4, 9), (256, 1), (16, 0))]
    pts = [random_points(field, dc, k, rng) for k in (cap() + 1, 1, 0, 2)]
    dms = [ctx.upload(m) for m in mats[:3]]
    for added_bits, bit_reversed, shift in ((0, True, None), (2, True, 1), (1, False, 12345)):
        host = ctx.open_points(mats, pts, added_bits=added_bits, shift=shift, bit_reversed=bit_reversed)
        dev = ctx.open_points_device(dms, pts[:3], added_bits=added_bits, shift=shift, bit_reversed=bit_reversed)
        assert host[3].shape == (2, 0, dc)
        for a, b in zip(host, dev):
            assert np.array_equal(a, b)
    for d in dms:
        d.free()


# ---------------------------------------------------------------- 8. refusals, and the context still proves
@pytest.mark.parametrize("field,dc", CTXS)
def test_refusals_are_einval_and_the_context_still_proves(ctxs, oracle, field, dc):
    import ctypes as C
    import plonky3_recursion_amd as p3r
    from plonky3_recursion_amd import _lib
    ctx, p, g, h = ctxs(field, dc), P(field), GEN(field), 8
    rng = np.random.default_rng(800 + dc)
    m = rng.integers(0, p, size=(4 * h, 2), dtype=np.uint32)
    dm = ctx.upload(m)
    w_h = field_ref.two_adic_generator(field, 3)

    def refused(fn):
        with pytest.raises(p3r.P3rError) as e:
            fn()
        assert e.value.code == P3R_EINVAL, e.value
        assert str(e.value), "a refusal carries a message"

    base = lambda x: np.array([[x] + [0] * (dc - 1)], dtype=np.uint32)
    for shift in (g, 1, 4321):
        for j in (0, h - 1):                                                   # a point IN the evaluation coset
            z = base(shift * pow(w_h, j, p) % p)
            for bit_reversed in (True, False):
                refused(lambda: ctx.open_points_device([dm], [z], added_bits=2, shift=shift, bit_reversed=bit_reversed))
                refused(lambda: ctx.open_points([m], [z], added_bits=2, shift=shift, bit_reversed=bit_reversed))
                # ... also behind good points and behind a good matrix
                good = random_points(field, dc, cap(), rng)
                refused(lambda: ctx.open_points_device([dm, dm], [good, np.concatenate([good, z])], added_bits=2, shift=shift,
                                                       bit_reversed=bit_reversed))
    ok = random_points(field, dc, 1, rng)
    bad = ok.copy()
    bad[0, dc - 1] = p
    refused(lambda: ctx.open_points_device([dm], [bad]))                       # non-canonical point word
    refused(lambda: ctx.open_points([m], [bad]))
    refused(lambda: ctx.open_points_device([dm], [ok], shift=p))               # non-canonical shift
    refused(lambda: ctx.open_points_device([dm], [ok], added_bits=6))          # height 32 < 2^6
    refused(lambda: ctx.open_points([np.zeros((3, 2), dtype=np.uint32)], [ok]))   # height not a power of two
    refused(lambda: ctx.open_points([np.zeros((0, 2), dtype=np.uint32)], [ok]))
    noncanon = m.copy()
    noncanon[5, 1] = p
    refused(lambda: ctx.open_points([noncanon], [ok]))
    out = np.empty(64, dtype=np.uint32)
    arr = (C.c_void_p * 2)(dm.h, dm.h)
    okp = ok.ctypes.data_as(_lib.u32p)
    raw = lambda offs, order=1: ctx.check(ctx.lib.p3r_open_points_dmat(ctx.h, arr, 2, 0, 0, order, (C.c_size_t * 3)(*offs), okp,
                                                                       out.ctypes.data_as(_lib.u32p)))
    refused(lambda: raw((0, 1, 0)))                                            # offsets that decrease
    refused(lambda: raw((1, 0, 0)))
    refused(lambda: raw((0, 1, 1), order=2))                                   # unknown order
    raw((0, 1, 1))                                                             # the accepted call still works
    one, = ctx.open_points_device([dm], [ok])
    assert np.array_equal(out[:2 * dc].reshape(1, 2, dc), one)
    dm.free()
    # the context proves the smallest layer of tests/test_gpu_prove.py, bytes equal to the oracle
    log_h, kw = PROVE[field]
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


# ---------------------------------------------------------------- 9. the tall case: closed-form columns only
TALL_H, TALL_W, TALL_BITS = 1 << 18, 24, 2


def tall_terms(field):
    p, h = P(field), TALL_H
    rng = np.random.default_rng(18)
    cols = [[(k, 1)] for k in (0, 1, 2, 3, h // 2, h - 1, 12345, h // 4 + 1)]                 # X^k -> z^k
    cols += [[(0, c)] for c in (0, 1, p - 1, 424242)]                                            # constants (one all zero)
    cols += [[(int(k), int(c)) for k, c in zip(rng.choice(h, size=n, replace=False), rng.integers(1, p, size=n))]
             for n in (2, 3, 4, 5, 6, 7, 8, 8, 8, 8, 8, 8)]                                      # sparse, at most 8 terms
    assert len(cols) == TALL_W
    return cols


@functools.lru_cache(maxsize=None)
def tall_matrix(field):
    """The committed shape: 2^20 x 24, the evaluations in the first 2^18 rows (bit-reversed), noise in the others."""
    p, g = P(field), GEN(field)
    rev = bitrev_indices(TALL_H)
    m = np.random.default_rng(19).integers(0, p, size=(TALL_H << TALL_BITS, TALL_W), dtype=np.uint32)
    for c, terms in enumerate(tall_terms(field)):
        m[:TALL_H, c] = evals_of_terms(field, TALL_H, g, terms)[rev]
    return m


@pytest.mark.parametrize("field,dc", CTXS)
def test_tall_matrix_by_closed_forms(ctxs, field, dc):
    ctx = ctxs(field, dc)
    pts = random_points(field, dc, 4, np.random.default_rng(900 + dc))
    dm = ctx.upload(tall_matrix(field))
    got, = ctx.open_points_device([dm], [pts], added_bits=TALL_BITS)
    dm.free()
    for j, z in enumerate(pts):
        for c, terms in enumerate(tall_terms(field)):
            assert [int(v) for v in got[j, c]] == want_terms(field, dc, terms, z), (j, c)
