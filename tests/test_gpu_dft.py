"""GPU: the public DFT seam (p3r_dft / p3r_dft_batch_dmat: TwoAdicSubgroupDft::dft_batch, idft_batch, coset_dft_batch,
coset_idft_batch) against the DEFINITION of the transform.  Every expected value is computed here with Python integers
or uint64 numpy from  e_i = sum_k c_k x_i^k,  x_i = shift * w_h^i  (natural order; row i of a bit-reversed matrix is the
point bitrev(i)) - no FFT on the expected side - plus bit-exact round trips, batching, the oracle-pinned LDE by
composition, cache isolation from the LDE and the refusals."""
import numpy as np
import pytest

import harness_lib
import layer_lib
import oracle_lib

pytestmark = pytest.mark.gpu

FIELDS = ["koala-bear", "baby-bear"]
TWO_ADICITY = {"koala-bear": 24, "baby-bear": 27}
P3R_EINVAL = -1

# the smallest layer of tests/test_gpu_prove.py per field: the contexts below are built for it, so that the refusal test
# can prove on the very context that refused
PROVE = {"koala-bear": (5, dict(log_blowup=1, max_log_arity=1, log_final_poly_len=0, query_pow_bits=3, num_queries=4)),
         "baby-bear": (6, dict(log_blowup=2, max_log_arity=2, log_final_poly_len=1, query_pow_bits=4, num_queries=5))}

SMALL = [(h, w) for h in (1, 2, 4, 8, 64) for w in (1, 3)]
# 2^11: the last single-tile size; 2^12: generic two-pass; 2^13, 2^14: the first lean sizes; 2^16: forward split capped
# at 2^8 rows; 2^20 x 2 (KoalaBear): the 2^14-cell tiles of the inverse column pass, the 2^12-cell line tiles
LARGE = [(1 << n, w) for n in (11, 12, 13, 14, 16) for w in (1, 16, 33)]
TALL = (1 << 20, 2)


def cases(sizes, tall=False):
    out = [(f, h, w) for f in FIELDS for (h, w) in sizes]
    if tall:
        out.append(("koala-bear",) + TALL)
    return out


@pytest.fixture(scope="module")
def ctxs():
    import plonky3_recursion_amd as p3r
    made = {}

    def get(field):
        if field not in made:
            made[field] = p3r.Context(field=field, cap_height=0, commit_pow_bits=0, **PROVE[field][1])
        return made[field]
    yield get
    for c in made.values():
        c.close()


def omega(field, h):
    p = oracle_lib.MODULUS[field]
    return pow(oracle_lib.GENERATOR[field], (p - 1) // h, p)


def bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def shifts_of(field, rng):
    p = oracle_lib.MODULUS[field]
    return [1, oracle_lib.GENERATOR[field], int(rng.integers(2, p))]


def point(field, h, shift, row, bit_reversed):
    """The evaluation point of row `row` of an h-row evaluation matrix."""
    p = oracle_lib.MODULUS[field]
    log_h = h.bit_length() - 1
    return shift * pow(omega(field, h), bitrev(row, log_h) if bit_reversed else row, p) % p


def power_table(x, h, p):
    """x^0 .. x^(h-1) mod p as uint64, built by doubling: [t, t * x^len(t)]."""
    t = np.ones(1, dtype=np.uint64)
    while t.size < h:
        t = np.concatenate([t, t * np.uint64(pow(x, t.size, p)) % np.uint64(p)])
    return t


def evaluate(coeffs64, powers, p):
    """Every column of `coeffs64` (h x w, canonical, uint64) at x, `powers` = power_table(x): sum_k c_k x^k."""
    return (coeffs64 * powers[:, None] % np.uint64(p)).sum(axis=0) % np.uint64(p)


# ---------------------------------------------------------------- 1. the definition, every cell
@pytest.mark.parametrize("field,h,w", cases(SMALL))
def test_every_cell_is_the_definition(ctxs, field, h, w):
    ctx, p = ctxs(field), oracle_lib.MODULUS[field]
    rng = np.random.default_rng(1000 + h * 7 + w)
    m = rng.integers(0, p, size=(h, w), dtype=np.uint32)
    cols = [[int(v) for v in m[:, c]] for c in range(w)]
    inv_h = pow(h, p - 2, p)
    for shift in shifts_of(field, rng):
        for bit_reversed in (False, True):
            xs = [point(field, h, shift, i, bit_reversed) for i in range(h)]
            # forward: e_i = sum_k c_k x_i^k
            want = np.array([[sum(c[k] * pow(xs[i], k, p) for k in range(h)) % p for c in cols] for i in range(h)], dtype=np.uint32)
            got, = ctx.dft_batch([m], shifts=shift, bit_reversed=bit_reversed)
            assert np.array_equal(got, want), (shift, bit_reversed, "forward")
            # inverse: c_k = 1/h * sum_i e_i x_i^-k  (the rows of m are the evaluations at x_i)
            xinv = [pow(x, p - 2, p) for x in xs]
            want = np.array([[inv_h * sum(c[i] * pow(xinv[i], k, p) for i in range(h)) % p for c in cols] for k in range(h)], dtype=np.uint32)
            got, = ctx.dft_batch([m], inverse=True, shifts=shift, bit_reversed=bit_reversed)
            assert np.array_equal(got, want), (shift, bit_reversed, "inverse")


# ---------------------------------------------------------------- 2. the definition where the path changes
@pytest.mark.parametrize("field,h,w", cases(LARGE, tall=True))
def test_sampled_rows_are_the_definition(ctxs, field, h, w):
    ctx, p = ctxs(field), oracle_lib.MODULUS[field]
    rng = np.random.default_rng(2000 + h + w)
    m = rng.integers(0, p, size=(h, w), dtype=np.uint32)
    m64, dm = m.astype(np.uint64), ctx.upload(m)
    rows = [int(r) for r in rng.choice(h, size=16, replace=False)]
    for shift in (1, oracle_lib.GENERATOR[field]):
        for bit_reversed in (False, True):
            fwd, = ctx.dft_batch_device([dm], shifts=shift, bit_reversed=bit_reversed)
            inv, = ctx.dft_batch_device([dm], inverse=True, shifts=shift, bit_reversed=bit_reversed)
            e, c = fwd.download(), inv.download().astype(np.uint64)
            fwd.free(), inv.free()
            for r in rows:
                t = power_table(point(field, h, shift, r, bit_reversed), h, p)
                # forward: row r of the result is the input polynomials at x_r
                assert np.array_equal(e[r], evaluate(m64, t, p)), (shift, bit_reversed, "forward", r)
                # inverse: the resulting polynomials take the input's row r at x_r
                assert np.array_equal(m[r], evaluate(c, t, p)), (shift, bit_reversed, "inverse", r)
    dm.free()


# ---------------------------------------------------------------- 3. round trips, bit-exact, inputs untouched
@pytest.mark.parametrize("field,h,w", cases(SMALL + LARGE, tall=True))
def test_round_trips_are_exact_and_leave_the_input_alone(ctxs, field, h, w):
    ctx, p = ctxs(field), oracle_lib.MODULUS[field]
    rng = np.random.default_rng(3000 + h + w)
    m = rng.integers(0, p, size=(h, w), dtype=np.uint32)
    dm = ctx.upload(m)
    for shift in (1, oracle_lib.GENERATOR[field]):
        for bit_reversed in (False, True):
            kw = dict(shifts=shift, bit_reversed=bit_reversed)
            e, = ctx.dft_batch_device([dm], **kw)
            back, = ctx.dft_batch_device([e], inverse=True, **kw)
            assert np.array_equal(back.download(), m), (shift, bit_reversed, "inverse(forward(c))")
            e.free(), back.free()
            c, = ctx.dft_batch_device([dm], inverse=True, **kw)
            back, = ctx.dft_batch_device([c], **kw)
            assert np.array_equal(back.download(), m), (shift, bit_reversed, "forward(inverse(e))")
            c.free(), back.free()
            assert np.array_equal(dm.download(), m), "the input matrix was modified"
    dm.free()


# ---------------------------------------------------------------- 4. one call, four heights, four shifts
@pytest.mark.parametrize("field", FIELDS)
def test_mixed_batch_equals_single_calls(ctxs, field):
    ctx, p = ctxs(field), oracle_lib.MODULUS[field]
    rng = np.random.default_rng(4000)
    # 2^13, 2^14 and 2^15 rows: two column sizes (2^6, 2^7) and two line lengths (2^7, 2^8) in one batch - both mixed kernels
    shapes = [(1 << 13, 5), (1 << 14, 3), (1 << 7, 2), (1, 1), (1 << 15, 2)]
    mats = [rng.integers(0, p, size=s, dtype=np.uint32) for s in shapes]
    shifts = [oracle_lib.GENERATOR[field], 1, int(rng.integers(2, p)), int(rng.integers(2, p)), int(rng.integers(2, p))]
    dms = [ctx.upload(m) for m in mats]
    for inverse in (False, True):
        for bit_reversed in (False, True):
            outs = ctx.dft_batch_device(dms, inverse=inverse, shifts=shifts, bit_reversed=bit_reversed)
            assert [o.shape for o in outs] == shapes
            for dm, s, o in zip(dms, shifts, outs):
                single, = ctx.dft_batch_device([dm], inverse=inverse, shifts=[s], bit_reversed=bit_reversed)
                assert np.array_equal(o.download(), single.download()), (inverse, bit_reversed, o.shape)
                single.free(), o.free()
    for dm, m in zip(dms, mats):
        assert np.array_equal(dm.download(), m)
        dm.free()


# ---------------------------------------------------------------- 5. the oracle-pinned LDE, by composition
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("h", [1 << 6, 1 << 12])
def test_composition_is_the_oracle_lde(ctxs, oracle, field, h):
    ctx, p, g = ctxs(field), oracle_lib.MODULUS[field], oracle_lib.GENERATOR[field]
    rng = np.random.default_rng(5000 + h)
    e = rng.integers(0, p, size=(h, 3), dtype=np.uint32)
    coef, = ctx.dft_batch([e], inverse=True)
    for added_bits in (1, 2):
        padded = np.zeros((h << added_bits, 3), dtype=np.uint32)
        padded[:h] = coef
        got, = ctx.dft_batch([padded], shifts=g, bit_reversed=True)
        assert np.array_equal(got, oracle.coset_lde(field, e, added_bits, g)), added_bits
        back, = ctx.dft_batch([ctx.coset_lde_batch(e, added_bits, g)], inverse=True, shifts=g, bit_reversed=True)
        assert not back[h:].any(), "an LDE of degree < h has no higher coefficients"
        assert np.array_equal(back[:h], coef), added_bits


# ---------------------------------------------------------------- 6. a DFT call changes nothing the LDE reads
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("h", [1 << 6, 1 << 12, 1 << 13])
def test_lde_is_the_same_before_and_after_dft_calls(field, h):
    import plonky3_recursion_amd as p3r
    p, g = oracle_lib.MODULUS[field], oracle_lib.GENERATOR[field]
    rng = np.random.default_rng(6000 + h)
    e = rng.integers(0, p, size=(h, 3), dtype=np.uint32)
    ctx = p3r.Context(field=field)   # its own context: the LDE below is the first thing it ever transforms
    try:
        before = [ctx.coset_lde_batch(e, ab, g) for ab in (0, 1)]
        for inverse in (False, True):
            for bit_reversed in (False, True):
                ctx.dft_batch([e], inverse=inverse, shifts=g, bit_reversed=bit_reversed)
                ctx.dft_batch([e], inverse=inverse, bit_reversed=bit_reversed)
        after = [ctx.coset_lde_batch(e, ab, g) for ab in (0, 1)]
        for a, b in zip(before, after):
            assert a.tobytes() == b.tobytes()
    finally:
        ctx.close()


# ---------------------------------------------------------------- 7. refusals, and the context still proves
@pytest.mark.parametrize("field", FIELDS)
def test_refusals_are_einval_and_the_context_still_proves(ctxs, oracle, field):
    import ctypes as C
    import plonky3_recursion_amd as p3r
    from plonky3_recursion_amd import _lib
    ctx, p = ctxs(field), oracle_lib.MODULUS[field]
    ok = np.arange(8, dtype=np.uint32).reshape(4, 2)

    def refused(fn):
        with pytest.raises(p3r.P3rError) as e:
            fn()
        assert e.value.code == P3R_EINVAL, e.value

    refused(lambda: ctx.dft_batch([np.zeros((3, 2), dtype=np.uint32)]))             # not a power of two
    refused(lambda: ctx.dft_batch([np.zeros((0, 2), dtype=np.uint32)]))
    refused(lambda: ctx.dft_batch([ok], shifts=0))                                   # shift 0
    refused(lambda: ctx.dft_batch([ok], shifts=p))                                   # shift >= P
    refused(lambda: ctx.dft_batch([ok], inverse=True, shifts=p + 5))
    bad = ok.copy()
    bad[2, 1] = p
    refused(lambda: ctx.dft_batch([bad]))                                            # non-canonical host word
    out = np.empty_like(ok)
    raw = lambda d, o: ctx.check(ctx.lib.p3r_dft(ctx.h, ok.ctypes.data_as(_lib.u32p), 4, 2, d, 1, o, out.ctypes.data_as(_lib.u32p)))
    refused(lambda: raw(2, 0))                                                       # unknown direction
    refused(lambda: raw(0, 2))                                                       # unknown order
    refused(lambda: ctx.dft_batch_device([]))                                        # n_mats == 0
    dm = ctx.upload(ok)
    refused(lambda: ctx.dft_batch_device([dm], shifts=[0]))
    refused(lambda: ctx.dft_batch_device([dm], shifts=[p]))
    arr, outs, sh = (C.c_void_p * 1)(dm.h), (C.c_void_p * 1)(), (C.c_uint32 * 1)(1)
    refused(lambda: ctx.check(ctx.lib.p3r_dft_batch_dmat(ctx.h, arr, 1, 7, sh, 0, outs)))
    refused(lambda: ctx.check(ctx.lib.p3r_dft_batch_dmat(ctx.h, arr, 1, 0, sh, 7, outs)))
    # above the two-adicity: refused on the height alone - the matrix is allocated (width 1), never transformed
    tall = p3r.device.DeviceMatrix(ctx, ctx.ptr(ctx.lib.p3r_dmat_alloc(ctx.h, 2 << TWO_ADICITY[field], 1)))
    refused(lambda: ctx.dft_batch_device([tall]))
    refused(lambda: ctx.dft_batch_device([dm, tall], inverse=True, bit_reversed=True))   # nothing of the batch runs
    tall.free()
    # the accepted call still works, and the context proves the smallest layer of tests/test_gpu_prove.py
    got, = ctx.dft_batch_device([dm])
    want, = ctx.dft_batch([ok])
    assert np.array_equal(got.download(), want)
    got.free(), dm.free()
    log_h, kw = PROVE[field]
    arrs = harness_lib.generate(field, log_h, seed=100 + log_h, horner_chain_len=20, sponge_chain_len=3, merkle_depth=5)
    L = layer_lib.OracleLayer(oracle, field, arrs, layer_lib.params(**kw))
    tables = L.tables()
    airs = [dict(kind=t["kind_id"], lanes=t["lanes"], horner_packed_steps=t["horner_k"], coeff_lookups=0) for t in tables]
    cap, pd = ctx.prep_create(airs, [t["prep"] for t in tables])
    assert np.array_equal(cap, L.prep_commit())
    proof = ctx.prove_batch(pd, [t["main"] for t in tables])
    L.verify(proof)
    assert proof == L.prove()
    pd.free()


# ---------------------------------------------------------------- 8. edge words, every cell, by closed forms
# Columns of the words where a butterfly's range argument is tightest (P - 1 and 0, constant, alternating, a single
# entry).  Such a column is a geometric sum, so F(z) = sum_j E_j z^j has a closed form that costs O(1) per point given
# z^h and z^(h/2), and EVERY cell of the transform is checked.  The closed forms are kept free of inverses by clearing
# the denominator:  den(z) * F(z) == num(z)  determines F(z) wherever den(z) != 0, and where it is zero (z = 1, z = -1)
# the sum is written out.  KINDS names a column by its entries in natural index order.
KINDS = ("zero", "const", "odd", "impulse0", "impulse_last", "alt", "upper", "signtop")
# a row pattern of a bit-reversed evaluation matrix, read in natural point order
BITREV_KIND = {"zero": "zero", "const": "const", "odd": "upper", "impulse0": "impulse0", "impulse_last": "impulse_last",
               "alt": "signtop"}


def kind_column(kind, h, p):
    """The column itself (uint64, natural order), c = P - 1."""
    c, e = p - 1, np.zeros(h, dtype=np.uint64)
    if kind == "const":
        e[:] = c
    elif kind == "odd":
        e[1::2] = c
    elif kind == "impulse0":
        e[0] = c
    elif kind == "impulse_last":
        e[h - 1] = c
    elif kind == "alt":             # c * (-1)^j
        e[0::2], e[1::2] = c, (p - c) % p
    elif kind == "upper":
        e[h // 2:] = c
    elif kind == "signtop":         # c below h/2, -c from there
        e[:h // 2], e[h // 2:] = c, (p - c) % p
    else:
        assert kind == "zero"
    return e


def closed_form_holds(kind, F, z, zhalf, zh, h, p):
    """Is F[i] = sum_j E_j z[i]^j for the column `kind`?  z, zhalf = z^(h/2), F: uint64 arrays; zh = z^h, one integer
    for all points (they lie on one coset)."""
    P, c, m1 = np.uint64(p), p - 1, p - 1
    if kind == "zero":
        return not F.any()
    if kind == "impulse0":
        return bool((F == c).all())
    if kind == "impulse_last":      # z * z^(h-1) = z^h
        return bool((F * z % P == c * zh % p).all())
    if kind == "const":             # (z - 1) sum z^j = z^h - 1
        den, num, at_zero = (z + m1) % P, c * (zh - 1) % p, c * h % p
    elif kind == "odd":             # sum of z^(2j+1):  (z^2 - 1) F = z (z^h - 1)
        den, num, at_zero = (z * z % P + m1) % P, c * (zh - 1) % p * z % P, c * (h // 2) % p * z % P
    elif kind == "alt":             # (-z - 1) sum (-z)^j = (z^h - 1), h even
        den, num, at_zero = (z + 1) % P, c * (1 - zh) % p, c * h % p
    elif kind == "upper":           # z^(h/2) sum_{j < h/2} z^j
        den, num, at_zero = (z + m1) % P, c * zhalf % P * ((zhalf + m1) % P) % P, c * (h // 2) % p
    else:                           # (1 - z^(h/2)) sum_{j < h/2} z^j
        assert kind == "signtop"
        t = (zhalf + m1) % P
        den, num, at_zero = (z + m1) % P, (p - c) % p * (t * t % P) % P, 0
    return bool(np.where(den != 0, F * den % P == num, F == at_zero).all())


def bitrev_indices(h):
    bits, idx = h.bit_length() - 1, np.arange(h, dtype=np.uint64)
    rev = np.zeros(h, dtype=np.uint64)
    for i in range(bits):
        rev |= ((idx >> np.uint64(i)) & np.uint64(1)) << np.uint64(bits - 1 - i)
    return rev.astype(np.int64)


def points_forward(field, h, shift, bit_reversed):
    """z, z^(h/2), z^h of the rows of a forward result: row i is the point shift * w^i (w^bitrev(i))."""
    p = oracle_lib.MODULUS[field]
    idx = bitrev_indices(h) if bit_reversed else np.arange(h, dtype=np.int64)
    z = power_table(omega(field, h), h, p)[idx] * np.uint64(shift) % np.uint64(p)
    zhalf = np.where(idx & 1, np.uint64(pow(shift, h // 2, p) * (p - 1) % p), np.uint64(pow(shift, h // 2, p)))
    return z, zhalf, pow(shift, h, p)


def points_inverse(field, h, shift):
    """Coefficient k of an inverse result is  shift^-k / h * F(w^-k),  F over the evaluations in natural point order:
    the points w^-k, their powers, and the factor h * shift^k that turns the coefficient into F."""
    p = oracle_lib.MODULUS[field]
    z = power_table(pow(omega(field, h), p - 2, p), h, p)
    zhalf = np.where(np.arange(h) & 1, np.uint64(p - 1), np.uint64(1))
    return z, zhalf, 1, power_table(shift, h, p) * np.uint64(h % p) % np.uint64(p)


def assert_closed_forms_are_the_definition(field):
    """At h = 64: closed_form_holds accepts exactly sum_j E_j z^j as evaluate() computes it, on a coset and on the subgroup
    (where z = 1 and z = -1 occur), and refuses a cell that is off by one; BITREV_KIND is the bit-reversal of the rows."""
    p, h = oracle_lib.MODULUS[field], 64
    rev = bitrev_indices(h)
    for kind, nat in BITREV_KIND.items():
        assert np.array_equal(kind_column(kind, h, p)[rev], kind_column(nat, h, p)), kind
    sets = [points_forward(field, h, s, br) for s in (1, oracle_lib.GENERATOR[field]) for br in (False, True)]
    sets.append(points_inverse(field, h, 1)[:3])
    for kind in KINDS:
        col = kind_column(kind, h, p)[:, None]
        for z, zhalf, zh in sets:
            F = np.array([evaluate(col, power_table(int(x), h, p), p)[0] for x in z], dtype=np.uint64)
            assert closed_form_holds(kind, F, z, zhalf, zh, h, p), (field, kind)
            for at in (0, 1, h // 2, h - 1):
                off = F.copy()
                off[at] = (off[at] + np.uint64(1)) % np.uint64(p)
                assert not closed_form_holds(kind, off, z, zhalf, zh, h, p), (field, kind, at)


def edge_word_matrices(p, h, w):
    """[(matrix, kind of each column)]: all P - 1; alternating 0 / P - 1 by row; alternating by column; a single P - 1
    at row 0; at row h - 1; the column (P - 1) * (-1)^i."""
    out = []
    for kinds in (["const"] * w, ["odd"] * w, [("const" if c & 1 else "zero") for c in range(w)], ["impulse0"] * w,
                  ["impulse_last"] * w, ["alt"] * w):
        out.append((np.stack([kind_column(k, h, p) for k in kinds], axis=1).astype(np.uint32), kinds))
    return out


@pytest.mark.parametrize("field,h,w", cases(LARGE, tall=True))
def test_edge_words_every_cell_by_closed_forms(ctxs, field, h, w):
    ctx, p = ctxs(field), oracle_lib.MODULUS[field]
    assert_closed_forms_are_the_definition(field)
    mats = edge_word_matrices(p, h, w)
    dms = [ctx.upload(m) for m, _ in mats]

    def check_columns(out, kinds, holds, what):
        # equal input columns give equal output columns: the closed form on the first of each kind, equality on the rest
        first = {}
        for c, kind in enumerate(kinds):
            if kind in first:
                assert np.array_equal(out[:, c], out[:, first[kind]]), what + (c, "differs from column", first[kind])
            else:
                first[kind] = c
                assert holds(kind, out[:, c].astype(np.uint64)), what + (c, kind)

    for shift in (1, oracle_lib.GENERATOR[field]):
        for bit_reversed in (False, True):
            z, zhalf, zh = points_forward(field, h, shift, bit_reversed)
            outs = ctx.dft_batch_device(dms, shifts=shift, bit_reversed=bit_reversed)
            for (m, kinds), o in zip(mats, outs):
                check_columns(o.download(), kinds, lambda kind, F: closed_form_holds(kind, F, z, zhalf, zh, h, p),
                              (shift, bit_reversed, "forward"))
                o.free()
            iz, izhalf, izh, scale = points_inverse(field, h, shift)
            outs = ctx.dft_batch_device(dms, inverse=True, shifts=shift, bit_reversed=bit_reversed)
            for (m, kinds), o in zip(mats, outs):
                nat = [BITREV_KIND[k] for k in kinds] if bit_reversed else kinds
                check_columns(o.download(), nat,
                              lambda kind, c: closed_form_holds(kind, c * scale % np.uint64(p), iz, izhalf, izh, h, p),
                              (shift, bit_reversed, "inverse"))
                o.free()
    for dm, (m, _) in zip(dms, mats):
        assert np.array_equal(dm.download(), m), "the input matrix was modified"
        dm.free()
