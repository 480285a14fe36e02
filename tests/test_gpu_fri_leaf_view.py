"""GPU: the commit-phase leaf view (p3r_fri_leaf_view_dmat, k_fri_leaf_view) by its closed form.  The view's row r is the
flattened extension elements r << LA .. (r + 1) << LA of the (n, DC) vector, so its row-major download is the vector's
row-major download reshaped to (n >> LA, DC << LA): every comparison is equality of words.  A workgroup is 256 lanes and
a lane owns one output row of one plane: L - LA from 0 to 9 puts the rows below, at and above one workgroup, and L = 13
makes several."""
import ctypes as C

import numpy as np
import pytest

import field_ref
import oracle_lib
import test_gpu_open_points as ref

pytestmark = pytest.mark.gpu
P3R_EINVAL, P3R_EUNSUPPORTED = -1, -5
ctxs = ref.ctxs


def vector(field, dc, L, la, rng):
    """Random words, with 0 and p - 1 in every position class: first / last element of a leaf row, first / last row."""
    p, n, a = ref.P(field), 1 << L, 1 << la
    v = rng.integers(0, p, size=(n, dc), dtype=np.uint32)
    edge = [0, p - 1]
    for i, r in enumerate((0, a - 1, n - a, n - 1)):   # first / last element of the first and of the last row
        v[r, :] = edge[i % 2]
        v[r, (i + 1) % dc] = edge[(i + 1) % 2]
    return v


def check(ctx, field, dc, L, la, rng):
    v = vector(field, dc, L, la, rng)
    d = ctx.upload(v)
    view = ctx.fri_leaf_view_device(d, la)
    assert view.shape == ((1 << L) >> la, dc << la)
    got, back = view.download(), d.download()
    view.free()
    d.free()
    assert np.array_equal(got, v.reshape((1 << L) >> la, dc << la)), (field, dc, L, la)
    assert np.array_equal(back, v), "the input is unchanged"


@pytest.mark.parametrize("field,dc", [("koala-bear", 4), ("koala-bear", 5), ("baby-bear", 4)])
@pytest.mark.parametrize("la", [1, 2, 3, 4])
def test_view_is_the_reshape(ctxs, field, dc, la):
    ctx, rng = ctxs(field, dc), np.random.default_rng(100 * la + dc)
    for L in range(la, 11):
        check(ctx, field, dc, L, la, rng)


@pytest.mark.parametrize("field,dc,la", [("koala-bear", 4, 2), ("koala-bear", 5, 4), ("baby-bear", 4, 1), ("koala-bear", 5, 3)])
def test_view_of_several_workgroups(ctxs, field, dc, la):
    check(ctxs(field, dc), field, dc, 13, la, np.random.default_rng(13 + la))


@pytest.mark.parametrize("field", ["koala-bear", "baby-bear"])
@pytest.mark.parametrize("mmcs", ["binary", "binary-cap1", "arity4"])
def test_view_commits_to_the_oracles_cap(oracle, field, mmcs):
    import plonky3_recursion_amd as p3r
    L, la, dc = 6, 2, 4
    kw = {"binary": {}, "binary-cap1": dict(cap_height=1), "arity4": dict(mmcs_arity=4, allow_unpinned_w32_defaults=True)}[mmcs]
    ctx = p3r.Context(field=field, **kw)
    v = vector(field, dc, L, la, np.random.default_rng(5))
    leaf = np.ascontiguousarray(v.reshape((1 << L) >> la, dc << la))
    want = oracle.commit4(field, [leaf])[0] if mmcs == "arity4" else oracle.commit(field, [leaf], kw.get("cap_height", 0))[0]
    d = ctx.upload(v)
    view = ctx.fri_leaf_view_device(d, la)
    cap, tree = ctx.commit_device([view])
    opened, _, proofs = tree.open_many([0, 5, 15])
    assert np.array_equal(cap, want)
    assert np.array_equal(opened, leaf[[0, 5, 15]])
    for i, q in enumerate((0, 5, 15)):
        p3r.mmcs_verify(ctx.cfg, cap, [leaf.shape], q, opened[i], proofs[i])
    tree.free()
    view.free()
    d.free()
    ctx.close()


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_refusals_and_the_context_is_usable_after_them(ctxs, field, dc):
    import plonky3_recursion_amd as p3r
    ctx, rng = ctxs(field, dc), np.random.default_rng(3)
    p = ref.P(field)
    good = ctx.upload(rng.integers(0, p, size=(8, dc), dtype=np.uint32))
    wide = ctx.upload(rng.integers(0, p, size=(8, dc + 1), dtype=np.uint32))
    narrow = ctx.upload(rng.integers(0, p, size=(8, dc - 1), dtype=np.uint32))

    def refused(fn, code):
        with pytest.raises(p3r.P3rError) as e:
            fn()
        assert e.value.code == code and str(e.value).split(": ", 1)[1].strip()

    refused(lambda: ctx.fri_leaf_view_device(good, 0), P3R_EINVAL)
    refused(lambda: ctx.fri_leaf_view_device(good, 5), P3R_EUNSUPPORTED)
    refused(lambda: ctx.fri_leaf_view_device(good, 4), P3R_EINVAL)        # 8 rows < 2^4
    refused(lambda: ctx.fri_leaf_view_device(wide, 1), P3R_EINVAL)
    refused(lambda: ctx.fri_leaf_view_device(narrow, 1), P3R_EINVAL)
    out = C.c_void_p(1)
    assert ctx.lib.p3r_fri_leaf_view_dmat(ctx.h, None, 1, C.byref(out)) == P3R_EINVAL and not out.value
    assert ctx.lib.p3r_fri_leaf_view_dmat(ctx.h, good.h, 1, None) == P3R_EINVAL
    # a height that is no power of two cannot be uploaded; the handle of a 0-width matrix has one and is refused by width
    empty = p3r.device.DeviceMatrix(ctx, ctx.ptr(ctx.lib.p3r_dmat_alloc(ctx.h, 8, 0)))
    refused(lambda: ctx.fri_leaf_view_device(empty, 1), P3R_EINVAL)
    for d in (wide, narrow, empty):
        d.free()
    check(ctx, field, dc, 3, 3, rng)       # one row: the whole vector
    view = ctx.fri_leaf_view_device(good, 1)
    assert np.array_equal(view.download(), good.download().reshape(4, 2 * dc))
    view.free()
    good.free()
