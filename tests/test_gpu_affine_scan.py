"""GPU: the recurrence seam (p3r_affine_scan_dmat: the three passes of k_affine_scan) word for word against the integer
loop tests/scan_ref.py.  No tolerance: field arithmetic is exact, so the result cannot depend on the tiling.

The heights come from the kernel's own constants (csrc/scan_plan.h; tests/test_affine_scan_host.py pins them to the ones
here): a thread of passes 0 and 2 owns ITEMS = 4 consecutive rows, a workgroup of BLOCK = 256 threads a tile of TILE = 1024
rows, and pass 1 is one workgroup whose threads carry ceil(tiles / BLOCK) tiles each.

  1              s[1] still goes to last_out; the 4-byte access path
  2              the same path, two rows
  4, 8           ITEMS and twice that: one and two threads, the first 16-byte accesses
  1024           one tile
  2048           two tiles: the first carry across workgroups
  2^19           512 tiles: the smallest height at which a thread of pass 1 carries more than one tile

The traces are those of tests/test_gpu_witness_program.py: base columns that walk 0, 1, p - 1, 2^30 before random words,
extension columns whose first rows take every coefficient from {0, 1, p - 1}."""
import functools

import numpy as np
import pytest

import scan_ref
import test_gpu_open_points as ref
from test_affine_scan_abi import valid_set
from test_gpu_witness_program import same, traces

pytestmark = pytest.mark.gpu
ctxs = ref.ctxs
P3R_EINVAL, P3R_EUNSUPPORTED = -1, -5
ITEMS, BLOCK, TILE = 4, 256, 1024
HEIGHTS = [1, 2, ITEMS, 2 * ITEMS, TILE, 2 * TILE, 2 * BLOCK * TILE]
SMALL = HEIGHTS[:-1]


@functools.lru_cache(maxsize=None)
def mixed_case(field, dc, h):
    """(traces, recurrences, the reference's matrix and totals) of the mixed set at one height: computed once."""
    mats = traces(field, dc, h, 2100 + dc)
    recs = valid_set(dc)
    p = ref.P(field)
    recs[0] = dict(recs[0], init=p - 1)   # a non-zero init on a sum, too
    want, last = scan_ref.columns(field, dc, recs, mats)
    want.setflags(write=False)
    last.setflags(write=False)
    return mats, recs, want, last


def run(ctx, recs, mats, want_last=True):
    dms = [ctx.upload(m) for m in mats]
    try:
        got = ctx.affine_scan_device(recs, dms, want_last=want_last)
        out, last = got if want_last else (got, None)
        m = out.download()
        out.free()
        return m, last
    finally:
        for d in dms:
            d.free()


@pytest.mark.parametrize("h", SMALL)
@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_every_form_in_one_call_word_for_word(ctxs, field, dc, h):
    """Base and extension recurrences of all three forms, both flag settings, interleaved outputs, non-zero inits."""
    ctx = ctxs(field, dc)
    mats, recs, want, want_last = mixed_case(field, dc, h)
    assert ctx.affine_scan_info(recs, [3, 2 * dc]) == {"n_out_columns": 3 * dc + 3, "n_products": 2, "n_sums": 2, "n_affine": 2}
    got, last = run(ctx, recs, mats)
    same(got, want)
    same(last, want_last)
    # an inclusive recurrence ends on its total, an exclusive one starts on its init
    assert got[h - 1, dc + 1] == want_last[2, 0] and np.array_equal(got[0, :dc], np.array([1, 2, 3, 4, 5][:dc], dtype=np.uint32))
    # a NULL last_out only enqueues; the download that follows sees the same matrix
    again, none = run(ctx, recs, mats, want_last=False)
    assert none is None
    same(again, want)


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_the_combine_is_applied_in_row_order(ctxs, field, dc):
    """Two adjacent maps swapped - inside a thread, across two threads, across two tiles - change the reference's result:
    a combine that commutes its operands cannot give both."""
    ctx, p, h = ctxs(field, dc), ref.P(field), 2 * TILE
    rng = np.random.default_rng(2110 + dc)
    base = rng.integers(2, p, size=(h, 2), dtype=np.uint32)
    ext = rng.integers(2, p, size=(h, 2 * dc), dtype=np.uint32)
    recs = [dict(out_col=0, mul=(0, 0), add=(0, 1), init=3), dict(out_col=1, mul=(1, 0), add=(1, dc), ext=True, init=[5] * dc)]
    want, want_last = scan_ref.columns(field, dc, recs, [base, ext])
    got, last = run(ctx, recs, [base, ext])
    same(got, want)
    same(last, want_last)
    for r in (1, ITEMS - 1, TILE - 1):   # rows r and r + 1
        b2, e2 = base.copy(), ext.copy()
        b2[[r, r + 1]], e2[[r, r + 1]] = base[[r + 1, r]], ext[[r + 1, r]]
        swapped, swapped_last = scan_ref.columns(field, dc, recs, [b2, e2])
        assert swapped_last[0, 0] != want_last[0, 0] and not np.array_equal(swapped_last[1], want_last[1]), r   # the reference first
        assert np.array_equal(swapped[:r + 1], want[:r + 1]) and not np.array_equal(swapped[r + 1], want[r + 1])
        got, last = run(ctx, recs, [b2, e2])
        same(got, swapped)
        same(last, swapped_last)


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_zeros_in_a_reset_the_accumulator(ctxs, field, dc):
    """a = 0 at tile boundaries, at thread boundaries and elsewhere: segmented sums.  And a column of zeros: s' = b."""
    ctx, p, h = ctxs(field, dc), ref.P(field), 2 * TILE
    mats = traces(field, dc, h, 2120 + dc)
    base, ext = mats[0].copy(), mats[1].copy()
    resets = [0, ITEMS - 1, ITEMS, 2 * ITEMS + 1, 700, TILE - 1, TILE, TILE + 1, TILE + ITEMS, h - 1]
    flag = np.ones(h, dtype=np.uint32)
    flag[resets] = 0
    base[:, 2] = flag                        # a in {0, 1}: a segmented sum of column 0
    ext[:, :dc] = 0
    ext[:, 0] = flag
    zeros = np.zeros((h, 1 + dc), dtype=np.uint32)
    recs = [dict(out_col=0, mul=(0, 2), add=(0, 0), init=9),
            dict(out_col=1, mul=(1, 0), add=(1, dc), ext=True, init=[1] * dc, inclusive=True),
            dict(out_col=1 + dc, mul=(2, 0), add=(0, 1), init=p - 1),
            dict(out_col=2 + dc, mul=(2, 1), add=(1, dc), ext=True, init=[p - 1] * dc),
            dict(out_col=2 + 2 * dc, mul=(2, 0), init=5, inclusive=True)]
    want, want_last = scan_ref.columns(field, dc, recs, [base, ext, zeros])
    # what the case is meant to hold, read off the reference: a reset row restarts the sum, a zero column copies b
    for r in resets[:-1]:
        assert want[r + 1, 0] == base[r, 0] and np.array_equal(want[r, 1:1 + dc], ext[r, dc:])
    assert np.array_equal(want[1:, 1 + dc], base[:-1, 1]) and np.array_equal(want[1:, 2 + dc:2 + 2 * dc], ext[:-1, dc:])
    assert not want[:, 2 + 2 * dc].any() and not want_last[4].any()
    got, last = run(ctx, recs, [base, ext, zeros])
    same(got, want)
    same(last, want_last)


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_the_height_at_which_pass_1_carries_two_tiles_per_thread(ctxs, field, dc):
    ctx, p, E, h = ctxs(field, dc), ref.P(field), ref.ext(field, dc), HEIGHTS[-1]
    assert h // TILE == 2 * BLOCK
    rng = np.random.default_rng(2130 + dc)
    base = rng.integers(0, p, size=(h, 2), dtype=np.uint32)
    base[::997, 0] = 0                                     # resets, at rows that drift across threads and tiles
    g = [int(v) for v in rng.integers(1, p, size=dc)]
    init = [int(v) for v in rng.integers(1, p, size=dc)]
    ext = np.empty((h, 2 * dc), dtype=np.uint32)
    ext[:, :dc] = g
    ext[:, dc:] = rng.integers(0, p, size=(h, dc), dtype=np.uint32)
    recs = [dict(out_col=0, mul=(0, 0), add=(0, 1), init=11),
            dict(out_col=1, mul=(1, 0), ext=True, init=init),
            dict(out_col=1 + dc, add=(1, dc), ext=True, init=init)]
    got, last = run(ctx, recs, [base, ext])
    assert got.shape == (h, 1 + 2 * dc)

    # the base affine recurrence in full, against a plain integer loop
    s, col = 11, np.empty(h, dtype=np.uint32)
    for r, (a, b) in enumerate(zip(base[:, 0].tolist(), base[:, 1].tolist())):
        col[r] = s
        s = (a * s + b) % p
    assert np.array_equal(got[:, 0], col) and last[0].tolist() == [s, 0, 0, 0, 0]

    # the product with the constant factor g: row r holds init * g^r.  Every tile boundary and its neighbours, walked with
    # g^TILE; 64 random rows and the total by fast exponentiation
    def row(r):
        return [int(v) for v in got[r, 1:1 + dc]]
    g_tile, g_inv = E.pow(g, TILE), E.inv(g)
    at = init                                              # init * g^(k TILE)
    for k in range(h // TILE):
        assert row(k * TILE) == at and row(k * TILE + 1) == E.mul(at, g), k
        if k:
            assert row(k * TILE - 1) == E.mul(at, g_inv), k
        at = E.mul(at, g_tile)
    assert [int(v) for v in last[1, :dc]] == at == E.mul(init, E.pow(g, h)) and not last[1, dc:].any()
    for r in [h - 1, 255 * TILE + 3] + rng.integers(0, h, size=62).tolist():
        assert row(r) == E.mul(init, E.pow(g, r)), r

    # the sum of a known column: cumulative sums per coefficient, mod p (2^19 words below 2^31 stay below 2^50)
    sums = (np.cumsum(ext[:, dc:].astype(np.uint64), axis=0) + np.array(init, dtype=np.uint64)) % p
    assert np.array_equal(got[0, 1 + dc:], np.array(init, dtype=np.uint32)) and np.array_equal(got[1:, 1 + dc:], sums[:-1].astype(np.uint32))
    assert np.array_equal(last[2, :dc], sums[-1].astype(np.uint32)) and not last[2, dc:].any()


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_refusals_leave_the_context_usable(ctxs, field, dc):
    import plonky3_recursion_amd as p3r
    ctx, p = ctxs(field, dc), ref.P(field)
    mats, recs, want, want_last = mixed_case(field, dc, 2 * ITEMS)
    d0, d1, d_short = ctx.upload(mats[0]), ctx.upload(mats[1]), ctx.upload(mats[0][:4])

    def valid():
        out, last = ctx.affine_scan_device(recs, [d0, d1], want_last=True)
        got = out.download()
        out.free()
        return np.array_equal(got, want) and np.array_equal(last, want_last)
    assert valid()

    def but(i, **kw):
        return recs[:i] + [dict(recs[i], **kw)] + recs[i + 1:]
    cases = [
        ("matrices of different heights", "share a height", dict(dmats=[d0, d1, d_short])),
        ("overlapping outputs", "overlap at column %d" % (dc - 1), dict(recs=but(0, out_col=dc - 1))),
        ("a gap below W", "is written by no recurrence", dict(recs=recs + [dict(out_col=3 * dc + 4, add=(0, 0))])),
        ("a non-canonical init", "non-canonical word 0 of init", dict(recs=but(4, init=p))),
        ("a non-zero-padded init", "of init is not zero", dict(recs=but(4, init=[1, 1]))),
        ("a column out of range", "reads column 3 of matrix 0", dict(recs=but(0, add=(0, 3)))),
        ("neither mul nor add", "neither mul nor add", dict(recs=but(2, mul=None))),
        ("no recurrence", "n_recs == 0", dict(recs=[])),
        ("no matrix", "n_mats == 0", dict(dmats=[])),
    ]
    for name, text, kw in cases:
        with pytest.raises(p3r.P3rError) as err:
            ctx.affine_scan_device(kw.get("recs", recs), kw.get("dmats", [d0, d1]), want_last=True)
        assert err.value.code == P3R_EINVAL and text in str(err.value), (name, str(err.value))
        assert valid(), "after: " + name
    # a NULL out, through the entry itself
    from plonky3_recursion_amd import device
    arr, n = device._recurrences(recs)
    assert ctx.lib.p3r_affine_scan_dmat(ctx.h, arr, n, None, 0, None, None) == P3R_EINVAL
    assert "out is NULL" in ctx.lib.p3r_last_error(ctx.h).decode() and valid()
    for d in (d0, d1, d_short):
        d.free()


def test_zk_contexts_are_refused(ctxs):
    import plonky3_recursion_amd as p3r
    recs = [p3r.Recurrence(0, add=(0, 0))]
    col = np.arange(8, dtype=np.uint32)[:, None]
    zk = p3r.Context(field="koala-bear", zk=1, zk_seed=1, log_blowup=1, max_log_arity=1, log_final_poly_len=0, query_pow_bits=3, num_queries=4)
    try:
        d = zk.upload(col)
        with pytest.raises(p3r.P3rError) as e:
            zk.affine_scan_device(recs, [d])
        assert e.value.code == P3R_EUNSUPPORTED and "zk" in str(e.value)
        d.free()
    finally:
        zk.close()
    got, last = run(ctxs("koala-bear", 4), recs, [col])
    assert got[:, 0].tolist() == [0, 0, 1, 3, 6, 10, 15, 21] and last.tolist() == [[28, 0, 0, 0, 0]]
