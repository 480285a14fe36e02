"""GPU: the witness seam (p3r_witness_program_dmat: k_trace_program<WitnessSink>, the interpreter with its fifth sink) word for word
against the integer interpreter tests/witness_ref.py.  No tolerance.

The traces: matrix 0 has three base columns - two that walk 0, 1, p - 1, 2^30 from different starts and then random
words, one random - and matrix 1 two flattened extension columns whose first rows take every coefficient from
{0, 1, p - 1}.  Heights 1 (the next row is the row itself), 2, 64 (one wave), 128 (two workgroups) and 2^12.  The edge
operands that a short trace cannot hold are in the program itself, as constants and challenges."""
import itertools

import numpy as np
import pytest

import test_gpu_open_points as ref
import witness_ref

pytestmark = pytest.mark.gpu
ctxs = ref.ctxs
P3R_EINVAL, P3R_EUNSUPPORTED = -1, -5
HEIGHTS = [1, 2, 64, 128, 1 << 12]


def traces(field, dc, h, seed):
    p = ref.P(field)
    rng = np.random.default_rng(seed)
    edge = np.array([0, 1, p - 1, 1 << 30], dtype=np.uint32)
    base = rng.integers(0, p, size=(max(h, 8), 3), dtype=np.uint32)
    base[:4, 0], base[:4, 1] = edge, np.roll(edge, 2)
    base[4:8, 0] = np.roll(edge, 1)
    ext = rng.integers(0, p, size=(max(h, 256), 2 * dc), dtype=np.uint32)
    pats = np.array(list(itertools.product([0, 1, p - 1], repeat=dc)), dtype=np.uint32)[:256]   # all-zero first
    ext[:len(pats), :dc] = pats
    ext[:len(pats), dc:] = pats[::-1]
    return [np.ascontiguousarray(base[:h]), np.ascontiguousarray(ext[:h])]


def every_op(field, dc):
    """Every op in both types, each value stored as soon as it stands: (the program, its width)."""
    import plonky3_recursion_amd as p3r
    p = ref.P(field)
    b = p3r.AirBuilder(field)
    x, y, z = b.local(0, 0), b.local(0, 1), b.next(0, 2)
    e, f = b.local_ext(1, 0), b.next_ext(1, dc)
    c_edge, c_rand, c_zero = b.challenge(0), b.challenge(1), b.challenge(2)
    pub = b.public(1)
    exprs = [
        lambda: x + y, lambda: x - y, lambda: x * y, lambda: -x, lambda: b.const(p - 1) * z + pub,      # base arithmetic
        lambda: e + f, lambda: e - f, lambda: e * f, lambda: -e,                                        # extension arithmetic
        lambda: e + x, lambda: y + e, lambda: e - x, lambda: y - e, lambda: e * z, lambda: z * e,       # mixed
        lambda: c_edge * e + c_rand, lambda: c_zero + x,
        lambda: b.inv(x), lambda: b.inv(y), lambda: x * b.inv(x), lambda: b.inv(0), lambda: b.inv(1),   # 0 for 0; x * x^-1 is 1 elsewhere
        lambda: b.inv(e), lambda: b.inv(p - 1),                                                         # an extension store between two base stores
        lambda: e * b.inv(e), lambda: b.inv(f), lambda: b.inv(c_edge), lambda: b.inv(c_zero), lambda: b.inv(c_rand * x),
        lambda: b.bits(x, 0, 31), lambda: b.bits(x, 30, 1), lambda: b.bits(x, 8, 8),
        lambda: b.bits(y, 0, 31), lambda: b.bits(y, 30, 1), lambda: b.bits(y, 8, 8),
        lambda: b.bits(p - 1, 0, 31), lambda: b.bits(p - 1, 30, 1), lambda: b.bits(p - 1, 8, 8),
        lambda: b.bits(0, 0, 31), lambda: b.bits(0, 30, 1), lambda: b.bits(0, 8, 8),
        lambda: b.bits(z, 3, 17), lambda: b.bits(x * y, 0, 16),
        lambda: b.row(), lambda: b.row() * b.row() - pub,
        lambda: b.is_first_row(), lambda: b.is_last_row(), lambda: b.is_transition(), lambda: b.is_transition() * (b.next(0, 0) - x),
        lambda: b.next(0, 0), lambda: b.next_ext(1, 0),                                                 # the last row reads row 0
    ]
    col, widths = 0, []
    for expr in exprs:
        v = expr()
        widths.append(dc if witness_ref.kinds(b.program())[v.idx] else 1)
        b.store(v, col)
        col += widths[-1]
    assert any(widths[i:i + 3] == [1, dc, 1] for i in range(len(widths) - 2))
    return b, col


def challenges_of(field, dc, seed):
    p = ref.P(field)
    rng = np.random.default_rng(seed)
    ch = np.zeros((3, dc), dtype=np.uint32)
    ch[0] = ([0, 1, p - 1] * 2)[:dc]
    ch[1] = rng.integers(1, p, size=dc, dtype=np.uint32)
    return ch


def run(ctx, prog, mats, height=None, publics=(), challenges=()):
    dms = [ctx.upload(m) for m in mats]
    try:
        out = ctx.witness_device(prog, dms, height=height, public_values=publics, challenges=challenges)
        got = out.download()
        out.free()
        return got
    finally:
        for d in dms:
            d.free()


def same(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint32
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]


@pytest.mark.parametrize("h", HEIGHTS)
@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_every_op_in_both_types_word_for_word(ctxs, field, dc, h):
    ctx, p = ctxs(field, dc), ref.P(field)
    prog, width = every_op(field, dc)
    mats = traces(field, dc, h, 2000 + dc)
    publics, ch = [7, p - 2], challenges_of(field, dc, 2001)
    info = ctx.witness_program_info(prog, [3, 2 * dc])
    assert info["n_out_columns"] == width and info["peak_live"] <= 48
    want = witness_ref.columns(field, dc, prog.program(), mats, None, publics, ch)
    got = run(ctx, prog, mats, None, publics, ch)
    same(got, want)
    # what the case is meant to hold, read off the reference: the wrap of NEXT, and INV's zero
    assert got[h - 1, width - 1 - dc] == mats[0][0, 0] and np.array_equal(got[h - 1, width - dc:], mats[1][0, :dc])
    if h >= 64:
        base = 5 + 10 * dc + 2 * dc   # the column of inv(x)
        assert want[0, base] == 0 and want[1, base] == 1 and want[2, base] == p - 1       # x = 0, 1, p - 1
        prod = want[:, base + 2]                                                           # x * inv(x)
        assert np.array_equal(prod, (mats[0][:, 0] != 0).astype(np.uint32)) and (prod == 0).any()
        e_inv = want[:, base + 5:base + 5 + dc]                                            # inv(e): the all-zero element first
        assert not e_inv[0].any() and e_inv[1:].any(axis=1).all()


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_a_table_of_the_row_index_has_no_input(ctxs, field, dc):
    import plonky3_recursion_amd as p3r
    ctx = ctxs(field, dc)
    b = p3r.AirBuilder(field)
    r = b.row()
    b.store(r, 0)
    b.store(b.bits(r, 4, 4), 1)
    b.store(b.is_last_row() * r, 2)
    want = witness_ref.columns(field, dc, b.program(), [], 256)
    assert want.shape == (256, 3) and want[:, 0].tolist() == list(range(256)) and want[255, 2] == 255
    same(run(ctx, b, [], 256), want)


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_forty_eight_live_values(ctxs, field, dc):
    """48 cells alive at once, then folded; with the 48 alive as extension values - the largest slot file - too."""
    import plonky3_recursion_amd as p3r
    from plonky3_recursion_amd import _lib as L
    ctx, h = ctxs(field, dc), 128
    mats = traces(field, dc, h, 2010 + dc)
    for ext in (False, True):
        b = p3r.AirBuilder(field)
        c = b.challenge(1)
        vals = [b.next(0, k % 3) if k % 5 == 0 else b.local(0, k % 3) for k in range(L.P3R_AIR_MAX_LIVE - (1 if ext else 0))]
        if ext:
            vals = [c * v for v in vals]   # c dies with the last product: 48 alive at the peak
        acc = vals[0]
        for k, v in enumerate(vals[1:]):
            acc = acc * v if k % 2 else acc + v
        b.store(acc, 0)
        assert ctx.witness_program_info(b, [3, 2 * dc])["peak_live"] == L.P3R_AIR_MAX_LIVE
        ch = challenges_of(field, dc, 2011)
        same(run(ctx, b, mats, None, (), ch), witness_ref.columns(field, dc, b.program(), mats, None, (), ch))


def limit_program(n_live):
    """n_live cells alive at once, summed and stored."""
    from plonky3_recursion_amd import _lib as L
    prog = [(L.P3R_AIR_LOCAL, 0, k % 3) for k in range(n_live)]
    acc = 0
    for k in range(1, n_live):
        prog.append((L.P3R_AIR_ADD, acc, k))
        acc = len(prog) - 1
    prog.append((L.P3R_AIR_STORE, acc, 0))
    return np.array(prog, dtype=np.uint32)


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_refusals_leave_the_context_usable(ctxs, field, dc):
    import plonky3_recursion_amd as p3r
    from plonky3_recursion_amd import _lib as L
    ctx, p = ctxs(field, dc), ref.P(field)
    two_adicity = ref.field_ref.PARAMS[field]["two_adicity"]
    mats = traces(field, dc, 8, 2020)
    d0, d1, d_short = ctx.upload(mats[0]), ctx.upload(mats[1]), ctx.upload(mats[0][:4])
    good = p3r.AirBuilder(field)
    good.store(good.inv(good.local(0, 0)) + good.public(0), 0)
    good.store(good.challenge(0) * good.local_ext(1, 0), 1)
    ch = challenges_of(field, dc, 2021)
    want = witness_ref.columns(field, dc, good.program(), mats, None, [5], ch)

    def valid(height=None):
        out = ctx.witness_device(good, [d0, d1], height=height, public_values=[5], challenges=ch)
        got = out.download()
        out.free()
        return np.array_equal(got, want)
    assert valid() and valid(8)
    LOC, ST, ROW = L.P3R_AIR_LOCAL, L.P3R_AIR_STORE, L.P3R_AIR_ROW
    table = [(ROW, 0, 0), (ST, 0, 0)]
    cases = [
        ("a height that is not the matrices'", P3R_EINVAL, "height", dict(height=16)),
        ("matrices of different heights", P3R_EINVAL, "share a height", dict(dmats=[d0, d_short], prog=[(LOC, 0, 0), (ST, 0, 0)])),
        ("no matrix and no height", P3R_EINVAL, "power of two", dict(dmats=[], prog=table, height=0)),
        ("no matrix and 3 rows", P3R_EINVAL, "power of two", dict(dmats=[], prog=table, height=3)),
        ("no matrix and 2^(two-adicity + 1) rows", P3R_EINVAL, "two-adicity", dict(dmats=[], prog=table, height=1 << (two_adicity + 1))),
        ("an input with no matrix", P3R_EINVAL, "matrix 0 of 0", dict(dmats=[], prog=[(LOC, 0, 0), (ST, 0, 0)], height=8)),
        ("a public value out of range", P3R_EINVAL, "public value 0 of 0", dict(publics=[])),
        ("a challenge out of range", P3R_EINVAL, "challenge 0 of 0", dict(challenges=[])),
        ("a matrix out of range", P3R_EINVAL, "matrix 2 of 2", dict(prog=[(LOC, 2, 0), (ST, 0, 0)])),
        ("a column out of range", P3R_EINVAL, "column 3 of matrix 0", dict(prog=[(LOC, 0, 3), (ST, 0, 0)])),
        ("extension columns out of range", P3R_EINVAL, "+ DC", dict(prog=[(L.P3R_AIR_LOCAL_EXT, 1, dc + 1), (ST, 0, 0)])),
        ("a non-canonical public value", P3R_EINVAL, "non-canonical public value 0", dict(publics=[p])),
        ("a non-canonical challenge", P3R_EINVAL, "non-canonical word 1 of challenge 0", dict(challenges=[[0, p] + [0] * (dc - 2)])),
        ("no STORE", P3R_EINVAL, "no STORE", dict(prog=[(LOC, 0, 0)])),
        ("a column stored twice", P3R_EINVAL, "stored twice", dict(prog=[(LOC, 0, 0), (ST, 0, 0), (ST, 0, 0)])),
        ("a column not stored", P3R_EINVAL, "stored by no instruction", dict(prog=[(LOC, 0, 0), (ST, 0, 0), (ST, 0, 2)])),
        ("a sink of another seam", P3R_EINVAL, "ASSERT_ZERO in a witness program", dict(prog=[(LOC, 0, 0), (ST, 0, 0), (L.P3R_AIR_ASSERT_ZERO, 0, 0)])),
        ("49 live values", P3R_EUNSUPPORTED, "P3R_AIR_MAX_LIVE", dict(prog=limit_program(L.P3R_AIR_MAX_LIVE + 1))),
    ]
    for name, code, text, kw in cases:
        with pytest.raises(p3r.P3rError) as err:
            ctx.witness_device(kw.get("prog", good), kw.get("dmats", [d0, d1]), height=kw.get("height"), public_values=kw.get("publics", [5]),
                               challenges=kw.get("challenges", ch))
        assert err.value.code == code and text in str(err.value), (name, str(err.value))
        assert valid(), "after: " + name
    # a NULL out, through the entry itself
    from plonky3_recursion_amd import device
    arr, n = device._air_insns(table)
    assert ctx.lib.p3r_witness_program_dmat(ctx.h, arr, n, None, 0, 8, None, 0, None, 0, None) == P3R_EINVAL
    assert "out is NULL" in ctx.lib.p3r_last_error(ctx.h).decode() and valid()

    # the entries that were here before still take the four ops for unknown ops
    for op in (L.P3R_AIR_INV, L.P3R_AIR_BITS, L.P3R_AIR_ROW, L.P3R_AIR_STORE):
        b = 8 << 8 if op == L.P3R_AIR_BITS else 0
        constraint = [(LOC, 0, 0), (op, 0, b), (L.P3R_AIR_ASSERT_ZERO, 0, 0)]
        lookup = [(LOC, 0, 0), (op, 0, b), (L.P3R_AIR_LOOKUP, 0, 0), (L.P3R_AIR_LOOKUP_END, 0, 0)]
        calls = [lambda: ctx.check_device(constraint, [d0]),
                 lambda: ctx.quotient_device(constraint, [d0], 1, 0, [1] + [0] * (dc - 1)),
                 lambda: ctx.logup_device(lookup, [d0]),
                 lambda: ctx.lookup_check_device([(lookup, [d0])]),
                 lambda: ctx.lookup_multiplicities_device((lookup, [d0]), [])]
        for call in calls:
            with pytest.raises(p3r.P3rError) as err:
                call()
            assert err.value.code == P3R_EINVAL and "unknown op %d" % op in str(err.value), str(err.value)
    assert valid()
    for d in (d0, d1, d_short):
        d.free()


def test_zk_contexts_are_refused(ctxs):
    import plonky3_recursion_amd as p3r
    b = p3r.AirBuilder("koala-bear")
    b.store(b.row(), 0)
    zk = p3r.Context(field="koala-bear", zk=1, zk_seed=1, log_blowup=1, max_log_arity=1, log_final_poly_len=0, query_pow_bits=3, num_queries=4)
    try:
        with pytest.raises(p3r.P3rError) as e:
            zk.witness_device(b, [], height=8)
        assert e.value.code == P3R_EUNSUPPORTED and "zk" in str(e.value)
    finally:
        zk.close()
    ctx = ctxs("koala-bear", 4)
    same(run(ctx, b, [], 8), np.arange(8, dtype=np.uint32)[:, None])
