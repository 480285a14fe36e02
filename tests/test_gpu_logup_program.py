"""GPU: the lookup-program seam (p3r_logup_program_dmat, k_trace_program<LogupProgSink> + k_ef_scan) word for word against the integer
reference tests/logup_ref.py.  Every comparison is exact equality of canonical words: the output's width, every word of
the running sum and of every fraction column, and the table's sum.  No tolerance, no case skipped.

Heights 1 and 2 (the next row wraps onto the row itself / the other row), 64 (one wave), 128, 1024 (exactly one scan tile
of k_ef_scan), 2048 and 4096 (several tiles), and one case of 2^19 rows - 512 scan tiles on the 256 threads of the scan's
middle pass, the smallest height at which a thread of it carries more than one tile - checked in closed form."""
import numpy as np
import pytest

import logup_ref
import test_gpu_open_points as ref

pytestmark = pytest.mark.gpu
ctxs = ref.ctxs
P3R_EINVAL, P3R_EUNSUPPORTED = -1, -5
HEIGHTS = (1, 2, 64, 128, 1024, 2048, 4096)


def builder(field):
    import plonky3_recursion_amd as p3r
    return p3r.AirBuilder(field)


def rand_ext(rng, p, dc, n=None):
    return rng.integers(0, p, size=dc if n is None else (n, dc), dtype=np.uint32)


def widths_of(dc):
    return (3, 2 * dc)


def term(b, dc, kind):
    """(multiplicity, denominator) of one of six terms over matrices of widths (3, 2 DC): every pairing of base and
    extension operands, LOCAL, NEXT, LOCAL_EXT and NEXT_EXT reads, publics and challenges in the denominators."""
    c0, c1 = b.challenge(0), b.challenge(1)
    if kind == 0:   # constant multiplicity, the plain bus form challenge + cell
        return b.const(1), c0 + b.local(0, 0)
    if kind == 1:   # base multiplicity, a next-row cell and a public value in the denominator
        return b.local(0, 1), c0 + c1 * b.next(0, 2) + b.public(0)
    if kind == 2:   # extension multiplicity, extension denominator
        return b.local_ext(1, 0), b.local_ext(1, dc) + c1
    if kind == 3:   # base multiplicity over a base denominator
        return b.next(0, 0), b.local(0, 2) + b.public(1)
    if kind == 4:   # extension multiplicity over a base denominator
        return b.local_ext(1, dc) * b.local(0, 0), b.next(0, 1)
    return b.public(0), c1 * b.local(0, 1) - b.next_ext(1, 0)


LAYOUTS = ([[0]], [[1, 2], [3]], [[0, 1, 2], [4], [5, 3]])   # 1 to 3 columns of 1 to 3 terms


def layout_program(field, dc, layout):
    b = builder(field)
    for column in layout:
        for kind in column:
            b.lookup(*term(b, dc, kind))
        b.end_lookup_column()
    return b


def run(ctx, prog, mats, publics=(), challenges=()):
    """The library's auxiliary trace and table sum for host matrices `mats`."""
    dm = [ctx.upload(m) for m in mats]
    try:
        out, total = ctx.logup_device(prog, dm, public_values=publics, challenges=challenges)
        got = out.download()
        out.free()
    finally:
        for d in dm:
            d.free()
    return got, [int(v) for v in total]


def check(ctx, field, dc, prog, mats, publics=(), challenges=()):
    insns = prog.program() if hasattr(prog, "program") else prog
    assert logup_ref.zero_rows(field, dc, insns, mats, publics, challenges) == [], "the case itself has a zero denominator"
    want, want_sum = logup_ref.logup_trace(field, dc, insns, mats, publics, challenges)
    got, got_sum = run(ctx, prog, mats, publics, challenges)
    assert got.shape == want.shape and got.dtype == np.uint32
    assert np.array_equal(got[:, :dc], want[:, :dc]), "running sum"
    for g in range(1, want.shape[1] // dc):
        assert np.array_equal(got[:, g * dc:(g + 1) * dc], want[:, g * dc:(g + 1) * dc]), "fraction column %d" % (g - 1)
    assert got_sum == want_sum, "table sum"
    return got, got_sum


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_every_shape_word_for_word(ctxs, field, dc):
    ctx, p = ctxs(field, dc), ref.P(field)
    rng = np.random.default_rng(1500 + dc)
    for h in HEIGHTS:
        for layout in LAYOUTS:
            mats = [rng.integers(0, p, size=(h, w), dtype=np.uint32) for w in widths_of(dc)]
            prog = layout_program(field, dc, layout)
            info = ctx.lookup_program_info(prog, widths_of(dc))
            assert info["n_columns"] == len(layout) and info["n_terms"] == sum(len(c) for c in layout)
            got, _ = check(ctx, field, dc, prog, mats, publics=rng.integers(0, p, size=2, dtype=np.uint32), challenges=rand_ext(rng, p, dc, 2))
            assert got.shape == (h, dc * (1 + len(layout))) and not got[0, :dc].any() and got[:, dc:].any()


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_two_to_the_19_rows_in_closed_form(ctxs, field, dc):
    """One column of one term 1 / c for a constant challenge c: every fraction is 1 / c, row r of the running sum r / c, the
    table's sum 2^19 / c.  512 scan tiles: every thread of the scan's middle pass carries two."""
    ctx, p, E = ctxs(field, dc), ref.P(field), ref.ext(field, dc)
    h = 1 << 19
    c = [int(v) for v in np.random.default_rng(1510 + dc).integers(1, p, size=dc)]
    inv_c = E.inv(c)
    assert E.mul(c, inv_c) == E.one(0)
    b = builder(field)
    b.lookup(1, b.challenge(0))
    b.end_lookup_column()
    got, got_sum = run(ctx, b, [np.zeros((h, 1), dtype=np.uint32)], challenges=[c])
    assert got.shape == (h, 2 * dc)
    rows = np.arange(h, dtype=np.uint64)
    for k in range(dc):
        assert np.array_equal(got[:, k], (rows * np.uint64(inv_c[k]) % np.uint64(p)).astype(np.uint32)), "running sum, coefficient %d" % k
        assert np.array_equal(got[:, dc + k], np.full(h, inv_c[k], dtype=np.uint32)), "fraction, coefficient %d" % k
    assert got_sum == E.scale(inv_c, h % p)


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_edge_operands(ctxs, field, dc):
    """Cells and challenge words from {0, 1, P - 1}; multiplicities 0 on some rows (a cell), 0 on all rows, P - 1 and an
    extension cell.  Every denominator keeps a challenge coefficient no cell can cancel: check() asserts, on the CPU first,
    that none vanishes."""
    ctx, p = ctxs(field, dc), ref.P(field)
    edges = [0, 1, p - 1]
    h = 64
    cells = np.array([edges[(r + 2 * c + r // 3) % 3] for r in range(h) for c in range(3 + dc)], dtype=np.uint32).reshape(h, 3 + dc)
    assert all((cells[:, c] == 0).any() and (cells[:, c] != 0).any() for c in range(3))
    b = builder(field)
    c0, c1 = b.challenge(0), b.challenge(1)
    b.lookup(b.local(0, 0), c0 + b.local(0, 1))         # multiplicity 0 on some rows
    b.lookup(0, c0 + b.next(0, 2))                      # ... and on all rows
    b.end_lookup_column()
    b.lookup(p - 1, c1 * b.local(0, 1) + c0)
    b.lookup(b.local_ext(0, 3), c0 - b.local(0, 2))
    b.end_lookup_column()
    b.lookup(b.const(0) * b.local(0, 0), c0)            # a column that is zero throughout
    b.end_lookup_column()
    sets = ([[0, 1, p - 1, 0, 1][:dc], [p - 1, p - 1, 0, 1, 0][:dc]], [[p - 1, p - 1, 1, 0, 0][:dc], [1, 0, p - 1, 1, p - 1][:dc]])
    for chal in sets:
        got, _ = check(ctx, field, dc, b, [cells], challenges=np.array(chal, dtype=np.uint32))
        assert not got[:, 3 * dc:].any()


def bus_tables(field, rng):
    """A sender of 256 rows, one tuple (t0, t1) with multiplicity 1 each, and a receiver of 64 rows holding the distinct
    tuples with minus the number of times each was sent (some often, some never)."""
    p = ref.P(field)
    tuples = np.stack([np.arange(64, dtype=np.uint32), rng.integers(0, p, size=64, dtype=np.uint32)], axis=1)
    sent = np.concatenate([rng.integers(0, 16, size=128), rng.integers(0, 60, size=128)])   # repeats; tuples 60 .. 63 are never sent
    counts = np.bincount(sent, minlength=64)
    assert counts.max() > 3 and (counts[60:] == 0).all() and counts.sum() == 256
    sender = tuples[sent]
    receiver = np.concatenate([tuples, ((p - counts) % p).astype(np.uint32)[:, None]], axis=1)
    return sender, receiver, int(np.argmax(counts))


def bus_program(field, multiplicity_column):
    """The reference's bus form: denominator bus_prefix + t0 + beta * t1, challenges [bus_prefix, beta]."""
    b = builder(field)
    d = b.challenge(0) + b.local(0, 0) + b.challenge(1) * b.local(0, 1)
    b.lookup(1 if multiplicity_column is None else b.local(0, multiplicity_column), d)
    b.end_lookup_column()
    return b


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_two_tables_on_one_bus_balance(ctxs, field, dc):
    ctx, p, E = ctxs(field, dc), ref.P(field), ref.ext(field, dc)
    rng = np.random.default_rng(1520 + dc)
    sender, receiver, most_sent = bus_tables(field, rng)
    chal = rand_ext(rng, p, dc, 2)
    _, sum_s = check(ctx, field, dc, bus_program(field, None), [sender], challenges=chal)
    _, sum_r = check(ctx, field, dc, bus_program(field, 2), [receiver], challenges=chal)
    assert any(sum_s) and E.add(sum_s, sum_r) == E.zero(0)
    spoiled = receiver.copy()
    spoiled[most_sent, 1] = (int(spoiled[most_sent, 1]) + 1) % p   # a tuple that was sent is received as another
    _, sum_x = check(ctx, field, dc, bus_program(field, 2), [spoiled], challenges=chal)
    assert E.add(sum_s, sum_x) != E.zero(0)


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_a_zero_denominator_is_refused_with_its_first_row(ctxs, field, dc):
    import plonky3_recursion_amd as p3r
    ctx, p = ctxs(field, dc), ref.P(field)
    rng = np.random.default_rng(1530 + dc)
    h, c = 128, 12345
    trace = rng.integers(0, p, size=(h, 2), dtype=np.uint32)
    trace[trace == c] = c + 1
    chal = np.array([[c] + [0] * (dc - 1)], dtype=np.uint32)   # an embedded base element
    b = builder(field)
    b.lookup(b.local(0, 1), b.challenge(0) - b.local(0, 0))
    b.end_lookup_column()
    bad = trace.copy()
    bad[37, 0] = bad[90, 0] = c
    assert logup_ref.zero_rows(field, dc, b.program(), [bad], (), chal) == [37, 90]
    d = ctx.upload(bad)
    with pytest.raises(p3r.P3rError) as e:
        ctx.logup_device(b, [d], challenges=chal)
    d.free()
    assert e.value.code == P3R_EINVAL and "zero denominator in row 37" in str(e.value)
    check(ctx, field, dc, b, [trace], challenges=chal)   # the same context, the clean trace


def full_house(field, dc, n_live, all_ext=False):
    """n_live values alive at one point (half of them extension values, or all): loaded first, then summed into the
    denominator."""
    b = builder(field)
    vals = [(b.local_ext(1, k % (dc + 1)) if all_ext or k % 2 else b.next(0, k % 3)) for k in range(n_live)]
    acc = vals[0]
    for v in vals[1:]:
        acc = acc + v
    b.lookup(1, acc)
    b.end_lookup_column()
    return b


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_exactly_the_live_limit_and_one_more(ctxs, field, dc):
    from plonky3_recursion_amd import _lib
    import plonky3_recursion_amd as p3r
    ctx, p = ctxs(field, dc), ref.P(field)
    rng = np.random.default_rng(1540 + dc)
    mats = [rng.integers(0, p, size=(128, w), dtype=np.uint32) for w in widths_of(dc)]
    for all_ext in (False, True):   # all extension values: the slot file is above 48 KiB, the launch asks for it
        prog = full_house(field, dc, _lib.P3R_AIR_MAX_LIVE, all_ext)
        assert ctx.lookup_program_info(prog, widths_of(dc))["peak_live"] == _lib.P3R_AIR_MAX_LIVE
        check(ctx, field, dc, prog, mats)
        dm = [ctx.upload(m) for m in mats]
        with pytest.raises(p3r.P3rError) as e:
            ctx.logup_device(full_house(field, dc, _lib.P3R_AIR_MAX_LIVE + 1, all_ext), dm)
        assert e.value.code == P3R_EUNSUPPORTED and "P3R_AIR_MAX_LIVE" in str(e.value)
        for d in dm:
            d.free()
        check(ctx, field, dc, prog, mats)


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_refusals_leave_the_context_usable(ctxs, field, dc):
    import ctypes as C
    import plonky3_recursion_amd as p3r
    from plonky3_recursion_amd import _lib as L
    from plonky3_recursion_amd import device
    ctx, p = ctxs(field, dc), ref.P(field)
    rng = np.random.default_rng(1550 + dc)
    h, widths = 8, widths_of(dc)
    mats = [rng.integers(0, p, size=(h, w), dtype=np.uint32) for w in widths]
    dm = [ctx.upload(m) for m in mats]
    short = ctx.upload(mats[0][:h // 2])
    pub, chal = [1, 2], rand_ext(rng, p, dc, 2)
    good = layout_program(field, dc, LAYOUTS[1])
    assert logup_ref.zero_rows(field, dc, good.program(), mats, pub, chal) == []
    want, want_sum = logup_ref.logup_trace(field, dc, good.program(), mats, pub, chal)

    def call(prog=good, mats_=None, publics=pub, challenges=chal):
        return ctx.logup_device(prog, dm if mats_ is None else mats_, public_values=publics, challenges=challenges)

    LOC, LK, END = L.P3R_AIR_LOCAL, L.P3R_AIR_LOOKUP, L.P3R_AIR_LOOKUP_END
    bad_chal = chal.copy()
    bad_chal[1, 0] = 0xFFFFFFFF
    cases = [
        ("n_mats == 0", P3R_EINVAL, dict(mats_=[])),
        ("matrices of different heights", P3R_EINVAL, dict(mats_=[dm[0], dm[1], short], prog=[(LOC, 2, 0), (LK, 0, 0), (END, 0, 0)])),
        ("matrix out of range", P3R_EINVAL, dict(prog=[(LOC, 2, 0), (LK, 0, 0), (END, 0, 0)])),
        ("column out of range", P3R_EINVAL, dict(prog=[(L.P3R_AIR_NEXT, 0, 3), (LK, 0, 0), (END, 0, 0)])),
        ("_EXT column + DC > width", P3R_EINVAL, dict(prog=[(L.P3R_AIR_LOCAL_EXT, 1, dc + 1), (LK, 0, 0), (END, 0, 0)])),
        ("public index out of range", P3R_EINVAL, dict(prog=[(L.P3R_AIR_PUBLIC, 2, 0), (LK, 0, 0), (END, 0, 0)])),
        ("challenge index out of range", P3R_EINVAL, dict(prog=[(L.P3R_AIR_CHALLENGE, 2, 0), (LK, 0, 0), (END, 0, 0)])),
        ("non-canonical constant", P3R_EINVAL, dict(prog=[(L.P3R_AIR_CONST, p, 0), (LK, 0, 0), (END, 0, 0)])),
        ("non-canonical public value", P3R_EINVAL, dict(publics=[1, p])),
        ("non-canonical challenge word", P3R_EINVAL, dict(challenges=bad_chal)),
        # what the plan refuses
        ("ASSERT_ZERO", P3R_EINVAL, dict(prog=[(LOC, 0, 0), (LK, 0, 0), (END, 0, 0), (L.P3R_AIR_ASSERT_ZERO, 0, 0)])),
        ("is_first_row", P3R_EINVAL, dict(prog=[(L.P3R_AIR_IS_FIRST_ROW, 0, 0), (LOC, 0, 0), (LK, 0, 1), (END, 0, 0)])),
        ("is_last_row", P3R_EINVAL, dict(prog=[(L.P3R_AIR_IS_LAST_ROW, 0, 0), (LOC, 0, 0), (LK, 0, 1), (END, 0, 0)])),
        ("is_transition", P3R_EINVAL, dict(prog=[(L.P3R_AIR_IS_TRANSITION, 0, 0), (LOC, 0, 0), (LK, 0, 1), (END, 0, 0)])),
        ("LOOKUP operand that is not an earlier value", P3R_EINVAL, dict(prog=[(LOC, 0, 0), (LK, 0, 1), (END, 0, 0)])),
        ("LOOKUP operand that is a sink", P3R_EINVAL, dict(prog=[(LOC, 0, 0), (LK, 0, 0), (LK, 0, 1), (END, 0, 0)])),
        ("LOOKUP_END with no open column", P3R_EINVAL, dict(prog=[(LOC, 0, 0), (END, 0, 0), (LK, 0, 0), (END, 0, 0)])),
        ("a column still open at the end", P3R_EINVAL, dict(prog=[(LOC, 0, 0), (LK, 0, 0)])),
        ("no LOOKUP", P3R_EINVAL, dict(prog=[(LOC, 0, 0), (L.P3R_AIR_NEG, 0, 0)])),
        ("unknown op", P3R_EINVAL, dict(prog=[(23, 0, 0), (LK, 0, 0), (END, 0, 0)])),
        ("more live values than the limit", P3R_EUNSUPPORTED, dict(prog=full_house(field, dc, L.P3R_AIR_MAX_LIVE + 1))),
    ]

    def good_call_gives_the_reference(name):
        out, total = call()
        got = out.download()
        out.free()
        assert np.array_equal(got, want) and [int(v) for v in total] == want_sum, "after: " + name

    for name, code, kw in cases:
        with pytest.raises(p3r.P3rError) as e:
            call(**kw)
        assert e.value.code == code, (name, str(e.value))
        assert len(str(e.value)) > 20, name
        good_call_gives_the_reference(name)
    # a NULL out or sum_out: through the C entry itself
    arr, n = device._air_insns(good)
    ptrs = (C.c_void_p * 2)(*[d.h for d in dm])
    pv, ch = np.array(pub, dtype=np.uint32), np.ascontiguousarray(chal)
    total, out = np.zeros(dc, dtype=np.uint32), C.c_void_p()
    for name, o, s in (("NULL out", None, total.ctypes.data_as(L.u32p)), ("NULL sum_out", C.byref(out), None)):
        rc = ctx.lib.p3r_logup_program_dmat(ctx.h, arr, n, ptrs, 2, pv.ctypes.data_as(L.u32p), 2, ch.ctypes.data_as(L.u32p), 2, o, s)
        assert rc == P3R_EINVAL and not out.value and len(ctx.lib.p3r_last_error(ctx.h)) > 5, name
        good_call_gives_the_reference(name)
    # a height that is not a power of two: the seam's own check of it (air_trace_log_height) is walked on the host by
    # tests/test_lookup_program_host.py, because no device matrix of such a height exists to hand to it - every way to
    # make one refuses that height first, with the same code.  That is what a caller with 6 or 12 rows meets, here:
    for rows in (6, 12):
        with pytest.raises(p3r.P3rError) as e:
            ctx.upload(np.ones((rows, 3), dtype=np.uint32))
        assert e.value.code == P3R_EINVAL and "power of two" in str(e.value) and str(rows) in str(e.value)
        assert not ctx.lib.p3r_dmat_alloc(ctx.h, rows, 3) and b"power of two" in ctx.lib.p3r_last_error(ctx.h)
        good_call_gives_the_reference("a height of %d rows" % rows)
    for d in dm + [short]:
        d.free()


def test_a_height_above_the_two_adicity_is_refused(ctxs):
    """2^25 rows of one column under KoalaBear (two-adicity 24): the smallest such matrix, 128 MiB.  BabyBear's would be
    2^28 rows; the check is the same line."""
    import plonky3_recursion_amd as p3r
    ctx = ctxs("koala-bear", 4)
    d = ctx.upload(np.ones((1 << 25, 1), dtype=np.uint32))
    b = builder("koala-bear")
    b.lookup(1, b.local(0, 0))
    b.end_lookup_column()
    with pytest.raises(p3r.P3rError) as e:
        ctx.logup_device(b, [d])
    d.free()
    assert e.value.code == P3R_EINVAL and "two-adicity" in str(e.value)
    small = np.ones((4, 1), dtype=np.uint32)
    got, total = run(ctx, b, [small])
    assert np.array_equal(got[:, 4], np.ones(4, dtype=np.uint32)) and total == [4, 0, 0, 0]


def test_zk_contexts_are_refused():
    import plonky3_recursion_amd as p3r
    ctx = p3r.Context(field="koala-bear", zk=1, zk_seed=1, log_blowup=1, max_log_arity=1, log_final_poly_len=0, query_pow_bits=3, num_queries=4)
    try:
        d = ctx.upload(np.ones((8, 1), dtype=np.uint32))
        b = builder("koala-bear")
        b.lookup(1, b.local(0, 0))
        b.end_lookup_column()
        with pytest.raises(p3r.P3rError) as e:
            ctx.logup_device(b, [d])
        assert e.value.code == P3R_EUNSUPPORTED and "zk" in str(e.value)
        d.free()
    finally:
        ctx.close()
