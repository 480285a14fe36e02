"""GPU: the constraint-program seam (p3r_quotient_program_dmat, k_quotient_program) word for word against the integer
interpreter tests/air_ref.py.  Every comparison is exact equality of canonical words of every chunk.  The definitions do
not ask the inputs to be low-degree extensions, so the matrices are random words: every row that is read matters, and a
row that must not be read (beyond the first h << q) would show.

Shapes: trace heights 1, 2, 4, 64 and 2^10, quotient degrees 2^0 .. 2^3 and blow-ups 2^q and 2^(q+1) put the domain
below one 64-lane workgroup (N = 1 .. 32), at exactly one (N = 64) and across many; the next row wraps at i + 2^q >= N in
every shape, and at h = 1 it is the row itself.  One to three matrices of widths (1), (3, 2 DC), (7, DC, 5)."""
import itertools

import numpy as np
import pytest

import air_ref
import field_ref
import test_gpu_open_points as ref

pytestmark = pytest.mark.gpu
ctxs = ref.ctxs
P3R_EINVAL, P3R_EUNSUPPORTED = -1, -5


def builder(field):
    import plonky3_recursion_amd as p3r
    return p3r.AirBuilder(field)


def rand_ext(rng, p, dc, n=None):
    return rng.integers(0, p, size=dc if n is None else (n, dc), dtype=np.uint32)


def run(ctx, field, dc, prog, mats, added_bits, q, shift=None, publics=(), challenges=(), alpha=None):
    """The library's chunks and the reference's, for host matrices `mats`."""
    dm = [ctx.upload(m) for m in mats]
    try:
        outs = ctx.quotient_device(prog, dm, added_bits, q, alpha, public_values=publics, challenges=challenges, shift=shift)
        got = [o.download() for o in outs]
        for o in outs:
            o.free()
    finally:
        for d in dm:
            d.free()
    insns = prog.program() if hasattr(prog, "program") else prog
    want = air_ref.quotient_chunks(field, dc, insns, mats, added_bits, q, shift, publics, challenges, alpha)
    return got, want


def check(ctx, field, dc, prog, mats, added_bits, q, **kw):
    got, want = run(ctx, field, dc, prog, mats, added_bits, q, **kw)
    h = mats[0].shape[0] >> added_bits
    assert len(got) == len(want) == 1 << q
    for c, (g, w) in enumerate(zip(got, want)):
        assert g.shape == (h, dc) and np.array_equal(g, w), "chunk %d" % c


def shape_program(field, dc, widths, q):
    """Every op and every matrix, with constraint degrees up to 2^q + 1 (what log_quotient_degree q admits)."""
    b = builder(field)
    cells = []
    for m, w in enumerate(widths):
        cells += [b.local(m, 0), b.next(m, w - 1), b.local(m, w // 2)]
    prod = cells[0]
    for k in range(1, (1 << q) + 1):   # degree 2^q + 1
        prod = prod * cells[k % len(cells)]
    b.assert_zero(prod - b.public(0))
    b.assert_zero(b.is_first_row() * (cells[1] - b.public(1)))
    b.assert_zero(b.is_last_row() * (cells[2] + 5))
    b.assert_zero(b.is_transition() * (cells[0] - cells[1]) * b.challenge(1))
    ch = b.challenge(0)
    b.assert_zero(ch * ch * cells[-1] - (-cells[0]))
    for m, w in enumerate(widths):
        if w >= dc:
            e, f = b.local_ext(m, 0), b.next_ext(m, w - dc)
            b.assert_zero(e * f - ch)                       # ext * ext
            b.assert_zero(b.is_transition() * (f - e * cells[0] - ch * 3))   # ext * base, ext * const
            b.assert_zero(cells[1] - e)                     # base - ext
            b.assert_zero(-(e + cells[2]))
    return b


def widths_sets(dc):
    return [(1,), (3, 2 * dc), (7, dc, 5)]


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_every_shape_word_for_word(ctxs, field, dc):
    ctx, p = ctxs(field, dc), ref.P(field)
    rng = np.random.default_rng(1400 + dc)
    for h, q, extra, widths in itertools.product((1, 2, 4, 64, 1 << 10), (0, 1, 2, 3), (0, 1), widths_sets(dc)):
        added_bits = q + extra
        mats = [rng.integers(0, p, size=(h << added_bits, w), dtype=np.uint32) for w in widths]
        prog = shape_program(field, dc, widths, q)
        info = ctx.air_program_info(prog, widths)
        assert info["log_quotient_degree"] == q and info["max_degree"] == (1 << q) + 1
        check(ctx, field, dc, prog, mats, added_bits, q, publics=rng.integers(0, p, size=2, dtype=np.uint32),
              challenges=rand_ext(rng, p, dc, 2), alpha=rand_ext(rng, p, dc))


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_a_caller_shift_and_a_larger_quotient_degree_than_needed(ctxs, field, dc):
    ctx, p = ctxs(field, dc), ref.P(field)
    rng = np.random.default_rng(1410 + dc)
    widths = (3, 2 * dc)
    prog = shape_program(field, dc, widths, 1)
    for shift, q, added_bits in ((7, 2, 2), (p - 2, 1, 3), (ref.GEN(field), 4, 4)):
        mats = [rng.integers(0, p, size=(8 << added_bits, w), dtype=np.uint32) for w in widths]
        check(ctx, field, dc, prog, mats, added_bits, q, shift=shift, publics=[3, 4], challenges=rand_ext(rng, p, dc, 2),
              alpha=rand_ext(rng, p, dc))


def single_op_programs(field, dc):
    """Each op alone (asserted as it is), the mixed-type forms of the arithmetic ops, each selector and all three."""
    progs = {}

    def one(name, fn):
        b = builder(field)
        b.assert_zero(fn(b))
        progs[name] = b
    one("const", lambda b: b.const(12345))
    one("public", lambda b: b.public(1))
    one("challenge", lambda b: b.challenge(1))
    one("local", lambda b: b.local(0, 2))
    one("next", lambda b: b.next(0, 1))
    one("local_ext", lambda b: b.local_ext(1, dc))
    one("next_ext", lambda b: b.next_ext(1, 0))
    one("is_first_row", lambda b: b.is_first_row())
    one("is_last_row", lambda b: b.is_last_row())
    one("is_transition", lambda b: b.is_transition())
    one("selectors", lambda b: b.is_first_row() * b.next(0, 0) + b.is_last_row() * b.local(0, 1) + b.is_transition() * b.local_ext(1, 1))
    base, ext = (lambda b: b.local(0, 0)), (lambda b: b.next_ext(1, 2))
    base2, ext2 = (lambda b: b.next(0, 2)), (lambda b: b.challenge(0))
    for name, f in (("add", lambda x, y: x + y), ("sub", lambda x, y: x - y), ("mul", lambda x, y: x * y)):
        one(name + "_bb", lambda b: f(base(b), base2(b)))
        one(name + "_be", lambda b: f(base(b), ext(b)))
        one(name + "_eb", lambda b: f(ext(b), base(b)))
        one(name + "_ee", lambda b: f(ext(b), ext2(b)))
    one("neg_b", lambda b: -base(b))
    one("neg_e", lambda b: -ext(b))
    one("self_operands", lambda b: (lambda v: v * v + v - v)(ext(b)))
    b = builder(field)   # Horner over mixed constraints: base, ext, base
    b.assert_zero(b.local(0, 0))
    b.assert_zero(b.local_ext(1, 0))
    b.assert_zero(b.next(0, 1))
    progs["horner"] = b
    return progs


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_each_op_alone(ctxs, field, dc):
    ctx, p = ctxs(field, dc), ref.P(field)
    rng = np.random.default_rng(1420 + dc)
    h, q, added_bits = 4, 1, 1
    mats = [rng.integers(0, p, size=(h << added_bits, w), dtype=np.uint32) for w in (3, 2 * dc)]
    pub, chal, alpha = rng.integers(0, p, size=2, dtype=np.uint32), rand_ext(rng, p, dc, 2), rand_ext(rng, p, dc)
    for name, prog in single_op_programs(field, dc).items():
        got, want = run(ctx, field, dc, prog, mats, added_bits, q, publics=pub, challenges=chal, alpha=alpha)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), name


def random_dag(field, dc, widths, rng, n_constraints, window, max_degree):
    """A random straight-line program: operands from the last `window` values (which bounds the live values), products
    only where the degree rule stays within max_degree."""
    b, vals = builder(field), []   # (value, degree)

    def leaf():
        k = int(rng.integers(0, 9))
        m = int(rng.integers(0, len(widths)))
        if k < 3:
            return ((b.local, b.next)[k % 2](m, int(rng.integers(0, widths[m]))), 1)
        if k == 3 and widths[m] >= dc:
            return ((b.local_ext, b.next_ext)[int(rng.integers(0, 2))](m, int(rng.integers(0, widths[m] - dc + 1))), 1)
        if k == 4:
            return (b.challenge(int(rng.integers(0, 3))), 0)
        if k == 5:
            return (b.public(int(rng.integers(0, 3))), 0)
        if k == 6:
            return ((b.is_first_row, b.is_last_row)[int(rng.integers(0, 2))](), 1)
        if k == 7:
            return (b.is_transition(), 0)
        return (b.const(int(rng.integers(0, b.p))), 0)

    done = 0
    while done < n_constraints:
        r = int(rng.integers(0, 16))
        recent = vals[-window:]
        if len(vals) < 2 or r < 3:
            vals.append(leaf())
        elif r < 12:
            (x, dx), (y, dy) = recent[int(rng.integers(0, len(recent)))], recent[int(rng.integers(0, len(recent)))]
            k = int(rng.integers(0, 3))
            if k == 2 and dx + dy <= max_degree:
                vals.append((x * y, dx + dy))
            else:
                vals.append((x + y if k == 0 else x - y, max(dx, dy)))
        elif r < 13:
            x, dx = recent[int(rng.integers(0, len(recent)))]
            vals.append((-x, dx))
        else:
            b.assert_zero(recent[int(rng.integers(0, len(recent)))][0])
            done += 1
    return b


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_a_random_dag_of_200_constraints(ctxs, field, dc):
    from plonky3_recursion_amd import _lib
    ctx, p = ctxs(field, dc), ref.P(field)
    rng = np.random.default_rng(1430 + dc)
    widths, q, added_bits, h = (7, dc, 5), 3, 3, 16
    prog = random_dag(field, dc, widths, rng, 200, 36, 9)
    info = ctx.air_program_info(prog, widths)
    assert info["n_constraints"] == 200 and info["log_quotient_degree"] <= q and 24 <= info["peak_live"] <= _lib.P3R_AIR_MAX_LIVE
    mats = [rng.integers(0, p, size=(h << added_bits, w), dtype=np.uint32) for w in widths]
    check(ctx, field, dc, prog, mats, added_bits, q, publics=rng.integers(0, p, size=3, dtype=np.uint32),
          challenges=rand_ext(rng, p, dc, 3), alpha=rand_ext(rng, p, dc))


def full_house(field, dc, n_live, all_ext=False):
    """n_live values alive at one point (half of them extension values, or all): loaded first, then summed and squared."""
    b = builder(field)
    vals = [(b.local_ext(1, k % (dc + 1)) if all_ext or k % 2 else b.next(0, k % 3)) for k in range(n_live)]
    acc = vals[0]
    for v in vals[1:]:
        acc = acc + v
    b.assert_zero(acc * acc)
    return b


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_exactly_the_live_limit_and_one_more(ctxs, field, dc):
    from plonky3_recursion_amd import _lib
    import plonky3_recursion_amd as p3r
    ctx, p = ctxs(field, dc), ref.P(field)
    rng = np.random.default_rng(1440 + dc)
    widths, q, added_bits, h = (3, 2 * dc), 1, 2, 64
    mats = [rng.integers(0, p, size=(h << added_bits, w), dtype=np.uint32) for w in widths]
    prog = full_house(field, dc, _lib.P3R_AIR_MAX_LIVE)
    assert ctx.air_program_info(prog, widths)["peak_live"] == _lib.P3R_AIR_MAX_LIVE
    alpha = rand_ext(rng, p, dc)
    check(ctx, field, dc, prog, mats, added_bits, q, alpha=alpha)
    dm = [ctx.upload(m) for m in mats]
    with pytest.raises(p3r.P3rError) as e:
        ctx.quotient_device(full_house(field, dc, _lib.P3R_AIR_MAX_LIVE + 1), dm, added_bits, q, alpha)
    assert e.value.code == P3R_EUNSUPPORTED and "P3R_AIR_MAX_LIVE" in str(e.value)
    for d in dm:
        d.free()
    check(ctx, field, dc, prog, mats, added_bits, q, alpha=alpha)


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_a_slot_file_of_extension_values_only(ctxs, field, dc):
    """P3R_AIR_MAX_LIVE extension values alive at once: a slot file of 48 x DC words for each of the 64 lanes.  In the
    KoalaBear quintic context that is 60 KiB, above the 48 KiB a kernel gets without asking, so the launch has to ask for
    it; at degree 4 it is exactly 48 KiB and does not cross the line.  A trace of 64 rows with blow-up 2 and quotient
    degree 2: a domain of 128 rows, two workgroups of one wave."""
    from plonky3_recursion_amd import _lib
    ctx, p = ctxs(field, dc), ref.P(field)
    rng = np.random.default_rng(1460 + dc)
    widths, q, added_bits, h = (3, 2 * dc), 1, 1, 64
    mats = [rng.integers(0, p, size=(h << added_bits, w), dtype=np.uint32) for w in widths]
    prog = full_house(field, dc, _lib.P3R_AIR_MAX_LIVE, all_ext=True)
    assert ctx.air_program_info(prog, widths)["peak_live"] == _lib.P3R_AIR_MAX_LIVE
    check(ctx, field, dc, prog, mats, added_bits, q, alpha=rand_ext(rng, p, dc))


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_edge_words_everywhere(ctxs, field, dc):
    ctx, p = ctxs(field, dc), ref.P(field)
    edges = [0, 1, p - 1]
    h, q, added_bits = 4, 2, 2
    cells = np.array([edges[(r + 2 * c) % 3] for r in range(h << added_bits) for c in range(3 + dc)], dtype=np.uint32).reshape(-1, 3 + dc)
    b = builder(field)
    acc = b.local_ext(0, 3) * b.challenge(0)
    for k, w in enumerate(edges):
        acc = acc + (b.const(w) * b.local(0, k) - b.public(k)) * b.next(0, (k + 1) % 3) * b.challenge(1 + k % 2)
        b.assert_zero(b.const(w) - b.public(2 - k))
        b.assert_zero(b.next_ext(0, 3) * b.local(0, k) + b.const(w))
    b.assert_zero(acc * b.is_transition())
    chal = np.array([[edges[(i + k) % 3] for k in range(dc)] for i in range(3)], dtype=np.uint32)
    for alpha in ([p - 1] * dc, [0] * dc, [1] + [0] * (dc - 1), [edges[(k + 1) % 3] for k in range(dc)]):
        check(ctx, field, dc, b, [cells], added_bits, q, publics=edges, challenges=chal, alpha=np.array(alpha, dtype=np.uint32))


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_refusals_leave_the_context_usable(ctxs, field, dc):
    import plonky3_recursion_amd as p3r
    from plonky3_recursion_amd import _lib as L
    ctx, p = ctxs(field, dc), ref.P(field)
    rng = np.random.default_rng(1450 + dc)
    h, q, added_bits, widths = 8, 1, 1, (3, 2 * dc)
    mats = [rng.integers(0, p, size=(h << added_bits, w), dtype=np.uint32) for w in widths]
    dm = [ctx.upload(m) for m in mats]
    short = ctx.upload(mats[0][:h])
    pub, chal, alpha = [1, 2], rand_ext(rng, p, dc, 2), rand_ext(rng, p, dc)
    good = shape_program(field, dc, widths, 1)
    want = air_ref.quotient_chunks(field, dc, good.program(), mats, added_bits, q, None, pub, chal, alpha)

    def call(prog=good, mats_=None, ab=added_bits, lq=q, shift=None, publics=pub, challenges=chal, al=alpha):
        return ctx.quotient_device(prog, dm if mats_ is None else mats_, ab, lq, al, public_values=publics, challenges=challenges, shift=shift)

    A, LOC = L.P3R_AIR_ASSERT_ZERO, L.P3R_AIR_LOCAL
    bad_word = np.array(alpha, dtype=np.uint32)
    bad_word[dc - 1] = p
    bad_chal = chal.copy()
    bad_chal[1, 0] = 0xFFFFFFFF
    w_h = field_ref.two_adic_generator(field, 3)
    cases = [
        ("operand that is not an earlier value", P3R_EINVAL, dict(prog=[(LOC, 0, 0), (L.P3R_AIR_ADD, 0, 1), (A, 1, 0)])),
        ("operand that is an ASSERT_ZERO", P3R_EINVAL, dict(prog=[(LOC, 0, 0), (A, 0, 0), (L.P3R_AIR_NEG, 1, 0), (A, 2, 0)])),
        ("unknown op", P3R_EINVAL, dict(prog=[(5, 0, 0), (A, 0, 0)])),
        ("matrix out of range", P3R_EINVAL, dict(prog=[(LOC, 2, 0), (A, 0, 0)])),
        ("column out of range", P3R_EINVAL, dict(prog=[(L.P3R_AIR_NEXT, 0, 3), (A, 0, 0)])),
        ("_EXT column + DC > width", P3R_EINVAL, dict(prog=[(L.P3R_AIR_LOCAL_EXT, 1, dc + 1), (A, 0, 0)])),
        ("public index out of range", P3R_EINVAL, dict(prog=[(L.P3R_AIR_PUBLIC, 2, 0), (A, 0, 0)])),
        ("challenge index out of range", P3R_EINVAL, dict(prog=[(L.P3R_AIR_CHALLENGE, 2, 0), (A, 0, 0)])),
        ("non-canonical constant", P3R_EINVAL, dict(prog=[(L.P3R_AIR_CONST, p, 0), (A, 0, 0)])),
        ("non-canonical public value", P3R_EINVAL, dict(publics=[1, p])),
        ("non-canonical challenge word", P3R_EINVAL, dict(challenges=bad_chal)),
        ("non-canonical alpha word", P3R_EINVAL, dict(al=bad_word)),
        ("non-canonical shift", P3R_EINVAL, dict(shift=p)),
        ("no ASSERT_ZERO", P3R_EINVAL, dict(prog=[(LOC, 0, 0), (L.P3R_AIR_NEG, 0, 0)])),
        ("matrices of different heights", P3R_EINVAL, dict(mats_=[dm[0], dm[1], short], prog=[(LOC, 2, 0), (A, 0, 0)])),
        ("added_bits < log_quotient_degree", P3R_EINVAL, dict(ab=1, lq=2)),
        ("log_quotient_degree below what the program needs", P3R_EINVAL, dict(lq=0)),
        ("a height below 2^added_bits", P3R_EINVAL, dict(ab=5, lq=1)),
        ("shift^h == 1", P3R_EINVAL, dict(shift=1)),
        ("shift in the trace domain", P3R_EINVAL, dict(shift=w_h)),
        ("more live values than the limit", P3R_EUNSUPPORTED, dict(prog=full_house(field, dc, L.P3R_AIR_MAX_LIVE + 1))),
        ("log_quotient_degree > 4", P3R_EUNSUPPORTED, dict(ab=5, lq=5)),
    ]
    for name, code, kw in cases:
        with pytest.raises(p3r.P3rError) as e:
            call(**kw)
        assert e.value.code == code, (name, str(e.value))
        assert len(str(e.value)) > 20, name
        outs = call()   # the context is usable: the good call gives the reference's words
        got = [o.download() for o in outs]
        for o in outs:
            o.free()
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), "after: " + name
    for d in dm + [short]:
        d.free()


def test_zk_contexts_are_refused():
    import plonky3_recursion_amd as p3r
    ctx = p3r.Context(field="koala-bear", zk=1, zk_seed=1, log_blowup=1, max_log_arity=1, log_final_poly_len=0, query_pow_bits=3, num_queries=4)
    try:
        d = ctx.upload(np.ones((8, 1), dtype=np.uint32))
        b = builder("koala-bear")
        b.assert_zero(b.local(0, 0))
        with pytest.raises(p3r.P3rError) as e:
            ctx.quotient_device(b, [d], 1, 0, [1, 0, 0, 0])
        assert e.value.code == P3R_EUNSUPPORTED and "zk" in str(e.value)
        d.free()
    finally:
        ctx.close()
