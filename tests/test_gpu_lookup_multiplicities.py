"""GPU: the multiplicity join (p3r_lookup_multiplicities_dmat: k_trace_program<RecordSink>, the compaction, the stable radix sort,
the head marks and the exclusive sums the lookup check runs on, then k_lookup_scatter) against the integer reference
tests/multiplicity_ref.py: the column cell for cell, the number of misses and the miss list entry for entry.  No
tolerance.

The keys are tuples (a, b, c) under the denominator a + b X + c X^(DC-1), the challenges being the basis elements 1, X and
X^(DC-1): a tuple is its own key - the words (a, b, 0.., c) - and the join is exact.  Term j of a table reads the columns
4 j .. 4 j + 2 as its tuple and 4 j + 3 as its multiplicity - for the table of the join, its enable flag."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import multiplicity_ref
import test_gpu_open_points as ref

pytestmark = pytest.mark.gpu
ctxs = ref.ctxs
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P3R_EINVAL, P3R_EUNSUPPORTED = -1, -5


def tuples_program(field, n_terms=1):
    import plonky3_recursion_amd as p3r
    b = p3r.AirBuilder(field)
    one, x, x_top = b.challenge(0), b.challenge(1), b.challenge(2)
    for j in range(n_terms):
        b.lookup(b.local(0, 4 * j + 3), one * b.local(0, 4 * j) + x * b.local(0, 4 * j + 1) + x_top * b.local(0, 4 * j + 2))
        b.end_lookup_column()
    return b


def basis(dc):
    """The challenges 1, X, X^(DC-1)."""
    ch = np.zeros((3, dc), dtype=np.uint32)
    ch[0, 0] = ch[1, 1] = ch[2, dc - 1] = 1
    return ch


def key_words(t, dc):
    """The key of the tuple (a, b, c): the words of a + b X + c X^(DC-1)."""
    w = [int(t[0]), int(t[1])] + [0] * (dc - 2)
    w[dc - 1] += int(t[2])
    return w


def rows_of(terms):
    """A trace from rows of terms, each ((a, b, c), multiplicity)."""
    return np.array([[v for t, m in row for v in (*t, m)] for row in terms], dtype=np.uint32)


def run(ctx, table, queries, challenges, cap=16):
    """table, queries[i]: (AirBuilder, [host matrices], publics).  (column as an array, n_missing, entries)."""
    insts = [table] + list(queries)
    dms = [[ctx.upload(m) for m in mats] for _, mats, _ in insts]
    try:
        dev = [(prog, dm, pub) for (prog, _, pub), dm in zip(insts, dms)]
        col, n, entries = ctx.lookup_multiplicities_device(dev[0], dev[1:], challenges=challenges, cap=cap)
        got = col.download()
        col.free()
        return got, n, entries
    finally:
        for dm in dms:
            for d in dm:
                d.free()


def check(ctx, field, dc, table, queries, cap=16):
    """Traces (one matrix per instance, 4 columns per term) through the reference and through the device."""
    inst = [(tuples_program(field, t.shape[1] // 4), [t], ()) for t in [table] + list(queries)]
    ref_inst = [(pr.program(), mats, pub) for pr, mats, pub in inst]
    want_col, want_n, want_entries = multiplicity_ref.multiplicities(field, dc, ref_inst[0], ref_inst[1:], basis(dc))
    got_col, n, entries = run(ctx, inst[0], inst[1:], basis(dc), cap)
    assert got_col.shape == want_col.shape == (table.shape[0], table.shape[1] // 4)
    assert np.array_equal(got_col, want_col), np.argwhere(got_col != want_col)[:8]
    assert n == want_n, (n, want_n)
    assert entries == want_entries[:cap]
    return want_col, want_n, want_entries


def random_case(field, h, rng):
    """A one-term table of h rows - distinct tuples but for a quarter that repeat earlier rows, an eighth disabled - and two
    one- and two-term queries of 2 h and 4 h rows that ask for table tuples and for absent ones with the multiplicities
    0, 1, 2 and p - 1."""
    p = ref.P(field)
    tuples = np.stack([np.arange(h, dtype=np.uint32) + 3, rng.integers(0, p, size=h, dtype=np.uint32), rng.integers(0, p, size=h, dtype=np.uint32)], axis=1)
    for r in range(1, h):
        if rng.random() < 0.25:
            tuples[r] = tuples[rng.integers(0, r)]
    enable = (rng.random(h) >= 0.125).astype(np.uint32) * rng.integers(1, p, size=h, dtype=np.uint32)   # any non-zero value enables
    table = np.concatenate([tuples, enable[:, None]], axis=1)
    absent = np.stack([np.arange(4, dtype=np.uint32) + h + 100, rng.integers(0, p, size=4, dtype=np.uint32), np.zeros(4, dtype=np.uint32)], axis=1)
    pool = np.concatenate([tuples, absent])
    mults = np.array([0, 1, 2, p - 1], dtype=np.uint32)

    def query(hq, n_terms):
        cols = []
        for _ in range(n_terms):
            cols += [pool[rng.integers(0, len(pool), size=hq)], mults[rng.integers(0, 4, size=hq)][:, None]]
        return np.concatenate(cols, axis=1)
    return table, [query(2 * h, 1), query(4 * h, 2)]


@pytest.mark.parametrize("h", [1, 2, 64, 128])   # one lane, two lanes, one wave, two workgroups of the interpreter
@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_table_heights_against_two_queries_of_other_heights(ctxs, field, dc, h):
    ctx = ctxs(field, dc)
    table, queries = random_case(field, h, np.random.default_rng(1900 + 10 * h + dc))
    assert queries[0].shape == (2 * h, 4) and queries[1].shape == (4 * h, 8)
    col, n_missing, _ = check(ctx, field, dc, table, queries)
    if h >= 64:   # the case holds what it is meant to hold
        assert n_missing >= 1 and np.count_nonzero(col) >= h // 4 and (col[table[:, 3] == 0] == 0).all()


def prims_tiles():
    """kScanTile and kSortTile of device_prims.hip.h, from its own constants."""
    src = open(os.path.join(ROOT, "plonky3_recursion_amd", "csrc", "device_prims.hip.h")).read()
    env = {}
    for name in ("kPB", "kScanItems", "kScanTile", "kSortItems", "kSortTile"):
        expr = re.search(r"constexpr int %s = ([^;,]+);" % name, src).group(1)
        env[name] = int(eval(expr, {"__builtins__": {}}, env))
    return env["kScanTile"], env["kSortTile"]


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_one_record_more_than_a_tile_of_the_scan_and_of_the_sort(ctxs, field, dc, which):
    """Every row of a table of one tile's height offers a distinct key, and one query record asks for one of them: tile + 1
    records, of which the query's sorts into the middle."""
    ctx, p = ctxs(field, dc), ref.P(field)
    h = prims_tiles()[which]
    assert h & (h - 1) == 0 and h >= 2048
    rng = np.random.default_rng(1950 + dc + which)
    table = np.stack([rng.permutation(h).astype(np.uint32), rng.integers(0, p, size=h, dtype=np.uint32), rng.integers(0, p, size=h, dtype=np.uint32),
                      np.ones(h, dtype=np.uint32)], axis=1)
    asked = h // 2 + 5
    q0 = np.array([[*table[asked, :3], 7]], dtype=np.uint32)
    q1 = np.array([[*table[3, :3], 0], [*table[4, :3], 0]], dtype=np.uint32)   # no records
    col, n_missing, _ = check(ctx, field, dc, table, [q0, q1])
    assert n_missing == 0 and col[asked, 0] == 7 and np.count_nonzero(col) == 1


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_duplicates_disabled_slots_one_word_differences_and_misses(ctxs, field, dc):
    ctx, p = ctxs(field, dc), ref.P(field)
    K = [(10, 20, 30), (11, 21, 31), (12, 22, 32), (13, 23, 33)]
    top, top2 = (50, 60, 70), (50, 60, 70 + (1 << 30))        # differ in the highest coefficient word only, in its bit 30
    low, low2 = (80, 90, 100), (81, 90, 100)                  # differ in the lowest word only, in its bit 0
    idle = (5, 5, 5)                                          # offered, never asked for
    absent, cancels = (200, 1, 2), (201, 1, 2)                # offered by no slot
    table = rows_of([
        [(K[0], 1), (K[0], 1)],        # the same key in both terms of one row: term 0 takes everything
        [(K[1], 1), (K[2], 0)],        # K2 is disabled here and offered nowhere else: a miss
        [(K[1], 9), (K[3], p - 1)],    # K1 again: a later duplicate, 0
        [(top, 1), (top2, 1)],
        [(low2, 1), (low, 1)],
        [(idle, 1), (absent, 0)],      # the absent key, disabled
        [(K[3], 1), (idle, 1)],
        [(idle, 0), (idle, 0)]])
    q0 = rows_of([[(absent, 5)], [(K[0], 1)], [(K[2], 2)], [(cancels, 1)]])
    q1 = rows_of([[(K[0], 2)], [(K[1], 1)], [(K[1], 1)], [(top, 3)], [(top2, 4)], [(low, 5)], [(low2, 6)], [(cancels, p - 1)],
                  [(K[3], p - 1)], [(K[2], 1)], [(absent, 1)], [(idle, 0)], [(K[0], p - 1)], [(K[3], 3)], [(top, 1)], [(low2, 1)]])
    want = np.zeros((8, 2), dtype=np.uint32)
    want[0, 0], want[1, 0], want[2, 1] = (1 + 2 + p - 1) % p, 2, (p - 1 + 3) % p
    want[3], want[4] = (4, 4), (7, 5)
    col, n_missing, entries = check(ctx, field, dc, table, [q0, q1])
    assert np.array_equal(col, want)
    # the misses by first record: the absent key (query 0 row 0), then K2 (query 0 row 2); +1 and p - 1 cancel: no miss
    assert n_missing == 2 and [(e["instance"], e["row"], e["term"], e["n_records"], e["net"][0]) for e in entries] == [(0, 0, 0, 2, 6), (0, 2, 0, 2, 3)]
    assert entries[0]["denominator"] == key_words(absent, dc) and entries[1]["denominator"] == key_words(K[2], dc)


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_sums_that_pass_the_modulus_several_times(ctxs, field, dc):
    """300 records of multiplicity p - 1 on one key: the integer sum is 300 (p - 1), which passes p 299 times."""
    ctx, p = ctxs(field, dc), ref.P(field)
    table = rows_of([[((1, 2, 3), 1)], [((4, 5, 6), 1)]])
    q0 = rows_of([[((1, 2, 3), p - 1)]] * 256 + [[((4, 5, 6), p - 1)]] * 256)
    q1 = rows_of([[((1, 2, 3), p - 1)]] * 44 + [[((9, 9, 9), p - 1)]] * 20)   # and an absent key: net p - 20
    col, n_missing, entries = check(ctx, field, dc, table, [q0, q1])
    assert col[0, 0] == p - 300 and col[1, 0] == p - 256
    assert n_missing == 1 and entries[0]["net"][0] == p - 20 and (entries[0]["instance"], entries[0]["row"], entries[0]["n_records"]) == (1, 44, 20)


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_no_query_zero_multiplicities_and_a_small_cap(ctxs, field, dc):
    ctx, p = ctxs(field, dc), ref.P(field)
    table = rows_of([[((r, 2 * r, 3 * r), 1)] for r in range(4)])
    col, n_missing, entries = check(ctx, field, dc, table, [])   # n_queries == 0
    assert not col.any() and n_missing == 0 and entries == []
    silent = rows_of([[((r % 4, 2 * (r % 4), 3 * (r % 4)), 0)] for r in range(8)] + [[((77, 0, 0), 0)]] * 8)
    col, n_missing, entries = check(ctx, field, dc, table, [silent, silent[:2]])   # every query multiplicity is 0: no record at all
    assert not col.any() and n_missing == 0
    # five absent keys, asked for in an order that is not the order of the keys
    q = rows_of([[((100 + k, 0, 0), 1 + k)] for k in (3, 0, 4, 1, 2)] + [[((1, 2, 3), 1)]] * 3)
    for cap in (0, 1, 3, 16):
        col, n_missing, entries = check(ctx, field, dc, table, [q, silent[:1]], cap=cap)
        assert n_missing == 5 and col[1, 0] == 3
    assert [e["row"] for e in entries] == [0, 1, 2, 3, 4] and [e["denominator"][0] for e in entries] == [103, 100, 104, 101, 102]


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_refusals_name_the_instance_and_leave_the_context_usable(ctxs, field, dc):
    import plonky3_recursion_amd as p3r
    from plonky3_recursion_amd import _lib as L
    ctx, p = ctxs(field, dc), ref.P(field)
    table = rows_of([[((r, 2 * r, 3 * r), 1)] for r in range(4)])
    query = rows_of([[((r % 5, 2 * (r % 5), 3 * (r % 5)), 1)] for r in range(8)])
    ch = basis(dc)
    prog = tuples_program(field)
    want = multiplicity_ref.multiplicities(field, dc, (prog.program(), [table], ()), [(prog.program(), [query], ())], ch)
    assert want[1] == 1 and want[0][:, 0].tolist() == [2, 2, 2, 1]
    d_t, d_q, d_e = ctx.upload(table), ctx.upload(query), ctx.upload(np.ones((8, dc + 1), dtype=np.uint32))

    def valid():
        col, n, entries = ctx.lookup_multiplicities_device((prog, [d_t]), [(prog, [d_q])], challenges=ch)
        got = col.download()
        col.free()
        return np.array_equal(got, want[0]) and (n, entries) == want[1:]
    assert valid()
    LOC, LK, END = L.P3R_AIR_LOCAL, L.P3R_AIR_LOOKUP, L.P3R_AIR_LOOKUP_END
    ext_mult = p3r.AirBuilder(field)
    ext_mult.lookup(ext_mult.local_ext(0, 0), ext_mult.local(0, dc))
    ext_mult.end_lookup_column()
    asserting = [(LOC, 0, 0), (LK, 0, 0), (END, 0, 0), (L.P3R_AIR_ASSERT_ZERO, 0, 0)]
    cases = [
        ("an extension-typed multiplicity in query 1", P3R_EUNSUPPORTED, "query 1", (prog, [d_t]), [(prog, [d_q]), (ext_mult, [d_e])]),
        ("an ASSERT_ZERO in the table", P3R_EINVAL, "table", (asserting, [d_t]), [(prog, [d_q])]),
        ("an ASSERT_ZERO in query 0", P3R_EINVAL, "query 0", (prog, [d_t]), [(asserting, [d_q])]),
        ("no matrix in query 1", P3R_EINVAL, "query 1", (prog, [d_t]), [(prog, [d_q]), (prog, [])]),
    ]
    for name, code, who, tab, qs in cases:
        with pytest.raises(p3r.P3rError) as e:
            ctx.lookup_multiplicities_device(tab, qs, challenges=ch)
        assert e.value.code == code and who in str(e.value), (name, str(e.value))
        assert valid(), "after: " + name
    # an extension-typed multiplicity is the table's right: it is an enable flag there
    col, n, _ = ctx.lookup_multiplicities_device((ext_mult, [d_e]), [], challenges=ch)
    assert col.shape == (8, 1) and n == 0
    col.free()

    # the NULL pointers, through the entry itself
    from plonky3_recursion_amd import device
    tab, keep_t = device._lookup_instances([(prog, [d_t])])
    qs, keep_q = device._lookup_instances([(prog, [d_q])])
    chal = np.ascontiguousarray(ch)
    chp = chal.ctypes.data_as(L.u32p)
    out, count, missing = C.c_void_p(), C.c_uint64(), (L.P3rLookupImbalance * 4)()
    call = ctx.lib.p3r_lookup_multiplicities_dmat
    for name, args in (("out", (tab, qs, 1, chp, 3, None, missing, 4, C.byref(count))),
                       ("table", (None, qs, 1, chp, 3, C.byref(out), missing, 4, C.byref(count))),
                       ("n_missing_out", (tab, qs, 1, chp, 3, C.byref(out), missing, 4, None)),
                       ("missing", (tab, qs, 1, chp, 3, C.byref(out), None, 4, C.byref(count)))):
        assert call(ctx.h, *args) == P3R_EINVAL, name
        assert name in ctx.lib.p3r_last_error(ctx.h).decode() and not out.value, name
        assert valid(), "after a NULL " + name
    for d in (d_t, d_q, d_e):
        d.free()


def test_zk_contexts_and_too_many_slots_are_refused(ctxs):
    import plonky3_recursion_amd as p3r
    b = p3r.AirBuilder("koala-bear")
    b.lookup(1, b.local(0, 0))
    b.end_lookup_column()
    zk = p3r.Context(field="koala-bear", zk=1, zk_seed=1, log_blowup=1, max_log_arity=1, log_final_poly_len=0, query_pow_bits=3, num_queries=4)
    try:
        d = zk.upload(np.ones((8, 1), dtype=np.uint32))
        with pytest.raises(p3r.P3rError) as e:
            zk.lookup_multiplicities_device((b, [d]), [(b, [d])])
        assert e.value.code == P3R_EUNSUPPORTED and "zk" in str(e.value)
        d.free()
    finally:
        zk.close()
    # 2^24 rows x 9 terms in the table and in the query: 2^28 + 2^25 slots.  Refused before anything is allocated.
    ctx = ctxs("koala-bear", 4)
    wide = p3r.AirBuilder("koala-bear")
    for _ in range(9):
        wide.lookup(1, wide.local(0, 0))
    wide.end_lookup_column()
    d = ctx.upload(np.ones((1 << 24, 1), dtype=np.uint32))
    with pytest.raises(p3r.P3rError) as e:
        ctx.lookup_multiplicities_device((wide, [d]), [(wide, [d])])
    assert e.value.code == P3R_EUNSUPPORTED and "P3R_LOOKUP_CHECK_MAX_RECORDS" in str(e.value)
    d.free()
    d = ctx.upload(np.ones((8, 1), dtype=np.uint32))
    col, n, _ = ctx.lookup_multiplicities_device((b, [d]), [(b, [d])])   # the context still serves
    assert col.download()[:, 0].tolist() == [8] + [0] * 7 and n == 0
    col.free()
    d.free()
