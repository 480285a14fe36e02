"""GPU: the lookup check (p3r_lookup_check_dmat: k_trace_program<RecordSink>, the stable radix sort and the exclusive sums of
device_prims.hip.h) against the integer reference tests/check_ref.py: the number of unbalanced keys and, entry by entry,
instance, row and term of the key's first record, the number of its records, the key and the net multiplicity.  No
tolerance.

The buses are in the reference's form, denominator bus_prefix + t0 + beta * t1 with the challenges [bus_prefix, beta],
term j of a table reading the columns (3 j, 3 j + 1) as its tuple and 3 j + 2 as its multiplicity.  Before the device is
asked, the reference is run twice - keyed by the denominators, as the device keys, and keyed by the tuples themselves -
and the two answers must agree: no two tuples of a case collide under the test's fixed challenges."""
import numpy as np
import pytest

import check_ref
import test_gpu_open_points as ref

pytestmark = pytest.mark.gpu
ctxs = ref.ctxs
P3R_EINVAL, P3R_EUNSUPPORTED = -1, -5


def bus(field, n_terms=1):
    import plonky3_recursion_amd as p3r
    b = p3r.AirBuilder(field)
    prefix, beta = b.challenge(0), b.challenge(1)
    for j in range(n_terms):
        b.lookup(b.local(0, 3 * j + 2), prefix + b.local(0, 3 * j) + beta * b.local(0, 3 * j + 1))
        if j % 3 == 2 or j == n_terms - 1:
            b.end_lookup_column()
    return b


def challenges_of(field, dc):
    return np.random.default_rng(1800 + dc).integers(1, ref.P(field), size=(2, dc), dtype=np.uint32)


def tuple_key(tables):
    return lambda i, r, t: (int(tables[i][r, 3 * t]), int(tables[i][r, 3 * t + 1]))


def run(ctx, instances, challenges, cap=16):
    """instances: (AirBuilder, [host matrices], publics)."""
    dms = [[ctx.upload(m) for m in mats] for _, mats, _ in instances]
    try:
        return ctx.lookup_check_device([(prog, dm, pub) for (prog, _, pub), dm in zip(instances, dms)], challenges=challenges, cap=cap)
    finally:
        for dm in dms:
            for d in dm:
                d.free()


def check(ctx, field, dc, tables, challenges=None, cap=16, progs=None):
    """Bus tables (one matrix each) through the reference - by denominator and by tuple - and through the device."""
    challenges = challenges_of(field, dc) if challenges is None else challenges
    progs = progs or [bus(field, t.shape[1] // 3) for t in tables]
    ref_inst = [(pr.program(), [t], ()) for pr, t in zip(progs, tables)]
    want = check_ref.lookup_balance(field, dc, ref_inst, challenges)
    assert want == check_ref.lookup_balance(field, dc, ref_inst, challenges, key_of=tuple_key(tables)), "two tuples collide under the test's challenges"
    n, got = run(ctx, [(pr, [t], ()) for pr, t in zip(progs, tables)], challenges, cap)
    assert n == want[0], (n, want[0])
    assert got == want[1][:cap]
    return n, got


def two_tables(field, rng, hs=64, hr=8):
    """A sender of hs rows - a tuple and the multiplicity 1 per row, the last quarter padding: multiplicity 0 over
    arbitrary tuples - and a receiver of hr rows: the distinct tuples with minus the number of times each was sent."""
    p = ref.P(field)
    tuples = np.stack([np.arange(hr, dtype=np.uint32) + 5, rng.integers(0, p, size=hr, dtype=np.uint32)], axis=1)
    live = 3 * hs // 4
    sent = rng.integers(0, hr, size=live)
    sender = np.concatenate([tuples[sent], np.ones((live, 1), dtype=np.uint32)], axis=1)
    padding = np.concatenate([rng.integers(0, p, size=(hs - live, 2), dtype=np.uint32), np.zeros((hs - live, 1), dtype=np.uint32)], axis=1)
    counts = np.bincount(sent, minlength=hr)
    receiver = np.concatenate([tuples, ((p - counts) % p).astype(np.uint32)[:, None]], axis=1)
    return np.concatenate([sender, padding]), receiver, sent


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_a_balanced_bus_and_one_dropped_send(ctxs, field, dc):
    ctx, p = ctxs(field, dc), ref.P(field)
    rng = np.random.default_rng(1810 + dc)
    sender, receiver, sent = two_tables(field, rng)
    assert sender.shape == (64, 3) and receiver.shape == (8, 3) and (sender[48:, 2] == 0).all() and sender[48:, :2].any()
    n, _ = check(ctx, field, dc, [receiver, sender])
    assert n == 0
    drop = 29
    spoiled = sender.copy()
    spoiled[drop, 2] = 0
    n, got = check(ctx, field, dc, [receiver, spoiled])
    assert n == 1 and got[0]["instance"] == 0 and got[0]["row"] == sent[drop] and got[0]["term"] == 0
    assert got[0]["net"] == [p - 1] + [0] * (dc - 1) and got[0]["n_records"] == np.count_nonzero(sent == sent[drop])   # the receive, the sends left
    n, got = check(ctx, field, dc, [spoiled, receiver])   # the other order of the instances: the first record is a send, or the receive
    first_send = [r for r in range(48) if sent[r] == sent[drop] and r != drop]
    assert n == 1 and (got[0]["instance"], got[0]["row"]) == ((0, first_send[0]) if first_send else (1, sent[drop]))


def full_house_bus(field, dc, n_live):
    """A bus over the tuple (column 0, column 1) with the multiplicity in column 2, whose denominator also takes in the
    sum of n_live extension values - windows of the 2 DC columns from column 3 on - that are all alive at one point."""
    import plonky3_recursion_amd as p3r
    b = p3r.AirBuilder(field)
    vals = [b.local_ext(0, 3 + k % (dc + 1)) for k in range(n_live)]
    acc = vals[0]
    for v in vals[1:]:
        acc = acc + v
    b.lookup(b.local(0, 2), acc + b.challenge(0) + b.local(0, 0) + b.challenge(1) * b.local(0, 1))
    b.end_lookup_column()
    return b


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_a_slot_file_of_extension_values_only(ctxs, field, dc):
    """P3R_AIR_MAX_LIVE extension values alive at once: a slot file of 48 x DC words for each of the 64 lanes.  In the
    KoalaBear quintic context that is 60 KiB, above the 48 KiB a kernel gets without asking, so the launch of
    k_trace_program<RecordSink> has to ask for it; at degree 4 it is exactly 48 KiB and does not cross the line.  A sender of 128 rows
    and a receiver of 64: two workgroups and one.  The 2 DC further columns of a row are a function of its tuple, so the
    key still is one - but a wrong word in any slot of any row unbalances the bus."""
    from plonky3_recursion_amd import _lib
    ctx, p = ctxs(field, dc), ref.P(field)
    rng = np.random.default_rng(1870 + dc)
    sender, receiver, sent = two_tables(field, rng, hs=128, hr=64)
    of_tuple = rng.integers(0, p, size=(64, 2 * dc), dtype=np.uint32)
    rest = rng.integers(0, p, size=(128, 2 * dc), dtype=np.uint32)   # the padding rows keep these: they are no records
    rest[:len(sent)] = of_tuple[sent]
    sender, receiver = np.concatenate([sender, rest], axis=1), np.concatenate([receiver, of_tuple], axis=1)
    prog = full_house_bus(field, dc, _lib.P3R_AIR_MAX_LIVE)
    assert ctx.lookup_program_info(prog, (3 + 2 * dc,))["peak_live"] == _lib.P3R_AIR_MAX_LIVE
    n, _ = check(ctx, field, dc, [receiver, sender], progs=[prog, prog])
    assert n == 0
    drop = 70
    sender[drop, 2] = 0
    n, got = check(ctx, field, dc, [receiver, sender], progs=[prog, prog])
    assert n == 1 and (got[0]["instance"], got[0]["row"], got[0]["term"]) == (0, sent[drop], 0)
    assert got[0]["net"] == [p - 1] + [0] * (dc - 1) and got[0]["n_records"] == np.count_nonzero(sent == sent[drop])


def direct(field, dc):
    """The denominator straight from DC columns, the multiplicity from the next: the test names the keys word by word."""
    import plonky3_recursion_amd as p3r
    b = p3r.AirBuilder(field)
    b.lookup(b.local(0, dc), b.local_ext(0, 0))
    b.end_lookup_column()
    return b


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_keys_that_differ_in_one_word_only_and_a_small_cap(ctxs, field, dc):
    """Three pairs of keys, one record each: the pair differs in the top coefficient word only (every coefficient must be
    sorted), in bit 30 of a word only (the whole 31-bit range), in the lowest bit of a word only.  Six unbalanced keys,
    reported by first record - the rows are laid out so that the order of the keys is not the order of the rows."""
    ctx, p = ctxs(field, dc), ref.P(field)
    base = [12345, 678, 91011, 1213, 1415][:dc]
    keys = []
    for word, delta in ((dc - 1, 1 << 20), (1, 1 << 30), (0, 1)):
        other = list(base)
        other[word] += delta
        keys += [other, list(base)]
        base = [v + 7 for v in base]
    assert all(v < p for k in keys for v in k) and len({tuple(k) for k in keys}) == 6
    order = [5, 0, 3, 4, 1, 2]
    table = np.zeros((8, dc + 1), dtype=np.uint32)
    for row, k in enumerate(order):
        table[row, :dc], table[row, dc] = keys[k], 1 + row
    table[6:, :dc] = keys[0]   # two rows of padding on an existing key: multiplicity 0, no records
    chal = np.zeros((0, dc), dtype=np.uint32)
    inst = [(direct(field, dc), [table], ())]
    want = check_ref.lookup_balance(field, dc, [(inst[0][0].program(), [table], ())], chal)
    assert want[0] == 6 and [e["row"] for e in want[1]] == list(range(6)) and all(e["n_records"] == 1 for e in want[1])
    assert [e["denominator"] for e in want[1]] == [keys[k] for k in order]
    n, got = run(ctx, inst, chal)
    assert (n, got) == want
    for cap in (0, 1, 4):   # fewer entries than keys: the first `cap` by first record, and the whole count
        n, got = run(ctx, inst, chal, cap=cap)
        assert n == 6 and got == want[1][:cap]


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_a_run_longer_than_a_block(ctxs, field, dc):
    """One tuple received in 300 rows with multiplicity 1 and sent once with 300: balanced.  Sent with 299: one record
    short.  The run of 301 records crosses a 256-thread block of the scans."""
    ctx, p = ctxs(field, dc), ref.P(field)
    rng = np.random.default_rng(1830 + dc)
    rows = np.sort(rng.choice(512, size=300, replace=False))
    receiver = np.concatenate([rng.integers(0, p, size=(512, 2), dtype=np.uint32), np.zeros((512, 1), dtype=np.uint32)], axis=1)
    receiver[rows] = (77, 4242, 1)
    for sent, unbalanced in ((300, 0), (299, 1)):
        sender = np.array([[77, 4242, p - sent]], dtype=np.uint32)
        n, got = check(ctx, field, dc, [receiver, sender])
        assert n == unbalanced
        if unbalanced:
            assert got[0]["net"] == [1] + [0] * (dc - 1) and got[0]["n_records"] == 301 and (got[0]["instance"], got[0]["row"]) == (0, rows[0])


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_edge_multiplicities(ctxs, field, dc):
    """A multiplicity of P - 1 against 1, and extension multiplicities: e against -e cancels, e against P - 1 does not."""
    import plonky3_recursion_amd as p3r
    ctx, p, E = ctxs(field, dc), ref.P(field), ref.ext(field, dc)
    rng = np.random.default_rng(1840 + dc)
    b = p3r.AirBuilder(field)
    b.lookup(b.local_ext(0, 2), b.challenge(0) + b.local(0, 0) + b.challenge(1) * b.local(0, 1))
    b.end_lookup_column()
    e = [int(v) for v in rng.integers(1, p, size=dc)]
    one = [1] + [0] * (dc - 1)
    rows = [(1, 10, one), (1, 10, E.neg(one)),          # 1 and P - 1: balanced
            (2, 20, e), (2, 20, E.neg(e)),              # e and -e: balanced
            (3, 30, e), (3, 30, E.neg(one)),            # e and P - 1: net e - 1
            (4, 40, [0] * (dc - 1) + [5]), (4, 40, [0] * dc)]   # only the top coefficient is not zero: a record; all zero: none
    table = np.array([[t0, t1] + list(m) for t0, t1, m in rows], dtype=np.uint32)
    chal = challenges_of(field, dc)
    want = check_ref.lookup_balance(field, dc, [(b.program(), [table], ())], chal)
    assert want == check_ref.lookup_balance(field, dc, [(b.program(), [table], ())], chal, key_of=lambda i, r, t: (int(table[r, 0]), int(table[r, 1])))
    assert want[0] == 2 and [x["row"] for x in want[1]] == [4, 6] and want[1][0]["net"] == E.sub(e, one) and want[1][1]["n_records"] == 1
    assert run(ctx, [(b, [table], ())], chal) == want


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_more_slots_than_one_pass_of_block_histograms(ctxs, field, dc):
    """2^12 rows of 20 terms and a receiver of 2^9 rows: 82,432 slots - the sort's histograms span 14 blocks, the scans
    several tiles.  Multiplicities 0, 1 and 2 over 500 tuples; three receives are then put off by one."""
    ctx, p = ctxs(field, dc), ref.P(field)
    rng = np.random.default_rng(1850 + dc)
    h, terms, n_tuples = 1 << 12, 20, 500
    second = rng.integers(0, p, size=512, dtype=np.uint32)
    ids = rng.integers(0, n_tuples, size=(h, terms))
    mult = rng.integers(0, 3, size=(h, terms))
    sender = np.empty((h, 3 * terms), dtype=np.uint32)
    sender[:, 0::3], sender[:, 1::3], sender[:, 2::3] = ids, second[ids], mult
    counts = np.bincount(ids.reshape(-1), weights=mult.reshape(-1), minlength=512).astype(np.int64)
    receiver = np.stack([np.arange(512, dtype=np.uint32), second, ((p - counts) % p).astype(np.uint32)], axis=1)
    assert h * terms + 512 > (1 << 8) * 256 and (counts[:n_tuples] > 0).all() and not counts[n_tuples:].any()
    n, _ = check(ctx, field, dc, [sender, receiver])
    assert n == 0
    for t in (3, 250, 499):
        receiver[t, 2] = (int(receiver[t, 2]) + 1) % p
    n, got = check(ctx, field, dc, [sender, receiver], cap=8)
    assert n == 3 and len(got) == 3
    assert all(e["instance"] == 0 and e["net"] == [1] + [0] * (dc - 1) for e in got)
    assert [(e["row"], e["term"]) for e in got] == sorted((e["row"], e["term"]) for e in got)


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_refusals_leave_the_context_usable(ctxs, field, dc):
    import plonky3_recursion_amd as p3r
    from plonky3_recursion_amd import _lib as L
    ctx, p = ctxs(field, dc), ref.P(field)
    rng = np.random.default_rng(1860 + dc)
    sender, receiver, _ = two_tables(field, rng)
    sender[3, 2] = 0
    chal = challenges_of(field, dc)
    progs = [bus(field), bus(field)]
    want = check_ref.lookup_balance(field, dc, [(progs[0].program(), [sender], ()), (progs[1].program(), [receiver], ())], chal)
    assert want[0] == 1
    dm = [ctx.upload(sender), ctx.upload(receiver)]
    short = ctx.upload(receiver[:4])
    good = [(progs[0], [dm[0]]), (progs[1], [dm[1]])]
    LOC, LK, END = L.P3R_AIR_LOCAL, L.P3R_AIR_LOOKUP, L.P3R_AIR_LOOKUP_END
    bad_chal = chal.copy()
    bad_chal[1, 0] = p
    cases = [
        ("n_inst == 0", P3R_EINVAL, [], chal),
        ("a selector in the second instance", P3R_EINVAL, [good[0], ([(L.P3R_AIR_IS_FIRST_ROW, 0, 0), (LOC, 0, 0), (LK, 0, 1), (END, 0, 0)], [dm[1]])], chal),
        ("an ASSERT_ZERO", P3R_EINVAL, [([(LOC, 0, 0), (LK, 0, 0), (END, 0, 0), (L.P3R_AIR_ASSERT_ZERO, 0, 0)], [dm[0]]), good[1]], chal),
        ("matrices of different heights in one instance", P3R_EINVAL, [good[0], ([(LOC, 1, 0), (LK, 0, 0), (END, 0, 0)], [dm[1], short])], chal),
        ("no matrix", P3R_EINVAL, [good[0], (progs[1], [])], chal),
        ("a non-canonical challenge word", P3R_EINVAL, good, bad_chal),
        ("a non-canonical public value", P3R_EINVAL, [good[0], (progs[1], [dm[1]], [p])], chal),
    ]
    for name, code, inst, ch in cases:
        with pytest.raises(p3r.P3rError) as e:
            ctx.lookup_check_device(inst, challenges=ch)
        assert e.value.code == code and len(str(e.value)) > 15, (name, str(e.value))
        if len(inst) == 2 and name != "a non-canonical challenge word":
            assert "instance" in str(e.value), (name, str(e.value))
        assert ctx.lookup_check_device(good, challenges=chal) == want, "after: " + name
    for d in dm + [short]:
        d.free()


def test_more_slots_than_the_limit_and_zk_contexts_are_refused(ctxs):
    """2^24 rows x 17 terms over one column: one slot more than 2^28 would be 2^28 + 2^24.  Refused before anything is
    allocated; 16 terms, exactly 2^28 slots, are not asked for here (11 GiB of records)."""
    import plonky3_recursion_amd as p3r
    ctx = ctxs("koala-bear", 4)
    d = ctx.upload(np.ones((1 << 24, 1), dtype=np.uint32))
    b = p3r.AirBuilder("koala-bear")
    for _ in range(17):
        b.lookup(1, b.local(0, 0))
    b.end_lookup_column()
    with pytest.raises(p3r.P3rError) as e:
        ctx.lookup_check_device([(b, [d])])
    d.free()
    assert e.value.code == P3R_EUNSUPPORTED and "P3R_LOOKUP_CHECK_MAX_RECORDS" in str(e.value)
    zk = p3r.Context(field="koala-bear", zk=1, zk_seed=1, log_blowup=1, max_log_arity=1, log_final_poly_len=0, query_pow_bits=3, num_queries=4)
    try:
        d = zk.upload(np.ones((8, 1), dtype=np.uint32))
        with pytest.raises(p3r.P3rError) as e:
            zk.lookup_check_device([(b, [d])])
        assert e.value.code == P3R_EUNSUPPORTED and "zk" in str(e.value)
        d.free()
    finally:
        zk.close()
