"""GPU: the hiding MMCS at the library's own Mmcs seam - Context.commit / commit_device (p3r_mmcs_commit / _dmat) honour
p3r_config.mmcs_salt_elems, and MerkleTree.open_many (p3r_mmcs_open_batch) opens many indices in one launch and returns
the `(salts, siblings)` openings that p3r_mmcs_verify_salted takes (recursion/src/pcs/mmcs.rs:315-413, :763-790).

The oracle side: a hiding commitment of [Mi] with salts [Si] IS the oracle's plain commitment of the widened matrices
[Mi | Si] (tests/test_hiding_mmcs.py::test_mmcs_seam_salted_opening).  The salts of a public commit come from a stream of
their own, so each Si is rebuilt from the device's opened salts - which must agree wherever two indices share a row."""
import ctypes as C

import numpy as np
import pytest

import harness_lib
import layer_lib
import oracle_lib

pytestmark = pytest.mark.gpu
S = 4
SHAPES = {2: [(64, 5), (64, 9), (16, 3)], 4: [(64, 5), (16, 3), (64, 2)]}


def rand_mats(field, shapes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, oracle_lib.MODULUS[field], size=s, dtype=np.uint32) for s in shapes]


def make_ctx(field, arity, salt=S, cap_height=0, **kw):
    import plonky3_recursion_amd as p3r
    kw.setdefault("zk_seed", 21)
    return p3r.Context(field=field, mmcs_arity=arity, cap_height=cap_height, mmcs_salt_elems=salt,
                       allow_unpinned_w32_defaults=True, **kw)


def oracle_commit(oracle, field, arity, mats, cap_height=0):
    return oracle.commit4(field, mats) if arity == 4 else oracle.commit(field, mats, cap_height)


def rebuild_salts(shapes, log_max_h, indices, salts):
    """Si (h_i x S) from the opened salts of `indices`, which must cover every row of every matrix."""
    idx = np.asarray(indices, dtype=np.int64)
    out = []
    for i, (h, _) in enumerate(shapes):
        rows = idx >> (log_max_h - (h.bit_length() - 1))
        assert set(rows.tolist()) == set(range(h))
        si = np.zeros((h, salts.shape[2]), dtype=np.uint32)
        si[rows] = salts[:, i, :]
        assert np.array_equal(si[rows], salts[:, i, :]), "indices that share a row of matrix %d opened different salts" % i
        out.append(si)
    return out


def check_openings(oracle, field, arity, shapes, cap, otree, indices, opened, salts, proofs):
    """Every opening equals the oracle's of the widened matrices; the native salted verifier accepts it and refuses one
    changed salt word."""
    import plonky3_recursion_amd as p3r
    P = oracle_lib.MODULUS[field]
    cfg, keep = p3r.make_config(field, cap_height=0, mmcs_arity=arity, mmcs_salt_elems=S, allow_unpinned_w32_defaults=True)
    cuts = np.cumsum([w + S for _, w in shapes])[:-1]
    for k, index in enumerate(indices):
        oo, op = otree.open(index)
        rows = np.split(np.asarray(oo, dtype=np.uint32), cuts)
        assert np.array_equal(opened[k], np.concatenate([r[:-S] for r in rows])), index
        assert np.array_equal(salts[k], np.stack([r[-S:] for r in rows])), index
        assert np.array_equal(proofs[k], op), index
        p3r.mmcs_verify(cfg, cap, shapes, index, opened[k], proofs[k], salts=salts[k])
        bad = salts[k].copy()
        bad[k % len(shapes), k % S] = (bad[k % len(shapes), k % S] + 1) % P
        with pytest.raises(p3r.P3rError, match="Merkle"):
            p3r.mmcs_verify(cfg, cap, shapes, index, opened[k], proofs[k], salts=bad)


@pytest.mark.parametrize("field,arity", [("koala-bear", 2), ("baby-bear", 2), ("koala-bear", 4)])
def test_commitment_and_every_opening_equal_the_oracle(oracle, field, arity):
    shapes = SHAPES[arity]
    mats = rand_mats(field, shapes, 5)
    ctx = make_ctx(field, arity)
    cap, tree = ctx.commit(mats)
    assert tree.salt_elems == S and tree.num_matrices == len(mats) and tree.log_max_height == 6
    indices = list(range(64))
    opened, salts, proofs = tree.open_many(indices)
    assert opened.shape == (64, sum(w for _, w in shapes)) and salts.shape == (64, len(mats), S)
    sm = rebuild_salts(shapes, 6, indices, salts)
    wide = [np.concatenate([m, s], axis=1) for m, s in zip(mats, sm)]
    ocap, otree = oracle_commit(oracle, field, arity, wide)
    assert np.array_equal(cap, ocap)
    check_openings(oracle, field, arity, shapes, cap, otree, indices, opened, salts, proofs)
    plain = make_ctx(field, arity, salt=0)
    pcap, ptree = plain.commit(mats)
    assert not np.array_equal(cap, pcap)
    ptree.free(); plain.close()
    tree.free(); ctx.close()


def test_throughput_kernels_under_salts(oracle):
    """2^16 rows: the FP64 leaf kernel (above the cooperative kernels' row limit) and a first compress level of more than
    16 K nodes (one permutation per lane) over salted classes, an injected salted class at 2^12; a batch of 2^16 indices."""
    field, arity = "koala-bear", 2
    shapes = [(1 << 16, 3), (1 << 12, 2)]
    mats = rand_mats(field, shapes, 6)
    ctx = make_ctx(field, arity)
    cap, tree = ctx.commit(mats)
    every = np.arange(1 << 16)
    o_all, s_all, p_all = tree.open_many(every)
    sm = rebuild_salts(shapes, 16, every, s_all)
    wide = [np.concatenate([m, s], axis=1) for m, s in zip(mats, sm)]
    ocap, otree = oracle_commit(oracle, field, arity, wide)
    assert np.array_equal(cap, ocap)
    rng = np.random.default_rng(7)
    indices = [(1 << 16) - 1] + [int(i) for i in rng.integers(0, 1 << 16, size=31)] + [0]
    indices.append(indices[5])    # a repeat; the list is unsorted
    assert len(indices) == 34 and sorted(indices) != indices
    opened, salts, proofs = tree.open_many(indices)
    for k, index in enumerate(indices):   # the small batch equals the large one
        assert np.array_equal(opened[k], o_all[index]) and np.array_equal(salts[k], s_all[index]) and np.array_equal(proofs[k], p_all[index])
    check_openings(oracle, field, arity, shapes, cap, otree, indices, opened, salts, proofs)
    tree.free(); ctx.close()


def test_freshness_and_replay():
    import plonky3_recursion_amd as p3r
    field = "koala-bear"
    mats = rand_mats(field, SHAPES[2], 8)
    ctx = make_ctx(field, 2)
    n0 = ctx.zk_nonce
    cap_a, ta = ctx.commit(mats)
    assert ctx.zk_nonce == n0 + 1
    cap_b, tb = ctx.commit(mats)
    assert ctx.zk_nonce == n0 + 2 and not np.array_equal(cap_a, cap_b)
    ctx.zk_nonce = n0
    cap_c, tc = ctx.commit(mats)
    assert np.array_equal(cap_c, cap_a) and ctx.zk_nonce == n0 + 1
    assert np.array_equal(tc.open_many([3, 60])[1], ta.open_many([3, 60])[1])
    for t in (ta, tb, tc):
        t.free()
    ctx.close()
    # keyed by the operating system: the same caller key, other salts
    key = [1, 2, 3, 4, 5, 6, 7, 8]
    caps = []
    for _ in range(2):
        c = make_ctx(field, 2, zk_seed=None, zk_key=key)
        cap, t = c.commit(mats)
        with pytest.raises(p3r.P3rError):
            c.zk_nonce = 0
        caps.append(cap)
        t.free(); c.close()
    assert not np.array_equal(caps[0], caps[1])
    # HidingFriPcs runs over the non-hiding MMCS: zk = 1 without salts stays a plain commit and takes no nonce
    c = make_ctx(field, 2, salt=0, zk=1)
    cap, t = c.commit(mats)
    plain = make_ctx(field, 2, salt=0)
    pcap, pt = plain.commit(mats)
    assert np.array_equal(cap, pcap) and c.zk_nonce == 0 and t.salt_elems == 0
    t.free(); c.close(); pt.free(); plain.close()


def test_proof_after_a_public_commit_equals_the_oracle_at_that_nonce(oracle):
    """A public commit takes a proof counter value: the proof made after it is the oracle's proof number 1."""
    import harness_adapters as wl
    import plonky3_recursion_amd as p3r
    field, log_h, salt = "koala-bear", 7, 4
    kw = dict(log_blowup=2, max_log_arity=2, log_final_poly_len=1, query_pow_bits=3, num_queries=4)
    arrs = harness_lib.generate(field, log_h, seed=100 + log_h, horner_chain_len=12, sponge_chain_len=3, merkle_depth=4)
    ctx = p3r.Context(field=field, mmcs_salt_elems=salt, zk_seed=21, allow_unpinned_w32_defaults=True, **kw)
    tp = p3r.TablePacking().with_fri_params(kw["log_final_poly_len"], kw["log_blowup"])
    cpd = p3r.CircuitProverData(ctx, wl.circuit_prep_from_arrays(arrs), tp)
    assert ctx.zk_nonce == 0
    cap, tree = ctx.commit(rand_mats(field, SHAPES[2], 9))
    assert ctx.zk_nonce == 1
    got = p3r.BatchStarkProver(ctx).prove_all_tables(wl.traces_from_arrays(arrs), cpd)
    prm1 = layer_lib.params(mmcs_salt_elems=salt, zk_seed=21, zk_nonce=1, **kw)
    assert got.proof == layer_lib.OracleLayer(oracle, field, arrs, prm1).prove() and ctx.zk_nonce == 2
    tree.free(); cpd.free(); ctx.close()


@pytest.mark.parametrize("arity,cap_height", [(2, 0), (2, 2), (4, 0)])
def test_plain_trees_open_many_equals_the_single_index_form(oracle, arity, cap_height):
    field = "koala-bear"
    shapes = SHAPES[arity]
    mats = rand_mats(field, shapes, 10)
    ctx = make_ctx(field, arity, salt=0, cap_height=cap_height)
    cap, tree = ctx.commit(mats)
    ocap, otree = oracle_commit(oracle, field, arity, mats, cap_height)
    assert np.array_equal(cap, ocap) and tree.salt_elems == 0 and tree.num_matrices == len(mats)
    indices = [63, 0, 17, 17, 40, 1, 62]
    opened, salts, proofs = tree.open_many(indices)
    assert salts is None
    for k, index in enumerate(indices):
        o1, p1 = tree.open_batch(index)
        oo, op = otree.open(index)
        assert np.array_equal(opened[k], o1) and np.array_equal(proofs[k], p1)
        assert np.array_equal(opened[k], oo) and np.array_equal(proofs[k], op)
    tree.free(); ctx.close()


@pytest.mark.parametrize("arity", [2, 4])
def test_commit_device_borrows_the_matrices_and_owns_its_salts(arity):
    field = "koala-bear"
    mats = rand_mats(field, SHAPES[arity], 11)
    ctx = make_ctx(field, arity)
    dmats = [ctx.upload(m) for m in mats]
    ctx.zk_nonce = 5
    cap_h, th = ctx.commit(mats)
    ctx.zk_nonce = 5
    cap_d, td = ctx.commit_device(dmats)
    assert np.array_equal(cap_h, cap_d) and ctx.zk_nonce == 6
    assert td.salt_elems == S and td.num_matrices == len(mats)
    indices = [9, 63, 0, 9]
    for a, b in zip(th.open_many(indices), td.open_many(indices)):
        assert np.array_equal(a, b)
    th.free(); td.free()
    for d, m in zip(dmats, mats):    # still the caller's
        assert np.array_equal(d.download(), m)
        d.free()
    ctx.close()


def test_refusals():
    import plonky3_recursion_amd as p3r
    from plonky3_recursion_amd import _lib
    field = "koala-bear"
    mats = rand_mats(field, SHAPES[2], 12)
    ctx = make_ctx(field, 2)
    cap, tree = ctx.commit(mats)
    with pytest.raises(p3r.P3rError, match="out of range") as e:
        tree.open_many([3, 64])
    assert e.value.code == -1
    with pytest.raises(p3r.P3rError, match="p3r_mmcs_open_batch") as e:
        tree.open_batch(3)
    assert e.value.code == -1
    w, depth = ctx.lib.p3r_tree_total_width(tree.h), ctx.lib.p3r_tree_proof_len(tree.h)
    assert w == sum(m.shape[1] for m in mats)     # the caller's widths, without the salts
    opened, proofs = np.zeros((1, w), dtype=np.uint32), np.zeros((1, depth, 8), dtype=np.uint32)
    idx = (C.c_size_t * 1)(3)
    rc = ctx.lib.p3r_mmcs_open_batch(ctx.h, tree.h, idx, 1, opened.ctypes.data_as(_lib.u32p), None, proofs.ctypes.data_as(_lib.u32p))
    assert rc == -1 and "salts" in ctx.lib.p3r_last_error(ctx.h).decode()
    assert ctx.lib.p3r_mmcs_open_batch(ctx.h, tree.h, None, 0, None, None, None) == 0     # n = 0 touches nothing
    o, s, p = tree.open_many([])
    assert o.shape == (0, w) and s.shape == (0, len(mats), S) and p.shape == (0, depth, 8)
    o, s, p = tree.open_many([3])   # the context is still good
    p3r.mmcs_verify(ctx.cfg, cap, SHAPES[2], 3, o[0], p[0], salts=s[0])
    tree.free(); ctx.close()
    plain = make_ctx(field, 2, salt=0)
    cap, tree = plain.commit(mats)
    with pytest.raises(p3r.P3rError, match="out of range"):
        tree.open_many([1 << 40])
    tree.free(); plain.close()
