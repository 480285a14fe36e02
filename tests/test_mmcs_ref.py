"""CPU: the plain Python tree (tests/mmcs_ref.py) against the oracle's trees (oracle/hash.hpp) on every geometry of
tests/mmcs_cases.py - caps, every opening (a fixed index list above 2^10 rows), both verifiers - so that the reference
and the case list are known to be right before the device is compared with them (tests/test_gpu_mmcs_geometry.py).
Equality of 32-bit words everywhere."""
import numpy as np
import pytest

import mmcs_cases
import mmcs_ref
import oracle_lib
from test_mmcs_reference_shapes import ARITY4_REF

FIELDS = mmcs_cases.FIELDS
KEYS = oracle_lib.FIELD_NAMES


def oracle_commit(oracle, field, case, mats, cap_height):
    return oracle.commit4(field, mats) if case.arity == 4 else oracle.commit(field, mats, cap_height)


def oracle_verify(oracle, field, case, cap, index, opened, proof):
    fn = oracle.verify4 if case.arity == 4 else oracle.verify
    return fn(field, cap, case.shapes, index, opened, proof)


def library_verify(cfg, case, cap, index, opened, proof):
    import plonky3_recursion_amd as p3r
    try:
        p3r.mmcs_verify(cfg, cap, case.shapes, index, opened, proof)
        return True
    except p3r.P3rError as e:
        assert "root mismatch" in str(e), str(e)
        return False


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("case", mmcs_cases.ALL, ids=repr)
def test_reference_tree_equals_oracle_tree(oracle, field, case):
    import plonky3_recursion_amd as p3r
    mats = case.mats(field)
    ref = mmcs_cases.reference_tree(oracle, field, case)
    indices = case.indices()
    for cap_height in case.caps:
        cap, otree = oracle_commit(oracle, field, case, mats, cap_height)
        assert np.array_equal(ref.cap(cap_height), cap), "%s cap %d: cap" % (case.name, cap_height)
        opened, proofs = ref.open_many(indices, cap_height)
        assert proofs.shape[1] == ref.proof_len(cap_height) == getattr(otree, "proof_len", case.log_h - cap_height)
        o_open = [otree.open(i) for i in indices]
        diff = mmcs_cases.first_difference(case, ref, cap_height, indices, np.stack([o for o, _ in o_open]),
                                           np.stack([p for _, p in o_open]), opened, proofs)
        assert diff is None, "oracle tree against the reference tree: " + diff
        for k, i in enumerate(indices):
            assert oracle_verify(oracle, field, case, cap, i, opened[k], proofs[k]), (case.name, cap_height, i)
        # the library's host verifier, and a changed sibling word, at the ends and the middle
        cfg, keep = p3r.make_config(field, cap_height=cap_height, mmcs_arity=case.arity, allow_unpinned_w32_defaults=True)
        for k in sorted({0, len(indices) // 2, len(indices) - 1}):
            i = indices[k]
            assert library_verify(cfg, case, cap, i, opened[k], proofs[k]), (case.name, cap_height, i)
            for sib in sorted({0, proofs.shape[1] - 1} & set(range(proofs.shape[1]))):
                bad = proofs[k].copy()
                bad[sib, (i + sib) % 8] ^= 1
                assert not oracle_verify(oracle, field, case, cap, i, opened[k], bad), (case.name, cap_height, i, sib)
                assert not library_verify(cfg, case, cap, i, opened[k], bad), (case.name, cap_height, i, sib)


SHORT = [(c, cap) for c in mmcs_cases.ALL for cap in c.caps if c.short_for(cap)]


def test_case_list_holds_matrices_shorter_than_the_cap():
    assert {c.log_h for c, _ in SHORT} == {6, 11} and len(SHORT) >= 16


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("case,cap_height", SHORT, ids=lambda v: repr(v))
def test_matrix_shorter_than_the_cap(oracle, field, case, cap_height):
    """The rule of mmcs_cases.py: the commit is accepted, the rows of such a matrix enter no digest, the opening carries its
    row, and both verifiers ignore that row."""
    import plonky3_recursion_amd as p3r
    mats = case.mats(field)
    short = case.short_for(cap_height)
    ref = mmcs_cases.reference_tree(oracle, field, case)
    cap, otree = oracle.commit(field, mats, cap_height)
    assert np.array_equal(ref.cap(cap_height), cap)
    # no digest depends on it: the same cap without it and with other contents
    kept = [m for k, m in enumerate(mats) if k not in short]
    assert np.array_equal(oracle.commit(field, kept, cap_height)[0], cap)
    assert np.array_equal(mmcs_ref.commit2(mmcs_cases.perms(oracle, field)[0], kept).cap(cap_height), cap)
    other = [(m + 1) % mmcs_cases.P[field] if k in short else m for k, m in enumerate(mats)]
    assert np.array_equal(oracle.commit(field, other, cap_height)[0], cap)
    # the opening carries its row at its own scale; the verifiers accept it, and any other words in its place
    cfg, keep = p3r.make_config(field, cap_height=cap_height)
    widths = [s[1] for s in case.shapes]
    for index in (0, case.hmax // 2 + 1, case.hmax - 1):
        opened, proof = ref.open(index, cap_height)
        o_opened, o_proof = otree.open(index)
        assert np.array_equal(opened, o_opened) and np.array_equal(proof, o_proof)
        changed = opened.copy()
        for k in short:
            at = sum(widths[:k])
            row = mats[k][index >> (case.log_h - (case.shapes[k][0].bit_length() - 1))]
            assert np.array_equal(opened[at:at + widths[k]], row)
            changed[at:at + widths[k]] = (row + 1) % mmcs_cases.P[field]
        for words in (opened, changed):
            assert oracle.verify(field, cap, case.shapes, index, words, proof)
            p3r.mmcs_verify(cfg, cap, case.shapes, index, words, proof)


def test_arity4_schedule_equals_the_oracle_schedule(oracle):
    seen = set()
    for case in mmcs_cases.GROUPS["e"]:
        heights = [s[0] for s in case.shapes]
        mine = [(step, inject) for step, _, _, inject in mmcs_ref.schedule4(heights)]
        assert mine == oracle.schedule4(heights), case.name
        seen |= {step for step, _ in mine}
    assert seen == {2, 4}   # the list holds bridges
    # every pair and triple of power-of-two heights up to 2^10
    for a in range(11):
        for b in range(a + 1):
            for c in range(b + 1):
                heights = [1 << b, 1 << a, 1 << c]
                mine = [(step, inject) for step, _, _, inject in mmcs_ref.schedule4(heights)]
                assert mine == oracle.schedule4(heights), heights


@pytest.mark.parametrize("name,mats,indices,steps", ARITY4_REF)
def test_arity4_schedule_equals_the_pinned_reference_shapes(name, mats, indices, steps):
    """The step lists test_mmcs_reference_shapes.py pins from the reference's own arity-4 tests."""
    sched = mmcs_ref.schedule4([m.shape[0] for m in mats])
    assert [s[0] for s in sched] == steps
    assert sum(s[0] - 1 for s in sched) == sum(s - 1 for s in steps)


@pytest.mark.parametrize("field", FIELDS)
def test_reference_sponge_and_compression_kats(oracle, golden, field):
    g = golden["prim"][KEYS[field]]
    p16, _ = mmcs_cases.perms(oracle, field)
    for kat in g["sponge"]:
        got = mmcs_ref.sponge(p16, 16, 8, np.array([kat["in"]], dtype=np.uint32))
        assert got[0].tolist() == kat["out"], len(kat["in"])
    kat = g["compress"]
    got = mmcs_ref.compress(p16, 16, [np.array([kat["left"]], dtype=np.uint32), np.array([kat["right"]], dtype=np.uint32)])
    assert got[0].tolist() == kat["out"]
    # a one-row commit is its sponge
    for kat in g["sponge"]:
        tree = mmcs_ref.commit2(p16, [np.array([kat["in"]], dtype=np.uint32)])
        assert tree.cap(0)[0].tolist() == kat["out"]
