"""GPU: the device Merkle tree (csrc/mmcs_impl.hip.h and its kernels) walked over every geometry of tests/mmcs_cases.py
against the plain Python tree of tests/mmcs_ref.py - the cap, every opened row and every sibling (so every digest of
every layer below the cap) up to 2^10 rows, a fixed index list above.  The oracle fixture serves the permutation only.
Equality of 32-bit words; a mismatch names the case, the layer, the level and the node.

The kernels below their regime (the knobs build, fresh processes): the one-permutation-per-lane level kernel down to
two nodes, one level per launch, eight levels per launch; and one proof with every Merkle threshold pushed down."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mmcs_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS_DIR = os.path.join(ROOT, "plonky3_recursion_amd", "knobs")
KNOBS = os.path.join(KNOBS_DIR, "libp3r_hip.so")
EXE = os.path.join(ROOT, "examples", "prove_next_layer")
FIELDS = mmcs_cases.FIELDS


def walk(oracle, field, group):
    import plonky3_recursion_amd as p3r
    bad = mmcs_cases.walk_device(p3r, oracle, field, mmcs_cases.GROUPS[group])
    assert not bad, "%d mismatches, the first ones:\n%s" % (len(bad), "\n".join(bad[:8]))


@pytest.mark.parametrize("field", FIELDS)
def test_group_a_height_and_cap(oracle, field):
    walk(oracle, field, "a")


@pytest.mark.parametrize("field", FIELDS)
def test_group_b_injection_position(oracle, field):
    walk(oracle, field, "b")


@pytest.mark.parametrize("field", FIELDS)
def test_group_c_regime_boundary(oracle, field):
    walk(oracle, field, "c")


@pytest.mark.parametrize("field", FIELDS)
def test_group_d_leaf_rows(oracle, field):
    walk(oracle, field, "d")


@pytest.mark.parametrize("field", FIELDS)
def test_group_e_arity4(oracle, field):
    walk(oracle, field, "e")


@pytest.mark.parametrize("field", FIELDS)
def test_matrix_shorter_than_the_cap_on_the_device(oracle, field):
    """The rule of mmcs_cases.py on the device tree: the cap does not depend on such a matrix, the opening carries its row,
    p3r_mmcs_verify accepts the device's opening and ignores that row."""
    import plonky3_recursion_amd as p3r
    case = next(c for c in mmcs_cases.GROUPS["b"] if c.name == "b/h06+s02")
    cap_height = 3
    assert case.short_for(cap_height) == [1]
    mats = case.mats(field)
    ref = mmcs_cases.reference_tree(oracle, field, case)
    ctx = p3r.Context(field=field, cap_height=cap_height)
    try:
        cap, tree = ctx.commit(mats)
        cap_alone, tree_alone = ctx.commit(mats[:1])
        assert np.array_equal(cap, ref.cap(cap_height)) and np.array_equal(cap_alone, cap)
        for index in (0, 37, 63):
            opened, proof = tree.open_batch(index)
            want_opened, want_proof = ref.open(index, cap_height)
            assert np.array_equal(opened, want_opened) and np.array_equal(proof, want_proof)
            assert np.array_equal(opened[2:], mats[1][index >> 4])
            p3r.mmcs_verify(ctx.cfg, cap, case.shapes, index, opened, proof)
            assert oracle.verify(field, cap, case.shapes, index, opened, proof)
            changed = opened.copy()
            changed[2:] = (changed[2:] + 1) % mmcs_cases.P[field]
            p3r.mmcs_verify(ctx.cfg, cap, case.shapes, index, changed, proof)
        tree.free()
        tree_alone.free()
    finally:
        ctx.close()


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("width", [3, 200], ids=["block_of_83_words", "block_of_280_words"])
def test_open_many_shape_edges(oracle, field, width):
    """p3r_mmcs_open_batch: one workgroup of 256 lanes per index walks the words of that index's block (rows, then
    siblings).  A block shorter and a block longer than a workgroup; one index, repeated and unsorted indices, and more
    indices than a workgroup has lanes."""
    import mmcs_ref
    import plonky3_recursion_amd as p3r
    h = 1 << 10
    rng = np.random.default_rng(width)
    mats = [rng.integers(0, mmcs_cases.P[field], size=(h, width), dtype=np.uint32)]
    ref = mmcs_ref.commit2(mmcs_cases.perms(oracle, field)[0], mats)
    assert (width + 8 * ref.proof_len(0) < 256) == (width == 3)
    ctx = p3r.Context(field=field)
    try:
        cap, tree = ctx.commit(mats)
        assert np.array_equal(cap, ref.cap(0))
        many = rng.integers(0, h, size=300).tolist()
        for indices in ([777], [5, 5, 1023, 0, 5, 512, 511, 0], many):
            opened, salts, proofs = tree.open_many(indices)
            want_opened, want_proofs = ref.open_many(indices)
            assert salts is None
            assert np.array_equal(opened, want_opened), indices[:8]
            assert np.array_equal(proofs, want_proofs), indices[:8]
        tree.free()
    finally:
        ctx.close()


def run_child(**knobs):
    if not os.path.exists(KNOBS):
        pytest.skip("knobs build of the library is absent (__graft_entry__.build() makes it)")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mmcs_geometry_child.py")], capture_output=True, text=True,
                       env=dict(os.environ, P3R_LIB_PATH=KNOBS, **knobs), timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["trees"] > 300
    assert res["mismatches"] == [], "%s: %d mismatches, the first ones:\n%s" % (knobs, len(res["mismatches"]),
                                                                             "\n".join(res["mismatches"][:8]))


def test_one_permutation_per_lane_levels_down_to_two_nodes():
    """P3R_COOP_MAX_NODES=1: k_mmcs_compress builds every level down to n = 2 (groups a and b, both fields)."""
    run_child(P3R_COOP_MAX_NODES="1")


def test_one_level_per_launch():
    """P3R_SUBTREE_NODES=2: k_mmcs_subtree with two digests per workgroup, one level per launch."""
    run_child(P3R_SUBTREE_NODES="2")


def test_eight_levels_per_launch():
    """P3R_SUBTREE_NODES=256: k_mmcs_subtree with 1024-lane workgroups, eight levels per launch."""
    run_child(P3R_SUBTREE_NODES="256")


def test_thresholds_pushed_down_give_the_same_proof(tmp_path):
    """P3R_COOP_MAX_NODES=1, P3R_COOP_MAX_LEAF_ROWS=1, P3R_SUBTREE_NODES=2 in the knobs build: the FRI commit phase hashes
    its small phases with the strided one-row-per-lane leaf kernel and builds every tree one level per launch, the
    transcript step riding on a two-digest launch; the proof must be the product's, byte for byte (the method of
    test_gpu_cpp_host.py::test_fallback_paths_give_the_same_proof, which moves the same knobs upward)."""
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "examples")], check=True)
    if not os.path.exists(KNOBS):
        pytest.skip("knobs build of the library is absent (__graft_entry__.build() makes it)")

    def proof(name, **env):
        out_file = str(tmp_path / (name + ".bin"))
        e = {**os.environ, **env}
        if env:   # the example's RUNPATH finds the product library; LD_LIBRARY_PATH goes first
            e["LD_LIBRARY_PATH"] = KNOBS_DIR + os.pathsep + e.get("LD_LIBRARY_PATH", "")
        r = subprocess.run([EXE, "koala-bear", "13", out_file, "1"], capture_output=True, text=True, timeout=300, env=e)
        assert r.returncode == 0, r.stdout + r.stderr
        return open(out_file, "rb").read()

    want = proof("product")
    assert proof("thresholds_down", P3R_COOP_MAX_NODES="1", P3R_COOP_MAX_LEAF_ROWS="1", P3R_SUBTREE_NODES="2") == want
