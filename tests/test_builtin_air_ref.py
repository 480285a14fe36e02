"""CPU: the built-in table AIRs as tests/builtin_air_ref.py states them (from the reference's Rust), checked on the oracle's
tables and on the fixture layers, and the coverage of the mutant walk of tests/builtin_air_mutants.py - decided by that
reference alone.  Every table of every configuration is walked; the coverage conditions are decided on the fixture layer
for the tables it changes (it holds every row of the generated table and the fixture rows)."""
import numpy as np
import pytest

import builtin_air_mutants as M
import builtin_air_ref as R
import oracle_lib

_layers, _selected = {}, {}


def layer_of(oracle, name):
    """name or name + "+fx"."""
    base = name.split("+")[0]
    if base not in _layers:
        _layers[base] = M.Layer(oracle, base)
        _layers[base + "+fx"] = M.FixtureLayer(_layers[base])
    return _layers[name]


def selected(oracle, name, kind):
    if (name, kind) not in _selected:
        layer = layer_of(oracle, name)
        _selected[(name, kind)] = M.select(layer, layer.instance(kind))
    return _selected[(name, kind)]


KINDS = ["const", "public", "alu", "poseidon2", "recompose"]
WALKS = [(n + ("+fx" if k in ("alu", "poseidon2_w32") else ""), k) for n in M.CONFIGS
         for k in KINDS + (["poseidon2_w32"] if n == "kb4-w32" else [])]


@pytest.mark.parametrize("field", ["koala-bear", "baby-bear"])
def test_permutation_against_the_golden_vectors(golden, field):
    """tests/golden/primitives.json (made by a pure-Python permutation, no oracle): the known answers of the width-16
    permutation."""
    kats = golden["prim"][R.NAMES[field]]["permute"]
    assert len(kats) >= 3
    for k in kats:
        assert R.permute(field, 16, k["in"]) == [int(x) for x in k["out"]]


@pytest.mark.parametrize("field", ["koala-bear", "baby-bear"])
def test_permutation_from_its_definition_equals_the_oracles(oracle, field):
    rng = np.random.default_rng(3)
    p = oracle_lib.MODULUS[field]
    for width, permute in ((16, oracle.permute), (32, oracle.p2w_permute)):
        st = rng.integers(0, p, size=(4, width), dtype=np.uint32)
        st[0] = 0
        st[1] = p - 1
        want = permute(field, st)
        for s, w in zip(st, want):
            assert R.permute(field, width, s) == [int(x) for x in w]
            cols = R.perm_columns(field, width, [int(x) for x in s])
            assert len(cols) == R.perm_num_cols(field, width) and cols[-width:] == [int(x) for x in w]


@pytest.mark.parametrize("name", list(M.CONFIGS) + [n + "+fx" for n in M.CONFIGS])
def test_reference_vanishes_on_the_oracles_tables(oracle, name):
    layer = layer_of(oracle, name)
    assert [t["kind"] for t in layer.tables] == [k for k in KINDS[:4] + ["poseidon2_w32", "recompose"]
                                                 if k != "poseidon2_w32" or name.startswith("kb4-w32")]
    if name.endswith("+fx"):
        assert layer.changed == (["alu", "poseidon2_w32"] if name.startswith("kb4-w32") else ["alu"])
    for desc, t in zip(layer.descs, layer.tables):
        assert R.widths(desc) == (t["main"].shape[1], t["prep"].shape[1]), desc
        m = R.constraint_matrix(desc, t["prep"], t["main"]) if R.num_constraints(desc) else np.zeros((0, 1))
        assert m.shape[0] == R.num_constraints(desc)
        assert not m.any(), (desc, np.argwhere(m)[:4])               # every row, the wrap row included
        assert R.failing(desc, t["prep"], t["main"]) == set()
        # the scalar interface agrees with the array one
        for r in (0, t["main"].shape[0] - 1):
            assert R.constraints(desc, t["prep"], t["main"], r) == [0] * R.num_constraints(desc)
    assert R.bus_balance([(d, t["prep"], t["main"]) for d, t in zip(layer.descs, layer.tables)])


def test_constraint_counts():
    """The length of the evaluated list (num_constraints counts nothing else) against the counts the statement implies:
    8 D for an ALU lane 0 plus D per pack step and 5 D per further lane; one constraint per committed permutation column
    past the inputs, after the circuit constraints."""
    d = R.make_desc
    assert R.num_constraints(d("alu", "koala-bear", 1, 2)) == 8 * 4
    assert R.num_constraints(d("alu", "koala-bear", 3, 4)) == 8 * 4 + 2 * 4 + 2 * 5 * 4
    assert R.num_constraints(d("alu", "koala-bear", 2, 5)) == 8 * 4 + (1 + 1 + 2) * 4 + 5 * 4
    assert R.num_constraints(d("alu", "koala-bear", 3, 4, ext_degree=5)) == 8 * 5 + 2 * 5 + 2 * 5 * 5
    assert R.num_constraints(d("poseidon2", "koala-bear")) == 34 + 8 * 16 + 20 == 182
    assert R.num_constraints(d("poseidon2", "baby-bear")) == 34 + 8 * 32 + 26 == 316
    assert R.num_constraints(d("poseidon2", "koala-bear", ext_degree=5)) == 42 + 8 * 16 + 20
    assert R.num_constraints(d("poseidon2_w32", "koala-bear")) == 68 + 8 * 32 + 31
    for k in ("const", "public", "recompose"):
        assert R.num_constraints(d(k, "koala-bear")) == 0


@pytest.mark.parametrize("name,kind", WALKS)
def test_coverage_conditions(oracle, name, kind):
    layer = layer_of(oracle, name)
    inst = layer.instance(kind)
    s = selected(oracle, name, kind)
    nc, w = s["num_constraints"], layer.tables[inst]["main"].shape[1]
    zero = M.structural_zero(layer.descs[inst]) if nc else []        # the zero polynomial: no constraint at all
    assert zero == ([21, 23, 25, 27] if name.startswith("kb4-l1k2") and kind == "alu" else [])
    # 1. every index lies in S of some mutant
    assert s["uncovered"] == zero, s["uncovered"]
    # 2. at most one in ten without an isolating mutant, and the committed list is the recomputed one
    unisolated = [i for i in range(nc) if i not in s["isolating"] and i not in zero]
    assert unisolated == sorted(i for idx, reason in M.UNISOLATED.get((name, kind), []) for i in idx), unisolated
    assert 10 * len(unisolated) <= nc
    # 3. every main column is mutated on a live row, and on a dead row where the table has one for it
    assert sorted(s["live"]) == list(range(w))
    no_dead = [c for c in range(w) if c not in s["dead"]]
    assert no_dead == M.no_dead_row_columns(layer, inst), no_dead
    # 4. each prediction class, or the table says which it cannot have
    missing = sorted(k for k, v in s["classes"].items() if not v)
    cannot = (["accepted"] if no_dead == list(range(w)) else []) + (["constraint"] if nc == 0 else [])
    assert missing == cannot, (missing, s["classes"])
    print(name, kind, "constraints", nc, "isolated", len(s["isolating"]), "exceptions", len(unisolated), "structurally zero",
          len(zero), "classes", s["classes"], "device walk", len(s["chosen"]))


def test_arbiter_on_a_hand_written_add_row(oracle):
    """One Add row of lane 0: out[2] + 1 breaks a + b - out in coefficient 2, constraint index 2 of instance 2, and
    nothing else; a[1] + 1 breaks coefficient 1 (index 1) and, a * b entering no active equation, nothing else."""
    layer = layer_of(oracle, "kb4-l3k4")
    inst = layer.instance("alu")
    assert inst == 2
    t = layer.tables[inst]
    row = int(np.nonzero(t["prep"][:, 1] == 1)[0][0])                  # sel_add of lane 0
    assert t["prep"][(row + 1) % len(t["prep"]), 4] == 0               # the next row is no Horner step
    for col, idx in ((12 + 2, 2), (1, 1)):
        new = t["main"][row].copy()
        new[col] = (int(new[col]) + 1) % layer.p
        (S, balanced), = M.judge(layer, inst, np.array([row]), new[None, :])
        assert S == frozenset([idx])
        assert M.expected_message(layer, [(dict(inst=inst), S, balanced)]) == \
            "instance 2: constraints do not match the quotient at zeta"
        # the whole-matrix interface says the same
        mains = M.apply(layer, (dict(inst=inst, row=row), new))
        assert R.failing(layer.descs[inst], t["prep"], mains[inst]) == {idx}


def test_arbiter_on_a_hand_written_partial_round_cell(oracle):
    """The post-S-box cell of partial round 3 on the last row (no transition constraint reads it): + 1 alone breaks that
    round's link (index 34 + 64 + 3) and what follows from the cell; with the later columns recomputed only the one link
    is broken."""
    layer = layer_of(oracle, "kb4-l3k4")
    inst = layer.instance("poseidon2")
    t = layer.tables[inst]
    row, col, idx = t["main"].shape[0] - 1, 16 + 4 * 16 + 3, 34 + 4 * 16 + 3
    new = t["main"][row].copy()
    new[col] = (int(new[col]) + 1) % layer.p
    (S, _), = M.judge(layer, inst, np.array([row]), new[None, :])
    # the changed cell re-enters elements 1..15 through the internal layer, and those are committed again only after the
    # first ending full round: every later partial link and that round's 16 post-states break with it
    assert S == frozenset(range(idx, 34 + 4 * 16 + 20 + 16))
    cols = R.perm_columns(layer.field, 16, [int(x) for x in t["main"][row, :16]], override=(col, int(new[col])))
    assert cols[:col] == [int(x) for x in t["main"][row, :col]] and cols[col] == int(new[col])
    new[:len(cols)] = cols
    (S, balanced), = M.judge(layer, inst, np.array([row]), new[None, :])
    assert S == frozenset([idx])
    # a dead cell: the index accumulator of a padding row
    new = t["main"][row].copy()
    new[-1] = (int(new[-1]) + 1) % layer.p
    (S, balanced), = M.judge(layer, inst, np.array([row]), new[None, :])
    assert (S, balanced) == (frozenset(), True) and M.expected_message(layer, [(dict(inst=inst), S, balanced)]) is None
