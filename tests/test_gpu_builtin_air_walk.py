"""GPU: the prover's self-check and both verifiers against tests/builtin_air_ref.py, mutant by mutant.

Per (layer, table) the walk of tests/builtin_air_mutants.py - the isolating mutant of every constraint index (a covering one
for the listed exceptions), one live-row and one dead-row single-cell mutant per main column, one mutant per prediction
class - goes through prove_batch on one prepared layer, and the reference alone says what must happen: a refusal that names
the smallest failing instance, a refusal for the lookup sum, or a proof that the oracle's verifier and the native one accept.
Every table of every configuration is walked on the generated layer, which then still proves byte-equal to the oracle on the
same context; the ALU and width-32 tables are walked again on the fixture layer ("+fx": rows for the selectors the generated
layers never set, its own preprocessed commitment), whose unmutated proof both verifiers accept."""
import time

import numpy as np
import pytest

import builtin_air_mutants as M
import layer_lib

pytestmark = pytest.mark.gpu

P3R_EINVAL = -1     # include/p3r.h
# the large walks are split by constraint range: the mutants are ordered by the smallest constraint index they fail (those
# that fail none come last) and cut into equal parts
PARTS = {"poseidon2": 2, "poseidon2_w32": 3}
KINDS = ["const", "public", "alu", "poseidon2", "recompose"]


def cases():
    out = []
    for n in M.CONFIGS:
        kinds = KINDS + (["poseidon2_w32"] if n == "kb4-w32" else [])
        out += [(n, k, part) for k in kinds for part in range(PARTS.get(k, 1))]
        out += [(n + "+fx", k, part) for k in kinds if k in ("alu", "poseidon2_w32") for part in range(PARTS.get(k, 1))]
    return out


class Prepared:
    """One context per configuration with the generated layer and its fixture layer prepared on it."""

    def __init__(self, oracle, name):
        import plonky3_recursion_amd as p3r
        base = M.Layer(oracle, name)
        self.layers = {name: base, name + "+fx": M.FixtureLayer(base)}
        self.ctx = p3r.Context(field=base.field, **M.FRI, **base.cfg["ctx"])
        self.pd, self.cap, self.sel = {}, {}, {}
        for n, layer in self.layers.items():
            self.cap[n], self.pd[n] = self.ctx.prep_create(layer.airs(), [t["prep"] for t in layer.tables])
        assert np.array_equal(self.cap[name], base.L.prep_commit())
        self.want = base.L.prove()

    def select(self, name, kind):
        if (name, kind) not in self.sel:
            layer = self.layers[name]
            s = M.select(layer, layer.instance(kind))
            nc = s["num_constraints"]
            s["ordered"] = sorted(s["chosen"], key=lambda pos: (min(s["survey"][pos][2]) if s["survey"][pos][2] else nc, pos))
            self.sel[(name, kind)] = s
        return self.sel[(name, kind)]

    def verify(self, name, proof):
        """Both verifiers, from the statement: the AIR list, the layer's preprocessed commitment, the heights."""
        import plonky3_recursion_amd as p3r
        layer = self.layers[name]
        airs = [dict(a, ext_degree=layer.d) for a in layer.airs()]
        layer_lib.oracle_verify_statement(layer.base.L.orc if hasattr(layer, "base") else layer.L.orc, layer.field, layer.prm,
                                          airs, self.cap[name], proof)
        p3r.verify_batch(self.ctx.cfg, layer.airs(), self.cap[name],
                         [int(t["main"].shape[0]).bit_length() - 1 for t in layer.tables], proof)

    def expect(self, name, changes):
        """changes: [(mutant, new row, S, balanced)] applied together."""
        import plonky3_recursion_amd as p3r
        layer = self.layers[name]
        want = M.expected_message(layer, [(m, S, bal) for m, new, S, bal in changes])
        mains = M.apply(layer, *[(m, new) for m, new, S, bal in changes])
        if want is None:
            self.verify(name, self.ctx.prove_batch(self.pd[name], mains))
        else:
            with pytest.raises(p3r.P3rError) as e:
                self.ctx.prove_batch(self.pd[name], mains)
            assert e.value.code == P3R_EINVAL and want in str(e.value), \
                ([(m, sorted(S), bal) for m, new, S, bal in changes], str(e.value))

    def unmutated(self):
        (name, base), (fx_name, fx) = self.layers.items()
        assert self.ctx.prove_batch(self.pd[name], [t["main"] for t in base.tables]) == self.want
        self.verify(fx_name, self.ctx.prove_batch(self.pd[fx_name], [t["main"] for t in fx.tables]))

    def close(self):
        for pd in self.pd.values():
            pd.free()
        self.ctx.close()


@pytest.fixture(scope="module")
def prepared(oracle):
    """The configuration in use: replaced when a case asks for another one, closed after the last case."""
    holder = {}

    def get(name):
        if holder.get("name") != name:
            if "st" in holder:
                holder.pop("st").close()
            holder["name"], holder["st"] = name, Prepared(oracle, name)
        return holder["st"]
    yield get
    if "st" in holder:
        holder.pop("st").close()


@pytest.mark.parametrize("name,kind,part", cases())
def test_walk(prepared, name, kind, part):
    t0 = time.time()
    st = prepared(name.split("+")[0])
    s = st.select(name, kind)
    n_parts = PARTS.get(kind, 1)
    per = -(-len(s["ordered"]) // n_parts)
    t1 = time.time()
    counts = {"constraint": 0, "lookup": 0, "accepted": 0}
    for pos in s["ordered"][part * per:(part + 1) * per]:
        m, new, S, balanced = s["survey"][pos]
        counts[M.classify(S, balanced)] += 1
        st.expect(name, [(m, new, S, balanced)])
    t2 = time.time()
    st.unmutated()
    print("walk %s %s part %d/%d: %s, selection %.2fs device %.2fs total %.2fs" %
          (name, kind, part + 1, n_parts, counts, t1 - t0, t2 - t1, time.time() - t0))


@pytest.mark.parametrize("name", ["kb4-l3k4", "bb4-l2k3", "kb5-coeff"])
def test_two_tables_at_once(prepared, name):
    """check_at_zeta tests the instances in order, then the global sum: with two tables broken the refusal names the smaller
    instance, whichever is changed first, and a broken lookup next to a broken constraint is refused for the constraint."""
    st = prepared(name)
    layer = st.layers[name]
    first = {}
    for kind in ("const", "alu", "poseidon2"):
        s = st.select(name, kind)
        for cl in ("constraint", "lookup"):
            pos = next((pos for pos in s["ordered"] if M.classify(*s["survey"][pos][2:]) == cl), None)
            if pos is not None:
                first[(kind, cl)] = s["survey"][pos]
    alu, p2, lookup = first[("alu", "constraint")], first[("poseidon2", "constraint")], first[("const", "lookup")]
    assert alu[0]["inst"] < p2[0]["inst"]
    assert M.expected_message(layer, [x[:1] + x[2:] for x in (p2, alu)]).startswith("instance %d:" % alu[0]["inst"])
    st.expect(name, [alu, p2])
    st.expect(name, [p2, alu])
    assert M.expected_message(layer, [x[:1] + x[2:] for x in (lookup, p2)]).startswith("instance %d:" % p2[0]["inst"])
    st.expect(name, [lookup, p2])
    st.expect(name, [lookup, first[("alu", "lookup")]])          # two unbalanced tables: the global sum
    st.unmutated()
