"""Mutants of satisfied recursion layers, judged by tests/builtin_air_ref.py alone.

A mutant is a set of cell changes to ONE row of one main matrix of a satisfied layer; every changed word stays canonical.

  (a)  one cell + 1 mod P
  (b)  permutation tables: one permutation cell + 1 and every later permutation column of that row recomputed from the
       permutation's definition (builtin_air_ref.perm_columns), so that only the link ending in that cell is broken; on an
       input cell this re-derives the whole row from the changed input

For each mutant the reference gives S, the set of (instance, constraint index) that fail, and whether the bus still
balances.  Nothing else predicts what the prover does:

  S non-empty             refused: "instance <min i>: constraints do not match the quotient at zeta"
  S empty, unbalanced     refused: "global lookup sum is not zero"
  S empty, balanced       a proof, accepted by both verifiers

The layer is satisfied (tests/test_builtin_air_ref.py checks that with the same reference), so a mutant of row r can only
fail on the (local, next) pairs (r - 1, r) and (r, r + 1), and only row r's tuples change."""
import numpy as np

import builtin_air_ref as R
import field_ref
import harness_lib
import layer_lib

GEN = dict(horner_chain_len=12, sponge_chain_len=3, merkle_depth=4)
FRI = dict(log_final_poly_len=1, query_pow_bits=2, num_queries=4)

# name: field, circuit degree D, harness flags, table packing, coefficient lookups of the Recompose table, Context extras
CONFIGS = {
    "kb4-l3k4": dict(field="koala-bear", d=4, flags=0, packing=dict(alu_lanes=3, horner_packed_steps=4), coeff=0, ctx={}),
    "kb4-l1k2": dict(field="koala-bear", d=4, flags=0, packing=dict(alu_lanes=1, horner_packed_steps=2), coeff=0, ctx={}),
    "kb4-l2k5": dict(field="koala-bear", d=4, flags=0, packing=dict(alu_lanes=2, horner_packed_steps=5), coeff=0, ctx={}),
    "bb4-l2k3": dict(field="baby-bear", d=4, flags=0, packing=dict(alu_lanes=2, horner_packed_steps=3), coeff=0, ctx={}),
    # D = 5 under the quartic STARK configuration: ALU, the compact-D1 table, Recompose with coefficient tuples
    "kb5-coeff": dict(field="koala-bear", d=5, flags=harness_lib.RECOMPOSE_COEFF, packing={}, coeff=1, ctx=dict(ext_degree=5)),
    "kb4-w32": dict(field="koala-bear", d=4, flags=harness_lib.P2_W32_OPS, packing={}, coeff=0,
                    ctx=dict(allow_unpinned_w32_defaults=True)),
}


class Layer:
    def __init__(self, oracle, name):
        c = CONFIGS[name]
        self.name, self.cfg, self.field, self.d = name, c, c["field"], c["d"]
        self.p = field_ref.PARAMS[self.field]["p"]
        self.arrs = harness_lib.generate(self.field, 6, flags=c["flags"], ext_degree=c["d"], **GEN)
        self.prm = layer_lib.params(**FRI)
        self.L = layer_lib.OracleLayer(oracle, self.field, self.arrs, self.prm,
                                       packing=dict(c["packing"], ext_degree=c["d"], recompose_coeff_lookups=c["coeff"]))
        self.tables = self.L.tables()
        self.descs = [R.make_desc(t["kind"], self.field, t["lanes"], t["horner_k"],
                                  c["coeff"] if t["kind"] == "recompose" else 0, c["d"]) for t in self.tables]

    def airs(self):
        return [dict(kind=t["kind_id"], lanes=t["lanes"], horner_packed_steps=t["horner_k"], coeff_lookups=d["coeff_lookups"])
                for t, d in zip(self.tables, self.descs)]

    def instance(self, kind):
        return [t["kind"] for t in self.tables].index(kind)


# ------------------------------------------------------------------ generators: (row, new row) per mutant
def single_cell(layer, inst):
    """(a): every cell of the table."""
    main = layer.tables[inst]["main"]
    h, w = main.shape
    rows = np.repeat(np.arange(h), w)
    cols = np.tile(np.arange(w), h)
    new = main[rows].astype(np.uint64)
    new[np.arange(h * w), cols] = (new[np.arange(h * w), cols] + 1) % layer.p
    return [dict(kind="a", inst=inst, row=int(r), col=int(c)) for r, c in zip(rows, cols)], rows, new.astype(np.uint32)


def single_cell_plus_two(layer, inst):
    """(c): one cell + 2 mod P - reaches a[0] (a[0] - 1) on Bool rows whose operand is 0, where + 1 gives the other bit."""
    muts, rows, new = single_cell(layer, inst)
    cols = np.array([m["col"] for m in muts])
    new = new.astype(np.uint64)
    new[np.arange(len(rows)), cols] = (new[np.arange(len(rows)), cols] + 1) % layer.p
    return [dict(m, kind="c") for m in muts], rows, new.astype(np.uint32)


def perm_relinked(layer, inst):
    """(b): every permutation cell of the table, the rest of its row's permutation columns recomputed."""
    desc, main = layer.descs[inst], layer.tables[inst]["main"]
    width = 32 if desc["kind"] == "poseidon2_w32" else 16
    h, w = main.shape
    pc = R.perm_num_cols(layer.field, width)
    inputs = [main[:, i].astype(np.uint64) for i in range(width)]
    muts, rows, new = [], [], []
    for c in range(pc):
        cols = R.perm_columns(layer.field, width, inputs, override=(c, (main[:, c].astype(np.uint64) + 1) % layer.p))
        block = main.copy()
        block[:, :pc] = np.stack(cols, axis=1).astype(np.uint32)
        muts += [dict(kind="b", inst=inst, row=r, col=c) for r in range(h)]
        rows.append(np.arange(h))
        new.append(block)
    return muts, np.concatenate(rows), np.concatenate(new)


# ------------------------------------------------------------------ the arbiter
def judge(layer, inst, rows, new, chunk=2048):
    """Per mutant (row r of instance `inst` replaced by new[m]): (frozenset of failing constraint indices, balanced)."""
    desc, t = layer.descs[inst], layer.tables[inst]
    main, prep = t["main"], t["prep"]
    h = main.shape[0]
    out = []
    nc = R.num_constraints(desc)
    for lo in range(0, len(rows), chunk):
        r = np.asarray(rows[lo:lo + chunk])
        nw = new[lo:lo + chunk]
        fails = np.zeros((len(r), nc), dtype=bool)
        if nc:
            prev, nxt = (r - 1) % h, (r + 1) % h
            T = lambda m: np.ascontiguousarray(m.T.astype(np.uint64))
            for (lm, nm, lp, np_, tr) in ((main[prev], nw, prep[prev], prep[r], prev != h - 1),
                                          (nw, main[nxt], prep[r], prep[nxt], r != h - 1)):
                a, b, c, d = T(lm), T(nm), T(lp), T(np_)
                vals = R.eval_cases(desc, lambda k: a[k], lambda k: b[k], lambda k: c[k], lambda k: d[k], tr.astype(np.uint64))
                fails |= (np.array(vals, dtype=np.uint64).reshape(nc, len(r)) != 0).T
        for m in range(len(r)):
            S = frozenset(int(i) for i in np.flatnonzero(fails[m]))
            balanced = True
            if not S:
                row = int(r[m])
                pr = np.stack([prep[row], prep[(row + 1) % h]])      # a row's tuples read its own main row only
                before = R.bus_multiset(desc, pr, np.stack([main[row], main[row]]), rows=[0])
                balanced = before == R.bus_multiset(desc, pr, np.stack([nw[m], nw[m]]), rows=[0])
            out.append((S, balanced))
    return out


def classify(S, balanced):
    return "constraint" if S else ("accepted" if balanced else "lookup")


def expected_message(layer, mutants):
    """What the prover must answer to a set of simultaneous mutants [(mutant, S, balanced)] of one layer; None: a proof."""
    bad = [m["inst"] for m, S, bal in mutants if S]
    if bad:
        return "instance %d: constraints do not match the quotient at zeta" % min(bad)
    if any(not bal for m, S, bal in mutants):
        return "global lookup sum is not zero"
    return None


def coverage_layers(base, fx):
    """[(layer, instance)] on which the coverage conditions are decided: the fixture layer for the tables it changes."""
    return [(fx if t["kind"] in fx.changed else base, i) for i, t in enumerate(base.tables)]


def dormant(layer, inst):
    """Constraint indices that vanish on this layer WHATEVER the main matrix holds: their preprocessed selectors are zero
    on every row, so no mutant of a main matrix can reach them here (two random matrices, decided by the reference)."""
    desc, t = layer.descs[inst], layer.tables[inst]
    if not R.num_constraints(desc):
        return []
    rng = np.random.default_rng(7)
    dead = None
    for _ in range(2):
        rnd = rng.integers(0, layer.p, size=t["main"].shape, dtype=np.uint32)
        zero = set(int(i) for i in np.flatnonzero(~R.constraint_matrix(desc, t["prep"], rnd).any(axis=1)))
        dead = zero if dead is None else dead & zero
    return sorted(dead)


# ------------------------------------------------------------------ the walk of one table
def survey(layer, inst):
    """Every generated mutant of the table with its verdict: [(mutant, new row, S, balanced)]."""
    desc = layer.descs[inst]
    muts, rows, new = single_cell(layer, inst)
    if desc["kind"] in ("poseidon2", "poseidon2_w32"):
        m2, r2, n2 = perm_relinked(layer, inst)
        muts, rows, new = muts + m2, np.concatenate([rows, r2]), np.concatenate([new, n2])
    if desc["kind"] == "alu":
        m2, r2, n2 = single_cell_plus_two(layer, inst)
        muts, rows, new = muts + m2, np.concatenate([rows, r2]), np.concatenate([new, n2])
    verdicts = judge(layer, inst, rows, new)
    return [(m, new[i], S, bal) for i, (m, (S, bal)) in enumerate(zip(muts, verdicts))]


def select(layer, inst, sv=None):
    """The walk of one table, decided by the reference alone.  Returns a dict:
      isolating   constraint index -> position in `sv` of a mutant with S == {index}
      covering    for the other indices: position of a mutant whose S holds the index (the smallest such S)
      uncovered   indices no mutant reaches
      live, dead  main column -> position of a type-(a) mutant that is refused / that still proves
      classes     class name -> number of surveyed mutants
      chosen      sorted positions of every mutant the device walk runs"""
    sv = survey(layer, inst) if sv is None else sv
    nc = R.num_constraints(layer.descs[inst])
    isolating, covering, live, dead = {}, {}, {}, {}
    classes = {"constraint": 0, "lookup": 0, "accepted": 0}
    first_of_class = {}
    for pos, (m, new, S, bal) in enumerate(sv):
        cl = classify(S, bal)
        classes[cl] += 1
        first_of_class.setdefault(cl, pos)
        if len(S) == 1:
            isolating.setdefault(next(iter(S)), pos)
        if m["kind"] == "a":
            (dead if cl == "accepted" else live).setdefault(m["col"], pos)
    for idx in range(nc):
        if idx in isolating:
            continue
        best = None
        for pos, (m, new, S, bal) in enumerate(sv):
            if idx in S and (best is None or len(S) < len(sv[best][2])):
                best = pos
        if best is not None:
            covering[idx] = best
    uncovered = [i for i in range(nc) if i not in isolating and i not in covering]
    chosen = sorted(set(isolating.values()) | set(covering.values()) | set(live.values()) | set(dead.values())
                    | set(first_of_class.values()))
    return dict(isolating=isolating, covering=covering, uncovered=uncovered, live=live, dead=dead, classes=classes,
                chosen=chosen, survey=sv, num_constraints=nc)


# ------------------------------------------------------------------ fixture rows
# The generated layers pack every Horner chain into lane 0 at the layer's full arity, and their width-32 rows are all Merkle
# rows: the selectors of the unpacked step, of Horner steps in the other lanes, of the lower arities and of sponge chaining
# into limb 0 of the width-32 table are zero on every row.  A fixture layer "<configuration>+fx" is the generated layer with
# such rows written into the padding of its ALU table (every multiplicity 0: the rows stay off the bus) and, where the layer
# has one, a width-32 table twice as high that ends in one sponge continuation row.  It has its own preprocessed commitment;
# the reference finds it satisfied and balanced (tests/test_builtin_air_ref.py) before any mutant is judged.
def _alu_fixture(layer, inst):
    desc, t = layer.descs[inst], layer.tables[inst]
    prep, main = t["prep"].copy(), t["main"].copy()
    p, D, lanes, K = layer.p, desc["ext_degree"], desc["lanes"], desc["horner_packed_steps"]
    E = field_ref.quartic(layer.field) if D == 4 else field_ref.quintic(layer.field)
    h = main.shape[0]
    rng = np.random.default_rng(11)
    rnd = lambda: [int(x) for x in rng.integers(0, p, size=D)]
    extra_main, extra_prep, num_int = lanes * 4 * D, lanes * 13, (K - 1) // 2
    ac = extra_main + num_int * D
    b_sq_col = ac + 2 * (K - 1) * D
    put = lambda q, col, v: main.__setitem__((q, slice(col, col + D)), v)
    sub = E.sub

    def horner_lane(q, lane, packed=0):
        m, pq = lane * 4 * D, lane * 13
        prev_out = [int(x) for x in main[q - 1, m + 3 * D:m + 4 * D]]
        a, b, c = rnd(), rnd(), rnd()
        prep[q, pq:pq + 13] = 0
        prep[q, pq], prep[q, pq + 4] = p - 1, 1                     # active, sel_horner; every multiplicity and reader flag 0
        if not packed:
            out = sub(E.add(E.mul(prev_out, b), c), a)
        else:
            prep[q, extra_prep + packed - 2] = 1                    # sel_k
            steps = {0: (a, c)}
            for step in range(1, packed):
                steps[step] = (rnd(), rnd())
                put(q, ac + 2 * (step - 1) * D, steps[step][0])
                put(q, ac + 2 * (step - 1) * D + D, steps[step][1])
            b_sq = E.mul(b, b)
            put(q, b_sq_col, b_sq)
            pair = lambda acc, s: sub(E.add(sub(E.add(E.mul(acc, b_sq), E.mul(steps[s][1], b)), E.mul(steps[s][0], b)),
                                            steps[s + 1][1]), steps[s + 1][0])
            out = pair(prev_out, 0)                                 # the first two steps fold into out (k = 2) or slot 0
            ints, s, slot = [out], 2, 0
            while s < packed:
                if s + 1 < packed:
                    out = pair(ints[slot], s)
                    if s + 2 < packed:
                        ints.append(out)
                        slot += 1
                    s += 2
                else:
                    out = sub(E.add(E.mul(ints[slot], b), steps[s][1]), steps[s][0])
                    s += 1
            if packed > 2:
                for k, v in enumerate(ints):
                    put(q, extra_main + k * D, v)
        put(q, m, a), put(q, m + D, b), put(q, m + 2 * D, c), put(q, m + 3 * D, out)

    q = int(np.flatnonzero(prep.any(axis=1)).max()) + 1
    specs = [0] + list(range(2, K + 1))                             # the unpacked step, then every packed arity
    for spec in specs:
        if q > h - 2:
            break
        horner_lane(q, 0, spec)
        if spec == 0:
            for lane in range(1, lanes):
                horner_lane(q, lane)
        q += 2                                                      # a blank row between fixture rows keeps each one alone
    return prep, main


def _w32_fixture(layer, inst):
    t = layer.tables[inst]
    h, w = t["main"].shape
    pc = R.perm_num_cols(layer.field, 32)
    blank = np.zeros(w, dtype=np.uint32)
    blank[:pc] = R.perm_columns(layer.field, 32, [0] * 32)
    main = np.concatenate([t["main"], np.tile(blank, (h, 1))])
    prep = np.concatenate([t["prep"], np.zeros_like(t["prep"])])
    prep[h, 46] = 1                                                 # the first padding row is a chain start
    q = h + 1                                                       # a sponge continuation into limb 0, off the bus
    prep[q, 2] = 1
    inputs = [0] * 32
    inputs[:4] = [int(x) for x in main[q - 1, pc - 32:pc - 28]]
    main[q, :pc] = R.perm_columns(layer.field, 32, inputs)
    return prep, main


class FixtureLayer:
    """The generated layer with fixture rows in its ALU table and in its width-32 table."""

    def __init__(self, base):
        self.base, self.name, self.cfg, self.field, self.d, self.p = base, base.name + "+fx", base.cfg, base.field, base.d, base.p
        self.descs, self.prm = base.descs, base.prm
        self.tables = [dict(t) for t in base.tables]
        self.changed = []
        for inst, t in enumerate(self.tables):
            if t["kind"] == "alu":
                t["prep"], t["main"] = _alu_fixture(base, inst)
            elif t["kind"] == "poseidon2_w32":
                t["prep"], t["main"] = _w32_fixture(base, inst)
            else:
                continue
            self.changed.append(t["kind"])

    airs = Layer.airs
    instance = Layer.instance


def structural_zero(desc):
    """Constraint indices that are the zero polynomial for this table shape - they vanish on random main AND random
    preprocessed rows (an empty selector sum: sel_ge3_next at K = 2).  No trace of any layer can fail them."""
    p = field_ref.PARAMS[desc["field"]]["p"]
    w, pw = R.widths(desc)
    rng = np.random.default_rng(5)
    m = R.constraint_matrix(desc, rng.integers(0, p, size=(8, pw), dtype=np.uint32), rng.integers(0, p, size=(8, w), dtype=np.uint32))
    return [int(i) for i in np.flatnonzero(~m.any(axis=1))]


# ------------------------------------------------------------------ committed exception lists (coverage condition 2)
# Constraint indices without an isolating mutant, per (layer, table), with the reason.  tests/test_builtin_air_ref.py
# recomputes these lists and fails when they differ; at most one index in ten per table may be listed.  The structurally zero
# indices of structural_zero() are no constraints and are not counted.
_B_SQ = ("the b^2 column of a packed Horner row enters its own definition and, times the previous output or an intermediate, "
         "the packed legs: no single change of it leaves one of the two standing")
_CHAIN = ("a chained input cell is also the input of its own row's permutation: re-deriving the row moves its outputs, which "
          "the following row chains from or the bus receives, and in the generated chains no last row carries this limb")
_D1 = [18, 20, 22, 24, 26, 28, 30, 32, 33, 34, 35, 36, 37, 38, 39, 40]
_W32 = [43, 44, 45, 46, 47, 48, 49, 50, 59, 60, 61, 62, 63, 64, 65, 66]
UNISOLATED = {
    ("kb4-l3k4+fx", "alu"): [([16, 17, 18, 19], _B_SQ)],
    ("kb4-l3k4", "poseidon2"): [([5, 6, 7, 8], _CHAIN)],
    ("kb4-l1k2", "poseidon2"): [([5, 6, 7, 8], _CHAIN)],
    ("kb4-l2k5", "poseidon2"): [([5, 6, 7, 8], _CHAIN)],
    ("bb4-l2k3", "poseidon2"): [([5, 6, 7, 8], _CHAIN)],
    ("kb4-w32", "poseidon2"): [([5, 6, 7, 8], _CHAIN)],
    ("kb5-coeff", "poseidon2"): [(_D1, _CHAIN)],
    ("kb4-w32+fx", "poseidon2_w32"): [(_W32, _CHAIN)],
}

def no_dead_row_columns(layer, inst):
    """Main columns without a dead row: the permutation constraints (and bit x bit2 of the width-32 table) are ungated, so
    every row of those columns is live; a table whose every row carries a multiplicity has no dead row at all."""
    desc, t = layer.descs[inst], layer.tables[inst]
    if desc["kind"] == "poseidon2":
        return list(range(R.perm_num_cols(layer.field, 16)))
    if desc["kind"] == "poseidon2_w32":
        pc = R.perm_num_cols(layer.field, 32)
        return list(range(pc)) + [pc + 2]
    if desc["kind"] in ("const", "public", "recompose"):
        plw = t["prep"].shape[1] // desc["lanes"]
        mult = 0 if desc["kind"] != "recompose" else 1
        D = desc["ext_degree"]
        out = []
        for lane in range(desc["lanes"]):
            cols = [lane * plw + mult] + ([lane * plw + 3 + 2 * i for i in range(D)] if desc["coeff_lookups"] else [])
            if t["prep"][:, cols].any(axis=1).all():
                out += list(range(lane * D, lane * D + D))
        return out
    return []


def apply(layer, *changes):
    """The layer's main matrices with (mutant, new row) changes applied."""
    mains = [t["main"] for t in layer.tables]
    for mutant, new_row in changes:
        if mains[mutant["inst"]] is layer.tables[mutant["inst"]]["main"]:
            mains[mutant["inst"]] = mains[mutant["inst"]].copy()
        mains[mutant["inst"]][mutant["row"]] = new_row
    return mains
