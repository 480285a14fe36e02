"""The cases and the assertions of the field-arithmetic check, shared by the host half (tests/test_field_host.py: field.h
compiled by g++) and the device half (tests/field_device_cases.py: the p3r_test_field_op seam of the knobs library).

An operation of csrc/field_test_ops.h takes raw Montgomery words and returns raw words.  OPS below restates its numbering
and operand layout and gives each operation its reference on canonical residues (tests/field_ref.py); the conversion to
and from Montgomery form (x * 2^32 mod P) happens here, with integers.  Every comparison is bit-exact."""
import collections
import os
import subprocess

import numpy as np

import field_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "plonky3_recursion_amd", "csrc")
FIELDS = ("koala-bear", "baby-bear")
N_RANDOM = 1 << 14
SEED = 20261018
SIZE = {"f": 1, "r": 1, "e1": 1, "e4": 4, "e5": 5}
RANDOM_EXPONENT = 0x9E3779B1
U32_MAX = 0xFFFFFFFF

Op = collections.namedtuple("Op", "name id ins outs ref")
Case = collections.namedtuple("Case", "op label aux inputs")   # inputs: uint32 [n, words in per case]


def params(field):
    return R.PARAMS[field]


def mont(field, x):
    return x * (1 << 32) % params(field)["p"]


def unmont(field, w):
    p = params(field)["p"]
    return w * pow(1 << 32, p - 2, p) % p


# ------------------------------------------------------------------ the operation table
def _ops():
    def base(fn):           # fn(p, *values) -> value
        return lambda field, aux, *a: [fn(params(field)["p"], *a)]

    def ext(make, fn):      # fn(E, aux, *args) -> list of outputs
        return lambda field, aux, *a: fn(make(field), aux, *a)

    def norm3(E, aux, a):
        n0, n1, d, odd0, odd1 = E.norm_tower(a)
        return [n0, n1, d]

    def inv_given(E, aux, a, d):
        # inv_given(norm, d) is linear in d and is the inverse at d = 1 / norm: a^-1 * norm * d
        return [E.scale(E.inv(a), R.mul(E.norm_tower(a)[2], d, E.p))]

    t = [
        Op("fp_add", 0, "ff", "f", base(lambda p, a, b: R.add(a, b, p))),
        Op("fp_sub", 1, "ff", "f", base(lambda p, a, b: R.sub(a, b, p))),
        Op("fp_neg", 2, "f", "f", base(lambda p, a: R.neg(a, p))),
        Op("fp_mul", 3, "ff", "f", base(lambda p, a, b: R.mul(a, b, p))),
        Op("fp_sqr", 4, "f", "f", base(lambda p, a: R.mul(a, a, p))),
        Op("fp_dbl", 5, "f", "f", base(lambda p, a: R.add(a, a, p))),
        Op("fp_halve", 6, "f", "f", base(lambda p, a: R.halve(a, p))),
        Op("fp_dot2", 7, "ffff", "f", base(lambda p, a1, b1, a2, b2: (a1 * b1 + a2 * b2) % p)),
        Op("fp_sqr_times", 8, "ff", "f", base(lambda p, a, x: a * a % p * x % p)),
        Op("fp_cube", 9, "f", "f", base(lambda p, a: a * a % p * a % p)),
        # reduce64_lazy(a * b): a representative in [0, 2P) of the Montgomery word of the product (see check)
        Op("fp_reduce_lazy", 10, "ff", "f", base(lambda p, a, b: R.mul(a, b, p))),
        Op("fp_from_canonical", 11, "r", "f", base(lambda p, x: x % p)),
        Op("fp_to_canonical", 12, "f", "r", base(lambda p, a: a % p)),
        Op("fp_pow", 13, "f", "f", lambda field, aux, a: [R.fpow(a, aux, params(field)["p"])]),
        Op("fp_inv", 14, "f", "f", base(lambda p, a: R.inv(a, p))),
        Op("fp_two_adic_generator", 15, "r", "f", None),    # enumerated: reference_words
        Op("bit_reverse", 16, "rr", "r", None),             # enumerated: reference_words
    ]
    for d, make, first in ((4, R.quartic, 32), (5, R.quintic, 64)):
        e, n = "e%d" % d, "fp%d_" % d
        t += [
            Op(n + "add", first + 0, [e, e], [e], ext(make, lambda E, aux, a, b: [E.add(a, b)])),
            Op(n + "sub", first + 1, [e, e], [e], ext(make, lambda E, aux, a, b: [E.sub(a, b)])),
            Op(n + "neg", first + 2, [e], [e], ext(make, lambda E, aux, a: [E.neg(a)])),
            Op(n + "mul", first + 3, [e, e], [e], ext(make, lambda E, aux, a, b: [E.mul(a, b)])),
            Op(n + "mul_base", first + 4, [e, "f"], [e], ext(make, lambda E, aux, a, s: [E.scale(a, s)])),
            Op(n + "dot2_base", first + 5, [e, "f", e, "f"], [e],
               ext(make, lambda E, aux, a1, b1, a2, b2: [E.add(E.scale(a1, b1), E.scale(a2, b2))])),
            Op(n + "sqr", first + 6, [e], [e], ext(make, lambda E, aux, a: [E.mul(a, a)])),
        ]
    t += [
        Op("fp4_dbl", 39, ["e4"], ["e4"], ext(R.quartic, lambda E, aux, a: [E.add(a, a)])),
        Op("fp4_halve", 40, ["e4"], ["e4"], ext(R.quartic, lambda E, aux, a: [E.halve(a)])),
        Op("fp4_pow", 41, ["e4"], ["e4"], ext(R.quartic, lambda E, aux, a: [E.pow(a, aux)])),
        Op("fp4_norm", 42, ["e4"], ["f", "f", "f"], ext(R.quartic, norm3)),
        Op("fp4_inv_given", 43, ["e4", "f"], ["e4"], ext(R.quartic, inv_given)),
        Op("fp4_inv", 44, ["e4"], ["e4"], ext(R.quartic, lambda E, aux, a: [E.inv(a)])),
        Op("fp5_frobenius1", 71, ["e5"], ["e5"], ext(R.quintic, lambda E, aux, a: [E.frobenius(a, 1)])),
        Op("fp5_frobenius2", 72, ["e5"], ["e5"], ext(R.quintic, lambda E, aux, a: [E.frobenius(a, 2)])),
        Op("fp5_mul_c0", 73, ["e5", "e5"], ["f"], ext(R.quintic, lambda E, aux, a, b: [E.mul_c0(a, b)])),
        Op("fp5_norm_cofactor", 74, ["e5"], ["e5"], ext(R.quintic, lambda E, aux, a: [E.norm_cofactor(a)])),
        Op("fp5_pow", 75, ["e5"], ["e5"], ext(R.quintic, lambda E, aux, a: [E.pow(a, aux)])),
        Op("fp5_inv", 76, ["e5"], ["e5"], ext(R.quintic, lambda E, aux, a: [E.inv(a)])),
        Op("fp5_dbl", 77, ["e5"], ["e5"], ext(R.quintic, lambda E, aux, a: [E.add(a, a)])),
        Op("fp5_halve", 78, ["e5"], ["e5"], ext(R.quintic, lambda E, aux, a: [E.halve(a)])),
        Op("fp1_mul", 96, ["e1", "e1"], ["e1"], ext(R.linear, lambda E, aux, a, b: [E.mul(a, b)])),
        Op("fp1_inv", 97, ["e1"], ["e1"], ext(R.linear, lambda E, aux, a: [E.inv(a)])),
    ]
    return collections.OrderedDict((o.name, o._replace(ins=list(o.ins), outs=list(o.outs))) for o in t)


OPS = _ops()


def words_in(op):
    return sum(SIZE[k] for k in op.ins)


def words_out(op):
    return sum(SIZE[k] for k in op.outs)


def ops_of(field):
    return [o for o in OPS.values() if params(field)["quintic"] or not o.name.startswith("fp5_")]


# ------------------------------------------------------------------ reference on words
def reference(field, op, aux, cols):
    """The result words of `op` for operand words `cols` (one entry per operand word: Python integers, or uint64 arrays
    with one entry per case)."""
    if op.name == "fp_two_adic_generator":
        return [_map(lambda bits: mont(field, R.two_adic_generator(field, bits)), cols[0])]
    if op.name == "bit_reverse":
        return [_map(R.bit_reverse, cols[0], cols[1])]
    args, at = [], 0
    for k in op.ins:
        vals = [cols[at + i] if k == "r" else unmont(field, cols[at + i]) for i in range(SIZE[k])]
        args.append(vals if k.startswith("e") else vals[0])
        at += SIZE[k]
    out = []
    for k, v in zip(op.outs, op.ref(field, aux, *args)):
        vals = v if k.startswith("e") else [v]
        assert len(vals) == SIZE[k]
        out += [x if k == "r" else mont(field, x) for x in vals]
    return out


def _map(fn, *cols):
    if isinstance(cols[0], np.ndarray):
        return np.array([fn(*(int(c[i]) for c in cols)) for i in range(len(cols[0]))], dtype=np.uint64)
    return fn(*cols)


def reference_words(field, case):
    """uint32 [n, words out per case]: the array evaluation of `reference`."""
    a = case.inputs.astype(np.uint64)
    out = reference(field, case.op, case.aux, [np.ascontiguousarray(a[:, i]) for i in range(a.shape[1])])
    return np.stack([np.broadcast_to(np.asarray(c, dtype=np.uint64), (a.shape[0],)) for c in out], axis=1).astype(np.uint32)


def reference_words_integers(field, case, rows):
    """The same for the chosen rows with Python integers only."""
    return np.array([[int(x) for x in reference(field, case.op, case.aux, [int(w) for w in case.inputs[r]])] for r in rows],
                    dtype=np.uint32)


# ------------------------------------------------------------------ operands
def edge_words(field):
    """The Montgomery words where a reduction or a conditional subtraction can go wrong."""
    p = params(field)["p"]
    r1 = (1 << 32) % p
    e = [0, 1, 2, r1, p - r1, r1 * r1 % p, (p - 1) // 2, (p + 1) // 2, p - 2, p - 1, (1 << 16) - 1, 1 << 16, 1 << 30,
         (1 << 31) - p - 1, (1 << 31) - p + 1]
    assert len(set(e)) == 15 and all(0 <= x < p for x in e)
    return e


def dot2_words(field):
    p = params(field)["p"]
    return [0, (1 << 32) % p, (p + 1) // 2, p - 2, p - 1]


def trits(field):
    p = params(field)["p"]
    return [0, (1 << 32) % p, p - 1]


def ext_elements(field, d):
    """Every element with coefficients from {0, one, P - 1}: zero, one, the base field, the subfields, single coefficients."""
    t = trits(field)
    return [[t[(i // 3 ** k) % 3] for k in range(d)] for i in range(3 ** d)]


def sparse_elements(field, d):
    """Zero and the elements with one nonzero coefficient."""
    return [e for e in ext_elements(field, d) if sum(1 for c in e if c) <= 1]


def product(*lists):
    """Rows: every combination of one entry per list (an entry is a word or a list of words), flattened."""
    rows = [[]]
    for lst in lists:
        rows = [r + (list(x) if isinstance(x, (list, tuple)) else [x]) for r in rows for x in lst]
    return np.array(rows, dtype=np.uint32)


def pow_exponents(field):
    p = params(field)["p"]
    return [0, 1, 2, 3, p - 2, p - 1, U32_MAX]


def ext_pow_exponents(field):
    return [0, 1, 2, 3, params(field)["p"] - 1, U32_MAX]


def build_cases(field):
    """Every case of `field`, in a fixed order, as launches of at most 59 049 cases."""
    f = params(field)
    p = f["p"]
    E, out = edge_words(field), []

    def rng_of(op):
        return np.random.default_rng([SEED, f["field_id"], op.id])

    def random_words(op, n=N_RANDOM):
        return rng_of(op).integers(0, p, size=(n, words_in(op)), dtype=np.uint32)

    def put(name, label, inputs, aux=0):
        op = OPS[name]
        inputs = np.ascontiguousarray(inputs, dtype=np.uint32).reshape(-1, words_in(op))
        out.append(Case(op, label, aux, inputs))

    for name in ("fp_neg", "fp_sqr", "fp_dbl", "fp_halve", "fp_cube", "fp_from_canonical", "fp_to_canonical", "fp_inv", "fp1_inv"):
        put(name, "edge", product(E))
        put(name, "random", random_words(OPS[name]))
    for name in ("fp_add", "fp_sub", "fp_mul", "fp_sqr_times", "fp_reduce_lazy", "fp1_mul"):
        put(name, "edge", product(E, E))
        put(name, "random", random_words(OPS[name]))
    d5 = dot2_words(field)
    put("fp_dot2", "edge", product(d5, d5, d5, d5))
    put("fp_dot2", "random", random_words(OPS["fp_dot2"]))
    for e in pow_exponents(field):
        put("fp_pow", "edge e=%d" % e, product(E), aux=e)
    put("fp_pow", "random", random_words(OPS["fp_pow"]), aux=RANDOM_EXPONENT)
    put("fp_two_adic_generator", "all", product(range(f["two_adicity"] + 1)))
    rows = []
    for bits in range(25):
        rows += [[x, bits] for x in sorted({0, 1, (1 << bits) - 1, (1 << bits) >> 1}) if x < (1 << bits)]
    put("bit_reverse", "edge", rows)
    rng = rng_of(OPS["bit_reverse"])
    bits = rng.integers(0, 25, size=N_RANDOM, dtype=np.uint32)
    x = rng.integers(0, 1 << 24, size=N_RANDOM, dtype=np.uint32) & ((np.uint32(1) << bits) - np.uint32(1))
    put("bit_reverse", "random", np.stack([x, bits], axis=1))

    for d in (4, 5) if f["quintic"] else (4,):
        n = "fp%d_" % d
        S, sparse, T = ext_elements(field, d), sparse_elements(field, d), trits(field)
        unary = ["neg", "sqr", "dbl", "halve", "inv"] + (["norm"] if d == 4 else ["frobenius1", "frobenius2", "norm_cofactor"])
        for s in unary:
            put(n + s, "edge", product(S))
            put(n + s, "random", random_words(OPS[n + s]))
        for s in ["add", "sub", "mul"] + (["mul_c0"] if d == 5 else []):
            put(n + s, "edge", product(S, S))
            put(n + s, "random", random_words(OPS[n + s]))
        put(n + "mul_base", "edge", product(S, E))
        put(n + "mul_base", "random", random_words(OPS[n + "mul_base"]))
        put(n + "dot2_base", "edge", product(sparse, T, sparse, T))
        put(n + "dot2_base", "random", random_words(OPS[n + "dot2_base"]))
        for e in ext_pow_exponents(field):
            put(n + "pow", "edge e=%d" % e, product(S), aux=e)
        put(n + "pow", "random", random_words(OPS[n + "pow"]), aux=RANDOM_EXPONENT)
    # inv_given: d at edge words, and at the d that makes it the inverse (1 / norm; zero for the zero element)
    S = ext_elements(field, 4)
    put("fp4_inv_given", "edge", product(S, dot2_words(field)))
    Eq = R.quartic(field)
    true_d = [mont(field, R.inv(Eq.norm_tower([unmont(field, c) for c in a])[2], p)) for a in S]
    put("fp4_inv_given", "true d", [a + [d] for a, d in zip(S, true_d)])
    put("fp4_inv_given", "random", random_words(OPS["fp4_inv_given"]))
    return out


def expected_totals(field):
    """Cases per operation, written out: 15 edge words, 81 / 243 extension elements, 9 / 11 sparse ones, 2^14 random."""
    r = N_RANDOM
    t = {n: 15 + r for n in ("fp_neg", "fp_sqr", "fp_dbl", "fp_halve", "fp_cube", "fp_from_canonical", "fp_to_canonical",
                             "fp_inv", "fp1_inv")}
    t.update({n: 225 + r for n in ("fp_add", "fp_sub", "fp_mul", "fp_sqr_times", "fp_reduce_lazy", "fp1_mul")})
    t.update(fp_dot2=625 + r, fp_pow=7 * 15 + r, fp_two_adic_generator=params(field)["two_adicity"] + 1,
             bit_reverse=1 + 2 + 4 * 23 + r)
    t.update({"fp4_" + n: 81 + r for n in ("neg", "sqr", "dbl", "halve", "inv", "norm")})
    t.update({"fp4_" + n: 6561 + r for n in ("add", "sub", "mul")})
    t.update(fp4_mul_base=81 * 15 + r, fp4_dot2_base=729 + r, fp4_pow=6 * 81 + r, fp4_inv_given=81 * 5 + 81 + r)
    if params(field)["quintic"]:
        t.update({"fp5_" + n: 243 + r for n in ("neg", "sqr", "dbl", "halve", "inv", "frobenius1", "frobenius2", "norm_cofactor")})
        t.update({"fp5_" + n: 59049 + r for n in ("add", "sub", "mul", "mul_c0")})
        t.update(fp5_mul_base=243 * 15 + r, fp5_dot2_base=1089 + r, fp5_pow=6 * 243 + r)
    return t


def totals(cases):
    t = collections.OrderedDict()
    for c in cases:
        t[c.op.name] = t.get(c.op.name, 0) + c.inputs.shape[0]
    return t


# ------------------------------------------------------------------ assertions
def check(field, case, got, want=None):
    """`got` (uint32 [n, words out]) is bit for bit what the reference says, and every field word is canonical."""
    p = params(field)["p"]
    op = case.op
    assert got.shape == (case.inputs.shape[0], words_out(op)) and got.dtype == np.uint32, (op.name, got.shape)
    if want is None:
        want = reference_words(field, case)
    what = (field, op.name, case.label)
    if op.name == "fp_reduce_lazy":
        # in [0, 2P), congruent to a * b * 2^-32, and one conditional subtraction gives what `*` returns
        g = got.astype(np.uint64)
        bad = np.flatnonzero((g >= 2 * p).any(axis=1))
        assert bad.size == 0, what + ("outside [0, 2P)", case.inputs[bad[0]].tolist(), got[bad[0]].tolist())
        got = np.where(g >= p, g - p, g).astype(np.uint32)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, what + ("%d of %d cases differ; first: operands, got, want" % (bad.size, got.shape[0]),
                                  case.inputs[bad[0]].tolist(), got[bad[0]].tolist(), want[bad[0]].tolist())
    at = 0
    for k in op.outs:
        if k != "r":
            assert (got[:, at:at + SIZE[k]] < p).all(), what + ("a result word is not below P",)
        at += SIZE[k]


INVERSES = ("fp_inv", "fp1_inv", "fp4_inv", "fp5_inv")


def check_inverse_of_zero(field, cases, results):
    """The inverse of zero is pinned to zero: what the code computes today (0^(P-2), zero norm, zero cofactor).  Callers
    are documented to check for zero first; this pins current behaviour, it does not bless calling inv on zero."""
    seen = set()
    for case, got in zip(cases, results):
        if case.op.name in INVERSES and case.label == "edge":
            assert not case.inputs[0].any(), "the first edge operand is zero"
            assert not got[0].any(), (field, case.op.name, "inverse of zero", got[0].tolist())
            seen.add(case.op.name)
    assert seen == {n for n in INVERSES if n in totals(cases)}
    return sorted(seen)


# ------------------------------------------------------------------ the host program
def build_host_program(outdir, csrc=CSRC, extra_flags=()):
    exe = os.path.join(str(outdir), "field_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", csrc, *extra_flags, os.path.join(ROOT, "tests", "field_host_main.cpp"),
                    "-o", exe], check=True)
    return exe


def run_host_program(exe, field, cases):
    """Every case through the host build, one process: a list of uint32 [n, words out] in the order of `cases`."""
    blob = b"".join(np.array([c.op.id, words_in(c.op), words_out(c.op), c.inputs.shape[0], c.aux], dtype=np.uint32).tobytes()
                    + c.inputs.tobytes() for c in cases)
    r = subprocess.run([exe, str(params(field)["field_id"])], input=blob, capture_output=True)
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-2000:])
    words = np.frombuffer(r.stdout, dtype=np.uint32)
    assert words.size == sum(c.inputs.shape[0] * words_out(c.op) for c in cases), "the host program wrote another number of words"
    out, at = [], 0
    for c in cases:
        n = c.inputs.shape[0] * words_out(c.op)
        out.append(words[at:at + n].reshape(-1, words_out(c.op)).copy())
        at += n
    return out
