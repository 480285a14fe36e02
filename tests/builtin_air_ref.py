"""Row-wise statement of the built-in table AIRs, on integers over tests/field_ref.py.

Written from the reference's Rust `Air::eval` and interaction code (cited per constraint group below) and from the public
definition of the Poseidon2 permutation AIR; it shares nothing with csrc/ or oracle/.  A table is described by

    desc = dict(kind=..., lanes=..., horner_packed_steps=..., coeff_lookups=..., ext_degree=..., field=...)

with kind one of const, public, alu, poseidon2 (the width-16 table for D = 4, the compact-D1 table for D = 5),
poseidon2_w32, recompose.  Matrices are 2-D arrays of canonical residues in natural row order.

    constraints(desc, prep, main, r)    constraint values at row r, in the reference's assert order; next row (r + 1) mod h,
                                        is_transition = [r != h - 1]
    num_constraints(desc)               the length of that list
    interactions(desc, prep, main, r)   [(multiplicity, (index, v_0 .. v_{D-1}))] in push order
    failing(desc, prep, main)           the set of constraint indices that are non-zero on some row
    bus_balance(tables)                 whether the tuples of [(desc, prep, main)] cancel with their multiplicities
    perm_columns(field, width, inputs)  one row's permutation columns from its 16 / 32 input limbs

Every expression also runs on numpy uint64 arrays (one entry per case: eval_cases), which is how the mutant walk evaluates
tens of thousands of (row, next row) pairs at once; values stay canonical after every operation (products of two residues
are below 2^62) and differences are written a + (p - b)."""
import json
import os

import numpy as np

import field_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"koala-bear": "koala_bear", "baby-bear": "baby_bear"}
HALF_FULL = 4
# S-box x^3 without a register (KoalaBear), x^7 with one register holding x^3 (BabyBear); partial rounds per width
SBOX_REGISTERS = {"koala-bear": 0, "baby-bear": 1}
PARTIAL_ROUNDS = {("koala-bear", 16): 20, ("baby-bear", 16): 13, ("koala-bear", 32): 31, ("baby-bear", 32): 30}


# ------------------------------------------------------------------ the permutation, from its definition
def _inv_pow2(k, p):
    return pow(pow(2, k, p), p - 2, p)


def internal_diagonal16(field):
    """V with the internal matrix 1 + diag(V): [-2, 1, 2, 1/2, 3, 4, -1/2, -3, -4, ...] then the field's inverse powers of
    two (the published Poseidon2 instances of KoalaBear and BabyBear at width 16)."""
    p = field_ref.PARAMS[field]["p"]
    h = _inv_pow2
    if field == "koala-bear":
        v = [-2, 1, 2, h(1, p), 3, 4, -h(1, p), -3, -4, h(8, p), h(3, p), h(24, p), -h(8, p), -h(3, p), -h(4, p), -h(24, p)]
    else:
        v = [-2, 1, 2, h(1, p), 3, 4, -h(1, p), -3, -4, h(8, p), h(2, p), h(3, p), h(27, p), -h(8, p), -h(4, p), -h(27, p)]
    return [x % p for x in v]


_CONST = {}


def perm_constants(field, width):
    """(round constants: [4][width] initial full rounds | partial rounds | [4][width] final full rounds, diagonal)."""
    key = (field, width)
    if key not in _CONST:
        if width == 16:
            with open(os.path.join(ROOT, "tests/golden/poseidon2_rc_default.json")) as fh:
                _CONST[key] = ([int(x) for x in json.load(fh)[NAMES[field]]], internal_diagonal16(field))
        else:
            with open(os.path.join(ROOT, "tests/golden/poseidon2_w32_default.json")) as fh:
                d = json.load(fh)[NAMES[field]]
            _CONST[key] = ([int(x) for x in d["rc"]], [int(x) for x in d["diag"]])
        assert len(_CONST[key][0]) == 2 * HALF_FULL * width + PARTIAL_ROUNDS[key] and len(_CONST[key][1]) == width
    return _CONST[key]


def _sum(xs, p):
    acc = xs[0]
    for x in xs[1:]:
        acc = (acc + x) % p
    return acc


def external_linear(s, p):
    """M4 = [[2,3,1,1],[1,2,3,1],[1,1,2,3],[3,1,1,2]] on every chunk of four, then every element gains the sum of the
    elements of its residue class mod 4 (the Poseidon2 paper's M_E for t = 4 t')."""
    out = []
    for c in range(0, len(s), 4):
        a, b, cc, d = s[c:c + 4]
        out += [(2 * a + 3 * b + cc + d) % p, (a + 2 * b + 3 * cc + d) % p, (a + b + 2 * cc + 3 * d) % p,
                (3 * a + b + cc + 2 * d) % p]
    sums = [_sum(out[j::4], p) for j in range(4)]
    return [(x + sums[i % 4]) % p for i, x in enumerate(out)]


def internal_linear(s, diag, p):
    tot = _sum(s, p)
    return [(x * d % p + tot) % p for x, d in zip(s, diag)]


class _Free:
    """Walks the permutation computing every column."""

    def __init__(self, override=None):
        self.cols, self.override, self.asserted = [], override, []

    def input(self, i, v=None):
        return self.column(v)

    def column(self, v):
        if self.override is not None and self.override[0] == len(self.cols):
            v = v - v + self.override[1]
        self.cols.append(v)
        return v


class _Given:
    """Walks the permutation over given columns, recording computed - committed of every column."""

    def __init__(self, cols):
        self.cols, self.k, self.asserted, self.p = cols, 0, [], None

    def column(self, v):
        c = self.cols[self.k]
        self.k += 1
        self.asserted.append((v + (self.p - c)) % self.p)
        return c


def _walk(field, width, inputs, w):
    """p3_poseidon2_air's eval: the external layer on the inputs; four full rounds (constants, S-box through its register,
    external layer, the post-state is a committed column and the state continues FROM it); the partial rounds (constant
    and S-box on element 0, its post-S-box value committed, internal layer); four full rounds.  Column order: per full
    round [width S-box registers] [width post], per partial round [register] [post-S-box]."""
    p = field_ref.PARAMS[field]["p"]
    rc, diag = perm_constants(field, width)
    regs = SBOX_REGISTERS[field]

    def sbox(x):
        x3 = x * x % p * x % p
        if regs:
            x3 = w.column(x3)          # assert committed x^3 = x^3, then x^7 = (x^3)^2 x
            return x3 * x3 % p * x % p
        return x3

    s, k = external_linear(list(inputs), p), 0

    def full(s, k):
        s = [sbox((x + rc[k + i]) % p) for i, x in enumerate(s)]
        s = external_linear(s, p)
        return [w.column(x) for x in s], k + width

    for _ in range(HALF_FULL):
        s, k = full(s, k)
    for _ in range(PARTIAL_ROUNDS[(field, width)]):
        s[0] = w.column(sbox((s[0] + rc[k]) % p))
        k += 1
        s = internal_linear(s, diag, p)
    for _ in range(HALF_FULL):
        s, k = full(s, k)
    return s


def perm_num_cols(field, width):
    r = SBOX_REGISTERS[field]
    return width + 2 * HALF_FULL * (width * r + width) + PARTIAL_ROUNDS[(field, width)] * (r + 1)


def perm_columns(field, width, inputs, override=None):
    """All permutation columns of a row whose input limbs are `inputs`.  override = (column, value): that column holds
    `value` instead of what the permutation gives, and every later column follows from it - the row then breaks exactly
    the one link that ends in that column (column < width: an input, nothing breaks)."""
    inputs = list(inputs)
    if override is not None and override[0] < width:
        inputs[override[0]] = inputs[override[0]] - inputs[override[0]] + override[1]
        override = None
    w = _Free(override)
    w.cols = list(inputs)
    _walk(field, width, inputs, w)
    assert len(w.cols) == perm_num_cols(field, width)
    return w.cols


def permute(field, width, state):
    return _walk(field, width, [int(x) for x in state], _Free())


def _perm_constraints(field, width, L):
    w = _Given([L(c) for c in range(width, perm_num_cols(field, width))])
    w.p = field_ref.PARAMS[field]["p"]
    _walk(field, width, [L(c) for c in range(width)], w)
    return w.asserted


# ------------------------------------------------------------------ descriptors and widths
def make_desc(kind, field, lanes=1, horner_packed_steps=2, coeff_lookups=0, ext_degree=4):
    return dict(kind=kind, field=field, lanes=lanes, horner_packed_steps=horner_packed_steps, coeff_lookups=coeff_lookups,
                ext_degree=ext_degree)


def _ext(desc):
    return field_ref.quartic(desc["field"]) if desc["ext_degree"] == 4 else field_ref.quintic(desc["field"])


def widths(desc):
    """(main width, preprocessed width)."""
    k, D, lanes, f = desc["kind"], desc["ext_degree"], desc["lanes"], desc["field"]
    if k in ("const", "public"):
        return lanes * D, lanes * 2                                    # column_layout.rs:22-29
    if k == "recompose":
        return lanes * D, lanes * (2 + (2 * D if desc["coeff_lookups"] else 0))   # recompose_air.rs:156-182
    if k == "alu":                                                     # alu_air.rs:872-879, alu_columns.rs:48-76
        K = desc["horner_packed_steps"]
        return lanes * 4 * D + ((K - 1) // 2 + 2 * (K - 1) + 1) * D, lanes * 13 + 7 * (K - 1)
    if k == "poseidon2":
        if D == 4:
            return perm_num_cols(f, 16) + 2, 4 * 4 + 2 * 2 + 4         # preprocessed.rs:104-108
        return perm_num_cols(f, 16) + 2, 8 + 2 + 8 + 8 + 16 + 8 + 8 + 4   # preprocessed.rs:127-141
    if k == "poseidon2_w32":
        return perm_num_cols(f, 32) + 4, 8 * 4 + 6 * 2 + 4
    raise ValueError(k)


def num_constraints(desc):
    """The length of the constraint list: counted by evaluating the statement once on an all-zero row."""
    w, pw = widths(desc)
    zero = lambda c: 0
    return len(eval_cases(desc, zero, zero, zero, zero, 0))


# ------------------------------------------------------------------ the statements over (local, next) cases
def _alu_constraints(desc, L, N, PL, PN):
    """alu_air.rs:811-994."""
    p, E, D = field_ref.PARAMS[desc["field"]]["p"], _ext(desc), desc["ext_degree"]
    lanes, K = desc["lanes"], desc["horner_packed_steps"]
    sub = lambda a, b: (a + (p - b)) % p
    vec = lambda X, c: [X(c + i) for i in range(D)]
    out = []
    extra_main, extra_prep, num_int = lanes * 4 * D, lanes * 13, (K - 1) // 2      # :872-875
    ac_base = extra_main + num_int * D                                             # :900
    b_sq_base = ac_base + 2 * (K - 1) * D                                          # :901
    for lane in range(lanes):
        m, q = lane * 4 * D, lane * 13
        a, b, c, o = vec(L, m), vec(L, m + D), vec(L, m + 2 * D), vec(L, m + 3 * D)
        mult_a, sel_add, sel_bool, sel_muladd, sel_horner = (PL(q + i) for i in range(5))   # alu_columns.rs:10-15
        active = (p - mult_a) % p                                                  # :836
        sel_mul = sub(sub(sub(sub(active, sel_bool), sel_muladd), sel_horner), sel_add)     # :837
        for i in range(D):                                                         # :840-842 add
            out.append(sel_add * sub((a[i] + b[i]) % p, o[i]) % p)
        ab = E.mul(a, b)
        for i in range(D):                                                         # :845-848 mul
            out.append(sel_mul * sub(ab[i], o[i]) % p)
        out.append(sel_bool * a[0] % p * sub(a[0], a[0] - a[0] + 1) % p)           # :852 bool
        for i in range(1, D):                                                      # :853-855
            out.append(sel_bool * a[i] % p)
        for i in range(D):                                                         # :858-860 mul-add
            out.append(sel_muladd * sub((ab[i] + c[i]) % p, o[i]) % p)
        next_sel_horner = PN(q + 4)                                                # :863
        na, nb, nc, no = vec(N, m), vec(N, m + D), vec(N, m + 2 * D), vec(N, m + 3 * D)
        out_next_b = E.mul(o, nb)                                                  # :870
        single = [sub(sub((out_next_b[i] + nc[i]) % p, na[i]), no[i]) for i in range(D)]
        if lane == 0:                                                              # :881
            next_int0 = vec(N, extra_main)
            any_cur, any_next, ge3_next = mult_a - mult_a, mult_a - mult_a, mult_a - mult_a
            for kk in range(2, K + 1):                                             # :884-892
                any_cur = (any_cur + PL(extra_prep + kk - 2)) % p
                any_next = (any_next + PN(extra_prep + kk - 2)) % p
            next_sel_k2 = PN(extra_prep)                                           # :894
            for kk in range(3, K + 1):                                             # :895-898
                ge3_next = (ge3_next + PN(extra_prep + kk - 2)) % p
            b_sq, b_sq_next = vec(L, b_sq_base), vec(N, b_sq_base)
            bb = E.mul(b, b)
            for i in range(D):                                                     # :905-907 b^2 column
                out.append(any_cur * sub(b_sq[i], bb[i]) % p)
            out_b_sq, c0b, a0b = E.mul(o, b_sq_next), E.mul(nc, nb), E.mul(na, nb)   # :909-911
            a1n, c1n = vec(N, ac_base), vec(N, ac_base + D)                        # :913-916
            for i in range(D):                                                     # :919-925 packed inter-row
                poly = sub((sub((out_b_sq[i] + c0b[i]) % p, a0b[i]) + c1n[i]) % p, a1n[i])
                out.append(next_sel_k2 * sub(poly, no[i]) % p)
                out.append(ge3_next * sub(poly, next_int0[i]) % p)
            next_sel_single = sub(next_sel_horner, any_next)                       # :928
            for i in range(D):                                                     # :929-934
                out.append(next_sel_single * single[i] % p)
            for kk in range(3, K + 1):                                             # :937-985 intra-row legs
                sel_kk = PL(extra_prep + kk - 2)
                s, slot = 2, 0
                while s < kk:
                    int_curr = vec(L, extra_main + slot * D)
                    off_s = ac_base + 2 * (s - 1) * D
                    a_s, c_s = vec(L, off_s), vec(L, off_s + D)
                    if s + 1 < kk:
                        off1 = ac_base + 2 * s * D
                        a_s1, c_s1 = vec(L, off1), vec(L, off1 + D)
                        ib2, csb, asb = E.mul(int_curr, b_sq), E.mul(c_s, b), E.mul(a_s, b)
                        if s + 2 >= kk:
                            target = o                                             # :956-962
                        else:
                            target = vec(L, extra_main + (slot + 1) * D)           # :963-973
                            slot += 1
                        for i in range(D):
                            prod = sub((sub((ib2[i] + csb[i]) % p, asb[i]) + c_s1[i]) % p, a_s1[i])
                            out.append(sel_kk * sub(prod, target[i]) % p)
                        s += 2
                    else:                                                          # :975-983
                        ib = E.mul(int_curr, b)
                        for i in range(D):
                            out.append(sel_kk * sub(sub((ib[i] + c_s[i]) % p, a_s[i]), o[i]) % p)
                        s += 1
        else:                                                                      # :986-993
            for i in range(D):
                out.append(next_sel_horner * single[i] % p)
    return out


def _alu_interactions(desc, L, PL, PN):
    """alu_air.rs:1013-1084."""
    p, D, lanes, K = field_ref.PARAMS[desc["field"]]["p"], desc["ext_degree"], desc["lanes"], desc["horner_packed_steps"]
    out = []
    for lane in range(lanes):
        m, q = lane * 4 * D, lane * 13
        mult_a, a_rd, c_rd = PL(q), PL(q + 11), PL(q + 12)                          # alu_columns.rs:10-23
        mults = [mult_a * a_rd % p, PL(q + 9), mult_a * c_rd % p, PL(q + 10)]       # :1028-1031
        for i in range(4):                                                         # :1041-1052
            out.append((mults[i], [PL(q + 5 + i)] + [L(m + i * D + j) for j in range(D)]))
    extra_main, extra_prep = lanes * 4 * D, lanes * 13
    ac_base = extra_main + ((K - 1) // 2) * D
    for t in range(1, K):                                                          # :1062-1084
        q = extra_prep + (K - 1) + 6 * (t - 1)                                     # alu_columns.rs:67-69
        off = ac_base + 2 * (t - 1) * D
        out.append((PL(q + 4), [PL(q)] + [L(off + j) for j in range(D)]))
        out.append((PL(q + 5), [PL(q + 1)] + [L(off + D + j) for j in range(D)]))
    return out


def _p2_constraints(desc, L, N, PL, PN, trans):
    """poseidon2-circuit-air/src/air.rs:921-1158, the non-compact branch (:1030-1123) for D = 4 and the compact-D1 one
    (:939-1029) for D = 5."""
    f = desc["field"]
    p = field_ref.PARAMS[f]["p"]
    sub = lambda a, b: (a + (p - b)) % p
    pc = perm_num_cols(f, 16)
    oc = pc - 16                                  # ending_full_rounds[3].post (:922)
    bit, isum, nbit, nisum = L(pc), L(pc + 1), N(pc), N(pc + 1)
    one = bit - bit + 1
    out = [bit * sub(bit, one) % p]               # :937
    is_left = sub(one, nbit)
    if desc["ext_degree"] == 4:
        for limb in range(4):                     # :1049-1057 sponge chaining; input limb = (idx, in_ctl, normal, merkle)
            for d in range(4):
                out.append(trans * PN(limb * 4 + 2) % p * sub(N(limb * 4 + d), L(oc + limb * 4 + d)) % p)
        for i in range(2):                        # :1064-1072 Merkle, left
            gate = PN(i * 4 + 3) * is_left % p
            for d in range(4):
                out.append(trans * gate % p * sub(N(i * 4 + d), L(oc + i * 4 + d)) % p)
        for i in range(2):                        # :1073-1081 Merkle, right
            gate = PN(i * 4 + 3) * nbit % p
            for d in range(4):
                out.append(trans * gate % p * sub(N((2 + i) * 4 + d), L(oc + i * 4 + d)) % p)
        not_ns, merkle = sub(one, PN(22)), PN(23)                                  # :1105, preprocessed.rs:160-200
    else:
        hdr, tail = 8 + 2 + 8 + 8, 8 + 2 + 8 + 8 + 16 + 8 + 8                       # :940,:949
        cap_chain, cap_tag = PN(9), PN(8)                                          # :946,:968
        next_ns, next_merkle = PN(tail + 2), PN(tail + 3)
        not_merkle = sub(one, next_merkle)
        for limb in range(8):                                                      # :955-963
            out.append(trans * PN(10 + limb) % p * sub(N(limb), L(oc + limb)) % p)
        for limb in range(8, 16):                                                  # :969-982
            gate = cap_chain * not_merkle % p
            v = sub(N(limb), L(oc + limb))
            if limb == 8:
                v = sub(v, cap_tag)
            out.append(trans * gate % p * v % p)
        for i in range(8):                                                         # :986-1002
            sel = PN(18 + i)
            out.append(trans * (sel * is_left % p) % p * sub(N(i), L(oc + i)) % p)
            out.append(trans * (sel * nbit % p) % p * sub(N(8 + i), L(oc + i)) % p)
        for slot in range(8, 16):                                                  # :1007-1020
            v = sub(N(slot), cap_tag) if slot == 8 else N(slot)
            out.append(trans * next_ns % p * not_merkle % p * v % p)
        not_ns, merkle = sub(one, next_ns), next_merkle
    out.append(trans * not_ns % p * merkle % p * sub(nisum, (isum * 2 + nbit) % p) % p)   # :1116-1122 / :1022-1028
    return out + _perm_constraints(f, 16, L)                                       # :1137-1158


def _p2_interactions(desc, L, PL, PN):
    """air.rs:1721-1788 (compact-D1) and :1790-1893 (D = 4, arity 2)."""
    f, D = desc["field"], desc["ext_degree"]
    p = field_ref.PARAMS[f]["p"]
    pc = perm_num_cols(f, 16)
    oc = pc - 16
    zero = L(0) - L(0)
    neg = lambda a: (p - a) % p
    out = []
    if D == 4:
        not_merkle = (zero + 1 + (p - PL(23))) % p                                 # :1796
        for limb in range(4):                                                      # :1798-1823
            out.append((neg(PL(limb * 4 + 1) * not_merkle % p), [PL(limb * 4)] + [L(limb * 4 + d) for d in range(4)]))
        for limb in range(2):                                                      # :1826-1846
            out.append((PL(16 + 2 * limb + 1), [PL(16 + 2 * limb)] + [L(oc + limb * 4 + d) for d in range(4)]))
        out.append((neg(PL(21) * PN(22) % p), [PL(20), L(pc + 1), zero, zero, zero]))   # :1878-1893
    else:
        hdr, tail = 26, 58
        not_merkle = (zero + 1 + (p - PL(tail + 3))) % p                           # :1727-1728
        pad = [zero] * (D - 1)
        for limb in range(8):                                                      # :1732-1752
            out.append((neg(PL(limb) * not_merkle % p), [PL(hdr + limb), L(limb)] + pad))
        for limb in range(8):                                                      # :1755-1772
            out.append((PL(hdr + 24 + limb), [PL(hdr + 16 + limb), L(oc + limb)] + pad))
        out.append((neg(PL(tail + 1) * PN(tail + 2) % p), [PL(tail), L(pc + 1)] + pad))   # :1775-1788
    return out


def _p2w_constraints(desc, L, N, PL, PN, trans):
    """eval_arity4, air.rs:1236-1341.  Row: [Poseidon2Cols<32> | mmcs_bit | bit2 | bit x bit2 | mmcs_index_sum]
    (poseidon-circuit-cols/src/cols.rs:35-113)."""
    f = desc["field"]
    p = field_ref.PARAMS[f]["p"]
    sub = lambda a, b: (a + (p - b)) % p
    pc = perm_num_cols(f, 32)
    oc = pc - 32
    bit, bit2, bxb, isum = L(pc), L(pc + 1), L(pc + 2), L(pc + 3)
    nbit, nbit2, nbxb, nisum = N(pc), N(pc + 1), N(pc + 2), N(pc + 3)
    one = bit - bit + 1
    out = [bit * sub(bit, one) % p, bit2 * sub(bit2, one) % p, sub(bxb, bit * bit2 % p)]   # :1243-1251
    for limb in range(8):                                                          # :1259-1267
        for d in range(4):
            out.append(trans * PN(limb * 4 + 2) % p * sub(N(limb * 4 + d), L(oc + limb * 4 + d)) % p)
    h = [(sub(sub(one, nbit), nbit2) + nbxb) % p, sub(nbit, nbxb), sub(nbit2, nbxb), nbxb]   # :1274-1278
    for chunk in range(4):                                                         # :1289-1302, CAPACITY_EXT = 2
        for slot in range(2):
            g = chunk * 2 + slot
            gate = PN(g * 4 + 3) * h[chunk] % p
            for d in range(4):
                out.append(trans * gate % p * sub(N(g * 4 + d), L(oc + slot * 4 + d)) % p)
    tail = 8 * 4 + 6 * 2
    acc = (isum * 4 + nbit + 2 * nbit2) % p                                        # :1306-1316
    out.append(trans * sub(one, PN(tail + 2)) % p * PN(tail + 3) % p * sub(nisum, acc) % p)
    return out + _perm_constraints(f, 32, L)                                       # :1320-1341


def _p2w_interactions(desc, L, PL, PN):
    """air.rs:1790-1876 with is_arity4."""
    f = desc["field"]
    p = field_ref.PARAMS[f]["p"]
    pc = perm_num_cols(f, 32)
    oc = pc - 32
    zero = L(0) - L(0)
    neg = lambda a: (p - a) % p
    out = []
    for limb in range(8):                                                          # :1798-1823, bare in_ctl
        out.append((neg(PL(limb * 4 + 1)), [PL(limb * 4)] + [L(limb * 4 + d) for d in range(4)]))
    for limb in range(6):                                                          # :1826-1846
        out.append((PL(32 + 2 * limb + 1), [PL(32 + 2 * limb)] + [L(oc + limb * 4 + d) for d in range(4)]))
    merkle = PL(47)
    out.append((neg(merkle), [PL(44), L(pc), zero, zero, zero]))                   # :1858-1868
    out.append((neg(merkle), [PL(45), L(pc + 1), zero, zero, zero]))               # :1870-1876
    return out


def _send_interactions(desc, L, PL, PN):
    """public_air.rs:212-228 (Const and Public): prep lane (multiplicity, witness_idx) (column_layout.rs:22-29)."""
    D = desc["ext_degree"]
    return [(PL(2 * lane), [PL(2 * lane + 1)] + [L(lane * D + j) for j in range(D)]) for lane in range(desc["lanes"])]


def _recompose_interactions(desc, L, PL, PN):
    """recompose_air.rs:159-197: prep lane (output_idx, out_mult) then D x (coeff_idx, coeff_mult)."""
    D = desc["ext_degree"]
    plw = 2 + (2 * D if desc["coeff_lookups"] else 0)
    zero = L(0) - L(0)
    out = []
    for lane in range(desc["lanes"]):
        q = lane * plw
        out.append((PL(q + 1), [PL(q)] + [L(lane * D + j) for j in range(D)]))     # :163-173
        if desc["coeff_lookups"]:
            for i in range(D):                                                     # :178-195
                out.append((PL(q + 2 + 2 * i + 1), [PL(q + 2 + 2 * i), L(lane * D + i)] + [zero] * (D - 1)))
    return out


def eval_cases(desc, L, N, PL, PN, trans):
    """Constraint values over cases: L / N / PL / PN map a column number to that column of the local / next main and
    preprocessed rows (ints, or uint64 arrays with one entry per case), trans is is_transition."""
    k = desc["kind"]
    if k == "alu":
        return _alu_constraints(desc, L, N, PL, PN)
    if k == "poseidon2":
        return _p2_constraints(desc, L, N, PL, PN, trans)
    if k == "poseidon2_w32":
        return _p2w_constraints(desc, L, N, PL, PN, trans)
    return []          # Const, Public, Recompose: interactions only


def interaction_cases(desc, L, PL, PN):
    return {"alu": _alu_interactions, "poseidon2": _p2_interactions, "poseidon2_w32": _p2w_interactions,
            "const": _send_interactions, "public": _send_interactions, "recompose": _recompose_interactions}[desc["kind"]](
                desc, L, PL, PN)


# ------------------------------------------------------------------ the interface on whole matrices
def _row(m, r):
    return lambda c: int(m[r, c])


def constraints(desc, prep, main, r):
    h = main.shape[0]
    n = (r + 1) % h
    out = eval_cases(desc, _row(main, r), _row(main, n), _row(prep, r), _row(prep, n), int(r != h - 1))
    assert len(out) == num_constraints(desc)
    return out


def interactions(desc, prep, main, r):
    n = (r + 1) % main.shape[0]
    return [(int(m), tuple(int(x) for x in t)) for m, t in interaction_cases(desc, _row(main, r), _row(prep, r), _row(prep, n))]


def _cols(m, rows):
    a = np.ascontiguousarray(m[rows].T.astype(np.uint64))
    return lambda c: a[c]


def constraint_matrix(desc, prep, main):
    """(constraints, rows) uint64: every constraint on every row (the wrap row included)."""
    h = main.shape[0]
    cur, nxt = np.arange(h), (np.arange(h) + 1) % h
    trans = (cur != h - 1).astype(np.uint64)
    out = eval_cases(desc, _cols(main, cur), _cols(main, nxt), _cols(prep, cur), _cols(prep, nxt), trans)
    return np.array(out, dtype=np.uint64).reshape(len(out), h)


def failing(desc, prep, main):
    m = constraint_matrix(desc, prep, main)
    return set(int(i) for i in np.flatnonzero(m.any(axis=1)))


def bus_multiset(desc, prep, main, rows=None, acc=None):
    """tuple -> multiplicity mod p, over `rows` (all by default); zero entries dropped."""
    p = field_ref.PARAMS[desc["field"]]["p"]
    acc = {} if acc is None else acc
    for r in (range(main.shape[0]) if rows is None else rows):
        for m, t in interactions(desc, prep, main, r):
            if m:
                acc[t] = (acc.get(t, 0) + m) % p
    return {t: m for t, m in acc.items() if m}


def bus_balance(tables):
    acc = {}
    for desc, prep, main in tables:
        acc = bus_multiset(desc, prep, main, acc=acc)
    return not acc
