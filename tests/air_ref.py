"""Reference interpreter for the constraint programs of the quotient seam (include/p3r.h: p3r_air_insn), on Python integers
over tests/field_ref.py.  It is written from the header's definitions and shares no code with the library: its own op
numbers, its own bit reversal of rows, its own domain points and selectors, division by the vanishing polynomial through
a^(p-2).

  quotient_chunks   a program over whole columns: the committed (bit-reversed) LDEs in, the 2^q quotient chunks out
  fold_at_point     a program at one out-of-domain point, from opened values: sum_k alpha^(n-1-k) C_k(zeta)

A value is a pair (is_ext, v): v a canonical residue (or a numpy uint64 array of them, one per row) for a base value, a
list of DC such coefficients for an extension value."""
import numpy as np

import field_ref

CONST, PUBLIC, CHALLENGE, LOCAL, NEXT, LOCAL_EXT, NEXT_EXT = 0, 1, 8, 9, 10, 11, 12
IS_FIRST_ROW, IS_LAST_ROW, IS_TRANSITION, ADD, SUB, MUL, NEG, ASSERT_ZERO = 13, 14, 15, 16, 17, 18, 19, 20


def ext_of(field, dc):
    return field_ref.quartic(field) if dc == 4 else field_ref.quintic(field)


def _lift(E, v):
    return v[1] if v[0] else [v[1]] + [v[1] - v[1] for _ in range(E.d - 1)]


def _run(prog, E, leaf):
    """Walks the program; leaf(op, a, b) gives the typed value of a non-arithmetic instruction.  Returns the asserted
    values in program order."""
    p, vals, asserted = E.p, [], []
    for op, a, b in prog:
        op, a, b = int(op), int(a), int(b)
        if op in (ADD, SUB):
            x, y = vals[a], vals[b]
            if x[0] or y[0]:
                v = (True, (E.add if op == ADD else E.sub)(_lift(E, x), _lift(E, y)))
            else:
                v = (False, (field_ref.add if op == ADD else field_ref.sub)(x[1], y[1], p))
        elif op == MUL:
            x, y = vals[a], vals[b]
            if x[0] and y[0]:
                v = (True, E.mul(x[1], y[1]))
            elif x[0] or y[0]:
                e, s = (x, y) if x[0] else (y, x)
                v = (True, E.scale(e[1], s[1]))
            else:
                v = (False, field_ref.mul(x[1], y[1], p))
        elif op == NEG:
            x = vals[a]
            v = (True, E.neg(x[1])) if x[0] else (False, field_ref.neg(x[1], p))
        elif op == ASSERT_ZERO:
            asserted.append(vals[a])
            v = None
        else:
            v = leaf(op, a, b)
        vals.append(v)
    return asserted


def _horner(E, asserted, alpha):
    acc = None
    for c in asserted:
        c = _lift(E, c)
        acc = c if acc is None else E.add(E.mul(acc, alpha), c)
    return acc


def quotient_chunks(field, dc, prog, mats, added_bits, q, shift, publics, challenges, alpha):
    """mats: the committed LDEs as the device holds them (2-D uint32 arrays of one height H = h << added_bits, rows in
    bit-reversed order over shift * <w_H>; shift None = the field's generator).  Returns 2^q arrays (h, dc) uint32: row r of
    chunk c is Q at the natural index r * 2^q + c."""
    f, E = field_ref.PARAMS[field], ext_of(field, dc)
    p, U = f["p"], np.uint64
    shift = f["gen"] if shift is None else shift
    H = mats[0].shape[0]
    h = H >> added_bits
    N, log_n = h << q, (h << q).bit_length() - 1
    cur = np.array([field_ref.bit_reverse(i, log_n) for i in range(N)], dtype=np.int64)
    nxt = np.array([field_ref.bit_reverse((i + (1 << q)) % N, log_n) for i in range(N)], dtype=np.int64)
    w_n, w_h = field_ref.two_adic_generator(field, log_n), field_ref.two_adic_generator(field, h.bit_length() - 1)
    xs, x = [], shift % p
    for _ in range(N):
        xs.append(x)
        x = x * w_n % p
    x = np.array(xs, dtype=U)
    zero = x - x
    zh = field_ref.sub(field_ref.fpow(x, h, p), zero + U(1), p)
    x_m1 = field_ref.sub(x, zero + U(1), p)
    x_mg = field_ref.sub(x, zero + U(field_ref.inv(w_h, p)), p)
    cols = [m.astype(U) for m in mats]

    def leaf(op, a, b):
        if op == CONST:
            return (False, zero + U(a))
        if op == PUBLIC:
            return (False, zero + U(int(publics[a])))
        if op == CHALLENGE:
            return (True, [zero + U(int(challenges[a][k])) for k in range(dc)])
        if op in (LOCAL, NEXT):
            return (False, cols[a][cur if op == LOCAL else nxt, b])
        if op in (LOCAL_EXT, NEXT_EXT):
            rows = cur if op == LOCAL_EXT else nxt
            return (True, [cols[a][rows, b + k] for k in range(dc)])
        if op == IS_FIRST_ROW:
            return (False, field_ref.mul(zh, field_ref.inv(x_m1, p), p))
        if op == IS_LAST_ROW:
            return (False, field_ref.mul(zh, field_ref.inv(x_mg, p), p))
        if op == IS_TRANSITION:
            return (False, x_mg)
        raise ValueError("unknown op %d" % op)

    folded = _horner(E, _run(prog, E, leaf), [zero + U(int(v)) for v in alpha])
    quot = np.stack(E.scale(folded, field_ref.inv(zh, p)), axis=1).astype(np.uint32)   # (N, dc), natural order
    return [quot[c::1 << q] for c in range(1 << q)]


def fold_at_point(field, dc, prog, local, nxt, zeta, h, publics, challenges, alpha):
    """The folded constraints at the point zeta (dc ints): local[m][col] / nxt[m][col] are the opened values of matrix m
    at zeta and zeta * w_h (dc ints each).  Every value is an extension element here."""
    f, E = field_ref.PARAMS[field], ext_of(field, dc)
    p = f["p"]
    zeta = [int(v) for v in zeta]
    one = E.one(0)
    g_inv = field_ref.inv(field_ref.two_adic_generator(field, h.bit_length() - 1), p)
    zh = E.sub(E.pow(zeta, h), one)
    z_m1, z_mg = E.sub(zeta, one), E.sub(zeta, E.scale(one, g_inv))

    def monomial(k):
        return [1 if i == k else 0 for i in range(dc)]

    def cell(rows, a, b):
        return [int(v) for v in rows[a][b]]

    def leaf(op, a, b):
        if op == CONST:
            return (True, E.scale(one, a))
        if op == PUBLIC:
            return (True, E.scale(one, int(publics[a])))
        if op == CHALLENGE:
            return (True, [int(v) for v in challenges[a]])
        if op in (LOCAL, NEXT):
            return (True, cell(local if op == LOCAL else nxt, a, b))
        if op in (LOCAL_EXT, NEXT_EXT):
            rows, acc = (local if op == LOCAL_EXT else nxt), E.zero(0)
            for k in range(dc):   # sum_k col[b + k](zeta) * X^k
                acc = E.add(acc, E.mul(cell(rows, a, b + k), monomial(k)))
            return (True, acc)
        if op == IS_FIRST_ROW:
            return (True, E.mul(zh, E.inv(z_m1)))
        if op == IS_LAST_ROW:
            return (True, E.mul(zh, E.inv(z_mg)))
        if op == IS_TRANSITION:
            return (True, z_mg)
        raise ValueError("unknown op %d" % op)

    return _horner(E, _run(prog, E, leaf), [int(v) for v in alpha])
