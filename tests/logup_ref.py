"""Reference for the lookup programs of the LogUp seam (include/p3r.h: p3r_logup_program_dmat), on Python integers over
tests/field_ref.py.  The values of a program are those of air_ref._run, evaluated on the rows of the traces themselves
(natural order, the next row (r + 1) mod h); the sinks are written from the header's definitions: every term is its own
division m / d through d^(p^DC - 2) - no fraction is ever combined with another before it is inverted, unlike the kernel -
the fractions of a column are added, the running sum is the exclusive prefix over the rows and the table's sum the total.

  logup_trace   the (h, DC * (1 + G)) auxiliary trace and the table's sum of a lookup program
  zero_rows     the rows in which a denominator of the program vanishes (none of them has a defined fraction)"""
import numpy as np

import air_ref
import field_ref

LOOKUP, LOOKUP_END = 21, 22


def _terms(field, dc, prog, mats, publics, challenges):
    """[(column, multiplicity, denominator)] in program order, each an extension value over all rows, and the number of
    closed columns."""
    E = air_ref.ext_of(field, dc)
    U, h = np.uint64, mats[0].shape[0]
    assert all(m.shape[0] == h for m in mats)
    cur = np.arange(h, dtype=np.int64)
    nxt = (cur + 1) % h
    zero = np.zeros(h, dtype=U)
    cols = [m.astype(U) for m in mats]

    def leaf(op, a, b):
        if op == air_ref.CONST:
            return (False, zero + U(a))
        if op == air_ref.PUBLIC:
            return (False, zero + U(int(publics[a])))
        if op == air_ref.CHALLENGE:
            return (True, [zero + U(int(challenges[a][k])) for k in range(dc)])
        if op in (air_ref.LOCAL, air_ref.NEXT):
            return (False, cols[a][cur if op == air_ref.LOCAL else nxt, b])
        if op in (air_ref.LOCAL_EXT, air_ref.NEXT_EXT):
            rows = cur if op == air_ref.LOCAL_EXT else nxt
            return (True, [cols[a][rows, b + k] for k in range(dc)])
        raise ValueError("op %d has no value in a lookup program" % op)

    # air_ref._run knows one sink, ASSERT_ZERO of one value: the multiplicities and the denominators are collected by a
    # walk each, with every LOOKUP asserting the operand in question and every LOOKUP_END an unused constant
    prog = [(int(op), int(a), int(b)) for op, a, b in prog]
    sides = []
    for side in (1, 2):
        shadow = [(air_ref.ASSERT_ZERO, ins[side], 0) if ins[0] == LOOKUP else (air_ref.CONST, 0, 0) if ins[0] == LOOKUP_END else ins
                  for ins in prog]
        sides.append([air_ref._lift(E, v) for v in air_ref._run(shadow, E, leaf)])
    column, terms = 0, []
    for op, _, _ in prog:
        if op == LOOKUP:
            terms.append((column, sides[0][len(terms)], sides[1][len(terms)]))
        elif op == LOOKUP_END:
            column += 1
    return terms, column


def zero_rows(field, dc, prog, mats, publics=(), challenges=()):
    """Sorted rows in which the denominator of some term is zero."""
    terms, _ = _terms(field, dc, prog, mats, publics, challenges)
    bad = np.zeros(mats[0].shape[0], dtype=bool)
    for _, _, d in terms:
        bad |= ~np.any(np.stack(d) != 0, axis=0)
    return [int(r) for r in np.nonzero(bad)[0]]


def logup_trace(field, dc, prog, mats, publics=(), challenges=()):
    """mats: the traces as 2-D uint32 arrays of one height h.  Returns (aux, table_sum): aux is (h, dc * (1 + G)) uint32,
    columns [0, dc) the running sum s (s[0] = 0, s[r + 1] = s[r] + sum_g f_g[r]), columns [dc * (1 + g), dc * (2 + g)) the
    fractions f_g; table_sum the dc ints of s[h - 1] + sum_g f_g[h - 1]."""
    E = air_ref.ext_of(field, dc)
    p, h = E.p, mats[0].shape[0]
    terms, n_columns = _terms(field, dc, prog, mats, publics, challenges)
    zero = np.zeros(h, dtype=np.uint64)
    fracs = [E.zero(zero) for _ in range(n_columns)]
    for g, m, d in terms:
        fracs[g] = E.add(fracs[g], E.mul(m, E.inv(d)))
    row_total = E.zero(zero)
    for f in fracs:
        row_total = E.add(row_total, f)
    aux = np.zeros((h, dc * (1 + n_columns)), dtype=np.uint32)
    table_sum = []
    for k in range(dc):
        inclusive = np.cumsum(row_total[k], dtype=np.uint64) % np.uint64(p)   # h values below 2^31: no wrap below 2^33 rows
        aux[1:, k] = inclusive[:-1]
        table_sum.append(int(inclusive[-1]))
        for g, f in enumerate(fracs):
            aux[:, dc * (1 + g) + k] = f[k]
    return aux, table_sum
