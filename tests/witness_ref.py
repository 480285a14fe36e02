"""Reference for the witness seam (include/p3r.h: p3r_witness_program_dmat), on integers over tests/field_ref.py: an
interpreter of witness programs written from the header's definitions, and the only source of expected values of the
witness tests.  Values are canonical residues, one numpy uint64 entry per row (field_ref's expressions take such arrays
as they take Python integers); an extension value is a list of dc such arrays.

  columns   the h x W matrix a witness program stores over host traces
  info      n_stores, n_out_columns, n_inversions of a program"""
import numpy as np

import field_ref

CONST, PUBLIC, CHALLENGE, LOCAL, NEXT, LOCAL_EXT, NEXT_EXT = 0, 1, 8, 9, 10, 11, 12
IS_FIRST_ROW, IS_LAST_ROW, IS_TRANSITION, ADD, SUB, MUL, NEG = 13, 14, 15, 16, 17, 18, 19
INV, BITS, ROW, STORE = 23, 24, 25, 26


def ext_of(field, dc):
    return field_ref.quartic(field) if dc == 4 else field_ref.quintic(field)


def kinds(prog):
    """Per instruction: True for an extension value, False for a base value, None for a STORE."""
    out = []
    for op, a, b in np.asarray(prog).reshape(-1, 3).tolist():
        if op == STORE:
            out.append(None)
        elif op in (ADD, SUB, MUL):
            out.append(bool(out[a] or out[b]))
        elif op in (NEG, INV):
            out.append(out[a])
        else:
            out.append(op in (CHALLENGE, LOCAL_EXT, NEXT_EXT))
    return out


def values(field, dc, prog, mats, height=None, publics=(), challenges=()):
    """Walks the program over the rows of the traces `mats` (2-D arrays of one height h, natural order; none: `height`
    rows).  Returns (h, vals, stores): vals[i] = (is_ext, value) of instruction i, or None for a STORE; stores = the
    (value id, first output column) pairs in program order."""
    U = np.uint64
    E, p = ext_of(field, dc), field_ref.PARAMS[field]["p"]
    h = mats[0].shape[0] if len(mats) else int(height)
    assert h >= 1 and h & (h - 1) == 0 and all(m.shape[0] == h for m in mats) and (height is None or len(mats) == 0 or int(height) in (0, h))
    cur = np.arange(h, dtype=np.int64)
    nxt = (cur + 1) % h
    zero = np.zeros(h, dtype=U)
    cols = [np.asarray(m).astype(U) for m in mats]

    def lift(v):
        return v[1] if v[0] else [v[1]] + [zero] * (dc - 1)

    vals, stores = [], []
    for i, (op, a, b) in enumerate(np.asarray(prog).reshape(-1, 3).tolist()):
        if op == CONST:
            assert a < p
            v = (False, zero + U(a))
        elif op == PUBLIC:
            v = (False, zero + U(int(publics[a])))
        elif op == CHALLENGE:
            v = (True, [zero + U(int(challenges[a][k])) for k in range(dc)])
        elif op in (LOCAL, NEXT):
            v = (False, cols[a][cur if op == LOCAL else nxt, b])
        elif op in (LOCAL_EXT, NEXT_EXT):
            rows = cur if op == LOCAL_EXT else nxt
            v = (True, [cols[a][rows, b + k] for k in range(dc)])
        elif op == IS_FIRST_ROW:
            v = (False, (cur == 0).astype(U))
        elif op == IS_LAST_ROW:
            v = (False, (cur == h - 1).astype(U))
        elif op == IS_TRANSITION:
            v = (False, (cur != h - 1).astype(U))
        elif op in (ADD, SUB, MUL):
            assert a < i and b < i and vals[a] is not None and vals[b] is not None
            x, y = vals[a], vals[b]
            if x[0] or y[0]:
                f = {ADD: E.add, SUB: E.sub, MUL: E.mul}[op]
                v = (True, f(lift(x), lift(y)))
            else:
                f = {ADD: field_ref.add, SUB: field_ref.sub, MUL: field_ref.mul}[op]
                v = (False, f(x[1], y[1], p))
        elif op == NEG:
            assert a < i and vals[a] is not None
            x = vals[a]
            v = (True, E.neg(x[1])) if x[0] else (False, field_ref.neg(x[1], p))
        elif op == INV:   # a^(p^d - 2), a^(p - 2): zero maps to zero
            assert a < i and vals[a] is not None
            x = vals[a]
            v = (True, E.inv(x[1])) if x[0] else (False, field_ref.inv(x[1], p))
        elif op == BITS:
            lo, n = b & 0xFF, b >> 8
            assert a < i and vals[a] is not None and not vals[a][0] and n >= 1 and lo + n <= 31
            v = (False, (vals[a][1] >> U(lo)) & U((1 << n) - 1))
        elif op == ROW:
            v = (False, cur.astype(U))
        elif op == STORE:
            assert a < i and vals[a] is not None
            stores.append((a, b))
            v = None
        else:
            raise ValueError("op %d is no op of a witness program" % op)
        vals.append(v)
    return h, vals, stores


def columns(field, dc, prog, mats, height=None, publics=(), challenges=()):
    """The (h, W) uint32 matrix of canonical words the program stores: W is one past the highest stored column, and every
    column below it is stored exactly once (asserted)."""
    h, vals, stores = values(field, dc, prog, mats, height, publics, challenges)
    placed = {}
    for a, b in stores:
        is_ext, v = vals[a]
        for k, c in enumerate(v if is_ext else [v]):
            assert b + k not in placed, "output column %d is stored twice" % (b + k)
            placed[b + k] = c
    W = max(placed) + 1
    assert sorted(placed) == list(range(W)), "a column below W is not stored"
    return np.stack([placed[c] for c in range(W)], axis=1).astype(np.uint32)


def info(field, dc, prog, widths):
    """n_stores, n_out_columns and n_inversions of p3r_witness_program_info (peak_live is the planner's own)."""
    mats = [np.zeros((1, w), dtype=np.uint32) for w in widths]
    prog = np.asarray(prog).reshape(-1, 3)
    n_pub = 1 + max([int(a) for op, a, b in prog.tolist() if op == PUBLIC], default=0)
    n_ch = 1 + max([int(a) for op, a, b in prog.tolist() if op == CHALLENGE], default=0)
    out = columns(field, dc, prog, mats, 1, [0] * n_pub, [[0] * dc] * n_ch)
    return {"n_stores": int(np.count_nonzero(prog[:, 0] == STORE)), "n_out_columns": out.shape[1],
            "n_inversions": int(np.count_nonzero(prog[:, 0] == INV))}
