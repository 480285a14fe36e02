"""Reference for the two trace checks (include/p3r.h: p3r_check_program_dmat, p3r_lookup_check_dmat), on Python integers
over tests/field_ref.py.  The values of a program are those of air_ref._run (and, for lookup programs, logup_ref._terms),
evaluated on the rows of the traces themselves: natural order, the next row (r + 1) mod h.  What is the checks' own is
written from the header's definitions: 0 / 1 selectors by the row, "fails" as any non-zero coefficient, records keyed by
their denominator with the first record of a key kept while a dict is filled in record order.

  check           the report and the two per-constraint arrays of a constraint program over traces
  lookup_balance  the unbalanced keys of lookup programs across tables, by denominator or by a key the caller names"""
import numpy as np

import air_ref
import logup_ref

NONE = 0xFFFFFFFF


def failing_rows(field, dc, prog, mats, publics=(), challenges=()):
    """Per constraint, a bool array over the rows: the asserted value is not zero there."""
    U, h = np.uint64, mats[0].shape[0]
    assert all(m.shape[0] == h for m in mats)
    E = air_ref.ext_of(field, dc)
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
        if op == air_ref.IS_FIRST_ROW:
            return (False, (cur == 0).astype(U))
        if op == air_ref.IS_LAST_ROW:
            return (False, (cur == h - 1).astype(U))
        if op == air_ref.IS_TRANSITION:
            return (False, (cur != h - 1).astype(U))
        raise ValueError("unknown op %d" % op)

    out = []
    for is_ext, v in air_ref._run(prog, E, leaf):
        out.append(np.any(np.stack(v) != 0, axis=0) if is_ext else v != 0)
    return out


def check(field, dc, prog, mats, publics=(), challenges=()):
    """What Context.check_device returns: n_failures, first_row, first_constraint, first_row_of, n_failed_of."""
    fails = failing_rows(field, dc, prog, mats, publics, challenges)
    first_of = np.array([int(np.argmax(f)) if f.any() else NONE for f in fails], dtype=np.uint32)
    n_of = np.array([int(f.sum()) for f in fails], dtype=np.uint64)
    first_row = int(first_of.min())
    first_constraint = NONE if first_row == NONE else int(np.argmax(first_of == first_row))
    return {"n_failures": int(n_of.sum()), "first_row": first_row, "first_constraint": first_constraint,
            "first_row_of": first_of, "n_failed_of": n_of}


def lookup_balance(field, dc, instances, challenges=(), key_of=None):
    """instances: (program as (op, a, b) rows, [host matrices], public values) each.  A record is a term whose
    multiplicity, lifted, is not zero; its key is its denominator's dc words, or key_of(instance, row, term) when the
    caller knows the tuple behind it.  Returns (n_unbalanced, entries): the keys whose multiplicities do not sum to zero,
    ascending by their first record (instance, row, term), each a dict as Context.lookup_check_device returns it - the
    denominator always that of the first record."""
    E = air_ref.ext_of(field, dc)
    p = E.p
    keys = {}   # key -> [net (dc ints), first (instance, row, term), denominator of the first, records]; filled in record order
    for i, (prog, mats, publics) in enumerate(instances):
        terms, _ = logup_ref._terms(field, dc, prog, mats, publics, challenges)
        h = mats[0].shape[0]
        m = np.stack([np.stack(t[1], axis=1) for t in terms], axis=1)   # (h, terms, dc)
        d = np.stack([np.stack(t[2], axis=1) for t in terms], axis=1)
        assert m.shape == d.shape == (h, len(terms), dc)
        for r, t in zip(*np.nonzero(m.any(axis=2))):   # ascending (row, term)
            mult, den = [int(v) for v in m[r, t]], [int(v) for v in d[r, t]]
            k = tuple(den) if key_of is None else key_of(i, int(r), int(t))
            if k not in keys:
                keys[k] = [[0] * dc, (i, int(r), int(t)), den, 0]
            e = keys[k]
            e[0] = [(x + y) % p for x, y in zip(e[0], mult)]
            e[3] += 1
    bad = sorted((e for e in keys.values() if any(e[0])), key=lambda e: e[1])
    return len(bad), [{"instance": e[1][0], "row": e[1][1], "term": e[1][2], "n_records": e[3], "denominator": e[2], "net": e[0]}
                      for e in bad]
