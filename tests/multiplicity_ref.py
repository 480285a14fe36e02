"""Reference for the multiplicity join (include/p3r.h: p3r_lookup_multiplicities_dmat), on Python integers and
dictionaries.  The values of the lookup programs are those logup_ref._terms evaluates for the LogUp reference and
check_ref.lookup_balance for the lookup check; what is the join's own is written from the header's rules, literally:

  - the key of a slot is the tuple of the dc canonical words of its denominator;
  - a table slot (row, term) offers its key when its multiplicity value is not zero, and the FIRST offering slot of a key
    in (row, term) order owns it;
  - a query term whose multiplicity is not zero is a record (key, m), m a base value: word 0, the other words zero;
  - the owner's cell holds the sum of m modulo p over the records of its key, every other cell 0;
  - a key that has records, no owner and a non-zero sum is missing; the misses are ordered by their first record."""
import numpy as np

import air_ref
import logup_ref


def _slots(field, dc, prog, mats, publics, challenges):
    """(h, terms, dc) integer arrays of the multiplicities and the denominators of a lookup program over its traces."""
    terms, _ = logup_ref._terms(field, dc, prog, mats, publics, challenges)
    m = np.stack([np.stack(t[1], axis=1) for t in terms], axis=1)
    d = np.stack([np.stack(t[2], axis=1) for t in terms], axis=1)
    assert m.shape == d.shape == (mats[0].shape[0], len(terms), dc)
    return m, d


def multiplicities(field, dc, table, queries, challenges=()):
    """table, queries[i]: (program as (op, a, b) rows, [host matrices], public values).  Returns (column, n_missing,
    entries) as Context.lookup_multiplicities_device does: column an (h_table, n_terms_table) uint32 array, entries the
    dicts of ALL misses in the order of their first records."""
    p = air_ref.ext_of(field, dc).p
    tm, td = _slots(field, dc, *table, challenges)
    h, n_terms = tm.shape[:2]
    owner = {}   # key -> (row, term) of the first offering slot
    for r in range(h):
        for t in range(n_terms):
            if tm[r, t].any():
                owner.setdefault(tuple(int(v) for v in td[r, t]), (r, t))
    asked = {}   # key -> [sum of m, first record (query, row, term), records]; filled in record order
    for q, query in enumerate(queries):
        qm, qd = _slots(field, dc, *query, challenges)
        for r, t in zip(*np.nonzero(qm.any(axis=2))):   # ascending (row, term)
            assert not qm[r, t, 1:].any(), "a query multiplicity must be a base value"
            e = asked.setdefault(tuple(int(v) for v in qd[r, t]), [0, (q, int(r), int(t)), 0])
            e[0] = (e[0] + int(qm[r, t, 0])) % p
            e[2] += 1
    column = np.zeros((h, n_terms), dtype=np.uint32)
    for key, (r, t) in owner.items():
        if key in asked:
            column[r, t] = asked[key][0]
    missing = sorted(((e[1], key, e) for key, e in asked.items() if key not in owner and e[0]), key=lambda x: x[0])
    entries = [{"instance": first[0], "row": first[1], "term": first[2], "n_records": e[2], "denominator": list(key),
                "net": [e[0]] + [0] * (dc - 1)} for first, key, e in missing]
    return column, len(entries), entries
