"""The recurrence seam (p3r_affine_scan_dmat) in plain Python integers: s[0] = init, s[r + 1] = a[r] * s[r] + b[r], row
after row, in Fp, Fp4 or Fp5 (tests/field_ref.py).  Nothing here knows about tiles, scans or the library.

A recurrence is a dict of the arguments of plonky3_recursion_amd.Recurrence: out_col, mul and add ((matrix, column) or
None), init (a word or a list of words), ext, inclusive."""
import numpy as np

import field_ref


def field_of(field, dc, ext):
    return (field_ref.quartic(field) if dc == 4 else field_ref.quintic(field)) if ext else field_ref.linear(field)


def width(dc, recs):
    return max(r["out_col"] + (dc if r.get("ext") else 1) for r in recs)


def one_column(field, dc, rec, mats):
    """(states, last): the h + 1 states s[0] .. s[h] of one recurrence as lists of d ints; last is s[h]."""
    E = field_of(field, dc, rec.get("ext"))
    d, h = E.d, mats[0].shape[0]
    init = [int(v) for v in np.atleast_1d(rec.get("init", 0))]
    s = init + [0] * (d - len(init))

    def element(src, r):
        return [int(v) for v in mats[src[0]][r, src[1]:src[1] + d]]
    states = [s]
    for r in range(h):
        if rec.get("mul") is not None:
            s = E.mul(element(rec["mul"], r), s)
        if rec.get("add") is not None:
            s = E.add(s, element(rec["add"], r))
        states.append(s)
    return states, states[h]


def columns(field, dc, recs, mats):
    """(the (h, W) uint32 matrix affine_scan_device returns, the (n, 5) uint32 array of s[h] per recurrence)."""
    h = mats[0].shape[0]
    out = np.zeros((h, width(dc, recs)), dtype=np.uint32)
    last = np.zeros((len(recs), 5), dtype=np.uint32)
    for i, rec in enumerate(recs):
        states, total = one_column(field, dc, rec, mats)
        d = len(total)
        first = 1 if rec.get("inclusive") else 0
        out[:, rec["out_col"]:rec["out_col"] + d] = np.array(states[first:first + h], dtype=np.uint32)
        last[i, :d] = total
    return out, last
