"""Times of the multiplicity join on resident KoalaBear traces, DC = 4, beside the lookup check on the same instances.
   python tools/time_lookup_multiplicities.py [--reps 10] [--out FILE]

Two cases, both a single-field range check under the key c - x, which is exact:
  small   a table of 2^16 rows (t = row, every row enabled) against one query of 2^20 rows (v uniform in [0, 2^16),
          multiplicity 1): 2^16 + 2^20 slots, all of them records
  large   a table of 2^20 rows against one query of 2^22 rows (v uniform in [0, 2^20))
For each, p3r_lookup_multiplicities_dmat and p3r_lookup_check_dmat are called on the SAME two instances (table, query), in
the same process, ALTERNATELY: join, check, join, check, ..  The check sees the table's enable flags as multiplicities, so
both passes record, compact, sort and sum the same slots; the check then flags every key as unbalanced and reports 16 of
them, the join zero-fills the column, scatters one sum per key and finds no miss.

Every figure is the median of --reps calls after two warm-up calls of each entry, in ms; call times are a host clock around
calls that end in the device synchronise the entry itself makes; stage times are the library's profile scopes (device
events on the context's stream) from a second set of alternated calls.  No hardware counter is collected.  Nothing here
is a threshold; the output goes to profiles/<round>/."""
import argparse
import os
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P, DC = 0x7F000001, 4
SHIFT = 1000003
JOIN = ["lookup_mult_records", "lookup_mult_sort", "lookup_mult_sums", "lookup_mult_scatter"]
CHECK = ["lookup_check_records", "lookup_check_sort", "lookup_check_sums"]


def alternated(fns, reps, measure):
    """measure(fn) for each fn in turn, `reps` rounds after two warm-up rounds; one list of results per fn."""
    for _ in range(2):
        for fn in fns:
            fn()
    out = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            out[k].append(measure(fn))
    return out


def wall_ms(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import plonky3_recursion_amd as p3r

    ctx = p3r.Context(field="koala-bear")
    rng = np.random.default_rng(19)
    prog = p3r.AirBuilder("koala-bear")
    prog.lookup(1, prog.const(SHIFT) - prog.local(0, 0))
    prog.end_lookup_column()
    lines = ["box: %s, %s; KoalaBear, DC = %d; medians of %d alternated calls after 2 warm-up calls each, ms (min .. max in brackets)"
             % (socket.gethostname(), torch.cuda.get_device_name(0), DC, a.reps)]

    def scoped(fn):
        ctx.profile_enable(True)
        fn()
        got = ctx.profile_read()
        ctx.profile_enable(False)
        return {n: v[0] for n, v in got.items()}

    for name, log_t, log_q in (("small", 16, 20), ("large", 20, 22)):
        ht, hq = 1 << log_t, 1 << log_q
        v = rng.integers(0, ht, size=hq, dtype=np.uint32)
        table = ctx.upload(np.arange(ht, dtype=np.uint32).reshape(ht, 1))
        query = ctx.upload(v.reshape(hq, 1))
        tab, qry = (prog, [table]), (prog, [query])

        def join():
            col, n, _ = ctx.lookup_multiplicities_device(tab, [qry])
            col.free()
            return n

        def check():
            return ctx.lookup_check_device([tab, qry])[0]
        col, n_missing, _ = ctx.lookup_multiplicities_device(tab, [qry])
        assert n_missing == 0 and np.array_equal(col.download()[:, 0], np.bincount(v, minlength=ht))
        col.free()
        keys = ht   # every table row is a key; every value of v is one of them
        assert check() == keys
        t_join, t_check = alternated([join, check], a.reps, wall_ms)
        s_join, s_check = alternated([join, check], a.reps, scoped)
        mj, mc = statistics.median(t_join), statistics.median(t_check)
        lines.append("-- %s: table 2^%d rows, query 2^%d rows; %d slots, all records, %d keys" % (name, log_t, log_q, ht + hq, keys))
        lines.append("join  call %.3f [%.3f .. %.3f]; " % (mj, min(t_join), max(t_join))
                     + ", ".join("%s %.3f" % (n[len("lookup_mult_"):], statistics.median(s.get(n, 0.0) for s in s_join)) for n in JOIN))
        lines.append("check call %.3f [%.3f .. %.3f]; " % (mc, min(t_check), max(t_check))
                     + ", ".join("%s %.3f" % (n[len("lookup_check_"):], statistics.median(s.get(n, 0.0) for s in s_check)) for n in CHECK))
        lines.append("join / check = %.3f (the join's scatter scope holds the scatter, the compaction of the misses and its blocking read; "
                     "the check's sums scope holds heads, DC exclusive sums, flags, the compaction and the report of 16 keys)" % (mj / mc))
        table.free()
        query.free()
    ctx.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
