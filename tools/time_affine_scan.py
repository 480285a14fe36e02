"""Times of the recurrence seam (Context.affine_scan_device: the three passes of k_affine_scan) on resident KoalaBear
traces, DC = 4, at h = 2^20 rows.
   python tools/time_affine_scan.py [--reps 20] [--log-h 20] [--out FILE]

Six forms: a base sum, a base affine recurrence, an extension sum, an extension product, an extension affine recurrence,
and eight extension affine recurrences in one call (eight pairs of input columns, one launch of each pass).

Every figure is in ms.  `kernel` is the library's profile scope around the three launches (device events on the
context's stream), the median of --reps calls after two warm-up calls; `call` is a host clock around the call and the
synchronise that follows it (the call only enqueues: no last_out is asked for).  `hbm` is the least time the passes' own
traffic takes at 6.3 TB/s, the bandwidth the chip achieves on a copy: every input column read twice (passes 0 and 2) and
every output column written once; `share` is hbm / kernel.  The tile composites and the descriptors are not counted: they
are 3 DC words per 1024 rows.  No hardware counter is collected.

For the extension sum the one existing kernel that does the same job stands beside it: k_ef_scan, as
p3r_logup_program_dmat runs it on a column of the same height.  The existing profile hooks give that entry ONE scope,
`logup_program`, which holds k_trace_program<LogupProgSink> (one fraction m / d per row: an extension inversion, DC words written twice)
and the three scan passes; the passes alone cannot be read through them.  So the figure beside the sum is an upper bound
of the scan passes.  The two are called ALTERNATELY, in five runs of --reps calls each; the spread of the five medians is
the run-to-run noise.  Nothing here is a threshold; the output goes to profiles/<round>/."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P, DC = 0x7F000001, 4
HBM_BYTES_PER_MS = 6.3e12 / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log-h", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import plonky3_recursion_amd as p3r
    R = p3r.Recurrence

    ctx = p3r.Context(field="koala-bear")
    rng = np.random.default_rng(21)
    h = 1 << a.log_h
    d_base = ctx.upload(rng.integers(0, P, size=(h, 2), dtype=np.uint32))
    d_ext = ctx.upload(rng.integers(0, P, size=(h, 16 * DC), dtype=np.uint32))   # eight (a, b) pairs of extension columns
    one = [1] + [0] * (DC - 1)
    forms = [
        ("base sum", [R(0, add=(0, 1))], 1, 1),
        ("base affine", [R(0, mul=(0, 0), add=(0, 1), init=1)], 2, 1),
        ("ext sum", [R(0, add=(1, DC), ext=True)], DC, DC),
        ("ext product", [R(0, mul=(1, 0), ext=True, init=one)], DC, DC),
        ("ext affine", [R(0, mul=(1, 0), add=(1, DC), ext=True, init=one)], 2 * DC, DC),
        ("ext affine x 8", [R(k * DC, mul=(1, 2 * k * DC), add=(1, (2 * k + 1) * DC), ext=True, init=one) for k in range(8)], 16 * DC, 8 * DC),
    ]
    lines = ["%s; KoalaBear, DC = %d, h = 2^%d; medians of %d calls after 2 warm-up calls, ms (min .. max in brackets)"
             % (torch.cuda.get_device_name(0), DC, a.log_h, a.reps)]

    def scope_ms(fn, name):
        ctx.profile_enable(True)
        fn()
        got = ctx.profile_read()
        ctx.profile_enable(False)
        return got[name][0]

    def wall_ms(fn):
        ctx.sync()
        t = time.perf_counter()
        fn()
        ctx.sync()
        return (time.perf_counter() - t) * 1e3

    def scan_of(recs):
        return lambda: ctx.affine_scan_device(recs, [d_base, d_ext]).free()

    for name, recs, n_in, n_out in forms:
        fn = scan_of(recs)
        for _ in range(2):
            fn()
        ctx.sync()
        call = [wall_ms(fn) for _ in range(a.reps)]
        kern = [scope_ms(fn, "affine_scan") for _ in range(a.reps)]
        hbm = 4.0 * h * (2 * n_in + n_out) / HBM_BYTES_PER_MS
        k = statistics.median(kern)
        lines.append("%-15s kernel %.4f [%.4f .. %.4f]; call %.3f [%.3f .. %.3f]; hbm %.4f (%d input columns twice, %d output columns once); "
                     "share %.2f" % (name, k, min(kern), max(kern), statistics.median(call), min(call), max(call), hbm, n_in, n_out, hbm / k))

    # ---- the extension sum beside the one existing kernel that does the same job
    lk = p3r.AirBuilder("koala-bear")
    lk.lookup(lk.local(0, 1), lk.challenge(0) - lk.local(0, 0))
    lk.end_lookup_column()
    gamma = rng.integers(1, P, size=(1, DC), dtype=np.uint32)
    ext_sum = scan_of(forms[2][1])

    def logup():
        aux, _ = ctx.logup_device(lk, [d_base], challenges=gamma)
        aux.free()
    for _ in range(2):
        ext_sum()
        logup()
    ctx.sync()
    runs = {"ext sum": [], "logup_program": []}
    for _ in range(5):
        s, l = [], []
        for _ in range(a.reps):
            s.append(scope_ms(ext_sum, "affine_scan"))
            l.append(scope_ms(logup, "logup_program"))
        runs["ext sum"].append(statistics.median(s))
        runs["logup_program"].append(statistics.median(l))
    lines.append("-- ext sum beside p3r_logup_program_dmat on a column of the same height, alternated; the medians of five runs of %d calls" % a.reps)
    for name, what in (("ext sum", "the three passes of k_affine_scan, pure-sum instance"),
                       ("logup_program", "k_trace_program<LogupProgSink> (one fraction per row) + the three passes of k_ef_scan: an UPPER bound of the scan passes")):
        m = runs[name]
        lines.append("%-15s %s; spread %.4f (%.1f%% of the median)   %s"
                     % (name, " ".join("%.4f" % v for v in m), max(m) - min(m), 100.0 * (max(m) - min(m)) / statistics.median(m), what))
    lines.append("ext sum / logup_program = %.2f" % (statistics.median(runs["ext sum"]) / statistics.median(runs["logup_program"])))
    d_base.free()
    d_ext.free()
    ctx.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
