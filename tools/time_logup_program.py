"""Time of the lookup-program seam (p3r_logup_program_dmat: k_trace_program<LogupProgSink> and the three k_ef_scan passes) on a resident
KoalaBear trace of 2^20 rows, DC = 4: 8 terms in 4 columns, each term a multiplicity cell over the reference's bus
denominator bus_prefix + t0 + beta * t1 of two cells - 24 input columns.
   python tools/time_logup_program.py [--log-rows 20] [--reps 10] [--bench-detail FILE] [--out FILE]

Printed: the call's ms (a host clock around calls that each end in the device synchronise the entry itself makes) and the
launches' ms (the library's own profile scope `logup_program`, the four kernels together); the bytes the pass must move -
every input column read once, DC * (1 + G) * 4 bytes written per row; the scan's re-read of the row totals is not counted
- and the rate that makes against HBM; the field products of the program per second against the Montgomery-product
rate tools/microbench recorded, with an extension inversion counted by the products of its square-and-multiply chain.
The product count is an ESTIMATE from the shapes (it leaves out the LDS traffic of the slot file and the interpreter's
address arithmetic) and no hardware counter is collected: which resource binds the pass is inferred, not measured, and
the output says so.
With --bench-detail (bench.py's --detail-out file of a run on the same box): the `logup_aux` family of that proof - the
prover's own k_logup_aux + k_ef_scan over ALL tables of the flagship proof in one launch each - for scale only.  It is a
DIFFERENT workload (five tables of other heights and interaction counts), not a like-for-like comparator: no table of
2^20 rows was run through K7 alone.  Nothing here is a threshold; the numbers go to profiles/<round>/."""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_GBS = 6300
TERMS, COLUMNS = 8, 4


def program(p3r):
    b = p3r.AirBuilder("koala-bear")
    prefix, beta = b.challenge(0), b.challenge(1)
    per = TERMS // COLUMNS
    for k in range(TERMS):
        b.lookup(b.local(0, 3 * k + 2), prefix + b.local(0, 3 * k) + beta * b.local(0, 3 * k + 1))
        if k % per == per - 1:
            b.end_lookup_column()
    return b, 3 * TERMS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--bench-detail", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import plonky3_recursion_amd as p3r

    p, dc = 0x7F000001, 4
    ctx = p3r.Context(field="koala-bear")
    h = 1 << a.log_rows
    prog, width = program(p3r)
    info = ctx.lookup_program_info(prog, [width])
    rng = np.random.default_rng(16)
    mat = ctx.upload(rng.integers(0, p, size=(h, width), dtype=np.uint32))
    chal = rng.integers(1, p, size=(2, dc), dtype=np.uint32)

    def call():
        out, total = ctx.logup_device(prog, [mat], challenges=chal)
        out.free()
        return total
    for _ in range(2):
        call()
    t = time.perf_counter()
    for _ in range(a.reps):
        call()
    call_ms = (time.perf_counter() - t) / a.reps * 1e3
    ctx.profile_enable(True)
    for _ in range(a.reps):
        call()
    tot, launches = ctx.profile_read()["logup_program"]
    ctx.profile_enable(False)
    k_ms = tot / launches
    mat.free()
    ctx.close()
    read, written = width * h * 4, dc * (1 + COLUMNS) * h * 4
    # per row: a denominator is one ext * base product (DC) and adds; a term into the open fraction num * d (DC^2), den * m
    # (DC), den * d (DC^2); a column end one inversion - the quartic's norm tower, about 3 DC^2 products and one base
    # inversion of 31 squarings and as many products at most - and num * den^-1 (DC^2)
    products = (TERMS * (dc + 2 * dc * dc + dc) + COLUMNS * (4 * dc * dc + 62)) * h
    rates = open(os.path.join(ROOT, "profiles", "r06", "microbench_int_rates.txt")).read()
    mont = float(re.search(r"Montgomery product\s+([0-9.]+) T", rates).group(1)) * 1e12
    lines = ["lookup program over a 2^%d-row KoalaBear trace, DC = %d: %d terms in %d columns, %d input columns, %d instructions, %d live values at most"
             % (a.log_rows, dc, TERMS, COLUMNS, width, len(prog.insns), info["peak_live"]),
             "call %.3f ms (upload of the program, four launches, the wait for the table's sum); launches %.3f ms (scope logup_program: k_trace_program<LogupProgSink> + 3 x k_ef_scan)"
             % (call_ms, k_ms),
             "must move %.1f MB read + %.1f MB written = %.1f MB: %.1f GB/s over the launches, %.3f of HBM %d GB/s"
             % (read / 1e6, written / 1e6, (read + written) / 1e6, (read + written) / k_ms / 1e6, (read + written) / k_ms / 1e6 / HBM_GBS, HBM_GBS),
             "about %.0f field products per row: %.1f Gmul/s, %.3f of the Montgomery-product rate %.2f T/s (profiles/r06/microbench_int_rates.txt)"
             % (products / h, products / k_ms / 1e6, products / (k_ms * 1e-3) / mont, mont / 1e12),
             "the product count is an estimate from the shapes (an inversion taken as about 3 DC^2 + 62 products; slot-file LDS traffic and address "
             "arithmetic left out) and no hardware counter was collected: that the pass is bound by instruction issue and not by HBM is inferred "
             "from these two shares, not measured",
             "per term: %.4f ms" % (k_ms / TERMS)]
    if a.bench_detail:
        detail = json.load(open(a.bench_detail))
        found = []

        def walk(node):   # the family's ms, wherever the detail file keeps it
            if isinstance(node, dict):
                for k, v in node.items():
                    if k == "logup_aux" and isinstance(v, (int, float)):
                        found.append(float(v))
                    elif k == "logup_aux" and isinstance(v, dict) and isinstance(v.get("ms"), (int, float)):
                        found.append(float(v["ms"]))
                    else:
                        walk(v)
        walk(detail)
        if not found:
            raise SystemExit("no logup_aux family in %s: it is written by a --full run of bench.py" % a.bench_detail)
        fam = found[0]
        lines.append("for scale only - a DIFFERENT workload, not like for like: the prover's own K7 on the same box as the `logup_aux` family of the "
                     "flagship proof of %s (k_logup_aux + 3 x k_ef_scan over all five of its tables, heights 2^16 .. 2^20, interactions compiled in): "
                     "%.3f ms.  K7 on one table of 2^%d rows alone, and so a per-term comparison, was not measured"
                     % (os.path.basename(a.bench_detail), fam, a.log_rows))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
