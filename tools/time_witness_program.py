"""Times of the witness seam on resident KoalaBear traces, DC = 4, beside the check seam on the same value ops.
   python tools/time_witness_program.py [--reps 20] [--out FILE]

Three programs, at h = 2^16 and 2^20 rows:
  thin       from one column x of 17-bit values: lo = bits [0, 8), hi = bits [8, 16) and the flag bits [16, 17); 3 stores
  inverse    the same limbs, the inverse witness w = 1 / x (0 for 0) and the is-zero flag 1 - x w; 4 stores, 1 inversion
  poseidon2  a width-16 Poseidon2 external round's worth of arithmetic on 16 columns - a round constant, the cube and the
             4 x 4 MDS blocks with the column sums - with 16 stores
Beside each stands p3r_check_program_dmat on a constraint program with the SAME value ops and one ASSERT_ZERO per store:
the interpreter's existing cost per value op.  What is asserted is v - v, one more SUB per store (counted among the
check's value ops), so that the trace SATISFIES the program: on a failing trace the check's time is that of its atomic
operations, not of the interpreter.  A constraint program has neither BITS nor INV: there a BITS is two products by
constants (what it costs: one multiplication to leave Montgomery form, one to re-enter) and the INV is left out, which
the line of `inverse` says.  The two entries are called ALTERNATELY in one process.

Every figure is the median of --reps calls after two warm-up calls of each entry, in ms.  `kernel` is the library's profile
scope around the one launch (device events on the context's stream); `call` is a host clock around the call and the
synchronise that follows it (the check waits by itself; the witness call only enqueues).  `hbm` is the least time the
call's columns take to be read once and written once at 6.3 TB/s, the bandwidth the chip achieves on a copy.  No hardware
counter is collected.  Nothing here is a threshold; the output goes to profiles/<round>/."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P, DC = 0x7F000001, 4
HBM_BYTES_PER_MS = 6.3e12 / 1e3


def thin(b, sink, witness):
    x = b.local(0, 0)
    for k, (lo, n) in enumerate(((0, 8), (8, 8), (16, 1))):
        sink(b.bits(x, lo, n) if witness else (x * b.const(3 + k)) * b.const(5 + k), k)
    return 3


def inverse(b, sink, witness):
    x = b.local(0, 0)
    for k, (lo, n) in enumerate(((0, 8), (8, 8))):
        sink(b.bits(x, lo, n) if witness else (x * b.const(3 + k)) * b.const(5 + k), k)
    w = b.inv(x) if witness else b.local(0, 0)
    sink(w, 2)
    sink(1 - x * w, 3)
    return 4


def poseidon2(b, sink, witness):
    s = [(b.local(0, i) + b.const(1000 + 7 * i)) for i in range(16)]
    s = [v * v * v for v in s]
    out = []
    for k in range(4):   # the 4 x 4 MDS block circ(2, 3, 1, 1) by additions
        x0, x1, x2, x3 = s[4 * k:4 * k + 4]
        t01, t23 = x0 + x1, x2 + x3
        t0123 = t01 + t23
        t01123, t01233 = t0123 + x1, t0123 + x3
        out += [t01123 + t01, t01123 + (x2 + x2), t01233 + t23, t01233 + (x0 + x0)]
    sums = [out[i] + out[4 + i] + out[8 + i] + out[12 + i] for i in range(4)]
    for i in range(16):
        sink(out[i] + sums[i % 4], i)
    return 16


def value_ops(builder):
    from plonky3_recursion_amd import _lib as L
    sinks = (L.P3R_AIR_STORE, L.P3R_AIR_ASSERT_ZERO)
    return sum(1 for op, _, _ in builder.insns if op not in sinks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import plonky3_recursion_amd as p3r

    ctx = p3r.Context(field="koala-bear")
    rng = np.random.default_rng(20)
    lines = ["%s; KoalaBear, DC = %d; medians of %d alternated calls after 2 warm-up calls each, ms (min .. max in brackets)"
             % (torch.cuda.get_device_name(0), DC, a.reps),
             "shared inversion (Montgomery's trick over the base INVs of a row): not built; every INV is one Fp::inv",
             "per value op, like stands against like in poseidon2 only; in thin and inverse a BITS of the witness program stands against "
             "two constants and two products of the check program"]

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

    for log_h in (16, 20):
        h = 1 << log_h
        for name, make, n_in in (("thin", thin, 1), ("inverse", inverse, 1), ("poseidon2", poseidon2, 16)):
            data = rng.integers(0, 1 << 17, size=(h, n_in), dtype=np.uint32) if n_in == 1 else rng.integers(0, P, size=(h, n_in), dtype=np.uint32)
            if n_in == 1:
                data[::8] = 0
            d_in = ctx.upload(data)
            wit, chk = p3r.AirBuilder("koala-bear"), p3r.AirBuilder("koala-bear")
            n_out = make(wit, wit.store, True)
            make(chk, lambda v, col: chk.assert_zero(v - v), False)
            info = ctx.witness_program_info(wit, [n_in])
            assert info["n_out_columns"] == n_out

            def witness():
                ctx.witness_device(wit, [d_in]).free()

            def check():
                assert ctx.check_device(chk, [d_in])["n_failures"] == 0
            times = {"w_call": [], "c_call": [], "w_kernel": [], "c_kernel": []}
            for _ in range(2):
                witness()
                check()
            ctx.sync()
            for _ in range(a.reps):
                times["w_call"].append(wall_ms(witness))
                times["c_call"].append(wall_ms(check))
            for _ in range(a.reps):
                times["w_kernel"].append(scope_ms(witness, "witness_program"))
                times["c_kernel"].append(scope_ms(check, "check_program"))
            med = {k: statistics.median(v) for k, v in times.items()}
            n_w, n_c = value_ops(wit), value_ops(chk)
            hbm = 4.0 * h * (n_in + n_out) / HBM_BYTES_PER_MS
            lines.append("-- %s, h = 2^%d: %d input and %d output columns; witness %d value ops (%d inversions, peak_live %d), check %d value ops%s"
                         % (name, log_h, n_in, n_out, n_w, info["n_inversions"], info["peak_live"], n_c,
                            " (no INV: not comparable per op)" if info["n_inversions"] else ""))
            for who, tag, n_ops in (("witness", "w", n_w), ("check  ", "c", n_c)):
                k, c = times[tag + "_kernel"], times[tag + "_call"]
                lines.append("%s kernel %.4f [%.4f .. %.4f], %.2f ps per row and value op; call %.3f [%.3f .. %.3f]"
                             % (who, med[tag + "_kernel"], min(k), max(k), med[tag + "_kernel"] * 1e9 / (h * n_ops), med[tag + "_call"], min(c), max(c)))
            lines.append("hbm %.4f (read once, write once, 6.3 TB/s); witness kernel / hbm = %.1f; witness / check per value op = %.2f"
                         % (hbm, med["w_kernel"] / hbm, (med["w_kernel"] / n_w) / (med["c_kernel"] / n_c)))
            d_in.free()
    ctx.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
