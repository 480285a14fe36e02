"""Times of the two trace checks on resident KoalaBear traces, DC = 4.
   python tools/time_check_program.py [--log-rows 20] [--reps 20] [--out FILE]

1. p3r_check_program_dmat (k_trace_program<CheckProgSink>) on a 2^log-rows x 32 trace that does NOT satisfy the program in most rows
   (random cells) and on one that satisfies it everywhere (random inputs, the constrained cells computed from them), for
   two programs:
     thin     two constraints over five cells;
     round    one external round of the width-16 Poseidon2 over columns 0 .. 15 (add a constant, cube, the M4-circulant
              layer) asserted against columns 16 .. 31: sixteen constraints of degree 3.
   Beside each, in the same run, p3r_quotient_program_dmat (k_quotient_program, unchanged) for the same program over the
   SAME NUMBER OF ROWS: the same matrix read as a committed LDE whose quotient domain is all of its rows - thin: q = 0,
   blow-up 1; round: degree 3 needs q = 1, so the matrix is read as an LDE of blow-up 2 of a trace of half the rows and the
   quotient domain is again every row.  Both interpret the same instruction stream once per row; the quotient pass adds
   the selector inversions (none here: neither program reads a selector), one Horner step per constraint and the chunk
   writes, the check a ballot per constraint and, on a failing wave, two atomics.
2. p3r_lookup_check_dmat on a bus of about 2^log-rows records: a sender of 2^log-rows rows (one term, the reference's bus
   denominator over two cells, multiplicity 1) and a receiver of 2^(log-rows - 4) rows; balanced.  Split by the library's
   own profile scopes into the record launches, the sort (DC passes groups of four 8-bit passes each with their gathers)
   and the rest (heads, exclusive sums, flags, compaction), beside the whole call on a host clock (it includes the two
   blocking reads of counts).

Every figure is the median of --reps calls after two warm-up calls, in ms; call times are a host clock around calls that
end in the device synchronise the entry itself makes (the quotient entry only enqueues: Context.sync ends its window),
launch times the library's profile scopes (device events on the context's stream) from a second set of calls.  No
hardware counter is collected.  Nothing here is a threshold; the output goes to profiles/<round>/."""
import argparse
import os
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P, DC = 0x7F000001, 4


def thin(p3r):
    b = p3r.AirBuilder("koala-bear")
    b.assert_zero(b.next(0, 0) - b.local(0, 1))
    b.assert_zero(b.local(0, 2) * b.local(0, 3) - b.local(0, 4))
    return b


def poseidon2_round(p3r):
    """out = M_ext((in + rc)^3) with the constants 0: a constant's value costs the interpreter nothing, and satisfying()
    need not carry a table."""
    b = p3r.AirBuilder("koala-bear")
    s = []
    for i in range(16):
        x = b.local(0, i) + b.const(0)
        s.append(x * x * x)
    t = []
    for k in range(4):   # M4 = circ(2, 3, 1, 1) on each block of four
        a = s[4 * k:4 * k + 4]
        total = a[0] + a[1] + a[2] + a[3]
        t += [total + a[j] + a[(j + 1) % 4] + a[(j + 1) % 4] for j in range(4)]
    sums = [t[j] + t[4 + j] + t[8 + j] + t[12 + j] for j in range(4)]
    for i in range(16):
        b.assert_zero(b.local(0, 16 + i) - (t[i] + sums[i % 4]))
    return b


def satisfying(np, rng, h):
    """One h x 32 matrix that satisfies both programs: random columns 0 .. 15 with column 1 = column 0 a row on and
    column 4 = column 2 * column 3 (thin), then columns 16 .. 31 = the round of columns 0 .. 15."""
    U, p = np.uint64, np.uint64(P)
    m = rng.integers(0, P, size=(h, 32), dtype=np.uint32).astype(U)
    m[:, 1] = np.roll(m[:, 0], -1)
    m[:, 4] = m[:, 2] * m[:, 3] % p
    s = m[:, :16] * m[:, :16] % p * m[:, :16] % p
    t = np.empty((h, 16), dtype=U)
    for k in range(4):
        a = s[:, 4 * k:4 * k + 4]
        total = a.sum(axis=1)
        for j in range(4):
            t[:, 4 * k + j] = (total + a[:, j] + 2 * a[:, (j + 1) % 4]) % p
    sums = (t[:, 0:4] + t[:, 4:8] + t[:, 8:12] + t[:, 12:16]) % p
    m[:, 16:] = (t + np.tile(sums, 4)) % p
    return m.astype(np.uint32)


def median_ms(fn, reps):
    for _ in range(2):
        fn()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out), min(out), max(out)


def scopes_ms(ctx, fn, reps, names):
    """Median per call of each profile scope, from `reps` calls profiled one by one."""
    per = {n: [] for n in names}
    ctx.profile_enable(True)
    for _ in range(reps):
        fn()
        got = ctx.profile_read()
        for n in names:
            per[n].append(got[n][0] if n in got else 0.0)
        ctx.profile_enable(False)
        ctx.profile_enable(True)
    ctx.profile_enable(False)
    return {n: statistics.median(v) for n, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import plonky3_recursion_amd as p3r

    ctx = p3r.Context(field="koala-bear")
    h, rng = 1 << a.log_rows, np.random.default_rng(17)
    lines = ["box: %s, %s; KoalaBear, DC = %d; medians of %d calls after 2 warm-up calls, ms (min .. max in brackets)"
             % (socket.gethostname(), torch.cuda.get_device_name(0), DC, a.reps)]
    random_trace = ctx.upload(rng.integers(0, P, size=(h, 32), dtype=np.uint32))
    good_trace = ctx.upload(satisfying(np, rng, h))
    alpha = rng.integers(1, P, size=DC, dtype=np.uint32)
    for name, prog, added_bits, q in (("thin", thin(p3r), 0, 0), ("round", poseidon2_round(p3r), 1, 1)):
        info = ctx.air_program_info(prog, [32])
        assert info["log_quotient_degree"] == q
        lines.append("-- %s: %d instructions, %d constraints, degree %d, %d live values at most; 2^%d x 32 trace"
                     % (name, len(prog.insns), info["n_constraints"], info["max_degree"], info["peak_live"], a.log_rows))
        for label, mat in (("failing (random cells)", random_trace), ("satisfying", good_trace)):
            rep = ctx.check_device(prog, [mat])
            assert (rep["n_failures"] == 0) == (mat is good_trace)
            call = median_ms(lambda: ctx.check_device(prog, [mat]), a.reps)
            k = scopes_ms(ctx, lambda: ctx.check_device(prog, [mat]), a.reps, ["check_program"])["check_program"]
            lines.append("check, %s: %d failures; call %.3f [%.3f .. %.3f], k_trace_program<CheckProgSink> %.3f" % ((label, rep["n_failures"]) + call + (k,)))

        def quotient():   # the same matrix as the satisfying check's (the pass does not care what its cells mean)
            for c in ctx.quotient_device(prog, [good_trace], added_bits, q, alpha):
                c.free()
            ctx.sync()
        call = median_ms(quotient, a.reps)
        k = scopes_ms(ctx, quotient, a.reps, ["quotient_program"])["quotient_program"]
        lines.append("quotient over the same 2^%d rows of the satisfying matrix (blow-up 2^%d, q = %d): call %.3f [%.3f .. %.3f], k_quotient_program %.3f"
                     % ((a.log_rows, added_bits, q) + call + (k,)))
    random_trace.free()
    good_trace.free()

    # ---- the bus
    hr = h >> 4
    second = rng.integers(0, P, size=hr, dtype=np.uint32)
    ids = rng.integers(0, hr, size=h)
    sender = ctx.upload(np.stack([ids.astype(np.uint32), second[ids], np.ones(h, dtype=np.uint32)], axis=1))
    counts = np.bincount(ids, minlength=hr)
    receiver = ctx.upload(np.stack([np.arange(hr, dtype=np.uint32), second, ((P - counts) % P).astype(np.uint32)], axis=1))
    b = p3r.AirBuilder("koala-bear")
    b.lookup(b.local(0, 2), b.challenge(0) + b.local(0, 0) + b.challenge(1) * b.local(0, 1))
    b.end_lookup_column()
    chal = rng.integers(1, P, size=(2, DC), dtype=np.uint32)
    inst = [(b, [sender]), (b, [receiver])]
    n, _ = ctx.lookup_check_device(inst, challenges=chal)
    assert n == 0
    records = h + int(np.count_nonzero(counts))
    call = median_ms(lambda: ctx.lookup_check_device(inst, challenges=chal), a.reps)
    names = ["lookup_check_records", "lookup_check_sort", "lookup_check_sums"]
    k = scopes_ms(ctx, lambda: ctx.lookup_check_device(inst, challenges=chal), a.reps, names)
    lines.append("-- lookup check: two instances, %d slots, %d records, %d keys, balanced" % (h + hr, records, int(np.count_nonzero(counts))))
    lines.append("call %.3f [%.3f .. %.3f]; record launches %.3f, sort %.3f, rest %.3f (sum of the three %.3f: the call also has two blocking "
                 "reads of counts, the compaction of the records before the sort and the uploads)"
                 % (call + (k[names[0]], k[names[1]], k[names[2]], sum(k.values()))))
    sender.free()
    receiver.free()
    ctx.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
