"""Time of the constraint-program seam (p3r_quotient_program_dmat, k_quotient_program) on resident KoalaBear LDEs of a
2^20-row trace, log_quotient_degree 1 (N = 2^21 rows), for two programs:
   thin   8 columns, 8 degree-2 constraints  local[k] * local[k+1] - next[k]
   thick  32 columns, 100 degree-3 constraints of three products each (about 300 multiplications)
   python tools/time_quotient_program.py [--log-rows 20] [--reps 10] [--out FILE]

Per program: the kernel's ms (the library's own launch timing) and the call's; the bytes it must read - every used column
once over the N rows, 4 bytes a word; the next row is a second read of the same words - and the rate that makes; the
field products per second (a product of the program is one, a Horner step of the DC = 4 constraint fold sixteen, the
final scaling four) against the Montgomery-product rate tools/microbench recorded; the LDS of a workgroup (both programs
hold base values only: 256 bytes per live value) and the waves per SIMD that leaves.  For scale only, the `quotient`
family of the committed benchmark line - the prover's own k_quotient on the five built-in tables of its workload, a
DIFFERENT workload and not a comparator.  Nothing here is a threshold; the numbers go to profiles/<round>/."""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_GBS, LDS_PER_CU, MAX_WAVES_PER_SIMD = 6300, 160 * 1024, 8


def thin(p3r):
    b = p3r.AirBuilder("koala-bear")
    for k in range(8):
        b.assert_zero(b.local(0, k) * b.local(0, (k + 1) % 8) - b.next(0, k))
    return b, 8, 8


def thick(p3r):
    b = p3r.AirBuilder("koala-bear")
    muls = 0
    for j in range(100):
        t = b.local(0, j % 32) * b.local(0, (j + 7) % 32) * b.next(0, (j + 13) % 32)
        b.assert_zero(t + b.next(0, (j + 3) % 32) * b.const(j + 2))
        muls += 3
    return b, 32, muls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import plonky3_recursion_amd as p3r

    p, dc, q, added_bits = 0x7F000001, 4, 1, 1
    ctx = p3r.Context(field="koala-bear")
    n = (1 << a.log_rows) << q
    rates = open(os.path.join(ROOT, "profiles", "r06", "microbench_int_rates.txt")).read()
    mont = float(re.search(r"Montgomery product\s+([0-9.]+) T", rates).group(1)) * 1e12
    lines = ["constraint programs over the quotient domain of a 2^%d-row KoalaBear trace: log_quotient_degree %d, N = %d rows, DC = %d"
             % (a.log_rows, q, n, dc),
             "%-6s %8s %8s %9s %9s %9s %11s %12s %10s %9s %10s" % ("", "insns", "live", "call ms", "kern ms", "MB read", "GB/s", "of HBM %d" % HBM_GBS,
                                                                  "Gmul/s", "of mont", "LDS B/wg")]
    notes = []
    for name, make in (("thin", thin), ("thick", thick)):
        prog, width, muls = make(p3r)
        info = ctx.air_program_info(prog, [width])
        mat = ctx.upload(np.random.default_rng(width).integers(0, p, size=(n << (added_bits - q), width), dtype=np.uint32))
        alpha = [3, 5, 7, 11]

        def call():
            for o in ctx.quotient_device(prog, [mat], added_bits, q, alpha):
                o.free()
        for _ in range(2):
            call()
        ctx.sync()
        t = time.perf_counter()
        for _ in range(a.reps):
            call()
        ctx.sync()
        call_ms = (time.perf_counter() - t) / a.reps * 1e3
        ctx.profile_enable(True)
        for _ in range(a.reps):
            call()
        ctx.sync()
        tot, launches = ctx.profile_read()["quotient_program"]
        ctx.profile_enable(False)
        k_ms = tot / launches
        must = width * n * 4
        products = (muls + 16 * info["n_constraints"] + dc) * n
        lds = info["peak_live"] * 256
        waves = min(MAX_WAVES_PER_SIMD, (LDS_PER_CU // lds) // 4)
        lines.append("%-6s %8d %8d %9.3f %9.3f %9.1f %11.1f %12.3f %10.1f %9.3f %10d" % (
            name, len(prog.insns), info["peak_live"], call_ms, k_ms, must / 1e6, must / k_ms / 1e6, must / k_ms / 1e6 / HBM_GBS,
            products / k_ms / 1e6, products / (k_ms * 1e-3) / mont, lds))
        notes.append("%s: %d workgroups of one wave per CU by LDS -> %d waves per SIMD (the cap is %d); + %.1f MB written"
                     % (name, LDS_PER_CU // lds, waves, MAX_WAVES_PER_SIMD, n * dc * 4 / 1e6))
        mat.free()
    ctx.close()
    lines += notes
    lines.append("Montgomery-product rate taken from profiles/r06/microbench_int_rates.txt: %.2f T lane-ops/s" % (mont / 1e12))
    detail = json.load(open(os.path.join(ROOT, "profiles", "r06", "bench_default_detail.json")))
    fam = detail.get("quotient")
    if not isinstance(fam, (int, float)):
        fam = [v for k, v in detail.items() if isinstance(v, dict) and isinstance(v.get("quotient"), (int, float))][0]["quotient"]
    lines.append("for scale only - a DIFFERENT workload, not a comparator: the `quotient` family (the prover's k_quotient over the built-in "
                 "tables) of the committed benchmark line profiles/r06/bench_default_detail.json: %.3f ms" % fam)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
