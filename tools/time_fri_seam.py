"""Time of the public FRI seam (p3r_fri_reduce_dmat, p3r_fri_fold_dmat) on one resident LDE-sized KoalaBear matrix.
   python tools/time_fri_seam.py [--log-rows 20] [--width 64] [--points 2] [--reps 10] [--out FILE]

Reduce: one (2^log_rows) x width matrix at `points` points.  The tool prints the host time of a call (uploads of the
values and job lists, three launches) and the library's own times (p3r_profile_read) of the inverse-vector launch
(`fri_seam_inv_points`) and of the column sums + pass (`fri_seam_reduce`), the latter against the bytes the pass MUST
move, each once: the matrix (H * w * 4), one inverse vector per point (points * DC * H * 4) and the output (DC * H * 4).
Fold: a (2^log_rows) x DC vector by 2, 4, 8 and 16 (`fri_seam_fold`), against DC * 4 * (n + (n >> la)) bytes, and with a
roll-in (another DC * 4 * (n >> la)).
Beside them: the prover's `fri_reduce` and `fri_inv_points` times of one proof from bench_detail.json (written by
`python bench.py --full`; else the newest committed profiles/r*/bench_line_final.json) - the same pass over ALL matrices
of that proof at at most two points, so a different byte count: it is quoted, not compared.
Nothing here is a threshold; the numbers go to profiles/<round>/fri_seam.txt."""
import argparse
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", type=int, default=20)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--points", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--challenge-degree", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import plonky3_recursion_amd as p3r

    p, dc = 0x7F000001, a.challenge_degree
    ctx = p3r.Context(field="koala-bear", challenge_degree=dc)
    rng = np.random.default_rng(a.log_rows)
    H = 1 << a.log_rows

    def ext(n):
        z = rng.integers(0, p, size=(n, dc), dtype=np.uint32)
        z[:, 1] |= 1   # outside the base field: in no coset
        return z

    def timed(fn, names):
        for _ in range(2):
            fn()
        ctx.sync()
        t = time.perf_counter()
        for _ in range(a.reps):
            fn()
        ctx.sync()
        call_ms = (time.perf_counter() - t) / a.reps * 1e3
        ctx.profile_enable(True)
        for _ in range(a.reps):
            fn()
        ctx.sync()
        prof = ctx.profile_read()
        ctx.profile_enable(False)
        return call_ms, [prof[n][0] / max(1, prof[n][1]) if n in prof else float("nan") for n in names]

    dm = ctx.upload(rng.integers(0, p, size=(H, a.width), dtype=np.uint32))
    pts, alpha = ext(a.points), ext(1)[0]
    vals = rng.integers(0, p, size=(a.points, a.width, dc), dtype=np.uint32)

    def reduce_once():
        for o in ctx.fri_reduce_device([dm], [pts], [vals], alpha):
            o.free()

    call_ms, (inv_ms, red_ms) = timed(reduce_once, ("fri_seam_inv_points", "fri_seam_reduce"))
    must = H * a.width * 4 + a.points * dc * H * 4 + dc * H * 4
    inv_bytes = a.points * dc * H * 4
    lines = ["fri_reduce on a %d x %d KoalaBear matrix at %d points, DC = %d" % (H, a.width, a.points, dc),
             "bytes the pass must move: matrix %.1f MB + inverse vectors %.1f MB + output %.1f MB = %.1f MB, each once"
             % (H * a.width * 4 / 1e6, inv_bytes / 1e6, dc * H * 4 / 1e6, must / 1e6),
             "(every repetition re-reads the same matrix: what of it still sits in the 256 MiB last-level cache is not read from HBM,"
             " so at 2^20 x 64 the rate is an upper estimate of a cold pass; --log-rows 22 is four times the cache)",
             "%-22s %10s %12s" % ("", "ms", "GB/s"),
             "%-22s %10.3f" % ("call (host, with free)", call_ms),
             "%-22s %10.3f %12.1f   (writes %d vectors: %.1f MB)" % ("fri_seam_inv_points", inv_ms, inv_bytes / inv_ms / 1e6, a.points, inv_bytes / 1e6),
             "%-22s %10.3f %12.1f   (column sums of the values + the pass)" % ("fri_seam_reduce", red_ms, must / red_ms / 1e6)]
    dm.free()

    vec = ctx.upload(rng.integers(0, p, size=(H, dc), dtype=np.uint32))
    lines += ["", "fri_fold of a %d x %d vector" % (H, dc), "%-10s %-8s %10s %10s %12s %12s" % ("log_arity", "roll-in", "call ms", "fold ms", "MB moved", "GB/s")]
    for la in (1, 2, 3, 4):
        roll = ctx.upload(rng.integers(0, p, size=(H >> la, dc), dtype=np.uint32))
        beta = ext(1)[0]
        for r in (None, roll):
            call_ms, (fold_ms,) = timed(lambda: ctx.fri_fold_device(vec, la, beta, roll_in=r).free(), ("fri_seam_fold",))
            moved = dc * 4 * (H + (H >> la) * (2 if r is not None else 1))
            lines.append("%-10d %-8s %10.3f %10.3f %12.1f %12.1f" % (la, "yes" if r is not None else "no", call_ms, fold_ms, moved / 1e6, moved / fold_ms / 1e6))
        roll.free()
    vec.free()
    ctx.close()

    def find(o, key):
        if isinstance(o, dict):
            for k2, v in o.items():
                if k2 == key and isinstance(v, (int, float)):
                    yield v
                yield from find(v, key)
        elif isinstance(o, list):
            for v in o:
                yield from find(v, key)
    quoted = None
    for path in [os.path.join(ROOT, "bench_detail.json")] + sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "bench_line_final.json")), reverse=True):
        if not os.path.exists(path):
            continue
        try:
            doc = json.load(open(path))
        except ValueError:
            continue
        red, inv = list(find(doc, "fri_reduce")), list(find(doc, "fri_inv_points"))
        if red and inv:
            quoted = (os.path.relpath(path, ROOT), red[0], inv[0])
            break
    lines.append("")
    if quoted:
        lines.append("prover's own launches (%s: all matrices of one proof, <= 2 points each): fri_reduce %.3f ms, fri_inv_points %.3f ms"
                     % quoted)
    else:
        lines.append("prover's own launches: no fri_reduce / fri_inv_points times in bench_detail.json or profiles/r*/bench_line_final.json")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
