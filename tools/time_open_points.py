"""Time of the value half of Pcs::open (p3r_open_points_dmat) on one resident LDE-sized KoalaBear matrix.
   python tools/time_open_points.py [--log-rows 22] [--width 64] [--added-bits 2] [--reps 10] [--out FILE]

The matrix is (2^log_rows) x width with added_bits of blow-up, i.e. the interpolant's evaluations are its first
h = 2^(log_rows - added_bits) rows (bit-reversed LDE).  For 1, 2 and P3R_OPEN_POINTS_PER_PASS points the tool prints
the host time of a call (upload of the job lists, three launches, copy back, one wait), the library's own time of the
dot launch (p3r_profile_read: `open_points_dot`), and the rate that time is against the bytes the pass MUST read:
h * width * 4, once, whatever the number of points.  Beside it: the prover's `open_dot` rate from bench_detail.json
(written by `python bench.py --full`; else the committed profiles/r06/bench_default_detail.json) - the same kind of read,
at most two points, natural order: ms, the bytes those launches must move, GB/s.
Nothing here is a threshold; the numbers go to profiles/<round>/open_points.txt."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", type=int, default=22)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--added-bits", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--challenge-degree", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import plonky3_recursion_amd as p3r
    from plonky3_recursion_amd import _lib

    p = 0x7F000001
    ctx = p3r.Context(field="koala-bear", challenge_degree=a.challenge_degree)
    rng = np.random.default_rng(a.log_rows)
    H, h = 1 << a.log_rows, 1 << (a.log_rows - a.added_bits)
    dm = ctx.upload(rng.integers(0, p, size=(H, a.width), dtype=np.uint32))
    must_read = h * a.width * 4
    lines = ["open_points on a %d x %d KoalaBear matrix, added_bits = %d (h = 2^%d evaluations per column), DC = %d, "
             "P3R_OPEN_POINTS_PER_PASS = %d" % (H, a.width, a.added_bits, a.log_rows - a.added_bits, a.challenge_degree,
                                                _lib.P3R_OPEN_POINTS_PER_PASS),
             "bytes the dot pass must read: h * w * 4 = %.1f MB, once" % (must_read / 1e6),
             "%-8s %12s %12s %14s %12s %12s" % ("points", "call ms", "dot ms", "dot GB/s", "weights ms", "reduce ms")]
    for k in (1, 2, _lib.P3R_OPEN_POINTS_PER_PASS):
        pts = rng.integers(0, p, size=(k, a.challenge_degree), dtype=np.uint32)
        for _ in range(2):
            ctx.open_points_device([dm], [pts], added_bits=a.added_bits)
        t = time.perf_counter()
        for _ in range(a.reps):
            ctx.open_points_device([dm], [pts], added_bits=a.added_bits)
        call_ms = (time.perf_counter() - t) / a.reps * 1e3
        ctx.profile_enable(True)
        for _ in range(a.reps):
            ctx.open_points_device([dm], [pts], added_bits=a.added_bits)
        prof = ctx.profile_read()
        ctx.profile_enable(False)
        ms = {n: prof[n][0] / max(1, prof[n][1]) for n in ("open_points_weights", "open_points_dot", "open_points_reduce") if n in prof}
        dot = ms.get("open_points_dot", float("nan"))
        lines.append("%-8d %12.3f %12.3f %14.1f %12.3f %12.3f" % (k, call_ms, dot, must_read / dot / 1e6,
                                                                 ms.get("open_points_weights", float("nan")),
                                                                 ms.get("open_points_reduce", float("nan"))))
    def find(o, key):
        if isinstance(o, dict):
            for k2, v in o.items():
                if k2 == key:
                    yield v
                yield from find(v, key)
        elif isinstance(o, list):
            for v in o:
                yield from find(v, key)
    # roofline family `openings` of bench.py: the bytes the prover's open_dot launches must move in one proof (each matrix
    # once, its weights once per eight-column group), the time of those launches, and their ratio.  A plain bench run
    # does not write it (`--full` does): then the committed detail file of the last full profile round is quoted.
    fam = None
    for name in ("bench_detail.json", os.path.join("profiles", "r06", "bench_default_detail.json")):
        path = os.path.join(ROOT, name)
        if os.path.exists(path):
            hit = [v for v in find(json.load(open(path)), "openings") if isinstance(v, dict) and "achieved" in v]
            if hit:
                fam = (name, hit[0])
                break
    if fam:
        lines.append("prover's open_dot (%s: one 2^20-row proof, <= 2 points per matrix, natural order): %.3f ms for %.1f MB "
                     "= %.1f GB/s" % (fam[0], fam[1]["ms"], fam[1]["algorithmic_bytes"] / 1e6, fam[1]["achieved"]))
    else:
        lines.append("prover's open_dot: no `openings` family in bench_detail.json (`python bench.py --full` writes it)")
    dm.free()
    ctx.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
