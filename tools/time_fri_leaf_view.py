"""Time of the commit-phase leaf view at the public seam (p3r_fri_leaf_view_dmat, k_fri_leaf_view) and of one commit
phase through the seam (leaf view + p3r_mmcs_commit_dmat) on a resident KoalaBear vector.
   python tools/time_fri_leaf_view.py [--log-rows 22] [--log-arity 2] [--reps 10] [--out FILE]

The kernel is a pure copy: it must read n * DC words once and write n * DC words once, so its time is set against
2 * n * DC * 4 bytes.  At n = 2^22, DC = 4 that is 134 MB - less than the 256 MiB last-level cache, and every repetition
reads the same vector, so the rate is an upper estimate of a cold pass.  The commit phase lists every launch the library
timed (p3r_profile_read) while the view was taken and committed.
Nothing here is a threshold; the numbers go to profiles/<round>/fri_leaf_view.txt."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", type=int, default=22)
    ap.add_argument("--log-arity", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--challenge-degree", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import plonky3_recursion_amd as p3r

    p, dc, la = 0x7F000001, a.challenge_degree, a.log_arity
    ctx = p3r.Context(field="koala-bear", challenge_degree=dc)
    n = 1 << a.log_rows
    vec = ctx.upload(np.random.default_rng(a.log_rows).integers(0, p, size=(n, dc), dtype=np.uint32))

    def timed(fn):
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
        prof = {k: v for k, v in ctx.profile_read().items() if not k.startswith("stage:")}   # launches only
        ctx.profile_enable(False)
        return call_ms, {k: v[0] / max(1, v[1]) for k, v in prof.items()}, {k: v[1] / a.reps for k, v in prof.items()}

    call_ms, ms, _ = timed(lambda: ctx.fri_leaf_view_device(vec, la).free())
    must = 2 * n * dc * 4
    k_ms = ms["fri_seam_leaf_view"]
    lines = ["leaf view of a %d x %d KoalaBear vector, log_arity %d -> %d x %d" % (n, dc, la, n >> la, dc << la),
             "bytes the copy must move: %.1f MB read + %.1f MB written = %.1f MB (below the 256 MiB last-level cache: an upper estimate"
             " of a cold pass)" % (must / 2e6, must / 2e6, must / 1e6),
             "%-24s %10s %12s %18s" % ("", "ms", "GB/s", "of 6300 GB/s HBM"),
             "%-24s %10.3f" % ("call (host, with free)", call_ms),
             "%-24s %10.3f %12.1f %18.2f" % ("fri_seam_leaf_view", k_ms, must / k_ms / 1e6, must / k_ms / 1e6 / 6300)]

    def phase():
        view = ctx.fri_leaf_view_device(vec, la)
        _, tree = ctx.commit_device([view])
        tree.free()
        view.free()

    call_ms, ms, per_call = timed(phase)
    lines += ["", "one commit phase through the seam: leaf view + commit_device of the %d x %d view" % (n >> la, dc << la),
              "%-24s %10.3f" % ("call (host, with frees)", call_ms),
              "%-24s %10s %10s" % ("launch", "ms each", "per phase")]
    total = 0.0
    for k in sorted(ms):
        lines.append("%-24s %10.3f %10.1f" % (k, ms[k], per_call[k]))
        total += ms[k] * per_call[k]
    lines.append("%-24s %10.3f   (the view is %.1f %% of it)" % ("sum of the launches", total, 100 * k_ms / total))
    vec.free()
    ctx.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
