"""Times of the single-direction transforms of the DFT seam on resident KoalaBear matrices, against the fused LDE.
   python tools/time_dft.py [--runs 5] [--sizes 20,15] [--width 64] [--out profiles/r08/dft.txt]

Legs, alternated `--runs` times, each a fresh child process under its own time limit:
  yardstick  p3r_coset_lde_dmat(added_bits = 0, shift = 1): one inverse plus one forward transform.  The library is
             P3R_LIB_PATH's if set (a build of the parent commit), else this tree's - only the entry points every
             build has are bound, so an older library loads.
  dft        forward to BITREV / to NATURAL, inverse from NATURAL / from BITREV, coset inverse (this tree's library).
One more child reads the library's per-kernel profile of the five calls (pass times, and the rate the forward line
pass reaches: it reads and writes the matrix once).  Times are host clock around calls that end in a synchronise."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CALLS = [("forward -> BITREV", dict(inverse=False, bit_reversed=True, shifts=1)),
         ("forward -> NATURAL", dict(inverse=False, bit_reversed=False, shifts=1)),
         ("inverse <- NATURAL", dict(inverse=True, bit_reversed=False, shifts=1)),
         ("inverse <- BITREV", dict(inverse=True, bit_reversed=True, shifts=1)),
         ("coset inverse <- NATURAL", dict(inverse=True, bit_reversed=False, shifts=3))]
REPS = 10


def matrix(log_rows, width):
    import numpy as np
    return np.random.default_rng(log_rows).integers(0, 0x7F000001, size=(1 << log_rows, width), dtype=np.uint32)


def leg_yardstick(sizes, width):
    from plonky3_recursion_amd import _lib, device
    vp = C.c_void_p
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("p3r_create", "p3r_destroy", "p3r_last_error", "p3r_dmat_upload", "p3r_dmat_free", "p3r_coset_lde_dmat", "p3r_sync"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SIGNATURES[name]
    cfg, keep = device.make_config()
    ctx = lib.p3r_create(C.byref(cfg))
    if not ctx:
        raise SystemExit(lib.p3r_last_error(None).decode())
    res = {}
    for n in sizes:
        m = matrix(n, width)
        dm = lib.p3r_dmat_upload(ctx, m.ctypes.data_as(_lib.u32p), m.shape[0], m.shape[1])

        def once():
            out = lib.p3r_coset_lde_dmat(ctx, dm, 0, 1)
            if not out:
                raise SystemExit(lib.p3r_last_error(ctx).decode())
            lib.p3r_dmat_free(ctx, out)   # synchronises
        for _ in range(3):
            once()
        t = time.perf_counter()
        for _ in range(REPS):
            once()
        res["2^%d lde(0, 1)" % n] = (time.perf_counter() - t) / REPS * 1e3
        lib.p3r_dmat_free(ctx, dm)
    lib.p3r_destroy(ctx)
    return res


def leg_dft(sizes, width, profile):
    import plonky3_recursion_amd as p3r
    ctx = p3r.Context(field="koala-bear")
    res = {}
    for n in sizes:
        dm = ctx.upload(matrix(n, width))
        for name, kw in CALLS:
            def once():
                out, = ctx.dft_batch_device([dm], **kw)
                out.free()   # synchronises
            for _ in range(3):
                once()
            if profile:
                ctx.profile_enable(True)
                once()
                for k, v in ctx.profile_read().items():
                    if not k.startswith("stage:"):
                        res["2^%d %s: %s" % (n, name, k)] = v[0]
                ctx.profile_enable(False)
                continue
            t = time.perf_counter()
            for _ in range(REPS):
                once()
            res["2^%d %s" % (n, name)] = (time.perf_counter() - t) / REPS * 1e3
        dm.free()
    ctx.close()
    return res


def child(leg, args, env):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--sizes", args.sizes, "--width", str(args.width)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.step_timeout)
    if out.returncode != 0:
        raise SystemExit("leg %s failed (%d): %s" % (leg, out.returncode, out.stderr[-2000:]))
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sizes", default="20,15")
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--leg", default=None)
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    if args.leg:
        res = leg_yardstick(sizes, args.width) if args.leg == "yardstick" else leg_dft(sizes, args.width, args.leg == "profile")
        print(json.dumps(res))
        return
    own = {k: v for k, v in os.environ.items() if k != "P3R_LIB_PATH"}
    runs = {}
    for _ in range(args.runs):   # a failed or timed-out leg ends the whole measurement (SystemExit / TimeoutExpired)
        for leg, env in (("yardstick", dict(os.environ)), ("dft", own)):
            for k, v in child(leg, args, env).items():
                runs.setdefault(k, []).append(v)
    prof = child("profile", args, own)
    lines = ["KoalaBear, width %d, resident in HBM; ms per call, median of %d alternated runs (min .. max), each run the mean of %d calls"
             % (args.width, args.runs, REPS),
             "yardstick library: %s" % (os.environ.get("P3R_LIB_PATH") or "this tree's")]
    for k, v in runs.items():
        lines.append("  %-34s %8.3f  (%.3f .. %.3f)" % (k, statistics.median(v), min(v), max(v)))
    lines.append("per-kernel times of one call (library profile, ms):")
    for k, v in prof.items():
        lines.append("  %-60s %8.3f" % (k, v))
    for n in sizes:
        key = "2^%d forward -> BITREV: ntt_forward_2" % n
        if key in prof and prof[key] > 0:
            gb = 2 * 4 * args.width * (1 << n) / 1e9
            lines.append("2^%d: the forward line pass reads and writes the matrix once (%.3f GB) in %.3f ms = %.0f GB/s" % (n, gb, prof[key], gb / prof[key] * 1e3))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
