"""Opening what a PCS opens - the bench's 54 query indices over a tree of one 2^22 x 64 LDE (the size of
tools/time_mmcs.py) - through the public MMCS seam, both arities:
  loop    one p3r_mmcs_open per index: one strided 4-byte copy command per opened cell and per sibling word column,
          one wait per index (the only form before p3r_mmcs_open_batch existed)
  batch   p3r_mmcs_open_batch: one gather launch, one copy back, one wait
Median of five alternated runs each, the two forms compared word for word; then the commit of the same matrix with and
without mmcs_salt_elems = 4, and the launch / copy counts of one pass of each form from a `rocprofv3 --kernel-trace
--stats` run of this script in a child process (its own run: tracing slows the host).  Everything is written to --out.
   python tools/time_mmcs_open.py [--log-rows 22] [--width 64] [--indices 54] [--out profiles/r08/mmcs_open_batch.txt]"""
import argparse
import csv
import glob
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import plonky3_recursion_amd as p3r  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log-rows", type=int, default=22)
ap.add_argument("--width", type=int, default=64)
ap.add_argument("--indices", type=int, default=54)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "mmcs_open_batch.txt"))
ap.add_argument("--trace-pass", choices=["loop", "batch"], help="one pass of one form per arity and nothing else (run under the profiler)")
ap.add_argument("--no-trace", action="store_true", help="skip the profiler run")
ap.add_argument("--trace-timeout", type=int, default=240)
args = ap.parse_args()

rng = np.random.default_rng(1)
base = rng.integers(0, 0x7F000001, size=(1 << (args.log_rows - 2), args.width), dtype=np.uint32)
indices = [int(i) for i in rng.integers(0, 1 << args.log_rows, size=args.indices)]
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def make(arity, salt=0):
    ctx = p3r.Context(field="koala-bear", mmcs_arity=arity, mmcs_salt_elems=salt, allow_unpinned_w32_defaults=True)
    return ctx, ctx.coset_lde_batch_device(ctx.upload(base), 2, 3)


def loop_form(tree):
    got = [tree.open_batch(i) for i in indices]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])


def batch_form(tree):
    o, _, p = tree.open_many(indices)
    return o, p


def timed(fn, *a):
    t = time.perf_counter()
    r = fn(*a)       # both forms end in a wait for the device: the host clock measures the call
    return (time.perf_counter() - t) * 1e3, r


if args.trace_pass:
    for arity in (2, 4):
        ctx, lde = make(arity)
        cap, tree = ctx.commit_device([lde])
        (loop_form if args.trace_pass == "loop" else batch_form)(tree)
        tree.free()
        ctx.close()
    sys.exit(0)

say(f"public MMCS opening of {args.indices} indices, tree of one 2^{args.log_rows} x {args.width} matrix, koala-bear; "
    "median of 5 alternated runs (min .. max), host clock around calls that end in a device wait")
for arity in (2, 4):
    ctx, lde = make(arity)
    cap, tree = ctx.commit_device([lde])
    depth = ctx.lib.p3r_tree_proof_len(tree.h)
    a, b = loop_form(tree), batch_form(tree)     # warm-up of both, and the comparison
    same = all(np.array_equal(x, y) for x, y in zip(a, b))
    t_loop, t_batch = [], []
    for _ in range(5):
        t_loop.append(timed(loop_form, tree)[0])
        t_batch.append(timed(batch_form, tree)[0])
    ml, mb = statistics.median(t_loop), statistics.median(t_batch)
    say(f"arity {arity}: proof_len {depth}; outputs {'identical' if same else 'DIFFER'}")
    say(f"  loop of p3r_mmcs_open : {ml:9.3f} ms ({min(t_loop):.3f} .. {max(t_loop):.3f}); from the code: "
        f"{args.indices * (1 + depth)} strided copy commands ({args.indices} x (1 matrix + {depth} siblings), "
        f"{args.indices * (args.width + depth * 8)} cells of 4 bytes), {args.indices} waits")
    say(f"  p3r_mmcs_open_batch   : {mb:9.3f} ms ({min(t_batch):.3f} .. {max(t_batch):.3f}); from the code: 1 gather launch, "
        "2 small uploads (item list, indices), 1 copy back, 1 wait")
    say(f"  batch / loop = {mb / ml:.3f}" + ("" if mb < ml else "   <- the batch form is NOT faster here"))
    tree.free()
    # the commit with and without salts, alternated between two contexts on the same matrix contents
    sctx, slde = make(arity, salt=4)
    for c, l in ((ctx, lde), (sctx, slde)):
        c.commit_device([l])[1].free()
    t_plain, t_salt = [], []
    for _ in range(5):
        for c, l, acc in ((ctx, lde, t_plain), (sctx, slde, t_salt)):
            c.sync()
            t = time.perf_counter()
            cap, tr = c.commit_device([l])    # returns the cap: the commit has finished
            acc.append((time.perf_counter() - t) * 1e3)
            tr.free()
    say(f"  commit, plain         : {statistics.median(t_plain):9.3f} ms ({min(t_plain):.3f} .. {max(t_plain):.3f})")
    say(f"  commit, salt_elems = 4: {statistics.median(t_salt):9.3f} ms ({min(t_salt):.3f} .. {max(t_salt):.3f})")
    slde.free(); sctx.close()
    lde.free(); ctx.close()


def trace(form):
    """One pass of `form` (both arities) in a fresh child process under the profiler; kernel and copy counts by name."""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    out = tempfile.mkdtemp(prefix="mmcs_open_trace_")
    cmd = [prof, "--kernel-trace", "--memory-copy-trace", "--stats", "-d", out, "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--trace-pass", form, "--log-rows", str(args.log_rows),
           "--width", str(args.width), "--indices", str(args.indices)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.trace_timeout)
    except (OSError, subprocess.TimeoutExpired) as e:
        say(f"  {form}: profiler run not completed ({type(e).__name__}): counts not measured")
        return
    if r.returncode != 0:
        say(f"  {form}: profiler run failed (rc {r.returncode}): counts not measured; {r.stderr.strip()[-300:]}")
        return
    found = False
    for kind in ("kernel_stats", "memory_copy_stats"):
        for path in glob.glob(os.path.join(out, "**", f"*{kind}.csv"), recursive=True):
            found = True
            rows = list(csv.DictReader(open(path)))
            total = sum(int(x.get("Calls", 0) or 0) for x in rows)
            say(f"  {form}: {kind}: {total} calls in all (whole pass: LDE, commit and the openings of both arities)")
            for x in rows:
                name = x.get("Name", "?")
                if kind == "memory_copy_stats" or "open_batch" in name or "copy" in name.lower() or "Cpy" in name:
                    say(f"      {int(x.get('Calls', 0) or 0):7d} x {name[:110]}")
    if not found:
        say(f"  {form}: the profiler wrote no stats file: counts not measured")
    shutil.rmtree(out, ignore_errors=True)


if not args.no_trace:
    say("launches and copies of one pass per form (rocprofv3 --kernel-trace --memory-copy-trace --stats, a run of its own):")
    for form in ("loop", "batch"):
        trace(form)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
