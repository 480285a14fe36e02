"""What the FRI folding arity costs and saves on the bench workload: for max_log_arity 2, 3 and 4 (folding by at most 4, 8
and 16) at 2^15 and 2^20 KoalaBear rows - warm ms per prove_next_layer with the circuit prepared and the inputs resident
(PreparedCircuit.prove = p3r_prove_next_layer_resident, bench.py's step; median of the steps), proof bytes, the number of
commit phases and their log-arities, and the fri_fold / mmcs_hash_rows_strided / mmcs_compress family times of one
profiled proof (p3r_profile_read).  One process, one layer at a time.  No threshold: a record (profiles/r07/fri_arity.txt).

usage: python tools/fri_arity_ab.py [--log-rows 15,20] [--arities 2,3,4] [--steps 7] [--out FILE]     (needs a GPU)
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

# the bench workload and the reference examples' FRI defaults (bench.py, tools/gen_proof_digests.py --large)
FRI = dict(log_blowup=2, cap_height=0, log_final_poly_len=5, commit_pow_bits=0, query_pow_bits=15, num_queries=54)
GEN_KNOBS = dict(horner_chain_len=64, sponge_chain_len=8, merkle_depth=20)
FAMILIES = ("fri_fold", "mmcs_hash_rows_strided", "mmcs_compress")


def measure(log_rows, max_log_arity, steps):
    import harness_adapters as wl
    import harness_lib
    import plonky3_recursion_amd as p3r
    import proof_codec
    arrs = harness_lib.generate("koala-bear", log_rows, seed=0x5EED0000, **GEN_KNOBS)
    ctx = p3r.Context(field="koala-bear", max_log_arity=max_log_arity, **FRI)
    tp = p3r.TablePacking().with_fri_params(FRI["log_final_poly_len"], FRI["log_blowup"])
    pc = p3r.PreparedCircuit(ctx, wl.circuit_from_arrays(arrs), tp)
    res = pc.upload_inputs(wl.circuit_inputs_from_arrays(arrs))
    proof = pc.prove(res)   # warm-up: tables, caches, the pool
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        pc.prove(res)
        ms.append((time.perf_counter() - t0) * 1e3)
    ctx.profile_enable(True)
    pc.prove(res)
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    p3r.BatchStarkProver(ctx).verify_all_tables(p3r.BatchStarkProver(ctx).wrap_proof(proof, pc.circuit_prover_data))
    las = [s["log_arity"] for s in proof_codec.decode(proof)["opening_proof"]["query_proofs"][0]["commit_phase_openings"]]
    res.free()
    pc.free()
    ctx.close()
    fam = {f: prof.get(f, (0.0, 0)) for f in FAMILIES}
    return dict(log_rows=log_rows, max_log_arity=max_log_arity, ms=statistics.median(ms), ms_min=min(ms), ms_max=max(ms),
                proof_bytes=len(proof), log_arities=las, families=fam)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--log-rows", default="15,20")
    ap.add_argument("--arities", default="2,3,4")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also append the table to this file")
    args = ap.parse_args()
    lines = ["FRI folding arity on the bench workload (KoalaBear, blow-up 4, final polynomial 2^5, 54 queries), %d warm steps per row;"
             % args.steps,
             "ms/proof: PreparedCircuit.prove over resident inputs (p3r_prove_next_layer_resident, the step bench.py times);",
             "family times: total ms (launches) of ONE profiled proof, profiling on (its launches are serialised)",
             "%8s %13s %9s %17s %11s %6s  %-22s %15s %23s %15s" % ("rows", "max_log_arity", "ms/proof", "(min - max)", "proof bytes",
                                                                    "phases", "log_arity per phase", "fri_fold", "mmcs_hash_rows_strided",
                                                                    "mmcs_compress")]
    print("\n".join(lines), flush=True)
    for lr in (int(x) for x in args.log_rows.split(",")):
        for la in (int(x) for x in args.arities.split(",")):
            r = measure(lr, la, args.steps)
            f = r["families"]
            line = "%8s %13d %9.2f %17s %11d %6d  %-22s %15s %23s %15s" % (
                "2^%d" % lr, la, r["ms"], "(%.2f - %.2f)" % (r["ms_min"], r["ms_max"]), r["proof_bytes"], len(r["log_arities"]),
                ",".join(str(x) for x in r["log_arities"]), *("%.3f (%d)" % f[k] for k in FAMILIES))
            print(line, flush=True)
            lines.append(line)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
