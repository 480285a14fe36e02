"""Digests of the oracle's proof bytes for a fixed list of small layers -> tests/golden/proof_digests.json.
   python3 tools/gen_proof_digests.py
   python3 tools/gen_proof_digests.py --large [--only NAME[,NAME]]    -> tests/golden/proof_digests_large.json
   python3 tools/gen_proof_digests.py --arity16 [--only NAME[,NAME]]  -> tests/golden/proof_digests_arity16.json
   python3 tools/gen_proof_digests.py --check NAME[,NAME] | all       regenerate and compare, write nothing
   python3 tools/gen_proof_digests.py --arity16 --check all           the same for the arity-16 fixture
Not a parity pin (the reference holds no proof bytes): a DRIFT pin.  The oracle, the generator and
the device prover change together from round to round; these digests make a change of the proof bytes of an existing
configuration visible in review instead of silently re-agreeing with itself.  `workload` is the digest of the
generator's arrays, so a generator change is told apart from a prover change.

--large: LARGE_CASES, the layers of 2^14 to 2^20 rows the metric and the bench legs are quoted on, with the reference
examples' FRI defaults.  CPU only (the oracle under OpenMP; minutes per case at 2^20).  The oracle's grinding takes the
smallest witness and its FRI schedule is the reference's rule, so at these sizes the digests are a PARITY pin for the
device prover: the branches it only takes there (balanced NTT splits, multi-launch Merkle levels, multi-tile scans and
sorts) must give the oracle's bytes, not merely bytes a verifier accepts.  --arity16: ARITY16_CASES, the bench workload
and the arity-4-MMCS recursion layer under max_log_arity = 4 (FRI folding by 16, the reference's documented default), in
a fixture of their own with the same record shape.  Next to the whole-proof digest every entry
holds one digest per decoded section of the proof (tests/proof_codec.py), in protocol order, so that a mismatch names
the first phase that differs.  One child process per case, so that `peak_rss_gb` is the case's own."""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = [
    # name, field, log_h, seed, flags, circuit degree, challenge degree, FRI parameters, packing
    ("d4_default", "koala-bear", 7, 11, 0, 4, 4, dict(log_blowup=2, max_log_arity=2, log_final_poly_len=2, query_pow_bits=4, num_queries=6), {}),
    ("d4_babybear_cap2", "baby-bear", 8, 12, 0, 4, 4, dict(log_blowup=1, max_log_arity=3, log_final_poly_len=1, cap_height=2, commit_pow_bits=2, query_pow_bits=3, num_queries=5),
     dict(public_lanes=2, alu_lanes=2, horner_packed_steps=3)),
    ("d4_recompose_coeff", "koala-bear", 7, 13, 32, 4, 4, dict(log_blowup=2, max_log_arity=1, log_final_poly_len=1, query_pow_bits=3, num_queries=4), {}),
    ("d1_base_field", "baby-bear", 7, 14, 0, 1, 4, dict(log_blowup=2, max_log_arity=2, log_final_poly_len=1, query_pow_bits=3, num_queries=4), dict(alu_lanes=1, horner_packed_steps=2)),
    ("d5_backend_tables", "koala-bear", 8, 15, 64, 5, 4, dict(log_blowup=2, max_log_arity=2, log_final_poly_len=2, query_pow_bits=4, num_queries=5), {}),
    ("d5_quintic_challenge", "koala-bear", 8, 16, 64, 5, 5, dict(log_blowup=2, max_log_arity=2, log_final_poly_len=2, query_pow_bits=4, num_queries=5),
     dict(public_lanes=1, alu_lanes=8, horner_packed_steps=2)),
    ("d1_quintic_challenge", "koala-bear", 7, 17, 2, 1, 5, dict(log_blowup=1, max_log_arity=2, log_final_poly_len=1, query_pow_bits=3, num_queries=4), {}),
    ("d4_arity4_mmcs", "koala-bear", 7, 19, 0, 4, 4, dict(log_blowup=2, max_log_arity=2, log_final_poly_len=1, query_pow_bits=3, num_queries=4, mmcs_arity=4), {}),
    ("d4_arity4_mmcs_w32_table", "baby-bear", 7, 20, 128, 4, 4, dict(log_blowup=1, max_log_arity=3, log_final_poly_len=1, query_pow_bits=3, num_queries=4, mmcs_arity=4), {}),
    # round 6: the width-32 rows as ops of the circuit (flag 4096 | 128), under the arity-4 MMCS: the arrays are the generator's own books
    ("d4_arity4_w32_ops", "koala-bear", 7, 21, 4096 | 128, 4, 4, dict(log_blowup=2, max_log_arity=2, log_final_poly_len=1, query_pow_bits=3, num_queries=4, mmcs_arity=4), {}),
    ("d8_binomial", "koala-bear", 7, 18, 1, 8, 4, dict(log_blowup=2, max_log_arity=2, log_final_poly_len=1, query_pow_bits=3, num_queries=4), dict(ext_w=3)),
]
GEN = dict(horner_chain_len=12, sponge_chain_len=3, merkle_depth=4)


def layer(oracle, case):
    import harness_lib
    import layer_lib
    name, field, log_h, seed, flags, d, dc, fri, packing = case
    arrs = harness_lib.generate(field, log_h, seed=seed, flags=flags, ext_degree=d, **GEN)
    prm = layer_lib.params(challenge_degree=dc, **fri)
    pk = dict(packing, ext_degree=d, recompose_coeff_lookups=1 if flags & harness_lib.RECOMPOSE_COEFF else 0)
    return arrs, prm, layer_lib.OracleLayer(oracle, field, arrs, prm, packing=pk)


def workload_digest(arrs):
    """sha256 over the generator's arrays.  Arrays added after the pins were made (the width-32 Poseidon2 table's,
    round 4) are left out while they are empty, and `counts` is hashed without its trailing zero entries for such
    tables - so the pins of the older layers keep telling a generator change apart from a layout extension."""
    late = ("p2w_inputs", "p2w_flags", "p2w_mmcs_index_sum", "p2w_prep", "pdw_op_ids", "pdw_siblings")   # (pdw_*: round 6)
    h = hashlib.sha256()
    for k in sorted(arrs):
        a = arrs[k]
        if k in late and not len(a):
            continue
        if k == "counts" and len(a) > 7 and not a[7:].any():
            a = a[:7]
        h.update(k.encode())
        h.update(a.tobytes())
    return h.hexdigest()


# ---- the large cases -------------------------------------------------------------------------------------------------
FRI = dict(log_blowup=2, max_log_arity=2, cap_height=0, log_final_poly_len=5, commit_pow_bits=0, query_pow_bits=15,
           num_queries=54)   # the reference examples' defaults (= bench.py, tests/test_gpu_headline.py)
GEN_KNOBS = dict(horner_chain_len=64, sponge_chain_len=8, merkle_depth=20)
CONFIG2_KNOBS = dict(horner_chain_len=2600, sponge_chain_len=330, merkle_depth=20)
ZK_KEY = [0x5EED0021, 0x9E3779B9, 0x7F4A7C15, 0x0badc0de, 0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344]
LARGE_PATH = os.path.join(ROOT, "tests", "golden", "proof_digests_large.json")
RECORDED = ("oracle_seconds", "threads", "peak_rss_gb")   # written, never compared


def _large(name, field, log_h, seed=0x5EED0000, flags=0, gen=GEN_KNOBS, d=4, circuit=True, **prm):
    """`prm`: what differs from FRI in layer_lib.params (and in the device Context).  `circuit`: the layer also exists
    as a circuit + inputs the oracle's sequential runner takes (D = 4), i.e. both device seams can be driven."""
    return dict(name=name, field=field, log_h=log_h, seed=seed, flags=flags, gen=gen, d=d, circuit=circuit, prm=prm)


LARGE_CASES = [
    # the bench workload (bench.py's headline leg, tests/test_gpu_headline.py) from 2^14 rows to the size of the metric
    _large("kb_headline_14", "koala-bear", 14),
    _large("kb_headline_16", "koala-bear", 16),
    _large("kb_headline_18", "koala-bear", 18),
    _large("kb_headline_20", "koala-bear", 20),
    _large("bb_headline_20", "baby-bear", 20),
    # config-2 knobs: tests/test_gpu_large.py::test_keccak_like_mix_long_chains, and bench.py's config-2 leg
    _large("kb_config2_15", "koala-bear", 15, seed=5, gen=CONFIG2_KNOBS),
    _large("kb_config2_17", "koala-bear", 17, flags=16, gen=CONFIG2_KNOBS),                     # INDEPENDENT_SPONGES
    # the arity-4 MMCS over the width-32 permutation: the headline circuit, and the arity-4 recursion layer of bench.py
    _large("kb_arity4_16", "koala-bear", 16, mmcs_arity=4),
    _large("kb_arity4_w32_ops_16", "koala-bear", 16, seed=0x5EED0032, flags=4096 | 128, mmcs_arity=4),   # P2_W32_OPS
    # D = 5 circuit, both Recompose tables, quintic challenge field (bench.py's quintic_challenge_layer)
    _large("kb_d5_quintic_16", "koala-bear", 16, seed=0x5EED0005, flags=64, d=5, circuit=False, challenge_degree=5),
    # HidingFriPcs under a fixed key, proof number 0 (tests/test_gpu_zk.py::make_ctx); with the hiding MMCS on top
    _large("kb_zk_16", "koala-bear", 16, zk=1, num_random_codewords=2, zk_key=ZK_KEY),
    _large("kb_zk_hiding_16", "koala-bear", 16, zk=1, num_random_codewords=2, zk_key=ZK_KEY, mmcs_salt_elems=4),
]
LARGE_BY_NAME = {c["name"]: c for c in LARGE_CASES}

# max_log_arity = 4: the bench workload at 2^14, 2^16 and 2^20 rows, and the arity-4-MMCS recursion layer at 2^16.  Each folds
# by 16 once the last table height is rolled in (2^14 rows: log_arity 1, 1, 2, 4, 1 - heights 2^16, 2^15, 2^14, 2^12, then
# 2^12 -> 2^8 -> the final 2^7); tests/test_fri_arity16.py asserts it on the decoded proof.
ARITY16_PATH = os.path.join(ROOT, "tests", "golden", "proof_digests_arity16.json")
ARITY16_CASES = [
    _large("kb_headline_14_la4", "koala-bear", 14, max_log_arity=4),
    _large("kb_headline_16_la4", "koala-bear", 16, max_log_arity=4),
    _large("kb_headline_20_la4", "koala-bear", 20, max_log_arity=4),
    _large("kb_arity4_w32_ops_16_la4", "koala-bear", 16, seed=0x5EED0032, flags=4096 | 128, mmcs_arity=4, max_log_arity=4),
]
ARITY16_BY_NAME = {c["name"]: c for c in ARITY16_CASES}


def fri_log_arities(proof, case):
    """The log2 arities of the commit phases, read off the first query of the proof."""
    import proof_codec
    p = proof_codec.decode(proof, **large_codec_kw(case))
    return [s["log_arity"] for s in p["opening_proof"]["query_proofs"][0]["commit_phase_openings"]]


def sha_json(x):
    return hashlib.sha256(json.dumps(x, separators=(",", ":")).encode()).hexdigest()


def large_codec_kw(case):
    prm = case["prm"]
    return dict(dc=prm.get("challenge_degree", 4), zk=bool(prm.get("zk")), salted=bool(prm.get("mmcs_salt_elems")))


def sections(proof, case):
    """Ordered (protocol order) name -> sha256 of every decoded part of the proof (field elements as the words the
    proof holds).  The whole proof must decode: a trailing or missing byte is an error here, not a digest."""
    import proof_codec
    p = proof_codec.decode(proof, **large_codec_kw(case))
    if p["_consumed"] != len(proof):
        raise ValueError(f"proof of {len(proof)} bytes decodes to {p['_consumed']}")
    fri = p["opening_proof"]
    out = {"degree_bits": sha_json(p["degree_bits"])}
    for k in ("main", "permutation"):
        out["commitments." + k] = sha_json(p["commitments"][k])
    out["lookup_terminals"] = sha_json(p["lookup_terminals"])
    for k in ("quotient", "random"):
        out["commitments." + k] = sha_json(p["commitments"][k])
    out["opened"] = sha_json(p["opened"])
    if "random_opened_values" in fri:
        out["random_opened_values"] = sha_json(fri["random_opened_values"])
    for i, c in enumerate(fri["commit_phase_commits"]):
        out["commit_phase_commits[%d]" % i] = sha_json(c)
    out["commit_pow_witnesses"] = sha_json(fri["commit_pow_witnesses"])
    out["final_poly"] = sha_json(fri["final_poly"])
    out["query_pow_witness"] = sha_json(fri["query_pow_witness"])
    out["query_proofs[0]"] = sha_json(fri["query_proofs"][0])
    out["query_proofs"] = sha_json(fri["query_proofs"])
    return out


def first_difference(pin_sections, got_sections):
    """The first section, in protocol order, whose digest differs (or that one side lacks); None if all agree."""
    for k in list(pin_sections) + [k for k in got_sections if k not in pin_sections]:
        if pin_sections.get(k) != got_sections.get(k):
            return k
    return None


def describe_mismatch(pin, proof, case):
    """For a failing assertion: where a proof departs from the pinned one, by `sections`."""
    try:
        got = sections(proof, case)
    except Exception as e:   # noqa: BLE001 - a proof that does not even decode is reported as such
        return f"{case['name']}: the proof does not decode: {e}"
    first = first_difference(pin["sections"], got)
    same = [k for k in pin["sections"] if got.get(k) == pin["sections"][k]]
    if first is None:
        return (f"{case['name']}: proof digest differs from the pin but every one of its sections agrees "
                f"({len(same)}): the fixture's `proof` and `sections` disagree with each other")
    return (f"{case['name']}: first differing sections entry: {first!r} "
            f"(agreeing: {', '.join(same) if same else 'none'}; {len(proof)} bytes, pinned {pin['proof_bytes']})")


def large_arrays(case):
    import harness_lib
    return harness_lib.generate(case["field"], case["log_h"], seed=case["seed"], flags=case["flags"], ext_degree=case["d"],
                                **case["gen"])


def large_params(case, **over):
    import layer_lib
    return layer_lib.params(**dict(FRI, **case["prm"], **over))


def large_layer(oracle, case, arrs, **over):
    import layer_lib
    pk = dict(ext_degree=case["d"]) if case["d"] != 4 else None
    return layer_lib.OracleLayer(oracle, case["field"], arrs, large_params(case, **over), packing=pk)


def omp_threads(oracle=None):
    """The OpenMP team the oracle runs with: OMP_NUM_THREADS if set, else what the OpenMP runtime itself reports (which
    respects the process's affinity mask).  Never the machine's CPU count."""
    env = os.environ.get("OMP_NUM_THREADS", "").split(",")[0].strip()
    if env.isdigit() and int(env) > 0:
        return int(env)
    try:
        return int(oracle.lib.omp_get_max_threads())
    except Exception:   # noqa: BLE001 - an oracle built without OpenMP runs one thread
        return len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 1


_CONSUMED = ("const_values", "const_prep", "public_values", "public_prep", "alu_values", "alu_prep13", "p2_inputs", "p2_flags",
             "p2_mmcs_index_sum", "p2_in_ctl", "p2_input_indices", "p2_out_ctl", "p2_output_indices", "p2_mmcs_index_sum_idx",
             "recompose_values", "recompose_prep", "recompose_coeff_values", "recompose_coeff_prep", "p2w_inputs", "p2w_flags",
             "p2w_mmcs_index_sum", "p2w_prep")   # what layer_lib.fill_workload reads at D = 4 (p2_absorb_len: D != 4 only)


def circuit_arrays(oracle, case, arrs):
    """The oracle's own circuit seam: preprocess + sequential run of the circuit the generator emitted, then the arrays
    prove_all_tables consumes (tests/test_gpu_large.py::test_circuit_run_and_prove_at_scale)."""
    import circuit_lib as cl
    import oracle_lib
    oc = cl.OracleCircuit(oracle, cl.Circuit.from_arrays(arrs)).preprocess(oracle_lib.MODULUS[case["field"]])
    oc.run(case["field"], cl.Inputs.from_arrays(arrs))
    return oc.workload_arrays()


def same_layer_inputs(a, b):
    import numpy as np
    ca, cb = ([int(x) for x in list(c[:8]) + [0] * (8 - len(c[:8]))] for c in (a["counts"], b["counts"]))
    if ca[:5] + ca[6:] != cb[:5] + cb[6:]:
        return False
    empty = np.zeros(0, np.uint32)
    return all(np.array_equal(a.get(k, empty), b.get(k, empty)) for k in _CONSUMED)


def large_entry(oracle, case):
    """One fixture entry, from the oracle alone."""
    import resource
    t0 = time.perf_counter()
    arrs = large_arrays(case)
    entry = {"workload": workload_digest(arrs)}
    L = large_layer(oracle, case, arrs)
    entry["prep_commit"] = hashlib.sha256(L.prep_commit().tobytes()).hexdigest()
    proof = L.prove()
    entry["proof_bytes"] = len(proof)
    entry["proof"] = hashlib.sha256(proof).hexdigest()
    entry["sections"] = sections(proof, case)
    L.verify(proof)
    if case["circuit"]:
        # both device seams must be pinned by ONE number: the arrays the oracle's circuit run produces give this proof.
        # Equal layer inputs give equal bytes (the oracle is deterministic: --check); unequal ones are proved and compared.
        want = circuit_arrays(oracle, case, arrs)
        if same_layer_inputs(arrs, want):
            entry["circuit_seam"] = "the oracle's circuit run reproduces the generator's layer arrays cell for cell"
        else:
            del L
            other = large_layer(oracle, case, want).prove()
            if hashlib.sha256(other).hexdigest() != entry["proof"]:
                raise SystemExit(case["name"] + ": the circuit's arrays and the generator's give different proofs: "
                                 + describe_mismatch(entry, other, case))
            entry["circuit_seam"] = "the oracle's circuit run gives other layer arrays and the same proof bytes"
    else:
        entry["circuit_seam"] = None
    entry["oracle_seconds"] = round(time.perf_counter() - t0, 1)
    entry["threads"] = omp_threads(oracle)
    entry["peak_rss_gb"] = round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20, 2)
    return entry


def _child_entry(name):
    import subprocess
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--emit", name], stdout=subprocess.PIPE, check=True)
    return json.loads(out.stdout.decode().strip().splitlines()[-1])


def _names(arg, cases=LARGE_CASES):
    known = [c["name"] for c in cases]
    names = known if arg in (None, "all") else [n for n in arg.split(",") if n]
    for n in names:
        if n not in known:
            raise SystemExit(f"unknown case {n!r}; known: {', '.join(known)}")
    return names


def compare_entries(pin, got):
    """Keys of `pin` / `got` that differ, recorded measurements aside."""
    return [k for k in sorted(set(pin) | set(got)) if k not in RECORDED and pin.get(k) != got.get(k)]


def main_large(only=None, check=None, path=LARGE_PATH, cases=LARGE_CASES):
    fixture = json.load(open(path)) if os.path.exists(path) else {"provenance": {}, "cases": {}}
    if check is not None:
        bad = 0
        for n in _names(check, cases):
            if n not in fixture["cases"]:
                print(f"{n}: not in the fixture")
                bad += 1
                continue
            got = _child_entry(n)
            diff = compare_entries(fixture["cases"][n], got)
            if "sections" in diff:
                diff.append("first section: %r" % first_difference(fixture["cases"][n]["sections"], got["sections"]))
            print(f"{n}: {'DIFFERS in ' + ', '.join(diff) if diff else 'agrees'} ({got['oracle_seconds']} s, {got['threads']} threads)",
                  flush=True)
            bad += bool(diff)
        sys.exit(1 if bad else 0)
    for n in _names(only, cases):   # written after every case: a case is minutes of work
        fixture["cases"][n] = _child_entry(n)
        print(f"{n}: {fixture['cases'][n]['proof_bytes']} bytes, {fixture['cases'][n]['oracle_seconds']} s", flush=True)
        fixture = _write_large(fixture, path, cases)


def _write_large(fixture, path=LARGE_PATH, cases=LARGE_CASES):
    prov = fixture["provenance"] if isinstance(fixture.get("provenance"), dict) else {}
    prov["tool"] = ("tools/gen_proof_digests.py " + ("--large" if path == LARGE_PATH else "--arity16") + ": sha256 of the CPU oracle's prove_batch bytes (Montgomery encoding), of the "
                    "preprocessed commitment and of every decoded section of the proof; digests only, no proof bytes. "
                    "oracle_seconds / threads / peak_rss_gb are recorded, not asserted")
    prov.setdefault("records", [])   # hand-kept: what was checked, and what was left out and why
    order = [c["name"] for c in cases]
    fixture = {"provenance": prov, "cases": {n: fixture["cases"][n] for n in order if n in fixture["cases"]}}
    with open(path, "w") as fh:
        json.dump(fixture, fh, indent=1)
        fh.write("\n")
    print("wrote", path, flush=True)
    return fixture


def main():
    import oracle_lib
    oracle = oracle_lib.Oracle()
    out = {"provenance": "tools/gen_proof_digests.py: sha256 of the oracle's prove_batch bytes (Montgomery and canonical "
                         "encodings) and of the preprocessed commitment; a drift pin, not a parity pin",
           "cases": {}}
    for case in CASES:
        arrs, prm, L = layer(oracle, case)
        out["cases"][case[0]] = {
            "workload": workload_digest(arrs),
            "prep_commit": hashlib.sha256(L.prep_commit().tobytes()).hexdigest(),
            "proof": hashlib.sha256(L.prove()).hexdigest(),
            "proof_canonical": hashlib.sha256(L.prove(field_encoding=1)).hexdigest(),
            "proof_bytes": len(L.prove()),
        }
    path = os.path.join(ROOT, "tests", "golden", "proof_digests.json")
    json.dump(out, open(path, "w"), indent=1)
    print("wrote", path)


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--large", action="store_true", help="write tests/golden/proof_digests_large.json (CPU only)")
    ap.add_argument("--arity16", action="store_true",
                    help="write tests/golden/proof_digests_arity16.json: max_log_arity = 4 (CPU only); with --check, re-derive it")
    ap.add_argument("--only", metavar="NAME[,NAME]", help="--large: regenerate these cases only, keep the others")
    ap.add_argument("--check", metavar="NAME[,NAME]", help="regenerate these large cases (or `all`) and compare; writes nothing")
    ap.add_argument("--emit", metavar="NAME", help=argparse.SUPPRESS)   # the child of --large / --check: one entry on stdout
    args = ap.parse_args()
    if args.emit:
        import oracle_lib
        print(json.dumps(large_entry(oracle_lib.Oracle(), dict(LARGE_BY_NAME, **ARITY16_BY_NAME)[args.emit])))
    elif args.arity16:
        main_large(only=args.only, check=args.check, path=ARITY16_PATH, cases=ARITY16_CASES)
    elif args.large or args.check or args.only:
        main_large(only=args.only, check=args.check)
    else:
        main()
