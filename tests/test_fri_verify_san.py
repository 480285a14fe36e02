"""CPU: p3r_fri_verify under the address and undefined-behaviour sanitizers, as a stand-alone program
(tests/fri_verify_san_main.cpp over the HIP-free csrc/fri_verify_abi.h, compiled here with g++; nothing is preloaded).
The test writes one accepted CPU-made proof to a file; the program applies a few thousand structure-aware mutations to it
- words changed, lengths shortened, counts raised - and every result must be P3R_OK, P3R_EINVAL or P3R_EVERIFY."""
import os
import subprocess

import numpy as np
import pytest

import fri_verify_ref as fv
import test_fri_verify_host as host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "plonky3_recursion_amd", "csrc")
N_MUTANTS = 4000


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("fri_verify_san")), "fri_verify_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "fri_verify_san_main.cpp"), "-o", out], check=True)
    return out


def words_of(field, dc, prm, proof, views):
    w = [0 if field == "koala-bear" else 1, dc, prm["log_blowup"], prm["max_log_arity"], prm["cap_height"], prm["log_final_poly_len"],
         prm["commit_pow_bits"], prm["query_pow_bits"], prm["num_queries"], prm["mmcs_arity"], 0]

    def vec(a):
        a = np.asarray(a, dtype=np.uint32).reshape(-1)
        w.append(a.size)
        w.extend(int(x) for x in a)

    vec([1, 2, 3])
    w.extend([proof.log_max_height, proof.query_pow_witness])
    vec(proof.log_arities)
    vec(np.concatenate([c.reshape(-1) for c in proof.commit_phase_caps]))
    vec(proof.commit_pow_witnesses)
    vec(proof.final_poly)
    w.append(len(proof.query_openings))
    for q, openings in enumerate(proof.query_openings):
        shift = 0
        for la, o in zip(proof.log_arities, openings):
            pos = (proof.query_indices[q] >> shift) & ((1 << la) - 1)
            shift += la
            vec(np.delete(o.row, pos, axis=0))
            vec([])
            vec(o.siblings)
    w.append(len(views))
    for log_h, values in views:
        w.append(log_h)
        vec(values)
    return np.array(w, dtype="<u4")


@pytest.mark.parametrize("field,over", [("koala-bear", dict(max_log_arity=2, cap_height=1, commit_pow_bits=2, query_pow_bits=2)),
                                        ("baby-bear", dict(max_log_arity=4, log_final_poly_len=0, mmcs_arity=4))])
def test_mutants_are_refused_or_rejected_cleanly(oracle, exe, tmp_path, field, over):
    prm = host.params(**over)
    proof, ins, _ = host.prove(oracle, field, 4, prm)
    path = os.path.join(str(tmp_path), "proof.u32")
    words_of(field, 4, prm, proof, fv.input_values(ins, proof.query_indices)).tofile(path)
    r = subprocess.run([exe, path, str(N_MUTANTS)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    got = dict(zip(r.stdout.split()[0::2], map(int, r.stdout.split()[1::2])))
    assert got["mutants"] == N_MUTANTS and got["refused"] > 100 and got["rejected"] > 100, r.stdout
