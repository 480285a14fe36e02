"""CPU: the one postcard grammar of a BatchProof (csrc/proof_grammar.h) through its two sinks - the checking sink behind
p3r_batch_proof_len_layout and p3r_batch_stark_proof_parse, the building sink behind p3r_verify_batch - on oracle proofs
of 2^5 rows: the five configurations of tests/test_sanitizers.py (plain, cap + proof of work, zk, zk + salts, arity-4
MMCS), one proof over the quintic challenge field and one written in a non-identity `proof_layout`.  Both entry points
frame the inner proof to its exact length whatever follows it, and refuse every truncation of it in the same words."""
import ctypes as C

import numpy as np
import pytest

import harness_lib
import layer_lib
import oracle_lib
from test_sanitizers import CASES, SMALL

LOG_H = 5
LAYOUT = [4, 0, 2, 1, 3] + [3, 4, 0, 2, 1] + [0, 2, 3, 1, 6, 7, 4, 5]   # batch | fri | opened, each a non-identity permutation
CONFIGS = [(name, kw, packing, flags) for name, kw, packing, flags in CASES] + [
    ("quintic_challenge", dict(log_blowup=1, max_log_arity=2, log_final_poly_len=0, query_pow_bits=2, num_queries=3, challenge_degree=5), None, 0),
    ("proof_layout", dict(log_blowup=1, max_log_arity=2, log_final_poly_len=0, query_pow_bits=2, num_queries=3, proof_layout=LAYOUT), None, 0),
]


def metadata_after(inner, field):
    """The bytes BatchStarkProof appends to its inner proof: any well-formed metadata will do."""
    from plonky3_recursion_amd import prover as pv
    outer = pv.BatchStarkProof(
        proof=inner, table_packing=pv.TablePacking(min_trace_height=8), rows=(3, 5, 7), w_binomial=3,
        non_primitives=(pv.NonPrimitiveTableEntry("recompose", 9, 2),),
        preprocessed_commitment=np.arange(8, dtype=np.uint32).reshape(1, 8), preprocessed_widths=(2, 2, 60, 24, 4),
        degree_bits=(3, 4, 5, 5, 3), monty_r=1, modulus=oracle_lib.MODULUS[field]).to_postcard()
    assert outer[:len(inner)] == inner
    return outer[len(inner):]


@pytest.mark.parametrize("name,kw,packing,flags", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_both_sinks_frame_and_refuse_alike(oracle, name, kw, packing, flags):
    import plonky3_recursion_amd as p3r
    from plonky3_recursion_amd import _lib
    field = "koala-bear"
    prm = layer_lib.params(**kw)
    arrs = harness_lib.generate(field, LOG_H, seed=40 + LOG_H, flags=flags, **SMALL)
    L = layer_lib.OracleLayer(oracle, field, arrs, prm, packing=packing)
    tables, cap, inner = L.tables(), L.prep_commit(), L.prove()
    lib = _lib.load()
    fid = oracle_lib.FIELD_IDS[field]
    layout = kw.get("proof_layout")
    lay = None if layout is None else (C.c_uint8 * 18)(*layout)
    wire = (2 if prm.challenge_degree == 5 else 0) | (4 if prm.zk else 0) | (8 if prm.mmcs_salt_elems else 0)
    err = C.create_string_buffer(512)

    def proof_len(data):
        n = C.c_size_t(0)
        buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
        rc = lib.p3r_batch_proof_len_layout(fid, buf, len(data), wire, lay, C.byref(n), err, len(err))
        return (rc, n.value) if rc == 0 else (rc, err.value.decode())

    meta = _lib.P3rBatchStarkMeta()

    def parse(data):
        rc = lib.p3r_batch_stark_proof_parse(fid, bytes(data), len(data), wire, lay, C.byref(meta), err, len(err))
        return (rc, int(meta.proof_len)) if rc == 0 else (rc, err.value.decode())

    # the length of the inner proof, whatever follows it
    assert proof_len(inner + b"\xff\x00\x81") == (0, len(inner))
    assert proof_len(inner) == (0, len(inner))
    assert parse(inner + metadata_after(inner, field)) == (0, len(inner))
    # every truncation is refused, by both in the same words
    cuts = list(range(min(len(inner), 2048))) + list(range(2048, len(inner), 61))
    for n in cuts:
        a, b = proof_len(inner[:n]), parse(inner[:n])
        assert a[0] != 0 and a == b, (n, a, b)
    # the building sink: the verifier accepts the untouched proof
    cfg, keep = p3r.make_config(field, prm.log_blowup, prm.max_log_arity, prm.cap_height, prm.log_final_poly_len, prm.commit_pow_bits,
                                prm.query_pow_bits, prm.num_queries, challenge_degree=prm.challenge_degree or 4, mmcs_arity=prm.mmcs_arity or 2,
                                zk=prm.zk, num_random_codewords=prm.num_random_codewords, mmcs_salt_elems=prm.mmcs_salt_elems,
                                proof_layout=layout, allow_unpinned_w32_defaults=True)
    airs = [dict(kind=t["kind_id"], lanes=t["lanes"], horner_packed_steps=t["horner_k"]) for t in tables]
    p3r.verify_batch(cfg, airs, cap, [int(t["main"].shape[0]).bit_length() - 1 + prm.zk for t in tables], inner)
