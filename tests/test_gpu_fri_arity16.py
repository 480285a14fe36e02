"""GPU: FRI folding by 16 on the device prover (`max_log_arity = 4`: k_fri_fold<.., LA = 4>, 64- and 80-column strided
commit-phase leaves, sixteen siblings per opening).  For the cases of tests/test_fri_arity16.py plus a ZK one with a hiding
MMCS, a tall one and an arity-4-MMCS one, the proof BYTES equal the CPU oracle's through both seams - `prove_next_layer`
from the circuit and its inputs, `prove_all_tables` from traces - and both verifiers accept.  Every case decodes its proof
and asserts that a phase really folded by 16.  Without arity 16 in the prover every case ends in P3R_EUNSUPPORTED.  A
log_arity of 5 is still refused."""
import os

import numpy as np
import pytest

import layer_lib
from test_fri_arity16 import CASES, EXPECTED, ONE_TALL_TABLE, arrays, case, log_arities, oracle_layer

pytestmark = pytest.mark.gpu

TALL_GEN = dict(horner_chain_len=20, sponge_chain_len=3, merkle_depth=5)
GPU_CASES = CASES + [
    # ZK (HidingFriPcs, deterministic mode under a fixed key) with a hiding MMCS: salted 16-ary leaves of 64 + 4 columns
    case("kb_2p9_zk_salted", "koala-bear", 9, log_blowup=2, max_log_arity=4, log_final_poly_len=1, zk=1, zk_seed=21, mmcs_salt_elems=4),
    # one tall table (2^13 rows, blow-up 32: LDE 2^18) over two short ones: the FIRST phase folds 2^18 -> 2^14, so its leaf
    # layer (2^14 rows of 64 columns) takes the one-permutation-per-lane kernel and its Merkle levels the per-level
    # launches; the second 16-ary phase (2^10 rows) takes the lane-cooperative one.  Device transcript.
    dict(case("kb_2p13_tall", "koala-bear", 13, flags=ONE_TALL_TABLE, log_blowup=5, max_log_arity=4, log_final_poly_len=3), gen=TALL_GEN),
    # the tall shape over the quintic challenge field: 2^14 leaf rows of 80 columns on the one-permutation-per-lane kernel
    dict(case("kb_2p13_tall_quintic", "koala-bear", 13, flags=ONE_TALL_TABLE, log_blowup=5, max_log_arity=4, log_final_poly_len=3,
              challenge_degree=5), gen=TALL_GEN),
    # the same shape under the arity-4 MMCS (width-32 leaves, lane-cooperative: 2^10 rows)
    dict(case("kb_2p11_tall_mmcs4", "koala-bear", 11, flags=ONE_TALL_TABLE, log_blowup=3, max_log_arity=4, log_final_poly_len=2, mmcs_arity=4),
         gen=TALL_GEN),
]
GPU_EXPECTED = dict(EXPECTED, kb_2p9_zk_salted=[1, 1, 2, 4, 1], kb_2p13_tall=[4, 4, 2], kb_2p13_tall_quintic=[4, 4, 2], kb_2p11_tall_mmcs4=[4, 1, 4])
LEAF_ROWS_PER_LANE_ABOVE = 8192   # mmcs_impl.hip.h::coop_max_leaf_rows: above, one permutation per lane (binary MMCS)


def device_transcript(kw):
    return kw.get("cap_height", 0) == 0 and kw.get("commit_pow_bits", 0) == 0


def rows_of_16ary_phases(L, kw, las):
    """Leaf rows of every phase that folds by 16: the height the phase folds from, over 16."""
    log_cur = max(int(t["main"].shape[0]).bit_length() - 1 for t in L.tables()) + kw["log_blowup"] + int(kw.get("zk", 0))
    out = []
    for la in las:
        if la == 4:
            out.append(1 << (log_cur - 4))
        log_cur -= la
    return out


def test_the_gpu_cases_cover_every_path(oracle):
    """The transcript on the device and on the host; a 16-ary phase on the one-permutation-per-lane leaf kernel and on the
    lane-cooperative one."""
    # the threshold below is the library's default; the tuning knob that moves it must not be set (it is read by the
    # `knobs` build only, which these tests do not load, but the statement should hold whatever is loaded)
    assert "P3R_COOP_MAX_LEAF_ROWS" not in os.environ
    assert any(device_transcript(c["kw"]) for c in GPU_CASES) and any(not device_transcript(c["kw"]) for c in GPU_CASES)
    assert any(c["kw"].get("zk") and c["kw"].get("mmcs_salt_elems") == 4 for c in GPU_CASES)
    tall = next(c for c in GPU_CASES if c["name"] == "kb_2p13_tall")
    assert tall["log_h"] >= 13 and tall["kw"].get("mmcs_arity", 2) == 2 and device_transcript(tall["kw"])
    # (the schedules are GPU_EXPECTED's: the byte test below asserts them on the decoded proofs)
    prm, L = oracle_layer(oracle, tall, arrays(tall))
    rows = rows_of_16ary_phases(L, tall["kw"], GPU_EXPECTED[tall["name"]])
    assert max(rows) > LEAF_ROWS_PER_LANE_ABOVE and min(rows) <= LEAF_ROWS_PER_LANE_ABOVE, rows
    quintic = next(c for c in GPU_CASES if c["name"] == "kb_2p13_tall_quintic")
    assert quintic["kw"]["challenge_degree"] == 5 and dict(quintic["kw"], challenge_degree=4) == dict(tall["kw"], challenge_degree=4)
    small = next(c for c in GPU_CASES if c["name"] == "kb_2p9")
    prm, L = oracle_layer(oracle, small, arrays(small))
    assert max(rows_of_16ary_phases(L, small["kw"], GPU_EXPECTED[small["name"]])) <= LEAF_ROWS_PER_LANE_ABOVE


def make_ctx(c):
    import plonky3_recursion_amd as p3r
    return p3r.Context(field=c["field"], allow_unpinned_w32_defaults=True, **c["kw"])


@pytest.mark.parametrize("c", GPU_CASES, ids=[c["name"] for c in GPU_CASES])
def test_device_proof_bytes_equal_the_oracle_under_arity_16(oracle, c):
    import harness_adapters as wl
    import plonky3_recursion_amd as p3r
    kw = c["kw"]
    arrs = arrays(c)
    prm, L = oracle_layer(oracle, c, arrs)
    want = L.prove()
    las = log_arities(want, c)
    print("%s: %d bytes, log_arity %s, 16-ary leaf rows %s" % (c["name"], len(want), las, rows_of_16ary_phases(L, kw, las)))
    assert 4 in las and las == GPU_EXPECTED[c["name"]]
    tp = p3r.TablePacking().with_fri_params(kw["log_final_poly_len"], kw["log_blowup"])
    params = p3r.ProveNextLayerParams(table_packing=tp)
    backend = p3r.FriRecursionBackend()
    # seam 1: the circuit and its inputs (device preparation, device runner, prover); proof number 0 of its context
    ctx = make_ctx(c)
    cache = p3r.build_next_layer_prep(ctx, wl.circuit_from_arrays(arrs), backend, params)
    out = p3r.prove_next_layer(p3r.RecursionInput(circuit_inputs=wl.circuit_inputs_from_arrays(arrs)), ctx, backend, params,
                               prep=cache)
    assert np.array_equal(cache.circuit_prover_data.preprocessed_commitment, L.prep_commit())
    got = out.proof.proof
    assert len(got) == len(want) and got == want, "prove_next_layer from the circuit: bytes differ from the oracle's"
    assert log_arities(got, c) == las
    L.verify(got)                                  # the oracle's verifier
    cache.prover.verify_all_tables(out.proof)      # the native one
    layer_lib.oracle_verify_statement(oracle, c["field"], prm, out.proof.airs(), cache.circuit_prover_data.preprocessed_commitment, got)
    cache.prepared_circuit.free()
    ctx.close()
    # seam 2: the generator's traces over a preparation made from its arrays
    ctx = make_ctx(c)
    cache = p3r.build_next_layer_prep(ctx, wl.circuit_prep_from_arrays(arrs), backend, params)
    cpd = cache.circuit_prover_data
    assert np.array_equal(cpd.preprocessed_commitment, L.prep_commit())
    traces = wl.traces_from_arrays(arrs)
    first = cache.prover.prove_all_tables(traces, cpd)
    assert first.proof == want, "prove_all_tables from traces: bytes differ from the oracle's"
    cache.prover.verify_all_tables(first)
    if c["log_h"] <= 10:
        # the canonical encoding (the small cases: an oracle proof more); under ZK / salts it is proof number 1 of the context
        nonce = 1 if (kw.get("zk") or kw.get("mmcs_salt_elems")) else 0
        canon = cache.prover.prove_all_tables(traces, cpd, canonical_field_encoding=True)
        assert canon.proof == oracle_layer(oracle, c, arrs, zk_nonce=nonce)[1].prove(field_encoding=1)
        cache.prover.verify_all_tables(canon)
    # the wire form round-trips through the native parser
    k = dict(challenge_degree=kw.get("challenge_degree", 4), zk=bool(kw.get("zk")), salted=bool(kw.get("mmcs_salt_elems")))
    back = p3r.BatchStarkProof.from_postcard(first.to_postcard(), c["field"], **k)
    assert back.proof == want
    cache.prover.verify_all_tables(back)
    # tampering with the 16-ary opening is refused
    bad = bytearray(want)
    bad[int(len(bad) * 0.97)] ^= 1
    with pytest.raises(p3r.P3rError):
        cache.prover.verify_all_tables(p3r.BatchStarkProver(ctx).wrap_proof(bytes(bad), cpd))
    cpd.free()
    ctx.close()


def test_a_log_arity_of_5_is_still_refused(oracle):
    """Folding by 32 is not built: the device refuses the phase with P3R_EUNSUPPORTED, whether the rule picks it
    (max_log_arity = 5) or an explicit schedule names it; under max_log_arity = 4 an entry of 5 is illegal for the device
    and for the oracle alike.  (The oracle has no arity limit of its own: under max_log_arity = 5 it folds by 32.)"""
    import harness_adapters as wl
    import plonky3_recursion_amd as p3r
    P3R_EINVAL, P3R_EUNSUPPORTED = -1, -5
    c = case("kb_2p9_la5", "koala-bear", 9, log_blowup=2, max_log_arity=5, log_final_poly_len=0)
    arrs = arrays(c)
    assert log_arities(oracle_layer(oracle, c, arrs)[1].prove(), c) == [1, 1, 2, 5]
    with pytest.raises(RuntimeError, match="fri_log_arities"):
        oracle_layer(oracle, c, arrs, max_log_arity=4, fri_log_arities=[1, 1, 2, 5])[1].prove()
    tp = p3r.TablePacking().with_fri_params(0, 2)
    for over, code, msg in ((dict(), P3R_EUNSUPPORTED, "max_log_arity > 4 is not supported"),
                            (dict(fri_log_arities=[1, 1, 2, 5]), P3R_EUNSUPPORTED, "max_log_arity > 4 is not supported"),
                            (dict(max_log_arity=4, fri_log_arities=[1, 1, 2, 5]), P3R_EINVAL, "fri_log_arities")):
        ctx = p3r.Context(field=c["field"], **dict(c["kw"], **over))
        cache = p3r.build_next_layer_prep(ctx, wl.circuit_prep_from_arrays(arrs), p3r.FriRecursionBackend(),
                                          p3r.ProveNextLayerParams(table_packing=tp))
        with pytest.raises(p3r.P3rError, match=msg) as e:
            cache.prover.prove_all_tables(wl.traces_from_arrays(arrs), cache.circuit_prover_data)
        assert e.value.code == code
        cache.circuit_prover_data.free()
        ctx.close()
    # and 4 + 1 over the same five halvings is fine
    ok = dict(case("kb_2p9_4_1", "koala-bear", 9, log_blowup=2, max_log_arity=4, log_final_poly_len=0))
    ctx = p3r.Context(field=ok["field"], **ok["kw"])
    cache = p3r.build_next_layer_prep(ctx, wl.circuit_prep_from_arrays(arrs), p3r.FriRecursionBackend(),
                                      p3r.ProveNextLayerParams(table_packing=tp))
    got = cache.prover.prove_all_tables(wl.traces_from_arrays(arrs), cache.circuit_prover_data).proof
    assert got == oracle_layer(oracle, ok, arrs)[1].prove() and log_arities(got, ok) == [1, 1, 2, 4, 1]
    cache.circuit_prover_data.free()
    ctx.close()
