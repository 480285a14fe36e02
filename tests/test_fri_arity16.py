"""CPU (no GPU): FRI folding by 16 (`max_log_arity = 4`, the setting the reference's documentation calls typical) around
the device prover: the CPU oracle proves layers whose commit phase really folds by 16 - every case decodes its proof and
asserts a log_arity of 4 in the first query - and the product's host code takes them: the native verifier in both field
encodings, its rejections (bit flips at several depths, truncation, a trailing byte, another `max_log_arity`), the inner
proof framer and the `BatchStarkProof` parser (P3R_PROOF_SALTED and the quintic challenge field included), and the 2^14
entry of tests/golden/proof_digests_arity16.json.  The device side is tests/test_gpu_fri_arity16.py, which runs the same
cases (CASES) plus a ZK one."""
import ctypes as C
import importlib.util
import json
import os

import pytest

import harness_lib
import layer_lib
import proof_codec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("gen_proof_digests", os.path.join(ROOT, "tools", "gen_proof_digests.py"))
gpd = importlib.util.module_from_spec(spec)
spec.loader.exec_module(gpd)

SMALL = dict(horner_chain_len=12, sponge_chain_len=3, merkle_depth=4)
Q = dict(query_pow_bits=3, num_queries=4)
ONE_TALL_TABLE = harness_lib.NO_POSEIDON2 | harness_lib.NO_RECOMPOSE | harness_lib.SINGLE_PUBLIC


def case(name, field, log_h, flags=0, **kw):
    return dict(name=name, field=field, log_h=log_h, flags=flags, kw=dict(kw, **Q))


# A phase folds by 16 only when neither the next table height nor the final height is nearer than four halvings: with the
# five tables of a layer that is the phase below the shortest table (LDE heights 2^11, 2^10, 2^9, 2^7 at 2^9 rows and
# blow-up 4: log_arity 1, 1, 2, then 4 down to the final 2^3).  EXPECTED holds what the oracle gave when the cases were
# picked; the tests assert it, so a case that stops folding by 16 fails instead of passing for nothing.
CASES = [
    case("kb_2p9", "koala-bear", 9, log_blowup=2, max_log_arity=4, log_final_poly_len=1),
    # host transcript: a cap of two digests and commit-phase proof of work
    case("bb_2p10_cap1_pow2", "baby-bear", 10, log_blowup=1, max_log_arity=4, log_final_poly_len=1, cap_height=1, commit_pow_bits=2),
    case("kb_2p8_mmcs4", "koala-bear", 8, log_blowup=2, max_log_arity=4, log_final_poly_len=0, mmcs_arity=4),
    case("kb_2p9_quintic", "koala-bear", 9, log_blowup=2, max_log_arity=4, log_final_poly_len=1, challenge_degree=5),
    case("bb_2p9_salted", "baby-bear", 9, log_blowup=2, max_log_arity=4, log_final_poly_len=1, mmcs_salt_elems=4, zk_seed=21),
    # an explicit schedule that is not the rule's (1, 1, 2, 4, 1): the 16-ary phase last, over two rows
    case("kb_2p10_schedule", "koala-bear", 10, log_blowup=2, max_log_arity=4, log_final_poly_len=1, fri_log_arities=[1, 1, 2, 1, 4]),
]
EXPECTED = {"kb_2p9": [1, 1, 2, 4], "bb_2p10_cap1_pow2": [1, 1, 2, 4, 1], "kb_2p8_mmcs4": [1, 1, 2, 4],
            "kb_2p9_quintic": [1, 1, 2, 4], "bb_2p9_salted": [1, 1, 2, 4], "kb_2p10_schedule": [1, 1, 2, 1, 4]}
IDS = [c["name"] for c in CASES]


def arrays(c):
    return harness_lib.generate(c["field"], c["log_h"], seed=160 + c["log_h"], flags=c["flags"], **c.get("gen", SMALL))


def oracle_layer(oracle, c, arrs, **over):
    prm = layer_lib.params(**dict(c["kw"], **over))
    return prm, layer_lib.OracleLayer(oracle, c["field"], arrs, prm)


def codec_kw(c):
    kw = c["kw"]
    return dict(dc=kw.get("challenge_degree", 4), zk=bool(kw.get("zk")), salted=bool(kw.get("mmcs_salt_elems")))


def log_arities(proof, c):
    """log2 of the arity of every commit phase, off the first query of the decoded proof; the whole proof must decode."""
    d = proof_codec.decode(proof, **codec_kw(c))
    assert d["_consumed"] == len(proof)
    per_query = [[s["log_arity"] for s in q["commit_phase_openings"]] for q in d["opening_proof"]["query_proofs"]]
    assert all(p == per_query[0] for p in per_query)
    for q in d["opening_proof"]["query_proofs"]:
        for s in q["commit_phase_openings"]:
            assert len(s["sibling_values"]) == (1 << s["log_arity"]) - 1
    return per_query[0]


def native_verify(c, tables, cap, proof, canonical=False, **over):
    import plonky3_recursion_amd as p3r
    kw = dict(c["kw"], **over)
    zk = int(kw.get("zk", 0))
    kw.pop("zk_seed", None)    # the verifier draws nothing
    cfg, keep = p3r.make_config(c["field"], allow_unpinned_w32_defaults=True, **kw)
    airs = [dict(kind=t["kind_id"], lanes=t["lanes"], horner_packed_steps=t["horner_k"]) for t in tables]
    p3r.verify_batch(cfg, airs, cap, [int(t["main"].shape[0]).bit_length() - 1 + zk for t in tables], proof, canonical)


def parser_flags(c, canonical=False):
    k = codec_kw(c)
    return (1 if canonical else 0) | (2 if k["dc"] == 5 else 0) | (4 if k["zk"] else 0) | (8 if k["salted"] else 0)


def wrapped(c, arrs, tables, cap, inner, canonical=False):
    """The `BatchStarkProof` around the oracle's inner proof, with the metadata the prover writes (default packing)."""
    from plonky3_recursion_amd import prover as pv
    counts = [int(x) for x in arrs["counts"]]
    prm = layer_lib.params(**c["kw"])
    tp = pv.TablePacking(min_trace_height=layer_lib.min_trace_height(prm))
    npo = (pv.NonPrimitiveTableEntry("poseidon2_perm/%s_d4_w16" % c["field"].replace("-", "_"), tables[3]["main"].shape[0], 1),
           pv.NonPrimitiveTableEntry("recompose", counts[4], 1))
    return pv.BatchStarkProof(
        proof=inner, table_packing=tp, rows=tuple(counts[:3]), w_binomial=pv.W_BINOMIAL[c["field"]], non_primitives=npo,
        preprocessed_commitment=cap, preprocessed_widths=tuple(t["prep"].shape[1] for t in tables),
        degree_bits=tuple(t["main"].shape[0].bit_length() - 1 for t in tables), monty_r=0 if canonical else 1,
        modulus=0x7F000001 if c["field"] == "koala-bear" else 0x78000001)


def test_the_cases_cover_what_they_should():
    kws = [c["kw"] for c in CASES]
    assert {c["field"] for c in CASES} == {"koala-bear", "baby-bear"}
    assert {k.get("challenge_degree", 4) for k in kws} == {4, 5} and {k.get("mmcs_arity", 2) for k in kws} == {2, 4}
    assert any(k.get("cap_height", 0) > 0 and k.get("commit_pow_bits", 0) > 0 for k in kws)
    assert any(k.get("mmcs_salt_elems") for k in kws)
    assert any(4 in (k.get("fri_log_arities") or []) and min(k["fri_log_arities"]) < 4 for k in kws)
    assert all(k["max_log_arity"] == 4 for k in kws)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_oracle_folds_by_16_and_the_host_code_takes_the_proof(oracle, c):
    import plonky3_recursion_amd as p3r
    from plonky3_recursion_amd import _lib
    from plonky3_recursion_amd import prover as pv
    arrs = arrays(c)
    prm, L = oracle_layer(oracle, c, arrs)
    tables, cap = L.tables(), L.prep_commit()
    proof = L.prove()
    las = log_arities(proof, c)
    print("%s: %d bytes, log_arity %s" % (c["name"], len(proof), las))
    assert 4 in las and las == EXPECTED[c["name"]]
    L.verify(proof)
    # the native verifier, both field encodings
    native_verify(c, tables, cap, proof)
    canon = L.prove(field_encoding=1)
    assert log_arities(canon, c) == las
    native_verify(c, tables, cap, canon, canonical=True)
    # every part of the proof is bound: one bit at several depths (the 16-ary openings are in the last ones), the length
    for frac in (0.02, 0.3, 0.55, 0.8, 0.9, 0.97, 0.995):
        bad = bytearray(proof)
        bad[int(len(bad) * frac)] ^= 1
        with pytest.raises(p3r.P3rError):
            native_verify(c, tables, cap, bytes(bad))
        with pytest.raises(RuntimeError):
            L.verify(bytes(bad))
    # a sibling value of the 16-ary opening itself, and its log_arity byte
    d = proof_codec.decode(proof, **codec_kw(c))
    step = d["opening_proof"]["query_proofs"][-1]["commit_phase_openings"][las.index(4)]
    assert step["log_arity"] == 4 and len(step["sibling_values"]) == 15
    step["sibling_values"][14][0] ^= 1
    with pytest.raises(p3r.P3rError):
        native_verify(c, tables, cap, proof_codec.encode(d))
    d = proof_codec.decode(proof, **codec_kw(c))
    d["opening_proof"]["query_proofs"][0]["commit_phase_openings"][las.index(4)]["log_arity"] = 3
    with pytest.raises(p3r.P3rError):
        native_verify(c, tables, cap, proof_codec.encode(d))
    with pytest.raises(p3r.P3rError):
        native_verify(c, tables, cap, proof[:-1])
    with pytest.raises(p3r.P3rError):
        native_verify(c, tables, cap, proof + b"\x00")
    # max_log_arity is part of the statement: under 3 the rule gives another schedule, and an explicit entry of 4 is illegal
    with pytest.raises(p3r.P3rError):
        native_verify(c, tables, cap, proof, max_log_arity=3)
    prm3, L3 = oracle_layer(oracle, c, arrs, max_log_arity=3)
    with pytest.raises(RuntimeError):
        L3.verify(proof)
    # the framer of the inner proof and the BatchStarkProof parser
    lib = _lib.load()
    fid = p3r.device.FIELD_IDS[c["field"]]
    for canonical, inner in ((False, proof), (True, canon)):
        flags = parser_flags(c, canonical)
        buf = (C.c_uint8 * (len(inner) + 3)).from_buffer_copy(inner + b"xyz")
        got, err = C.c_size_t(), C.create_string_buffer(256)
        assert lib.p3r_batch_proof_len(fid, buf, len(inner) + 3, flags, C.byref(got), err, 256) == 0, err.value
        assert got.value == len(inner)
        assert lib.p3r_batch_proof_len(fid, buf, len(inner) - 1, flags, C.byref(got), err, 256) != 0
        w = wrapped(c, arrs, tables, cap, inner, canonical)
        wire = w.to_postcard()
        k = codec_kw(c)
        back = pv.BatchStarkProof.from_postcard(wire, c["field"], canonical_field_encoding=canonical, challenge_degree=k["dc"],
                                                zk=k["zk"], salted=k["salted"])
        assert back.proof == inner and back.to_postcard() == wire
        with pytest.raises(p3r.P3rError):
            pv.BatchStarkProof.from_postcard(wire[:len(inner) - 5], c["field"], canonical_field_encoding=canonical,
                                             challenge_degree=k["dc"], zk=k["zk"], salted=k["salted"])
        if k["salted"]:   # the proof type is the caller's to tell: unsalted framing does not fit
            with pytest.raises(p3r.P3rError):
                pv.BatchStarkProof.from_postcard(wire, c["field"], canonical_field_encoding=canonical)
        if not canonical:
            kw = {a: b for a, b in c["kw"].items() if a != "zk_seed"}
            cfg, keep = p3r.make_config(c["field"], allow_unpinned_w32_defaults=True, **kw)
            p3r.verify_all_tables(cfg, back)


def test_explicit_schedule_differs_from_the_rule(oracle):
    c = next(x for x in CASES if x["name"] == "kb_2p10_schedule")
    arrs = arrays(c)
    prm, L = oracle_layer(oracle, c, arrs)
    prm0, L0 = oracle_layer(oracle, c, arrs, fri_log_arities=None)
    p, p0 = L.prove(), L0.prove()
    assert log_arities(p0, c) == [1, 1, 2, 4, 1] and log_arities(p, c) == [1, 1, 2, 1, 4] and p != p0
    # the schedule is part of the native verifier's statement (the oracle's reads a legal one off the proof); an entry of 4
    # needs max_log_arity >= 4
    import plonky3_recursion_amd as p3r
    native_verify(c, L.tables(), L.prep_commit(), p)
    with pytest.raises(p3r.P3rError):
        native_verify(c, L.tables(), L.prep_commit(), p, fri_log_arities=None)
    with pytest.raises(p3r.P3rError):
        native_verify(c, L.tables(), L.prep_commit(), p, max_log_arity=3)
    with pytest.raises(RuntimeError):
        oracle_layer(oracle, c, arrs, max_log_arity=3)[1].prove()


# ---- tests/golden/proof_digests_arity16.json ---------------------------------------------------------------------------
def pins():
    return json.load(open(gpd.ARITY16_PATH))["cases"]


def test_arity16_fixture_holds_exactly_its_cases():
    P = pins()
    assert list(P) == [c["name"] for c in gpd.ARITY16_CASES]
    assert len(open(gpd.ARITY16_PATH, "rb").read()) < 64 << 10    # digests only
    large = json.load(open(gpd.LARGE_PATH))["cases"]
    for c in gpd.ARITY16_CASES:
        pin = P[c["name"]]
        assert set(pin) == set(large["kb_headline_14"])            # the record shape of the large fixture
        assert c["prm"]["max_log_arity"] == 4 and pin["circuit_seam"] is not None
        twin = c["name"][:-len("_la4")]
        # the same workload and preprocessed commitment as the max_log_arity = 2 twin, fewer commit phases, a shorter proof
        assert pin["workload"] == large[twin]["workload"] and pin["prep_commit"] == large[twin]["prep_commit"]
        assert pin["proof"] != large[twin]["proof"] and pin["proof_bytes"] < large[twin]["proof_bytes"]
        rounds = lambda e: len([k for k in e["sections"] if k.startswith("commit_phase_commits[")])   # noqa: E731
        assert rounds(pin) < rounds(large[twin])


def test_oracle_reproduces_the_2p14_arity16_entry(oracle):
    c = gpd.ARITY16_BY_NAME["kb_headline_14_la4"]
    pin = pins()[c["name"]]
    got = gpd.large_entry(oracle, c)
    assert gpd.compare_entries(pin, got) == [], gpd.first_difference(pin["sections"], got["sections"])
    proof = gpd.large_layer(oracle, c, gpd.large_arrays(c)).prove()
    las = gpd.fri_log_arities(proof, c)
    print("kb_headline_14_la4: log_arity", las)
    assert las == [1, 1, 2, 4, 1]
