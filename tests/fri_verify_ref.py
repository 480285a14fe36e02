"""Helpers of the FRI verifier tests: a whole FriProof made on the CPU - fri_ref.prove_fri_ref for everything it
restates (caps, witnesses, arities, indices, opened rows), the siblings from the CPU oracle's trees over the same leaf
matrices, and the final polynomial by a plain inverse DFT on Python integers - low-degree inputs of three heights, and
the mutations the negative tests apply.  Nothing here calls the library under test."""
import copy

import numpy as np

import field_ref
import fri_ref
import test_gpu_fri_seam as seam

P3R_EINVAL, P3R_EUNSUPPORTED, P3R_EVERIFY = -1, -5, -7
LOGS = (8, 6, 5)


def low_degree_inputs(field, dc, log_blowup, rng, logs=LOGS):
    """One (2^l, dc) vector per height: the values over <w_2^l>, bit-reversed, of a random polynomial of degree
    < 2^(l - log_blowup) - the backbone at the first height and roll-ins that keep every folded sum of low degree."""
    p = seam.P(field)
    return [fri_ref.eval_at_rows(field, rng.integers(0, p, size=(1 << (l - log_blowup), dc), dtype=np.uint32), 1 << l) for l in logs]


def interpolate_rows(field, vec):
    """The (m, dc) coefficients, natural order, of the polynomials whose values over <w_m> in bit-reversed row order are
    the (m, dc) vector: c_k = 1/m sum_i v_i x_i^-k."""
    p, m = seam.P(field), vec.shape[0]
    x_inv = [pow(int(x), p - 2, p) for x in seam.row_points(field, m, 1)]
    m_inv = pow(m, p - 2, p)
    out = np.zeros(vec.shape, dtype=np.uint32)
    for k in range(m):
        xs = [pow(xi, k, p) for xi in x_inv]
        for j in range(vec.shape[1]):
            out[k, j] = sum(int(vec[i, j]) * xs[i] for i in range(m)) % p * m_inv % p
    return out


def last_vector(orc, field, dc, prm, inputs, ch):
    """The last folded vector of prove_fri_ref for these inputs (a first pass, on a clone of the challenger)."""
    zero = np.zeros((1 << prm["log_final_poly_len"], dc), dtype=np.uint32)
    return fri_ref.prove_fri_ref(orc, field, dc, prm, inputs, ch.clone(), zero).last


def prove_on_cpu(orc, field, dc, prm, inputs, ch, keep=None):
    """A FriProof for `inputs` under `prm` (the dict of fri_ref.prove_fri_ref; binary MMCS or, mmcs_arity = 4, the
    arity-4 one), made on the CPU.  `ch` is left where the prover's challenger is."""
    from plonky3_recursion_amd.device import FriPhaseOpening, FriProof
    last = last_vector(orc, field, dc, prm, inputs, ch)
    coeffs = interpolate_rows(field, last)
    flen = 1 << prm["log_final_poly_len"]
    assert not coeffs[flen:].any(), "the inputs are not of low degree"
    want = fri_ref.prove_fri_ref(orc, field, dc, prm, inputs, ch, coeffs[:flen])
    assert want.final_ok
    proof = FriProof(log_max_height=inputs[0].shape[0].bit_length() - 1)
    proof.commit_phase_caps = [np.array(c) for c in want.caps]
    proof.commit_pow_witnesses = list(want.pow)
    proof.log_arities = list(want.arities)
    proof.final_poly = coeffs[:flen].copy()
    proof.query_pow_witness = want.query_pow
    proof.query_indices = list(want.indices)
    trees = []
    for leaf in want.leaves:
        if prm.get("mmcs_arity", 2) == 4:
            cap, tree = orc.commit4(field, [leaf])
        else:
            cap, tree = orc.commit(field, [leaf], prm["cap_height"])
        trees.append(tree)
    if keep is not None:
        keep.append((list(want.arities), trees))
    proof.query_openings = open_at(want.arities, trees, want.indices, dc)
    return proof


def open_at(arities, trees, indices, dc):
    """The commit-phase openings of every query index, from the phase trees."""
    from plonky3_recursion_amd.device import FriPhaseOpening
    out = []
    for q in indices:
        openings, shift = [], 0
        for la, tree in zip(arities, trees):
            shift += la
            row, sibs = tree.open(q >> shift)
            openings.append(FriPhaseOpening(row.reshape(-1, dc).copy(), None, sibs.copy()))
        out.append(openings)
    return out


def input_values(inputs, indices, log_max=None):
    """The p3r_fri_input_view of every input vector at these query indices: (log_height, (n_queries, dc))."""
    logs = [a.shape[0].bit_length() - 1 for a in inputs]
    log_max = logs[0] if log_max is None else log_max
    return [(l, np.array([a[i >> (log_max - l)] for i in indices], dtype=np.uint32).reshape(len(indices), -1)) for l, a in zip(logs, inputs)]


def bump(a, at, p):
    """`a` with the word at flat position `at` replaced by another canonical word."""
    a = np.array(a, dtype=np.uint32)
    flat = a.reshape(-1)
    flat[at] = (int(flat[at]) + 1) % p
    return a


# name -> (mutation of (proof, inputs) in place, what the message must name).  Every one leaves a well-formed proof, so
# the verifier rejects it (P3R_EVERIFY) rather than refusing it as malformed.
def mutations(p):
    def cap_word(pr, ins):
        pr.commit_phase_caps[0] = bump(pr.commit_phase_caps[0], 3, p)

    def commit_pow(pr, ins):
        pr.commit_pow_witnesses[-1] = (pr.commit_pow_witnesses[-1] + 1) % p

    def query_pow(pr, ins):
        pr.query_pow_witness = (pr.query_pow_witness + 1) % p

    def final_coeff(pr, ins):
        pr.final_poly = bump(pr.final_poly, 1, p)

    def row_word(pr, ins):
        # a sibling of the queried element in the first phase of the last query: the leaf hash changes
        o = pr.query_openings[-1][0]
        pos = pr.query_indices[-1] & (o.row.shape[0] - 1)
        o.row = bump(o.row, ((pos + 1) % o.row.shape[0]) * o.row.shape[1], p)

    def sibling(pr, ins):
        o = pr.query_openings[1][0]
        o.siblings = bump(o.siblings, 5, p)

    def input_value(pr, ins):
        ins[1] = (ins[1][0], bump(ins[1][1], 2, p))

    return {
        "cap_word": (cap_word, None),   # the transcript moves: a proof of work, an index and so a root or the final value
        "commit_pow": (commit_pow, "commit proof-of-work of phase"),
        "query_pow": (query_pow, "query proof of work"),
        "final_coeff": (final_coeff, None),
        "row_word": (row_word, "FRI commit phase 0 of query"),
        "sibling": (sibling, "FRI commit phase 0 of query 1: Merkle root mismatch"),
        "input_value": (input_value, None),
    }


def drop_phase(pr):
    """The proof without its last commit phase, consistently in every array."""
    pr.commit_phase_caps.pop()
    pr.commit_pow_witnesses.pop()
    pr.log_arities.pop()
    for o in pr.query_openings:
        o.pop()


def drop_query(pr):
    pr.query_openings.pop()
    pr.query_indices.pop()


def clone_proof(pr):
    return copy.deepcopy(pr)
