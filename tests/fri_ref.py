"""An independent restatement of p3_fri::prover::prove_fri for the tests of Context.prove_fri, written from the
definitions and built from pieces that do not call the library under test:

  fold_ref, row_points      tests/test_gpu_fri_seam.py (fold2 on Python integers)
  field_ref                 field and extension arithmetic on Python integers
  log_arity_rule            the schedule rule quoted in csrc/host_transcript.h
  oracle commit / commit4   the CPU oracle's MMCS on the reshaped host matrices
  oracle challenger_script  the CPU oracle's DuplexChallenger (and its proof-of-work search: the smallest witness)

The final polynomial is not computed by an inverse DFT here: the candidate coefficients are evaluated at the last
vector's points and must give the last vector; at most 2^log_final_poly_len <= m coefficients through m points are
unique, so equality with the vector pins every coefficient."""
import numpy as np

import field_ref
import test_gpu_fri_seam as seam

U = np.uint64


def log_arity_rule(schedule, phase, max_log_arity, log_cur, log_final, log_next_input):
    """Fold as far as max_log_arity allows without passing the next roll-in height or the final height; with an explicit
    schedule its entry is used if it is legal, -1 otherwise."""
    limit = log_cur - log_final
    if 0 <= log_next_input < log_cur:
        limit = min(limit, log_cur - log_next_input)
    if not schedule:
        return max(min(max_log_arity, limit), 1)
    if phase >= len(schedule):
        return -1
    la = schedule[phase]
    return la if 1 <= la <= limit and la <= max_log_arity else -1


class ScriptChallenger:
    """The oracle's challenger as an object: the script so far is replayed for every output (the scripts are short)."""

    def __init__(self, orc, field, dc=4):
        self.orc, self.field, self.dc, self.ops, self.args = orc, field, dc, [], []

    def clone(self):
        c = ScriptChallenger(self.orc, self.field, self.dc)
        c.ops, c.args = list(self.ops), list(self.args)
        return c

    def _out(self, op, arg, n):
        self.ops.append(op)
        self.args.append(int(arg))
        return self.orc.challenger_script(self.field, self.ops, self.args)[-n:]

    def observe(self, words):
        for w in np.asarray(words, dtype=np.uint64).reshape(-1):
            self.ops.append(0)
            self.args.append(int(w))

    def sample(self):
        return int(self._out(1, 0, 1)[0])

    def sample_ext(self):
        if self.dc == 4:
            return self._out(2, 0, 4).copy()
        return np.array([self.sample() for _ in range(self.dc)], dtype=np.uint32)   # DC consecutive samples

    def sample_bits(self, bits):
        return int(self._out(3, bits, 1)[0])

    def grind(self, bits):
        return 0 if bits == 0 else int(self._out(4, bits, 1)[0])   # bits == 0: witness 0, transcript untouched


def eval_at_rows(field, coeffs, m):
    """(flen, dc) coefficients -> (m, dc) values at x_i = w_m^bitrev(i), every coordinate a base-field polynomial."""
    p = seam.P(field)
    x = [int(v) for v in seam.row_points(field, m, 1)]
    c = [[int(v) for v in row] for row in coeffs]
    out = np.zeros((m, len(c[0])), dtype=np.uint32)
    for i, xi in enumerate(x):
        for k in range(len(c[0])):
            acc = 0
            for row in reversed(c):
                acc = (acc * xi + row[k]) % p
            out[i, k] = acc
    return out


class Expected:
    pass


def prove_fri_ref(orc, field, dc, prm, inputs, ch, candidate_final_poly, given_caps=None):
    """prm: dict(log_blowup, log_final_poly_len, max_log_arity, cap_height, commit_pow_bits, query_pow_bits, num_queries,
    mmcs_arity, fri_log_arities).  inputs: (h, dc) host arrays, tallest first.  ch: a ScriptChallenger in the caller's
    state.  given_caps: the caps of a hiding context (its salts are the library's; everything else is still restated)."""
    logs = [a.shape[0].bit_length() - 1 for a in inputs]
    log_max, log_final = logs[0], prm["log_final_poly_len"] + prm["log_blowup"]
    e = Expected()
    e.caps, e.pow, e.arities, e.leaves = [], [], [], []
    cur, log_cur, nxt = inputs[0], log_max, 1
    while log_cur > log_final:
        la = log_arity_rule(prm.get("fri_log_arities") or [], len(e.arities), prm["max_log_arity"], log_cur, log_final,
                            logs[nxt] if nxt < len(inputs) else -1)
        assert la >= 1, "the schedule does not fit"
        leaf = np.ascontiguousarray(cur.reshape(cur.shape[0] >> la, dc << la))
        if given_caps is not None:
            cap = given_caps[len(e.caps)]
        elif prm.get("mmcs_arity", 2) == 4:
            cap, _ = orc.commit4(field, [leaf])
        else:
            cap, _ = orc.commit(field, [leaf], prm["cap_height"])
        e.caps.append(cap)
        e.leaves.append(leaf)
        ch.observe(cap.reshape(-1))
        e.pow.append(ch.grind(prm["commit_pow_bits"]))
        beta = ch.sample_ext()
        roll = nxt < len(inputs) and logs[nxt] == log_cur - la
        cur = seam.fold_ref(field, dc, cur, la, beta, inputs[nxt] if roll else None)
        nxt += 1 if roll else 0
        log_cur -= la
        e.arities.append(la)
    assert nxt == len(inputs), "an input height was never rolled in"
    e.last = cur
    cand = np.asarray(candidate_final_poly, dtype=np.uint32)
    assert cand.shape == (1 << prm["log_final_poly_len"], dc)
    e.final_ok = np.array_equal(eval_at_rows(field, cand, cur.shape[0]), cur)
    ch.observe(cand.reshape(-1))
    ch.observe(e.arities)
    e.query_pow = ch.grind(prm["query_pow_bits"])
    e.indices = [ch.sample_bits(log_max) for _ in range(prm["num_queries"])]
    e.rows, shift = [], 0
    for q in e.indices:
        rows, shift = [], 0
        for la, leaf in zip(e.arities, e.leaves):
            shift += la
            rows.append(leaf[q >> shift])
        e.rows.append(rows)
    return e
