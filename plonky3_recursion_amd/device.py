"""Thin object layer over the C ABI: context, device matrices, Poseidon2, LDE, MMCS.

Names follow the reference's traits where one exists:
  Context               StarkConfig built by circuit-prover/src/config.rs:92-137 /
                        recursion/examples/common/mod.rs:464-486 (FRI params + Poseidon2 perms)
  MerkleTree.commit/open_batch   p3_commit::Mmcs::{commit, open_batch}
  coset_lde_batch       p3_dft::TwoAdicSubgroupDft::coset_lde_batch (+ bit_reverse_rows)
  dft_batch             p3_dft::TwoAdicSubgroupDft::{dft_batch, idft_batch, coset_dft_batch, coset_idft_batch}
  open_points           the opened values of p3_fri::TwoAdicFriPcs::open (interpolate_coset on the committed LDEs)
  fri_reduce_device     the reduced openings of p3_fri::TwoAdicFriPcs::open (one vector per LDE height)
  fri_fold_device       p3_fri::FriFoldingStrategy::fold_matrix of TwoAdicFriFolding, with the roll-in of the next height
  Challenger            DuplexChallenger<F, Perm16, 16, 8> (circuit-prover/src/config.rs), with the proof-of-work search
  fri_leaf_view_device  the matrix ExtensionMmcs::commit_matrix commits in a FRI commit phase
  prove_fri             p3_fri::prover::prove_fri (commit phase, final polynomial, query openings) from the calls above
  AirBuilder            p3_uni_stark::SymbolicAirBuilder: an Air::eval recorded as a p3r_air_insn program
  quotient_device       p3_uni_stark::prove's quotient_values + split_evals for that program, on resident LDEs
  logup_device          p3_lookup's LogUp gadget: the permutation trace and the table's sum for a lookup program, on resident traces
  permute_batch         CryptographicPermutation<[F;16]>::permute over a batch
  generate_trace_rows   Poseidon2CircuitAir::generate_trace_rows (poseidon2-circuit-air/src/air.rs:280)
"""
import ctypes as C

import numpy as np

from . import _lib

FIELD_IDS = {"koala-bear": _lib.FIELD_KOALA_BEAR, "baby-bear": _lib.FIELD_BABY_BEAR}
MODULUS = {"koala-bear": 0x7F000001, "baby-bear": 0x78000001}
GENERATOR = {"koala-bear": 3, "baby-bear": 31}


class P3rError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"p3r error {code}: {msg}")
        self.code = code


def _u32(a):
    a = np.ascontiguousarray(a, dtype=np.uint32)
    return a, a.ctypes.data_as(_lib.u32p)


def _u8(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint8))


def make_config(field="koala-bear", log_blowup=2, max_log_arity=2, cap_height=0, log_final_poly_len=5,
                commit_pow_bits=0, query_pow_bits=15, num_queries=54, device=0, poseidon2_rc=None, ext_choices=0,
                fri_log_arities=None, proof_layout=None, ext_degree=4, ext_w=0, challenge_degree=4,
                poseidon2_w32_rc=None, poseidon2_w32_diag=None, mmcs_arity=2, zk=0, num_random_codewords=2, zk_seed=None,
                zk_key=None, zk_deterministic=None, allow_unpinned_w32_defaults=False, mmcs_salt_elems=0):
    """A `p3r_config` (+ the arrays it points into, which must stay alive with it).  `ext_choices` /
    `fri_log_arities`: the selectable protocol details of include/p3r.h.
    `ext_degree`: the circuit extension degree D of the traces - 4, or 5 for KoalaBear circuits over the quintic
    trinomial extension (primitive tables; the STARK itself stays on the D = 4 configuration)."""
    cfg = _lib.P3rConfig()
    cfg.abi_version = _lib.P3R_ABI_VERSION
    cfg.field = FIELD_IDS[field]
    cfg.ext_degree = ext_degree
    cfg.ext_w = ext_w     # W of x^D = W for ext_degree 2 / 6 / 8 (include/p3r.h)
    cfg.challenge_degree = challenge_degree   # 5: KoalaBear's quintic challenge field
    cfg.mmcs_arity = mmcs_arity               # 4: the arity-4 MMCS over the width-32 permutation (recursive_aggregation --arity4)
    # ZK: HidingFriPcs with `num_random_codewords` random codewords and a seeded RNG (create_config_zk)
    # `zk_key`: the 256-bit key of its generator (eight u32 words, or 32 bytes); the library mixes operating-system
    # entropy into it unless `zk_deterministic`.  `zk_seed` is the test harness's shorthand: key = (seed, 0, ..) taken
    # as it is - reproducible proofs, which is what a comparison with the CPU oracle needs and a deployment must not use.
    cfg.zk, cfg.num_random_codewords = int(zk), int(num_random_codewords) if zk else 0
    cfg.mmcs_salt_elems = int(mmcs_salt_elems)   # MerkleTreeHidingMmcs (recursion/tests/zk_hiding_mmcs.rs: 4); 0 = plain
    if zk_seed is not None and zk_key is not None:
        raise P3rError(-1, "pass zk_key or zk_seed, not both")
    if zk_seed is not None:
        zk_key = [int(zk_seed) & 0xFFFFFFFF, (int(zk_seed) >> 32) & 0xFFFFFFFF, 0, 0, 0, 0, 0, 0]
        zk_deterministic = True if zk_deterministic is None else zk_deterministic
    if zk_key is not None:
        words = np.frombuffer(bytes(zk_key), dtype="<u4") if isinstance(zk_key, (bytes, bytearray)) else np.asarray(zk_key, dtype=np.uint32)
        if words.size != 8:
            raise P3rError(-1, "zk_key must hold 256 bits (eight u32 words or 32 bytes)")
        for i in range(8):
            cfg.zk_key[i] = int(words[i])
    if zk_deterministic:
        ext_choices |= _lib.P3R_EXT_ZK_DETERMINISTIC
    cfg.log_blowup = log_blowup
    cfg.max_log_arity = max_log_arity
    cfg.cap_height = cap_height
    cfg.log_final_poly_len = log_final_poly_len
    cfg.commit_pow_bits = commit_pow_bits
    cfg.query_pow_bits = query_pow_bits
    cfg.num_queries = num_queries
    cfg.device = device
    rc = None
    if poseidon2_rc is not None:
        rc, ptr = _u32(poseidon2_rc)
        cfg.poseidon2_rc = ptr
        cfg.poseidon2_rc_len = rc.size
    # The width-32 permutation's constants live in un-vendored crates; the library's defaults for them are self-generated
    # and the C ABI wants that acknowledged (P3R_EXT_UNPINNED_W32_DEFAULTS): so does this mirror - a caller that uses
    # the arity-4 MMCS or the width-32 table without upstream's statics says `allow_unpinned_w32_defaults=True` (the
    # tests, bench.py's "unpinned" legs and the profiling tools do), as p3r.hpp's FriParams has it.
    if allow_unpinned_w32_defaults and (poseidon2_w32_rc is None or poseidon2_w32_diag is None):
        ext_choices |= _lib.P3R_EXT_UNPINNED_W32_DEFAULTS
    cfg.ext_choices = ext_choices
    ar = None
    if fri_log_arities is not None:
        ar, aptr = _u8(fri_log_arities)
        cfg.fri_log_arities = aptr
        cfg.fri_log_arities_len = ar.size
    pl = None
    if proof_layout is not None:
        pl, pptr = _u8(proof_layout)
        cfg.proof_layout = pptr
        cfg.proof_layout_len = pl.size
    # constants of the width-32 permutation (the table of the arity-4 MMCS rows); None = the library's defaults
    w_rc = w_dg = None
    if poseidon2_w32_rc is not None:
        w_rc, wptr = _u32(poseidon2_w32_rc)
        cfg.poseidon2_w32_rc = wptr
        cfg.poseidon2_w32_rc_len = w_rc.size
    if poseidon2_w32_diag is not None:
        w_dg, dptr = _u32(poseidon2_w32_diag)
        if w_dg.size != 32:
            raise P3rError(-1, "poseidon2_w32_diag must hold 32 values")
        cfg.poseidon2_w32_diag = dptr
    return cfg, (rc, ar, pl, w_rc, w_dg)


def verify_batch(cfg, airs, preprocessed_commitment, degree_bits, proof: bytes, canonical_field_encoding=False):
    """`verify_batch` behind `verify_all_tables` (batch_stark_prover.rs:1649-1727): host code in the
    C-ABI library, no GPU needed.  `cfg` is a `p3r_config` (e.g. `Context.cfg`), `airs` a list of
    dicts(kind, lanes, horner_packed_steps, coeff_lookups), `degree_bits` the verifier-side log2 trace
    height of every instance (the proof must declare the same).  Raises P3rError with the verifier's
    reason when the proof is rejected."""
    lib = _lib.load()
    arr = (_lib.P3rAirDesc * len(airs))()
    for i, a in enumerate(airs):
        arr[i].kind, arr[i].lanes = a["kind"], a.get("lanes", 1)
        arr[i].horner_packed_steps, arr[i].coeff_lookups = a.get("horner_packed_steps", 2), a.get("coeff_lookups", 0)
    cap, cap_p = _u32(preprocessed_commitment)
    if cap.size != 8 << cfg.cap_height:
        raise P3rError(-1, "preprocessed commitment must hold %d digests" % (1 << cfg.cap_height))
    if len(degree_bits) != len(airs):
        raise P3rError(-1, "degree_bits must have one entry per AIR (%d given, %d AIRs)" % (len(degree_bits), len(airs)))
    db, db_p = _u32(list(degree_bits) or [0])
    buf = (C.c_uint8 * max(len(proof), 1)).from_buffer_copy(proof if proof else b"\0")
    err = C.create_string_buffer(512)
    rc = lib.p3r_verify_batch(C.byref(cfg), arr, len(airs), cap_p, db_p, buf, len(proof), 1 if canonical_field_encoding else 0,
                              err, len(err))
    if rc != 0:
        raise P3rError(rc, err.value.decode())


def mmcs_verify(cfg, cap, dims, index, opened_values, proof, salts=None):
    """`Mmcs::verify_batch` on the host (p3r_mmcs_verify; no GPU): `dims` = (height, width) of the committed matrices in
    commit order, `opened_values` their opened rows concatenated, `proof` the sibling digests.  Honours cfg.mmcs_arity.
    `salts` (n_mats x cfg.mmcs_salt_elems): the hiding MMCS's opening (p3r_mmcs_verify_salted).
    Raises P3rError with the reason when the opening is rejected."""
    lib = _lib.load()
    c, cp = _u32(cap)
    o, op = _u32(opened_values)
    pf, pp = _u32(np.asarray(proof, dtype=np.uint32).reshape(-1, 8))
    n = len(dims)
    hs = (C.c_size_t * n)(*[int(d[0]) for d in dims])
    ws = (C.c_size_t * n)(*[int(d[1]) for d in dims])
    err = C.create_string_buffer(512)
    if salts is not None:
        sl, sp = _u32(np.asarray(salts, dtype=np.uint32).reshape(-1))
        if sl.size != n * cfg.mmcs_salt_elems:
            raise P3rError(-1, "salts must hold %d x %d values" % (n, cfg.mmcs_salt_elems))
        rc = lib.p3r_mmcs_verify_salted(C.byref(cfg), cp, n, hs, ws, int(index), op, sp, pp, pf.shape[0], err, len(err))
    else:
        rc = lib.p3r_mmcs_verify(C.byref(cfg), cp, n, hs, ws, int(index), op, pp, pf.shape[0], err, len(err))
    if rc != 0:
        raise P3rError(rc, err.value.decode())


class _HostSide:
    """What a Challenger needs of its owner when there is no context: the library, the challenge degree and the error
    text of p3r_last_error(NULL)."""
    h = None

    def __init__(self, cfg):
        self.lib, self.cfg, self.challenge_degree = _lib.load(), cfg, 5 if cfg.challenge_degree == 5 else 4

    def check(self, rc):
        if rc != 0:
            raise P3rError(rc, self.lib.p3r_last_error(None).decode())

    def ptr(self, p):
        if not p:
            raise P3rError(-1, self.lib.p3r_last_error(None).decode())
        return p


def host_challenger(cfg):
    """A fresh DuplexChallenger made from a p3r_config alone (p3r_challenger_create_host; no GPU): the transcript of
    Context.challenger() for the same configuration, word for word.  Only `grind` refuses it."""
    side = _HostSide(cfg)
    return Challenger(side, side.ptr(side.lib.p3r_challenger_create_host(C.byref(cfg))))


def fri_log_arity(cfg, phase, log_cur, log_final, log_next_input=-1):
    """Context.fri_log_arity from a p3r_config alone (p3r_fri_log_arity_cfg)."""
    return int(_lib.load().p3r_fri_log_arity_cfg(C.byref(cfg), int(phase), int(log_cur), int(log_final), int(log_next_input)))


def _fri_proof_view(cfg, proof, indices):
    """The p3r_fri_proof_view of a FriProof, and the arrays it points into.  `indices`: the query indices, which say what
    element of every opened row is the queried one (the view carries the row without it); None: rows are passed whole
    minus element 0 (the transcript entry does not read them)."""
    dc = 5 if cfg.challenge_degree == 5 else 4
    keep = []

    def arr(a, dtype=np.uint32):
        a = np.ascontiguousarray(np.asarray(a, dtype=dtype).reshape(-1))
        keep.append(a)
        return a.ctypes.data_as(C.POINTER(C.c_uint8 if dtype == np.uint8 else C.c_uint32)), a.size

    v = _lib.P3rFriProofView()
    v.log_max_height, v.query_pow = int(proof.log_max_height), int(proof.query_pow_witness)
    caps = [np.asarray(c, dtype=np.uint32).reshape(-1) for c in proof.commit_phase_caps]
    v.commit_caps, v.commit_caps_len = arr(np.concatenate(caps) if caps else [])
    v.commit_pow, v.commit_pow_len = arr(proof.commit_pow_witnesses)
    v.log_arities, v.log_arities_len = arr(proof.log_arities, np.uint8)
    v.final_poly, v.final_poly_len = arr(proof.final_poly if proof.final_poly is not None else [])
    nq = len(proof.query_openings)
    flat = [(q, ph, o) for q, openings in enumerate(proof.query_openings) for ph, o in enumerate(openings)]
    ops = (_lib.P3rFriPhaseOpeningView * max(1, len(flat)))()
    for k, (q, ph, o) in enumerate(flat):
        row = np.asarray(o.row, dtype=np.uint32).reshape(-1, dc)
        pos = 0
        if indices is not None and ph < len(proof.log_arities):
            shift = sum(int(a) for a in proof.log_arities[:ph])
            pos = (int(indices[q]) >> shift) & (row.shape[0] - 1) if row.shape[0] else 0
        ops[k].row, ops[k].row_len = arr(np.delete(row, pos, axis=0) if row.shape[0] else row)
        ops[k].salts, ops[k].salts_len = arr(o.salts if o.salts is not None else [])
        ops[k].siblings, ops[k].siblings_len = arr(o.siblings)
    keep.append(ops)
    v.openings, v.openings_len, v.n_queries = ops, len(flat), nq
    return v, keep


def fri_verify_transcript(cfg, ch, proof):
    """The transcript of verify_fri up to the query indices (p3r_fri_verify_transcript; no GPU): replays the FriProof
    `proof` on the challenger `ch`, checking both proofs of work.  Returns (betas[(n_phases, DC)], indices) and leaves `ch`
    where prove_fri left the prover's.  Raises P3rError (P3R_EVERIFY: rejected; P3R_EINVAL: malformed); `ch` then has not
    moved."""
    lib = _lib.load()
    dc = 5 if cfg.challenge_degree == 5 else 4
    view, keep = _fri_proof_view(cfg, proof, None)
    betas = np.zeros((max(1, len(proof.log_arities)), dc), dtype=np.uint32)
    idx = np.zeros(max(1, view.n_queries), dtype=np.uint32)
    rc = lib.p3r_fri_verify_transcript(C.byref(cfg), ch.h, C.byref(view), betas.ctypes.data_as(_lib.u32p), idx.ctypes.data_as(_lib.u32p))
    if rc != 0:
        raise P3rError(rc, lib.p3r_last_error(None).decode())
    return betas[:len(proof.log_arities)], [int(i) for i in idx[:view.n_queries]]


def fri_verify(cfg, ch, proof, inputs):
    """p3_fri::verifier::verify_fri on the host (p3r_fri_verify; no GPU).  `ch`: the challenger BEFORE the proof; `proof`: a
    FriProof; `inputs`: (log_height, values[(n_queries, DC)]) per input height, tallest first - values[q] the reduced
    opening of that height at index_q >> (log_max_height - log_height), the indices being fri_verify_transcript's on a
    clone of `ch`.  Accepted: returns None and leaves `ch` where the prover's challenger is.  Raises P3rError: P3R_EVERIFY
    with the rule and the place when the proof is rejected, P3R_EINVAL when it is malformed."""
    lib = _lib.load()
    # the queried element of every opened row is left out of the view; which one it is comes from the verifier's own
    # replay, never from the prover
    probe = ch.clone()
    try:
        _, indices = fri_verify_transcript(cfg, probe, proof)
    finally:
        probe.free()
    view, keep = _fri_proof_view(cfg, proof, indices)
    ins = (_lib.P3rFriInputView * max(1, len(inputs)))()
    for k, (log_h, values) in enumerate(inputs):
        a, p = _u32(np.asarray(values, dtype=np.uint32).reshape(-1))
        keep.append(a)
        ins[k].log_height, ins[k].values, ins[k].values_len = int(log_h), p, a.size
    rc = lib.p3r_fri_verify(C.byref(cfg), ch.h, C.byref(view), ins, len(inputs))
    if rc != 0:
        raise P3rError(rc, lib.p3r_last_error(None).decode())


class _ChallengeField:
    """The challenge field on Python integers, for the few elements a verifier's wrapper handles (num_queries rows): the
    quartic binomial extension x^4 = W (W = 3 / 11) or KoalaBear's quintic trinomial extension x^5 + x^2 - 1."""

    def __init__(self, field, dc):
        self.p, self.dc, self.w = MODULUS[field], dc, {"koala-bear": 3, "baby-bear": 11}[field]
        if dc == 5 and field != "koala-bear":
            raise P3rError(-5, "UnsupportedChallengeDegree: the quintic challenge field is KoalaBear's")

    def lift(self, x):
        return [int(x) % self.p] + [0] * (self.dc - 1)

    def add(self, a, b):
        return [(x + y) % self.p for x, y in zip(a, b)]

    def sub(self, a, b):
        return [(x - y) % self.p for x, y in zip(a, b)]

    def mul(self, a, b):
        p, dc = self.p, self.dc
        t = [0] * (2 * dc - 1)
        for i, x in enumerate(a):
            for j, y in enumerate(b):
                t[i + j] += x * y
        for k in range(2 * dc - 2, dc - 1, -1):   # x^k, k >= dc, in lower powers
            c = t[k] % p
            if dc == 4:
                t[k - 4] += c * self.w            # x^4 = W
            else:
                t[k - 5] += c                     # x^5 = 1 - x^2
                t[k - 3] -= c
        return [v % p for v in t[:dc]]

    def pow(self, a, e):
        r, b = self.lift(1), list(a)
        while e:
            if e & 1:
                r = self.mul(r, b)
            b = self.mul(b, b)
            e >>= 1
        return r

    def inv(self, a):
        if not any(a):
            raise P3rError(-1, "division by zero in the challenge field")
        return self.pow(a, self.p ** self.dc - 2)


def _bit_reverse(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def observe_opened_values(ch, values):
    """Observes the opened values of a PCS opening on the challenger `ch`: values[round][matrix] is (points, width, DC);
    rounds, matrices, points and columns in order, DC words per value - what Context.pcs_open observes before it samples
    alpha, and what the caller of pcs_verify observes for the claimed values."""
    for rnd in values:
        for v in rnd:
            ch.observe(np.asarray(v, dtype=np.uint32).reshape(-1))


def pcs_verify(cfg, ch, rounds, fri_proof, input_openings):
    """TwoAdicFriPcs::verify on the host, composed from public calls (no GPU).  `rounds`: per commitment a tuple
    (cap, dims, points, values) - the cap, the (LDE height, width) of its matrices in commit order, per matrix its (k, DC)
    opening points and its claimed (k, width, DC) values.  `fri_proof`: the FriProof; `input_openings`: per round
    (opened[(n_queries, total_width)], salts[(n_queries, n_mats, S)] or None, siblings[(n_queries, depth, 8)]) - what
    MerkleTree.open_many gave at index_q >> (log_max_height - the round's tallest height).  `ch`: the challenger after the
    caller observed the claimed values (observe_opened_values); this call observes nothing itself: it samples alpha,
    replays the FRI transcript on a clone for the query indices, checks every input opening with mmcs_verify, forms the
    reduced openings with the formula of p3r_fri_reduce_dmat on Python integers, and calls fri_verify, which leaves `ch`
    where the prover's challenger is.  Raises P3rError: P3R_EVERIFY with the rule and the place for a rejected opening,
    P3R_EINVAL for a malformed one."""
    field = [k for k, v in FIELD_IDS.items() if v == cfg.field][0]
    dc = 5 if cfg.challenge_degree == 5 else 4
    E, p, g = _ChallengeField(field, dc), MODULUS[field], GENERATOR[field]
    if len(input_openings) != len(rounds) or not rounds:
        raise P3rError(-1, "one input opening per round (%d given, %d rounds)" % (len(input_openings), len(rounds)))
    alpha = [int(v) for v in ch.sample_ext()]
    logs = [[int(h).bit_length() - 1 for h, w in dims] for cap, dims, points, values in rounds]
    log_max = max(max(l) for l in logs)
    if int(fri_proof.log_max_height) != log_max:
        raise P3rError(-1, "the FRI proof is over 2^%d rows, the tallest committed matrix has 2^%d" % (fri_proof.log_max_height, log_max))
    probe = ch.clone()
    try:
        _, indices = fri_verify_transcript(cfg, probe, fri_proof)
    finally:
        probe.free()
    max_w = max(int(w) for cap, dims, points, values in rounds for h, w in dims)
    apow = [E.lift(1)]
    for _ in range(max_w):
        apow.append(E.mul(apow[-1], alpha))
    heights = sorted({l for ls in logs for l in ls}, reverse=True)
    reduced = {l: [E.lift(0) for _ in indices] for l in heights}
    for q, index in enumerate(indices):
        running = {l: E.lift(1) for l in heights}   # one running alpha power per height, restarted per query
        for r, ((cap, dims, points, values), (opened, salts, siblings)) in enumerate(zip(rounds, input_openings)):
            opened = np.asarray(opened, dtype=np.uint32)
            if opened.shape[0] != len(indices) or opened.shape[1] != sum(int(w) for h, w in dims):
                raise P3rError(-1, "round %d: opened rows must be (n_queries, total width)" % r)
            try:
                mmcs_verify(cfg, cap, dims, index >> (log_max - max(logs[r])), opened[q], np.asarray(siblings)[q],
                            salts=None if salts is None else np.asarray(salts)[q])
            except P3rError as e:
                raise P3rError(_lib.P3R_EVERIFY if "mismatch" in str(e) else e.code, "input batch %d of query %d: %s" % (r, q, e)) from None
            at = 0
            for m, ((h, w), l) in enumerate(zip(dims, logs[r])):
                row = [int(v) for v in opened[q, at:at + int(w)]]
                at += int(w)
                pts = np.asarray(points[m], dtype=np.uint32).reshape(-1, dc)
                vals = np.asarray(values[m], dtype=np.uint32).reshape(len(pts), int(w), dc)
                if not len(pts) or not int(w):
                    continue   # adds nothing and does not advance the running power (p3r_fri_reduce_dmat)
                x = g * pow(pow(g, (p - 1) >> l, p), _bit_reverse(index >> (log_max - l), l), p) % p
                s_row = E.lift(0)
                for c, cell in enumerate(row):
                    s_row = E.add(s_row, [a * cell % p for a in apow[c]])
                for k, z in enumerate(pts):
                    v_pt = E.lift(0)
                    for c in range(int(w)):
                        v_pt = E.add(v_pt, E.mul(apow[c], [int(t) for t in vals[k, c]]))
                    quot = E.mul(E.sub(v_pt, s_row), E.inv(E.sub([int(t) for t in z], E.lift(x))))
                    reduced[l][q] = E.add(reduced[l][q], E.mul(running[l], quot))
                    running[l] = E.mul(running[l], apow[int(w)])
    fri_verify(cfg, ch, fri_proof, [(l, np.array(reduced[l], dtype=np.uint32)) for l in heights])


class AirValue:
    """A value of an AirBuilder program: the id of the instruction that defines it.  + - * and unary - record
    instructions; a Python int operand becomes a constant (reduced into the field)."""

    def __init__(self, builder, idx):
        self.builder, self.idx = builder, idx

    def _lift(self, o):
        if isinstance(o, AirValue):
            if o.builder is not self.builder:
                raise P3rError(-1, "a value of another AirBuilder")
            return o
        return self.builder.const(int(o) % self.builder.p)

    def __add__(self, o):
        return self.builder._emit(_lib.P3R_AIR_ADD, self.idx, self._lift(o).idx)

    def __radd__(self, o):
        return self._lift(o) + self

    def __sub__(self, o):
        return self.builder._emit(_lib.P3R_AIR_SUB, self.idx, self._lift(o).idx)

    def __rsub__(self, o):
        return self._lift(o) - self

    def __mul__(self, o):
        return self.builder._emit(_lib.P3R_AIR_MUL, self.idx, self._lift(o).idx)

    def __rmul__(self, o):
        return self._lift(o) * self

    def __neg__(self):
        return self.builder._emit(_lib.P3R_AIR_NEG, self.idx, 0)


class AirBuilder:
    """The SymbolicAirBuilder of the seam: an AIR's `eval` written against this object records the straight-line
    p3r_air_insn program Context.quotient_device evaluates (include/p3r.h has the format and the semantics).  Values are
    base-field or challenge-field elements; the type follows from the operands.  Nothing is checked here: the library
    validates a program (air_program_info, quotient_device)."""

    def __init__(self, field="koala-bear"):
        self.field, self.p, self.insns = field, MODULUS[field], []

    def _emit(self, op, a=0, b=0):
        self.insns.append((int(op), int(a), int(b)))
        return AirValue(self, len(self.insns) - 1)

    def const(self, word):
        return self._emit(_lib.P3R_AIR_CONST, word)

    def public(self, index):
        return self._emit(_lib.P3R_AIR_PUBLIC, index)

    def challenge(self, index):
        return self._emit(_lib.P3R_AIR_CHALLENGE, index)

    def local(self, matrix, column):
        return self._emit(_lib.P3R_AIR_LOCAL, matrix, column)

    def next(self, matrix, column):
        return self._emit(_lib.P3R_AIR_NEXT, matrix, column)

    def local_ext(self, matrix, column):
        """The extension element stored flattened in DC consecutive columns from `column` on."""
        return self._emit(_lib.P3R_AIR_LOCAL_EXT, matrix, column)

    def next_ext(self, matrix, column):
        return self._emit(_lib.P3R_AIR_NEXT_EXT, matrix, column)

    def is_first_row(self):
        return self._emit(_lib.P3R_AIR_IS_FIRST_ROW)

    def is_last_row(self):
        return self._emit(_lib.P3R_AIR_IS_LAST_ROW)

    def is_transition(self):
        return self._emit(_lib.P3R_AIR_IS_TRANSITION)

    def assert_zero(self, value):
        self._emit(_lib.P3R_AIR_ASSERT_ZERO, value.idx)

    def lookup(self, multiplicity, denominator):
        """A lookup program's sink: adds the term multiplicity / denominator to the open auxiliary column (and opens one if
        none is open).  Python ints become constants."""
        m, d = [v if isinstance(v, AirValue) else self.const(int(v) % self.p) for v in (multiplicity, denominator)]
        self._emit(_lib.P3R_AIR_LOOKUP, m.idx, d.idx)

    def end_lookup_column(self):
        """Closes the open auxiliary column of a lookup program."""
        self._emit(_lib.P3R_AIR_LOOKUP_END)

    # ---- a witness program (Context.witness_device): values become the columns of a new trace
    def _value(self, v):
        return v if isinstance(v, AirValue) else self.const(int(v) % self.p)

    def inv(self, value):
        """The inverse of a base or extension value, and 0 for 0: the witness of an is-zero gadget."""
        return self._emit(_lib.P3R_AIR_INV, self._value(value).idx)

    def bits(self, value, lo, n):
        """Bits [lo, lo + n) of the canonical word of a base value (n >= 1, lo + n <= 31)."""
        return self._emit(_lib.P3R_AIR_BITS, self._value(value).idx, int(lo) | int(n) << 8)

    def row(self):
        """The row index, as a base value."""
        return self._emit(_lib.P3R_AIR_ROW)

    def store(self, value, column):
        """A witness program's sink: a base value fills output column `column`, an extension value the columns
        column .. column + DC (coefficient k in column + k, the flattening local_ext reads).  Python ints become constants."""
        self._emit(_lib.P3R_AIR_STORE, self._value(value).idx, column)

    def program(self):
        """The instructions as an (n, 3) uint32 array of (op, a, b)."""
        return np.array(self.insns, dtype=np.uint32).reshape(-1, 3)


def _lookup_instances(instances):
    """(P3rLookupInstance array, what its pointers keep alive) for (program, dmats[, public_values]) tuples."""
    arr = (_lib.P3rLookupInstance * max(1, len(instances)))()
    keep = []
    for k, inst in enumerate(instances):
        program, dmats = inst[0], inst[1]
        insns, n = _air_insns(program)
        mats = (C.c_void_p * max(1, len(dmats)))(*[d.h for d in dmats])
        pv, pvp = _u32(np.asarray(inst[2] if len(inst) > 2 else (), dtype=np.uint32).reshape(-1))
        keep.append((insns, mats, pv))
        arr[k].prog, arr[k].n_insns = insns, n
        arr[k].mats, arr[k].n_mats = mats, len(dmats)
        arr[k].public_values, arr[k].n_public = pvp, pv.size
    return arr, keep


def _lookup_entries(out, n, dc):
    return [{"instance": int(e.instance), "row": int(e.row), "term": int(e.term), "n_records": int(e.n_records),
             "denominator": [int(v) for v in e.denominator[:dc]], "net": [int(v) for v in e.net[:dc]]} for e in out[:n]]


def _air_insns(program):
    prog = program.program() if isinstance(program, AirBuilder) else np.ascontiguousarray(program, dtype=np.uint32).reshape(-1, 3)
    arr = (_lib.P3rAirInsn * max(1, len(prog)))()
    for i, (op, a, b) in enumerate(prog.tolist()):
        arr[i].op, arr[i].a, arr[i].b = op, a, b
    return arr, len(prog)


def air_program_info(cfg, program, widths):
    """p3r_air_program_info on the host (no GPU): validates `program` (an AirBuilder or an (n, 3) array of (op, a, b))
    against the matrix `widths` under the field and challenge degree of the p3r_config `cfg`; returns a dict of
    n_constraints, max_degree, log_quotient_degree (the smallest the program may be evaluated with) and peak_live.
    Raises P3rError with the reason when the program is refused."""
    lib = _lib.load()
    arr, n = _air_insns(program)
    ws = (C.c_size_t * max(1, len(widths)))(*[int(w) for w in widths])
    info = _lib.P3rAirInfo()
    rc = lib.p3r_air_program_info(C.byref(cfg), arr, n, ws, len(widths), C.byref(info))
    if rc != 0:
        raise P3rError(rc, lib.p3r_last_error(None).decode())
    return {k: int(getattr(info, k)) for k, _ in _lib.P3rAirInfo._fields_}


def air_program_eval(cfg, program, widths, local, next, log_height, zeta, public_values=(), challenges=(), alpha=None):
    """p3r_air_program_eval on the host (no GPU): the constraint `program` at the out-of-domain point `zeta` from opened
    values.  `local` / `next`: (sum(widths), DC) canonical words, the opened values at zeta and zeta * w_h, matrices in
    order; `alpha`: DC words.  Returns (folded, inv_zh), DC words each: the Horner fold of the constraints with alpha and
    1 / (zeta^h - 1).  Raises P3rError: what air_program_info refuses, index ranges, non-canonical words, and a zeta
    with zeta^h == 1, zeta == 1 or zeta == w_h^-1."""
    lib = _lib.load()
    dc = 5 if cfg.challenge_degree == 5 else 4
    arr, n = _air_insns(program)
    ws = (C.c_size_t * max(1, len(widths)))(*[int(w) for w in widths])
    lo, lop = _u32(np.asarray(local, dtype=np.uint32).reshape(-1))
    nx, nxp = _u32(np.asarray(next, dtype=np.uint32).reshape(-1))
    total = sum(int(w) for w in widths) * dc
    if lo.size != total or nx.size != total:
        raise P3rError(-1, "the opened values must hold sum(widths) x DC = %d words (%d and %d given)" % (total, lo.size, nx.size))
    z, zp = _u32(np.asarray(zeta, dtype=np.uint32).reshape(dc))
    pv, pvp = _u32(np.asarray(public_values, dtype=np.uint32).reshape(-1))
    chs, chp = _u32(np.asarray(challenges, dtype=np.uint32).reshape(-1, dc))
    al, alp = _u32(np.asarray(alpha, dtype=np.uint32).reshape(dc))
    folded, inv_zh = np.zeros(dc, dtype=np.uint32), np.zeros(dc, dtype=np.uint32)
    rc = lib.p3r_air_program_eval(C.byref(cfg), arr, n, ws, len(widths), lop, nxp, int(log_height), zp, pvp, pv.size, chp, len(chs), alp,
                                  folded.ctypes.data_as(_lib.u32p), inv_zh.ctypes.data_as(_lib.u32p))
    if rc != 0:
        raise P3rError(rc, lib.p3r_last_error(None).decode())
    return folded, inv_zh


def lookup_program_info(cfg, program, widths):
    """p3r_lookup_program_info on the host (no GPU): validates the lookup `program` (an AirBuilder or an (n, 3) array of
    (op, a, b)) against the matrix `widths` under the field and challenge degree of the p3r_config `cfg`; returns a dict of
    n_terms, n_columns, max_terms_per_column, max_constraint_degree (the largest degree of a column's constraint: what
    the quotient must admit) and peak_live.  Raises P3rError with the reason when the program is refused."""
    lib = _lib.load()
    arr, n = _air_insns(program)
    ws = (C.c_size_t * max(1, len(widths)))(*[int(w) for w in widths])
    info = _lib.P3rLookupInfo()
    rc = lib.p3r_lookup_program_info(C.byref(cfg), arr, n, ws, len(widths), C.byref(info))
    if rc != 0:
        raise P3rError(rc, lib.p3r_last_error(None).decode())
    return {k: int(getattr(info, k)) for k, _ in _lib.P3rLookupInfo._fields_}


def witness_program_info(cfg, program, widths):
    """p3r_witness_program_info on the host (no GPU): validates the witness `program` (an AirBuilder or an (n, 3) array of
    (op, a, b)) against the matrix `widths` (none for a program without inputs) under the field and challenge degree of
    the p3r_config `cfg`; returns a dict of n_stores, n_out_columns (the width of the matrix witness_device returns),
    n_inversions and peak_live.  Raises P3rError with the reason when the program is refused."""
    lib = _lib.load()
    arr, n = _air_insns(program)
    ws = (C.c_size_t * max(1, len(widths)))(*[int(w) for w in widths])
    info = _lib.P3rWitnessInfo()
    rc = lib.p3r_witness_program_info(C.byref(cfg), arr, n, ws, len(widths), C.byref(info))
    if rc != 0:
        raise P3rError(rc, lib.p3r_last_error(None).decode())
    return {k: int(getattr(info, k)) for k, _ in _lib.P3rWitnessInfo._fields_}


class Recurrence:
    """One p3r_recurrence of Context.affine_scan_device: s[0] = init, s[r + 1] = a[r] * s[r] + b[r].  `mul` and `add` are
    (matrix, column) pairs - the first of DC consecutive columns with ext=True - or None: no `mul` is a = 1 everywhere (a
    running sum), no `add` is b = 0 everywhere (a running product).  `out_col`: the (first) output column.  `init`: a
    canonical word, or up to DC of them for an extension recurrence.  `inclusive`: row r holds s[r + 1] instead of s[r]."""

    def __init__(self, out_col, mul=None, add=None, init=0, ext=False, inclusive=False):
        self.out_col, self.mul, self.add, self.ext, self.inclusive = int(out_col), mul, add, bool(ext), bool(inclusive)
        self.init = [int(v) for v in np.atleast_1d(init)]

    def raw(self):
        none = (_lib.P3R_SCAN_NONE, 0)
        (mm, mc), (am, ac) = self.mul or none, self.add or none
        if len(self.init) > 5:
            raise ValueError("init has at most 5 words")
        return _lib.P3rRecurrence((_lib.P3R_SCAN_EXT if self.ext else 0) | (_lib.P3R_SCAN_INCLUSIVE if self.inclusive else 0),
                                  int(mm), int(mc), int(am), int(ac), self.out_col, (C.c_uint32 * 5)(*self.init))


def _recurrences(recurrences):
    """(array of p3r_recurrence, n) from Recurrence objects, dicts of Recurrence's arguments or raw P3rRecurrence structs."""
    raws = [r if isinstance(r, _lib.P3rRecurrence) else (Recurrence(**r) if isinstance(r, dict) else r).raw() for r in recurrences]
    return (_lib.P3rRecurrence * max(1, len(raws)))(*raws), len(raws)


def affine_scan_info(cfg, recurrences, widths):
    """p3r_affine_scan_info on the host (no GPU): validates the `recurrences` (as Context.affine_scan_device takes them)
    against the matrix `widths` under the field and challenge degree of the p3r_config `cfg`; returns a dict of
    n_out_columns (the width of the matrix affine_scan_device returns), n_products, n_sums and n_affine.  Raises P3rError
    with the reason when they are refused."""
    lib = _lib.load()
    arr, n = _recurrences(recurrences)
    ws = (C.c_size_t * max(1, len(widths)))(*[int(w) for w in widths])
    info = _lib.P3rScanInfo()
    rc = lib.p3r_affine_scan_info(C.byref(cfg), arr, n, ws, len(widths), C.byref(info))
    if rc != 0:
        raise P3rError(rc, lib.p3r_last_error(None).decode())
    return {k: int(getattr(info, k)) for k, _ in _lib.P3rScanInfo._fields_}


class Context:
    """One per GPU; not thread-safe; one call in flight (include/p3r.h)."""

    def __init__(self, field="koala-bear", log_blowup=2, max_log_arity=2, cap_height=0,
                 log_final_poly_len=5, commit_pow_bits=0, query_pow_bits=15, num_queries=54,
                 device=0, poseidon2_rc=None, ext_choices=0, fri_log_arities=None, proof_layout=None, ext_degree=4, ext_w=0,
                 challenge_degree=4, poseidon2_w32_rc=None, poseidon2_w32_diag=None, mmcs_arity=2, zk=0,
                 num_random_codewords=2, zk_seed=None, zk_key=None, zk_deterministic=None, allow_unpinned_w32_defaults=False,
                 mmcs_salt_elems=0):
        self.lib = _lib.load()
        self.mmcs_arity = mmcs_arity
        self.zk = int(zk)
        self.field = field
        self.ext_degree = ext_degree
        self.ext_w = ext_w
        self.challenge_degree = challenge_degree
        self.p = MODULUS[field]
        cfg, self._rc_keep = make_config(field, log_blowup, max_log_arity, cap_height, log_final_poly_len,
                                         commit_pow_bits, query_pow_bits, num_queries, device, poseidon2_rc, ext_choices,
                                         fri_log_arities, proof_layout, ext_degree, ext_w, challenge_degree,
                                         poseidon2_w32_rc, poseidon2_w32_diag, mmcs_arity, zk, num_random_codewords, zk_seed,
                                         zk_key, zk_deterministic, allow_unpinned_w32_defaults, mmcs_salt_elems)
        self.cfg = cfg
        self.cap_height = cap_height
        self.log_blowup = log_blowup
        self.h = self.lib.p3r_create(C.byref(cfg))
        if not self.h:
            raise P3rError(-2, self.lib.p3r_last_error(None).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.p3r_destroy(self.h)
            self.h = None

    @property
    def zk_nonce(self):
        """Proofs made so far under a ZK configuration (the hiding PCS's RNG state: p3r_zk_nonce)."""
        return int(self.lib.p3r_zk_nonce(self.h))

    @zk_nonce.setter
    def zk_nonce(self, v):
        self.check(self.lib.p3r_zk_set_nonce(self.h, C.c_uint64(int(v))))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        if rc != 0:
            raise P3rError(rc, self.lib.p3r_last_error(self.h).decode())

    def ptr(self, p):
        if not p:
            raise P3rError(-1, self.lib.p3r_last_error(self.h).decode())
        return p

    def sync(self):
        self.check(self.lib.p3r_sync(self.h))

    @property
    def poseidon2_trace_width(self):
        return self.lib.p3r_poseidon2_trace_width(self.h)

    # ---- matrices
    def upload(self, rowmajor):
        a, p = _u32(rowmajor)
        assert a.ndim == 2
        return DeviceMatrix(self, self.ptr(self.lib.p3r_dmat_upload(self.h, p, a.shape[0], a.shape[1])))

    # ---- Poseidon2
    def permute_batch(self, states):
        a, p = _u32(states)
        assert a.ndim == 2 and a.shape[1] == 16
        out = np.empty_like(a)
        self.check(self.lib.p3r_poseidon2_permute_batch(self.h, p, out.ctypes.data_as(_lib.u32p), a.shape[0]))
        return out

    def _p2_rows(self, inputs, new_start, merkle_path, mmcs_bit, mmcs_index_sum):
        keep = []
        rows = _lib.P3rP2Rows()
        a, rows.input_values = _u32(inputs)
        keep.append(a)
        rows.n = a.shape[0]
        for name, v in (("new_start", new_start), ("merkle_path", merkle_path), ("mmcs_bit", mmcs_bit)):
            b, p = _u8(v)
            keep.append(b)
            setattr(rows, name, p)
        b, rows.mmcs_index_sum = _u32(mmcs_index_sum)
        keep.append(b)
        return rows, keep

    def generate_trace_rows(self, inputs, new_start, merkle_path, mmcs_bit, mmcs_index_sum):
        rows, keep = self._p2_rows(inputs, new_start, merkle_path, mmcs_bit, mmcs_index_sum)
        out = np.empty((rows.n, self.poseidon2_trace_width), dtype=np.uint32)
        self.check(self.lib.p3r_poseidon2_trace_fill(self.h, C.byref(rows), out.ctypes.data_as(_lib.u32p)))
        return out

    def generate_trace_rows_device(self, inputs, new_start, merkle_path, mmcs_bit, mmcs_index_sum):
        rows, keep = self._p2_rows(inputs, new_start, merkle_path, mmcs_bit, mmcs_index_sum)
        return DeviceMatrix(self, self.ptr(self.lib.p3r_poseidon2_trace_fill_dmat(self.h, C.byref(rows))))

    # ---- the width-32 permutation (the arity-4 MMCS) and its table's trace rows (include/p3r.h, ABI 6)
    def poseidon2_w32_permute_batch(self, states):
        a, p = _u32(states)
        if a.ndim != 2 or a.shape[1] != 32:
            raise P3rError(-1, "states must have shape (n, 32)")
        out = np.empty_like(a)
        self.check(self.lib.p3r_poseidon2_w32_permute_batch(self.h, p, out.ctypes.data_as(_lib.u32p), a.shape[0]))
        return out

    def generate_w32_trace_rows(self, inputs, new_start, merkle_path, mmcs_bit, mmcs_bit2, mmcs_index_sum, height=None):
        """Poseidon2CircuitAir::generate_trace_rows of the arity-4 layout; rows are padded to `height` (a power of two)
        with filler rows (new_start = 1, zero state)."""
        a = np.ascontiguousarray(inputs, dtype=np.uint32).reshape(-1, 32)
        n = a.shape[0]
        h = height or (1 << max(n - 1, 0).bit_length())

        def pad(x, fill, dt):   # explicit shapes: n == 0 (a table of filler rows only) has no rows to take the width from
            x = np.asarray(x, dt)
            w = 32 if x.ndim == 2 else 1
            return np.concatenate([x.reshape(n, w), np.full((h - n, w), fill, dt)])
        rows = _lib.P3rP2wRows()
        keep = []

        def put(name, arr, ptr_of):
            x, p = ptr_of(np.ascontiguousarray(arr))
            keep.append(x)
            setattr(rows, name, p)
        rows.n = h
        put("input_values", pad(a, 0, np.uint32), _u32)
        put("new_start", pad(new_start, 1, np.uint8).reshape(-1), _u8)
        put("merkle_path", pad(merkle_path, 0, np.uint8).reshape(-1), _u8)
        put("mmcs_bit", pad(mmcs_bit, 0, np.uint8).reshape(-1), _u8)
        put("mmcs_bit2", pad(mmcs_bit2, 0, np.uint8).reshape(-1), _u8)
        put("mmcs_index_sum", pad(mmcs_index_sum, 0, np.uint32).reshape(-1), _u32)
        out = np.empty((h, int(self.lib.p3r_poseidon2_w32_trace_width(self.h))), dtype=np.uint32)
        self.check(self.lib.p3r_poseidon2_w32_trace_fill(self.h, C.byref(rows), out.ctypes.data_as(_lib.u32p)))
        return out

    def upload_p2_rows(self, inputs, new_start, merkle_path, mmcs_bit, mmcs_index_sum):
        rows, keep = self._p2_rows(inputs, new_start, merkle_path, mmcs_bit, mmcs_index_sum)
        return DeviceP2Rows(self, self.ptr(self.lib.p3r_p2_rows_upload(self.h, C.byref(rows))))

    def generate_trace_rows_resident(self, dev_rows):
        return DeviceMatrix(self, self.ptr(self.lib.p3r_poseidon2_trace_fill_dev(self.h, dev_rows.h)))

    # ---- LDE
    def coset_lde_batch(self, evals, added_bits, shift):
        a, p = _u32(evals)
        out = np.empty((a.shape[0] << added_bits, a.shape[1]), dtype=np.uint32)
        self.check(self.lib.p3r_coset_lde(self.h, p, a.shape[0], a.shape[1], added_bits, shift,
                                          out.ctypes.data_as(_lib.u32p)))
        return out

    def coset_lde_batch_device(self, dmat, added_bits, shift):
        return DeviceMatrix(self, self.ptr(self.lib.p3r_coset_lde_dmat(self.h, dmat.h, added_bits, shift)))

    # ---- DFT: the two halves of the LDE on their own
    def dft_batch(self, mats, inverse=False, shifts=None, bit_reversed=False):
        """TwoAdicSubgroupDft::dft_batch (`inverse`: idft_batch; `shifts`: coset_dft_batch / coset_idft_batch, one
        canonical shift per matrix or one for all) over host matrices (2-D uint32 arrays, one polynomial per column,
        canonical words).  Coefficients are in natural order; `bit_reversed` says whether evaluation row i is the point
        shift * w^bitrev(i) instead of shift * w^i - the output of a forward call, the input of an inverse one.
        Returns the list of transformed matrices."""
        outs = []
        for m, s in zip(mats, self._dft_shifts(shifts, len(mats))):
            a, p = _u32(m)
            assert a.ndim == 2
            out = np.empty(a.shape, dtype=np.uint32)
            self.check(self.lib.p3r_dft(self.h, p, a.shape[0], a.shape[1], _lib.P3R_DFT_INVERSE if inverse else _lib.P3R_DFT_FORWARD,
                                        s, _lib.P3R_DFT_BITREV if bit_reversed else _lib.P3R_DFT_NATURAL,
                                        out.ctypes.data_as(_lib.u32p)))
            outs.append(out)
        return outs

    def dft_batch_device(self, dmats, inverse=False, shifts=None, bit_reversed=False):
        """The same over DeviceMatrix handles, all matrices in one call (one launch per pass whatever their heights);
        the inputs are left as they are, the results are new DeviceMatrix objects."""
        n = len(dmats)
        arr = (C.c_void_p * n)(*[d.h for d in dmats])
        sh, sp = _u32(self._dft_shifts(shifts, n))
        outs = (C.c_void_p * n)()
        self.check(self.lib.p3r_dft_batch_dmat(self.h, arr, n, _lib.P3R_DFT_INVERSE if inverse else _lib.P3R_DFT_FORWARD, sp,
                                               _lib.P3R_DFT_BITREV if bit_reversed else _lib.P3R_DFT_NATURAL, outs))
        return [DeviceMatrix(self, self.ptr(h)) for h in outs]

    @staticmethod
    def _dft_shifts(shifts, n):
        if shifts is None:
            return [1] * n
        if np.ndim(shifts) == 0:
            return [int(shifts)] * n
        if len(shifts) != n:
            raise P3rError(-1, "one shift per matrix")
        return [int(s) for s in shifts]

    # ---- the value half of Pcs::open
    def open_points(self, mats, points, added_bits=0, shift=None, bit_reversed=True):
        """The opened values of TwoAdicFriPcs::open over host matrices (2-D uint32 arrays, canonical): every column of
        mats[i] - rows 0 .. h >> added_bits of a bit-reversed LDE (`bit_reversed`), or rows k << added_bits of a
        natural-order one, taken as evaluations over shift * <w> - at the points points[i], a (k_i, DC) array of
        canonical words (DC = the context's challenge degree).  `shift` None: the field's generator.  Returns a list of
        (k_i, w_i, DC) arrays.  A point in the evaluation coset is refused (P3R_EINVAL)."""
        keep = []
        arr = (_lib.P3rMatrix * max(1, len(mats)))()
        for i, m in enumerate(mats):
            a, p = _u32(m)
            assert a.ndim == 2
            keep.append(a)
            arr[i].values, arr[i].height, arr[i].width = p, a.shape[0], a.shape[1]
        return self._open_points(self.lib.p3r_open_points, arr, [a.shape[1] for a in keep], points, added_bits, shift, bit_reversed)

    def open_points_device(self, dmats, points, added_bits=0, shift=None, bit_reversed=True):
        """The same over DeviceMatrix handles (what coset_lde_batch_device returns and commit_device commits): all
        matrices and points in one call - one weights launch, one dot launch, one reduce launch, one wait."""
        arr = (C.c_void_p * max(1, len(dmats)))(*[d.h for d in dmats])
        return self._open_points(self.lib.p3r_open_points_dmat, arr, [d.shape[1] for d in dmats], points, added_bits, shift, bit_reversed)

    def _open_points(self, fn, arr, widths, points, added_bits, shift, bit_reversed):
        n, dc = len(widths), self.challenge_degree
        if len(points) != n:
            raise P3rError(-1, "one array of points per matrix")
        pts = [np.ascontiguousarray(p, dtype=np.uint32).reshape(-1, dc) for p in points]
        offs = (C.c_size_t * (n + 1))(*np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.int64).tolist())
        flat, fp = _u32(np.concatenate(pts + [np.empty((0, dc), dtype=np.uint32)]))
        out = np.empty(sum(len(p) * w for p, w in zip(pts, widths)) * dc, dtype=np.uint32)
        self.check(fn(self.h, arr, n, added_bits, 0 if shift is None else int(shift),
                      _lib.P3R_DFT_BITREV if bit_reversed else _lib.P3R_DFT_NATURAL, offs, fp, out.ctypes.data_as(_lib.u32p)))
        res, at = [], 0
        for p, w in zip(pts, widths):
            res.append(out[at:at + len(p) * w * dc].reshape(len(p), w, dc))
            at += len(p) * w * dc
        return res

    # ---- the reduced openings of Pcs::open, and FriFoldingStrategy::fold_matrix with the roll-in
    def fri_reduce_device(self, dmats, points, values, alpha, shift=None):
        """The per-height reduced openings FRI starts from: dmats[i] is a whole committed LDE (bit-reversed rows over
        shift * <w>; `shift` None: the field's generator), points[i] its (k_i, DC) opening points, values[i] its
        (k_i, w_i, DC) opened values - exactly what open_points_device returned for the same matrices and points - and
        `alpha` the DC canonical words of the batching challenge.  Returns a list of (H, DC) DeviceMatrix, one per
        distinct height that has a point, tallest first; column k is coefficient k, rows stay in the committed order."""
        n, dc = len(dmats), self.challenge_degree
        if len(points) != n or len(values) != n:
            raise P3rError(-1, "one array of points and one of values per matrix")
        pts = [np.ascontiguousarray(p, dtype=np.uint32).reshape(-1, dc) for p in points]
        vals = [np.ascontiguousarray(v, dtype=np.uint32).reshape(-1) for v in values]
        for d, p, v in zip(dmats, pts, vals):
            if v.size != len(p) * d.shape[1] * dc:
                raise P3rError(-1, "values of a matrix must be (points, width, DC)")
        arr = (C.c_void_p * max(1, n))(*[d.h for d in dmats])
        offs = (C.c_size_t * (n + 1))(*np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.int64).tolist())
        flat, fp = _u32(np.concatenate(pts + [np.empty((0, dc), dtype=np.uint32)]))
        vflat, vp = _u32(np.concatenate(vals + [np.empty(0, dtype=np.uint32)]))
        al, ap = _u32(np.asarray(alpha, dtype=np.uint32).reshape(dc))
        outs = (C.c_void_p * max(1, n))()
        n_outs = C.c_size_t(0)
        self.check(self.lib.p3r_fri_reduce_dmat(self.h, arr, n, 0 if shift is None else int(shift), offs, fp, vp, ap, outs,
                                                C.byref(n_outs)))
        return [DeviceMatrix(self, self.ptr(outs[i])) for i in range(n_outs.value)]

    def fri_fold_device(self, dmat, log_arity, beta, roll_in=None):
        """FriFoldingStrategy::fold_matrix of TwoAdicFriFolding, then the roll-in: `dmat` is (n, DC), row i the value at
        w_n^bitrev(i); row r of the result is `log_arity` (1 .. 4) sequential arity-2 folds of rows r << log_arity ..
        with beta, beta^2, beta^4, .., plus beta^(2^log_arity) * roll_in[r] when `roll_in` ((n >> log_arity, DC)) is
        given.  Returns a new DeviceMatrix; the inputs are left as they are."""
        b, bp = _u32(np.asarray(beta, dtype=np.uint32).reshape(self.challenge_degree))
        out = C.c_void_p()
        self.check(self.lib.p3r_fri_fold_dmat(self.h, dmat.h, log_arity, bp, None if roll_in is None else roll_in.h, C.byref(out)))
        return DeviceMatrix(self, self.ptr(out.value))

    # ---- the caller's AIR: quotient_values + split_evals for a constraint program
    def air_program_info(self, program, widths):
        """air_program_info under this context's field and challenge degree."""
        return air_program_info(self.cfg, program, widths)

    def quotient_device(self, program, dmats, added_bits, log_quotient_degree, alpha, public_values=(), challenges=(), shift=None):
        """The quotient chunks of the AIR `program` (an AirBuilder or an (n, 3) array of (op, a, b)) over the committed LDEs
        `dmats` - one height, blow-up 2^added_bits, bit-reversed rows over shift * <w> as coset_lde_batch_device returns
        them (`shift` None: the field's generator); only their first h << log_quotient_degree rows are read.
        `public_values`: canonical words; `challenges`: (n, DC) canonical words; `alpha`: the DC words of the constraint
        folding challenge.  Returns 2^log_quotient_degree new (h, DC) DeviceMatrix: row r of chunk c is the quotient at
        (shift * w_N^c) * w_h^r - what split_evals returns; coset_lde_batch_device(chunk, added_bits, G / (shift * w_N^c))
        extends it onto the commit coset.  The inputs are left as they are."""
        dc = self.challenge_degree
        arr, n = _air_insns(program)
        mats = (C.c_void_p * max(1, len(dmats)))(*[d.h for d in dmats])
        pv, pvp = _u32(np.asarray(public_values, dtype=np.uint32).reshape(-1))
        ch, chp = _u32(np.asarray(challenges, dtype=np.uint32).reshape(-1, dc))
        al, alp = _u32(np.asarray(alpha, dtype=np.uint32).reshape(dc))
        n_out = 1 << min(int(log_quotient_degree), 4)   # a larger log_quotient_degree is refused by the library
        outs = (C.c_void_p * n_out)()
        self.check(self.lib.p3r_quotient_program_dmat(self.h, arr, n, mats, len(dmats), int(added_bits), 0 if shift is None else int(shift),
                                                      int(log_quotient_degree), pvp, pv.size, chp, len(ch), alp, outs))
        return [DeviceMatrix(self, self.ptr(h)) for h in outs]

    # ---- the caller's lookups: the LogUp permutation trace for a lookup program
    def lookup_program_info(self, program, widths):
        """lookup_program_info under this context's field and challenge degree."""
        return lookup_program_info(self.cfg, program, widths)

    def logup_device(self, program, dmats, public_values=(), challenges=()):
        """The LogUp auxiliary trace of the lookup `program` (an AirBuilder or an (n, 3) array of (op, a, b), with
        AirBuilder.lookup / end_lookup_column as its sinks) over the traces `dmats`: one height h, natural row order, not
        LDEs.  `public_values`: canonical words; `challenges`: (n, DC) canonical words.  Returns (DeviceMatrix, table_sum):
        the new (h, DC * (1 + G)) matrix holds the running sum s (s[0] = 0, s[r + 1] = s[r] + sum_g f_g[r]) in its first DC
        columns and the fractions f_g of column g in columns DC * (1 + g) .., the flattening local_ext reads;
        table_sum is the DC canonical words of s[h - 1] + sum_g f_g[h - 1].  Waits for the device.  A zero denominator
        raises P3rError (P3R_EINVAL) naming the smallest such row.  The inputs are left as they are."""
        dc = self.challenge_degree
        arr, n = _air_insns(program)
        mats = (C.c_void_p * max(1, len(dmats)))(*[d.h for d in dmats])
        pv, pvp = _u32(np.asarray(public_values, dtype=np.uint32).reshape(-1))
        ch, chp = _u32(np.asarray(challenges, dtype=np.uint32).reshape(-1, dc))
        total = np.zeros(dc, dtype=np.uint32)
        out = C.c_void_p()
        self.check(self.lib.p3r_logup_program_dmat(self.h, arr, n, mats, len(dmats), pvp, pv.size, chp, len(ch), C.byref(out),
                                                   total.ctypes.data_as(_lib.u32p)))
        return DeviceMatrix(self, self.ptr(out.value)), total

    # ---- is the caller's trace right: unsatisfied constraints and unbalanced lookups, located
    def check_device(self, program, dmats, public_values=(), challenges=()):
        """check_air_satisfies for the constraint `program` (an AirBuilder or an (n, 3) array of (op, a, b)) over the TRACES
        `dmats`: one height h, natural row order, not LDEs; the next row of r is (r + 1) mod h and the selectors are 0 / 1
        (is_first_row = [r == 0], is_last_row = [r == h - 1], is_transition = [r != h - 1]).  Returns a dict: n_failures (the
        (row, constraint) pairs whose value is not zero), first_row (the smallest failing row; 0xffffffff: the trace
        satisfies the program), first_constraint (the smallest failing constraint in that row), and per constraint the arrays
        first_row_of (uint32; 0xffffffff: it holds everywhere) and n_failed_of (uint64).  A failing trace is a result, not an
        error.  Waits for the device."""
        dc = self.challenge_degree
        arr, n = _air_insns(program)
        prog = program.program() if isinstance(program, AirBuilder) else np.asarray(program).reshape(-1, 3)
        n_constraints = int(np.count_nonzero(prog[:, 0] == _lib.P3R_AIR_ASSERT_ZERO)) if len(prog) else 0
        mats = (C.c_void_p * max(1, len(dmats)))(*[d.h for d in dmats])
        pv, pvp = _u32(np.asarray(public_values, dtype=np.uint32).reshape(-1))
        ch, chp = _u32(np.asarray(challenges, dtype=np.uint32).reshape(-1, dc))
        first = np.zeros(max(1, n_constraints), dtype=np.uint32)
        failed = np.zeros(max(1, n_constraints), dtype=np.uint64)
        report = _lib.P3rCheckReport()
        self.check(self.lib.p3r_check_program_dmat(self.h, arr, n, mats, len(dmats), pvp, pv.size, chp, len(ch), C.byref(report),
                                                   first.ctypes.data_as(_lib.u32p), failed.ctypes.data_as(C.POINTER(C.c_uint64))))
        return {"n_failures": int(report.n_failures), "first_row": int(report.first_row), "first_constraint": int(report.first_constraint),
                "first_row_of": first[:n_constraints], "n_failed_of": failed[:n_constraints]}

    def lookup_check_device(self, instances, challenges=(), cap=16):
        """check_lookups over the tables of a bus.  `instances`: (program, dmats) or (program, dmats, public_values) each -
        a lookup program as logup_device takes it and its traces (one height per instance); `challenges` ((n, DC) canonical
        words) are shared.  Every term with a non-zero multiplicity is a record keyed by its denominator value; a key whose
        multiplicities do not sum to zero is unbalanced.  Returns (n_unbalanced, entries): the number of unbalanced keys
        and, for the min(cap, n_unbalanced) of them whose first records come earliest in (instance, row, term) order, a
        dict of instance, row, term (the key's first record), n_records, denominator and net (DC canonical words each).
        Waits for the device."""
        dc = self.challenge_degree
        ch, chp = _u32(np.asarray(challenges, dtype=np.uint32).reshape(-1, dc))
        arr, keep = _lookup_instances(instances)
        out = (_lib.P3rLookupImbalance * max(1, int(cap)))()
        count = C.c_uint64()
        self.check(self.lib.p3r_lookup_check_dmat(self.h, arr, len(instances), chp, len(ch), out, int(cap), C.byref(count)))
        return count.value, _lookup_entries(out, min(int(cap), count.value), dc)

    def lookup_multiplicities_device(self, table, queries, challenges=(), cap=16):
        """The multiplicity column of `table` against its `queries`, built on the device.  An instance is (program, dmats) or
        (program, dmats, public_values), as lookup_check_device takes it; the key of a term is its denominator value under
        `challenges` ((n, DC) canonical words).  A table term OFFERS its key where its multiplicity value is non-zero (an
        enable flag, otherwise unused); a query term with a non-zero multiplicity m - a base value - asks for its key m
        times.  Returns (DeviceMatrix, n_missing, entries): the new (h_table, n_terms_table) matrix holds, at the first
        offering table slot of a key in (row, term) order, the sum modulo p of the m asked of that key, and 0 everywhere
        else; n_missing counts the keys that are asked for (net non-zero) and offered by no table slot, and entries are the
        min(cap, n_missing) of them whose first query records come earliest, as lookup_check_device's, `instance` being the
        index into `queries`.  The column is part of the main trace, which is committed before the transcript yields any
        challenge: `challenges` are the caller's own - with the basis elements 1, X, .. a tuple of up to DC base fields is
        its own key and the join is exact (p3r.h).  Waits for the device."""
        dc = self.challenge_degree
        ch, chp = _u32(np.asarray(challenges, dtype=np.uint32).reshape(-1, dc))
        tab, keep_t = _lookup_instances([table])
        qs, keep_q = _lookup_instances(queries)
        missing = (_lib.P3rLookupImbalance * max(1, int(cap)))()
        count = C.c_uint64()
        out = C.c_void_p()
        self.check(self.lib.p3r_lookup_multiplicities_dmat(self.h, tab, qs, len(queries), chp, len(ch), C.byref(out), missing, int(cap),
                                                           C.byref(count)))
        return DeviceMatrix(self, self.ptr(out.value)), count.value, _lookup_entries(missing, min(int(cap), count.value), dc)

    # ---- derived trace columns: a witness program's stored values as a new resident trace
    def witness_program_info(self, program, widths):
        """witness_program_info under this context's field and challenge degree."""
        return witness_program_info(self.cfg, program, widths)

    def witness_device(self, program, dmats, height=None, public_values=(), challenges=()):
        """The columns the witness `program` (an AirBuilder or an (n, 3) array of (op, a, b), with AirBuilder.store as its
        sink and inv / bits / row among its value ops) derives from the traces `dmats`: one height h, natural row order, not
        LDEs; `next` reads row (r + 1) mod h of an input.  With no input matrix `height` gives h; otherwise it is None or
        the matrices' height.  `public_values`: canonical words; `challenges`: (n, DC) canonical words.  Returns a new
        (h, W) DeviceMatrix, W one past the highest stored column: a trace like any other, for coset_lde_batch_device,
        check_device and the lookup entries.  Only enqueues; the inputs are left as they are."""
        dc = self.challenge_degree
        arr, n = _air_insns(program)
        mats = (C.c_void_p * max(1, len(dmats)))(*[d.h for d in dmats])
        pv, pvp = _u32(np.asarray(public_values, dtype=np.uint32).reshape(-1))
        ch, chp = _u32(np.asarray(challenges, dtype=np.uint32).reshape(-1, dc))
        out = C.c_void_p()
        self.check(self.lib.p3r_witness_program_dmat(self.h, arr, n, mats, len(dmats), 0 if height is None else int(height), pvp, pv.size,
                                                     chp, len(ch), C.byref(out)))
        return DeviceMatrix(self, self.ptr(out.value))

    # ---- accumulator columns: first-order affine recurrences down the rows of resident traces
    def affine_scan_info(self, recurrences, widths):
        """affine_scan_info under this context's field and challenge degree."""
        return affine_scan_info(self.cfg, recurrences, widths)

    def affine_scan_device(self, recurrences, dmats, want_last=False):
        """The accumulator columns s[0] = init, s[r + 1] = a[r] * s[r] + b[r] of the `recurrences` (Recurrence objects, or
        dicts of Recurrence's arguments) over the traces `dmats`: one height h, natural row order, not LDEs.  Returns a new
        (h, W) DeviceMatrix, W one past the highest written column; row r holds s[r], the state entering the row, or
        s[r + 1] for an inclusive recurrence.  A trace like any other, for coset_lde_batch_device and check_device.  With
        `want_last` returns (matrix, last): `last` an (n, 5) uint32 array of s[h] per recurrence, canonical, DC words used
        for an extension recurrence and one otherwise, the rest zero - and the call waits for the stream.  Without it the
        call only enqueues.  The inputs are left as they are."""
        arr, n = _recurrences(recurrences)
        mats = (C.c_void_p * max(1, len(dmats)))(*[d.h for d in dmats])
        out = C.c_void_p()
        last = np.zeros((n, 5), dtype=np.uint32) if want_last else None
        self.check(self.lib.p3r_affine_scan_dmat(self.h, arr, n, mats, len(dmats), C.byref(out),
                                                 last.ctypes.data_as(_lib.u32p) if want_last else None))
        dm = DeviceMatrix(self, self.ptr(out.value))
        return (dm, last) if want_last else dm

    # ---- the rest of prove_fri: challenger, commit-phase leaf view, final polynomial, schedule, and their composition
    def challenger(self):
        """A fresh DuplexChallenger over the context's width-16 Poseidon2 constants (p3r_challenger)."""
        return Challenger(self, self.ptr(self.lib.p3r_challenger_create(self.h)))

    def fri_leaf_view_device(self, dmat, log_arity):
        """The commit-phase leaf matrix of the (n, DC) vector `dmat`: (n >> log_arity, DC << log_arity), row r the flattened
        extension elements r << log_arity .. (r + 1) << log_arity - a plain DeviceMatrix for commit_device / open_many."""
        out = C.c_void_p()
        self.check(self.lib.p3r_fri_leaf_view_dmat(self.h, dmat.h, log_arity, C.byref(out)))
        return DeviceMatrix(self, self.ptr(out.value))

    def fri_final_poly_device(self, dmat, log_final_poly_len=None):
        """The final polynomial of the last folded (m, DC) vector (bit-reversed over <w_m>): (2^log_final_poly_len, DC)
        canonical coefficients in natural order.  Raises when a coefficient above them is not zero."""
        lf = self.cfg.log_final_poly_len if log_final_poly_len is None else int(log_final_poly_len)
        out = np.empty((1 << lf, self.challenge_degree), dtype=np.uint32)
        self.check(self.lib.p3r_fri_final_poly_dmat(self.h, dmat.h, lf, out.ctypes.data_as(_lib.u32p)))
        return out

    def fri_log_arity(self, phase, log_cur, log_final, log_next_input=-1):
        """log2 of the arity of commit phase `phase` at height 2^log_cur under the context's max_log_arity and
        fri_log_arities (the prover's rule); -1 where the schedule does not fit."""
        return int(self.lib.p3r_fri_log_arity(self.h, int(phase), int(log_cur), int(log_final), int(log_next_input)))

    def prove_fri(self, challenger, inputs):
        """p3_fri::prover::prove_fri over the per-height reduced openings `inputs` (tallest first, strictly decreasing
        heights, as fri_reduce_device returns them), with public calls only: per commit phase the leaf view, its
        commitment, the cap observed, the commit proof of work, beta, the fold with the roll-in of the next input; then
        the final polynomial, the log arities, the query proof of work, the query indices and the opening of every phase
        tree at every index.  The input-round openings stay the caller's (open_many on its own trees at
        `query_indices`).  The inputs are left as they are.  Returns a FriProof."""
        cfg, n_in = self.cfg, len(inputs)
        if n_in == 0:
            raise P3rError(-1, "prove_fri: no input vector")
        logs = [int(d.shape[0]).bit_length() - 1 for d in inputs]
        if any(a <= b for a, b in zip(logs, logs[1:])):
            raise P3rError(-1, "prove_fri: the inputs must be one vector per height, tallest first")
        log_max, log_final = logs[0], int(cfg.log_final_poly_len + cfg.log_blowup)
        proof = FriProof(log_max_height=log_max)
        cur, log_cur, nxt, trees, views, mine = inputs[0], log_max, 1, [], [], []
        try:
            while log_cur > log_final:
                la = self.fri_log_arity(len(trees), log_cur, log_final, logs[nxt] if nxt < n_in else -1)
                if la < 0:
                    raise P3rError(-1, "fri_log_arities does not fit the proof: phase %d at height 2^%d" % (len(trees), log_cur))
                if la > 4:
                    raise P3rError(-5, "max_log_arity > 4 is not supported")
                views.append(self.fri_leaf_view_device(cur, la))
                cap, tree = self.commit_device([views[-1]])
                trees.append(tree)
                challenger.observe(cap.reshape(-1))
                proof.commit_phase_caps.append(cap)
                proof.commit_pow_witnesses.append(challenger.grind(cfg.commit_pow_bits))
                beta = challenger.sample_ext()
                roll = nxt < n_in and logs[nxt] == log_cur - la
                folded = self.fri_fold_device(cur, la, beta, inputs[nxt] if roll else None)
                mine.append(folded)
                nxt += 1 if roll else 0
                cur, log_cur = folded, log_cur - la
                proof.log_arities.append(la)
            if nxt != n_in:
                raise P3rError(-1, "FRI: an input height was never rolled in")
            proof.final_poly = self.fri_final_poly_device(cur)
            challenger.observe(proof.final_poly.reshape(-1))
            challenger.observe(proof.log_arities)
            proof.query_pow_witness = challenger.grind(cfg.query_pow_bits)
            proof.query_indices = [challenger.sample_bits(log_max) for _ in range(cfg.num_queries)]
            per_phase, shift = [], 0
            for la, tree in zip(proof.log_arities, trees):
                shift += la   # the phase's tree index: the query index without the bits folded so far and this phase's
                per_phase.append(tree.open_many([i >> shift for i in proof.query_indices]))
            for q in range(len(proof.query_indices)):
                proof.query_openings.append([FriPhaseOpening(o[q], None if s is None else s[q], pf[q]) for o, s, pf in per_phase])
            return proof
        finally:
            for t in trees:
                t.free()
            for d in views + mine:
                d.free()

    def pcs_open(self, ch, rounds):
        """TwoAdicFriPcs::open composed from public calls, all resident.  `rounds`: per commitment a tuple
        (tree, dmats, points) - the MerkleTree of commit_device, the committed LDEs it was made from (bit-reversed rows over
        the generator's coset, blow-up 2^log_blowup) and per matrix its (k, DC) opening points.  open_points_device gives
        the opened values, which are observed (observe_opened_values); alpha is sampled; fri_reduce_device forms the
        per-height reduced openings; prove_fri runs over them; every round's tree is opened at every query index with
        MerkleTree.open_many.  Returns (values, fri_proof, input_openings): values[round][matrix] is (k, width, DC), and
        input_openings[round] = (opened, salts or None, siblings) - what pcs_verify takes."""
        flat_d = [d for tree, dmats, points in rounds for d in dmats]
        flat_p = [np.asarray(pt, dtype=np.uint32).reshape(-1, self.challenge_degree) for tree, dmats, points in rounds for pt in points]
        if len(flat_d) != len(flat_p) or not flat_d:
            raise P3rError(-1, "pcs_open: one array of points per committed matrix")
        flat_v = self.open_points_device(flat_d, flat_p, added_bits=self.log_blowup)
        values, at = [], 0
        for tree, dmats, points in rounds:
            values.append(flat_v[at:at + len(dmats)])
            at += len(dmats)
        observe_opened_values(ch, values)
        alpha = ch.sample_ext()
        inputs = self.fri_reduce_device(flat_d, flat_p, flat_v, alpha)
        try:
            proof = self.prove_fri(ch, inputs)
        finally:
            for d in inputs:
                d.free()
        openings = []
        for tree, dmats, points in rounds:
            shift = proof.log_max_height - int(tree.log_max_height)
            openings.append(tree.open_many([i >> shift for i in proof.query_indices]))
        return values, proof, openings

    # ---- MMCS
    def commit(self, mats):
        """Mmcs::commit over host matrices (list of 2-D uint32 arrays). Returns (cap, tree)."""
        keep = []
        arr = (_lib.P3rMatrix * len(mats))()
        for i, m in enumerate(mats):
            a, p = _u32(m)
            keep.append(a)
            arr[i].values, arr[i].height, arr[i].width = p, a.shape[0], a.shape[1]
        cap = np.empty((1 << self.cap_height, 8), dtype=np.uint32)
        tree = C.c_void_p()
        self.check(self.lib.p3r_mmcs_commit(self.h, arr, len(mats), cap.ctypes.data_as(_lib.u32p), C.byref(tree)))
        return cap, MerkleTree(self, tree.value, [])

    def commit_device(self, dmats):
        arr = (C.c_void_p * len(dmats))(*[d.h for d in dmats])
        cap = np.empty((1 << self.cap_height, 8), dtype=np.uint32)
        tree = C.c_void_p()
        self.check(self.lib.p3r_mmcs_commit_dmat(self.h, arr, len(dmats), cap.ctypes.data_as(_lib.u32p), C.byref(tree)))
        return cap, MerkleTree(self, tree.value, list(dmats))

    # ---- batch-STARK proving
    def prep_create(self, airs, prep_mats):
        """airs: list of dicts(kind, lanes, horner_packed_steps, coeff_lookups); prep_mats: 2-D arrays.
        Returns (commitment, ProverData)."""
        n = len(airs)
        descs = (_lib.P3rAirDesc * n)()
        arr = (_lib.P3rMatrix * n)()
        keep = []
        for i, (a, m) in enumerate(zip(airs, prep_mats)):
            descs[i].kind = a["kind"]
            descs[i].lanes = a.get("lanes", 1)
            descs[i].horner_packed_steps = a.get("horner_packed_steps", 2)
            descs[i].coeff_lookups = a.get("coeff_lookups", 0)
            x, p = _u32(m)
            keep.append(x)
            arr[i].values, arr[i].height, arr[i].width = p, x.shape[0], x.shape[1]
        cap = np.empty((1 << self.cap_height, 8), dtype=np.uint32)
        h = self.ptr(self.lib.p3r_prep_create(self.h, descs, arr, n, cap.ctypes.data_as(_lib.u32p)))
        return cap, ProverData(self, h)

    def _proof_call(self, fn, *args):
        buf = getattr(self, "_proof_buf", None)
        if buf is None:
            buf = self._proof_buf = C.create_string_buffer(1 << 20)
        n = C.c_size_t()
        rc = fn(*args, C.cast(buf, C.POINTER(C.c_uint8)), len(buf), C.byref(n))
        if rc == -6 and n.value > len(buf):  # P3R_EBUFFER: the library kept the proof (p3r_take_proof) - it is not made again
            buf = self._proof_buf = C.create_string_buffer(max(n.value + n.value // 4, 2 * len(buf)))
            rc = self.lib.p3r_take_proof(self.h, C.cast(buf, C.POINTER(C.c_uint8)), len(buf), C.byref(n))
        self.check(rc)
        return C.string_at(buf, n.value)   # one memcpy (slicing a ctypes array builds a list first)

    def prove_batch(self, prover_data, main_traces, canonical_field_encoding=False):
        """main_traces: DeviceMatrix list (resident) or 2-D uint32 arrays (host)."""
        flags = 1 if canonical_field_encoding else 0
        n = len(main_traces)
        if all(isinstance(m, DeviceMatrix) for m in main_traces):
            arr = (C.c_void_p * n)(*[m.h for m in main_traces])
            return self._proof_call(self.lib.p3r_prove_batch, self.h, prover_data.h, arr, n, flags)
        arr = (_lib.P3rMatrix * n)()
        keep = []
        for i, m in enumerate(main_traces):
            x, p = _u32(m)
            keep.append(x)
            arr[i].values, arr[i].height, arr[i].width = p, x.shape[0], x.shape[1]
        return self._proof_call(self.lib.p3r_prove_batch_host, self.h, prover_data.h, arr, n, flags)

    # ---- profiling
    def profile_enable(self, on=True):
        self.check(self.lib.p3r_profile_enable(self.h, 1 if on else 0))

    def trim(self):
        """Return this ctx's cached device memory to the driver; returns the number of bytes released."""
        n = C.c_uint64()
        self.check(self.lib.p3r_trim(self.h, C.byref(n)))
        return n.value

    def profile_read(self):
        buf = (_lib.P3rProfileEntry * 64)()
        n = C.c_size_t()
        self.check(self.lib.p3r_profile_read(self.h, buf, 64, C.byref(n)))
        return {buf[i].name.decode(): (buf[i].total_ms, buf[i].launches) for i in range(n.value)}

    def time_permute(self, dmat, iters):
        ms = C.c_double()
        self.check(self.lib.p3r_time_permute_dmat(self.h, dmat.h, iters, C.byref(ms)))
        return ms.value


class Challenger:
    """DuplexChallenger<F, Perm16, 16, 8> over the context's Poseidon2 constants (p3r_challenger): host state, except the
    proof-of-work search of `grind`.  Words are canonical."""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    def observe(self, words):
        a, p = _u32(np.asarray(words, dtype=np.uint32).reshape(-1))
        self.ctx.check(self.ctx.lib.p3r_challenger_observe(self.h, p, a.size))

    def sample(self, n=None):
        """One base element (an int), or `n` of them (an array)."""
        out = np.empty(1 if n is None else int(n), dtype=np.uint32)
        self.ctx.check(self.ctx.lib.p3r_challenger_sample(self.h, out.ctypes.data_as(_lib.u32p), out.size))
        return int(out[0]) if n is None else out

    def sample_ext(self):
        """One challenge-field element: DC words (DC consecutive samples)."""
        out = np.empty(self.ctx.challenge_degree, dtype=np.uint32)
        self.ctx.check(self.ctx.lib.p3r_challenger_sample_ext(self.h, out.ctypes.data_as(_lib.u32p)))
        return out

    def sample_bits(self, bits):
        out = C.c_uint32()
        self.ctx.check(self.ctx.lib.p3r_challenger_sample_bits(self.h, int(bits), C.byref(out)))
        return int(out.value)

    def check_witness(self, bits, witness):
        """Observes the witness and samples, as check_witness does; True when the low `bits` bits are zero."""
        ok = C.c_int()
        self.ctx.check(self.ctx.lib.p3r_challenger_check_witness(self.h, int(bits), int(witness), C.byref(ok)))
        return bool(ok.value)

    def grind(self, bits):
        """The smallest canonical proof-of-work witness (device search); the challenger is left in the post-check state.
        bits == 0: witness 0, transcript untouched."""
        w = C.c_uint32()
        self.ctx.check(self.ctx.lib.p3r_challenger_grind(self.ctx.h, self.h, int(bits), C.byref(w)))
        return int(w.value)

    def clone(self):
        return Challenger(self.ctx, self.ctx.ptr(self.ctx.lib.p3r_challenger_clone(self.h)))

    def free(self):
        if self.h:
            self.ctx.lib.p3r_challenger_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class FriPhaseOpening:
    """One commit-phase opening of a query: the opened leaf row (2^log_arity elements of DC words; the proof's
    sibling_values are the row without element index & (arity - 1)), its salts (hiding MMCS; else None) and siblings."""

    def __init__(self, row, salts, siblings):
        self.row, self.salts, self.siblings = row, salts, siblings


class FriProof:
    """What p3_fri::prover::prove_fri returns (Context.prove_fri), as canonical words."""

    def __init__(self, log_max_height=0):
        self.log_max_height = log_max_height
        self.commit_phase_caps = []      # per phase: (1 << cap_height, 8)
        self.commit_pow_witnesses = []   # per phase
        self.log_arities = []            # per phase
        self.final_poly = None           # (2^log_final_poly_len, DC)
        self.query_pow_witness = 0
        self.query_indices = []
        self.query_openings = []         # per query, per phase: FriPhaseOpening


class DeviceMatrix:
    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    @property
    def shape(self):
        return (self.ctx.lib.p3r_dmat_height(self.h), self.ctx.lib.p3r_dmat_width(self.h))

    def download(self):
        out = np.empty(self.shape, dtype=np.uint32)
        self.ctx.check(self.ctx.lib.p3r_dmat_download(self.ctx.h, self.h, out.ctypes.data_as(_lib.u32p)))
        return out

    def free(self):
        if self.h and self.ctx.h:
            self.ctx.lib.p3r_dmat_free(self.ctx.h, self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class ProverData:
    """Device-resident preprocessed LDEs + commitment (ProverData::from_airs_and_degrees)."""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    def free(self):
        if self.h and self.ctx.h:
            self.ctx.lib.p3r_prep_free(self.ctx.h, self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceP2Rows:
    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    def free(self):
        if self.h and self.ctx.h:
            self.ctx.lib.p3r_p2_rows_free(self.ctx.h, self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class MerkleTree:
    def __init__(self, ctx, handle, borrowed):
        self.ctx, self.h, self._borrowed = ctx, handle, borrowed

    @property
    def log_max_height(self):
        return self.ctx.lib.p3r_tree_log_max_height(self.h)

    @property
    def salt_elems(self):
        """Salt elements per committed row (0: a plain tree)."""
        return self.ctx.lib.p3r_tree_salt_elems(self.h)

    @property
    def num_matrices(self):
        """Matrices the caller committed (the salt matrices of a hiding tree are not counted)."""
        return self.ctx.lib.p3r_tree_num_matrices(self.h)

    def open_many(self, indices):
        """Mmcs::open_batch for every index in one launch (p3r_mmcs_open_batch).  Returns (opened[n, total_width],
        salts[n, num_matrices, salt_elems] or None for a plain tree, proofs[n, depth, 8])."""
        lib = self.ctx.lib
        idx = [int(i) for i in indices]
        n, S = len(idx), self.salt_elems
        opened = np.empty((n, lib.p3r_tree_total_width(self.h)), dtype=np.uint32)
        salts = np.empty((n, self.num_matrices, S), dtype=np.uint32) if S else None
        proofs = np.empty((n, lib.p3r_tree_proof_len(self.h), 8), dtype=np.uint32)
        arr = (C.c_size_t * max(n, 1))(*idx)
        self.ctx.check(lib.p3r_mmcs_open_batch(self.ctx.h, self.h, arr, n, opened.ctypes.data_as(_lib.u32p),
                                               salts.ctypes.data_as(_lib.u32p) if S else None,
                                               proofs.ctypes.data_as(_lib.u32p)))
        return opened, salts, proofs

    def open_batch(self, index):
        """Returns (opened_values concatenated in commit order, proof[(depth, 8)]).  A hiding tree (salt_elems > 0) is
        opened with open_many: this form has no salt output and raises the library's error there."""
        w = self.ctx.lib.p3r_tree_total_width(self.h)
        depth = self.ctx.lib.p3r_tree_proof_len(self.h)   # binary: log_max_height - cap_height; arity 4: sum of (step - 1)
        opened = np.empty(w, dtype=np.uint32)
        proof = np.empty((depth, 8), dtype=np.uint32)
        self.ctx.check(self.ctx.lib.p3r_mmcs_open(self.ctx.h, self.h, index, opened.ctypes.data_as(_lib.u32p),
                                                  proof.ctypes.data_as(_lib.u32p)))
        return opened, proof

    def free(self):
        if self.h and self.ctx.h:
            self.ctx.lib.p3r_tree_free(self.ctx.h, self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
