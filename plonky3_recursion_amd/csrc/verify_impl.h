// Native verifier for the proofs prove_impl.hip.h produces: `verify_batch` behind
// `BatchStarkProver::verify_all_tables` (circuit-prover/src/batch_stark_prover.rs:1230-1268,
// 1649-1727).  Host code: verification is a few thousand permutations and is serial in the
// reference too.  It replays the prover's transcript and checks, following the in-tree circuit
// verifier (the only in-tree statement of what p3-batch-stark / p3-fri 0.6 verify):
//   transcript order, domains, opening points      recursion/src/verifier/batch_stark.rs:521-852
//   folded constraints * 1/Z_H == quotient(zeta)   :886-1021, recursion/src/verifier/quotient.rs:60-
//   selectors at zeta                               recursion/src/pcs/fri/targets.rs:868-908
//   LogUp constraints, global sum of terminals      batch_stark.rs:1026-1112
//   MMCS openings (mixed heights, injection, cap)   recursion/src/pcs/mmcs.rs:319-426, circuit/src/ops/mmcs.rs:81-209
//   FRI: reduced openings, folds, roll-ins, final polynomial, proofs of work
//                                                   recursion/src/pcs/fri/verifier.rs:424-465,562-781,887-981,1068-1356
//   ZK (HidingFriPcs, p3r_config.zk)                batch_stark.rs:424-428 (randomisation presence), :487-490,536 (degree
//                                                   bits), :623-661 (random commitment, its round), :701-735 (quotient
//                                                   domains), :855-864,1116-1260 and pcs/fri/targets.rs:1076-1130 (the
//                                                   opening proof's random opened values, merged into every point)
// The AIR statements are the ones the quotient kernel evaluates (air_device.hip.h), instantiated
// over the extension field at zeta.
#pragma once
#include <map>
#include <string>

#include "../../include/p3r.h"
#include "fri_verify.h"
#include "proof_grammar.h"

namespace p3r {

// The metadata fields that follow the inner BatchProof (BatchStarkProof, batch_stark_prover.rs:610-636).
template <class PP>
void parse_batch_stark_meta(const uint8_t* bytes, size_t len, bool canonical, const ProofLayout& PL, int dc,
                            p3r_batch_stark_meta* M, bool zk = false, bool salted = false) {
  std::memset(M, 0, sizeof *M);
  ProofChecker<PP> R(bytes, len, dc);
  M->proof_len = walk_batch_proof(R, PL, zk, salted, true);
  auto u32 = [&](const char* what) {
    const uint64_t v = R.varint();
    if (v > 0xFFFFFFFFull) vfail("%s does not fit 32 bits", what);
    return (uint32_t)v;
  };
  auto fe = [&]() -> uint32_t {
    const uint64_t v = R.varint();
    if (v >= PP::P) vfail("field element out of range");
    return canonical ? (uint32_t)v : Fp<PP>::raw((uint32_t)v).to_canonical();
  };
  auto str = [&](char (&dst)[64]) {  // NpoTypeId(String): valid UTF-8 (serde rejects anything else), no NUL (the C struct ends there)
    const size_t k = R.len(63);
    if ((size_t)(R.end - R.p) < k) vfail("proof metadata truncated");
    for (size_t i = 0; i < k;) {
      const uint8_t b = R.p[i];
      size_t n = b < 0x80 ? 1 : (b >> 5) == 6 ? 2 : (b >> 4) == 14 ? 3 : (b >> 3) == 30 ? 4 : 0;
      bool ok = n != 0 && b != 0 && i + n <= k;
      uint32_t cp = n == 1 ? b : n == 2 ? (b & 0x1F) : n == 3 ? (b & 0x0F) : (b & 0x07);
      for (size_t j = 1; ok && j < n; ++j) {
        ok = (R.p[i + j] >> 6) == 2;
        cp = (cp << 6) | (R.p[i + j] & 0x3F);
      }
      // shortest form only, no surrogates, nothing beyond U+10FFFF
      if (ok && ((n == 2 && cp < 0x80) || (n == 3 && (cp < 0x800 || (cp >= 0xD800 && cp < 0xE000))) ||
                 (n == 4 && (cp < 0x10000 || cp > 0x10FFFF))))
        ok = false;
      if (!ok) vfail("invalid UTF-8 in an operation type name");
      i += n;
    }
    std::memcpy(dst, R.p, k);
    dst[k] = 0;
    R.p += k;
  };
  // TablePacking { public_lanes, alu_lanes, npo_lanes, min_trace_height, horner_packed_steps } (packing.rs:9-27)
  M->public_lanes = u32("public_lanes");
  M->alu_lanes = u32("alu_lanes");
  M->n_npo_lanes = (uint32_t)R.len(P3R_META_MAX_NPO);
  for (uint32_t i = 0; i < M->n_npo_lanes; ++i) { str(M->npo_lanes[i].op_type); M->npo_lanes[i].lanes = u32("npo lanes"); }
  M->min_trace_height = u32("min_trace_height");
  M->horner_packed_steps = u32("horner_packed_steps");
  for (int i = 0; i < 3; ++i) M->rows[i] = R.varint();  // RowCounts([usize; 3]): no length prefix
  M->alu_variant = u32("alu_variant");
  if (M->alu_variant > 1) vfail("unknown AirVariant %u", M->alu_variant);
  M->ext_degree = u32("ext_degree");
  M->has_w_binomial = R.flag();
  if (M->has_w_binomial) M->w_binomial = fe();
  M->alu_quintic_trinomial = R.flag();
  M->n_non_primitives = (uint32_t)R.len(P3R_META_MAX_NPO);
  for (uint32_t i = 0; i < M->n_non_primitives; ++i) {
    p3r_npo_table_entry& e = M->non_primitives[i];
    str(e.op_type);
    e.rows = R.varint();
    e.lanes = u32("npo lanes");
    e.n_public_values = (uint32_t)R.len(8);
    for (uint32_t k = 0; k < e.n_public_values; ++k) e.public_values[k] = fe();
    e.air_variant = u32("air_variant");
    if (e.air_variant > 1) vfail("unknown AirVariant %u", e.air_variant);
  }
  M->has_stark_common = R.flag();
  if (M->has_stark_common) {
    M->cap_len = (uint32_t)R.len(P3R_META_MAX_CAP);
    for (uint32_t i = 0; i < 8 * M->cap_len; ++i) M->commitment[i] = fe();
    const size_t n_inst = R.len(P3R_META_MAX_INSTANCES);
    for (size_t i = 0; i < n_inst; ++i) {
      if (!R.flag()) continue;
      (void)R.varint();  // matrix index
      M->preprocessed_widths[M->n_instances] = u32("preprocessed width");
      M->degree_bits[M->n_instances] = (uint32_t)R.len(40);
      M->n_instances++;
    }
    const size_t n_map = R.len(P3R_META_MAX_INSTANCES);
    for (size_t i = 0; i < n_map; ++i) (void)R.varint();  // matrix_to_instance
  }
  if (R.p != R.end) vfail("%zu trailing bytes after the proof metadata", (size_t)(R.end - R.p));
  // structural invariants a derived Deserialize bypasses (batch_stark_prover.rs:666-681, packing.rs:140-161)
  const uint32_t d = M->ext_degree;
  if (!(d == 1 || d == 2 || d == 4 || d == 5 || d == 6 || d == 8)) vfail("UnsupportedExtDegree(%u)", d);
  for (int i = 0; i < 3; ++i)
    if (!M->rows[i]) vfail("ZeroRowCount");  // RowCounts::validate, batch_stark_prover.rs:475-479
  // TablePacking::validate, packing.rs:140-161
  if (!M->public_lanes) vfail("ZeroLanes(\"public_lanes\")");
  if (!M->alu_lanes) vfail("ZeroLanes(\"alu_lanes\")");
  for (uint32_t i = 0; i < M->n_npo_lanes; ++i)
    if (!M->npo_lanes[i].lanes) vfail("ZeroNpoLanes(%s)", M->npo_lanes[i].op_type);
  if (!M->min_trace_height || (M->min_trace_height & (M->min_trace_height - 1))) vfail("BadMinTraceHeight(%u)", M->min_trace_height);
  if (M->horner_packed_steps < 2) vfail("BadHornerPackedSteps(%u)", M->horner_packed_steps);
  // NonPrimitiveTableEntry::validate, batch_stark_prover.rs:292-300
  for (uint32_t i = 0; i < M->n_non_primitives; ++i)
    if (!M->non_primitives[i].lanes) vfail("ZeroNpoLanes(%s)", M->non_primitives[i].op_type);
}

// ---- the opened values of one instance as an AIR view over the extension field
template <class PP, int DC = 4>
struct ZetaView {
  using V = typename Chal<PP, DC>::type;
  const std::vector<V>*ml, *mn, *pl, *pn;
  V L(int c) const { return (*ml).at(c); }
  V N(int c) const { return (*mn).at(c); }
  V PL(int c) const { return (*pl).at(c); }
  V PN(int c) const { return (*pn).at(c); }
};

// acc <- acc * alpha + c over every constraint, base-field constraints first
// (recursion/src/traits/air.rs:162-182)
template <class PP, int DC = 4>
struct ZetaFold {
  using E = typename Chal<PP, DC>::type;
  E alpha, acc = E::zero();
  int count = 0;
  void base(const E& c) { acc = acc * alpha + c; ++count; }
  void base2(const E& c0, const E& c1) { base(c0); base(c1); }
  void ext(const E& c) { base(c); }
};

// LogUp group constraints at zeta: f_g * prod d_k - sum_k m_k prod_{l != k} d_l (same grouping as QuotSink)
template <class PP, int DC = 4>
struct ZetaLookupSink {
  using E = typename Chal<PP, DC>::type;
  E prefix;
  E beta_pow[kMaxExtD + 1];
  const std::vector<E>& aux;  // EF aux columns at zeta: [0] running sum, [g + 1] fraction of group g
  ZetaFold<PP, DC>& fold;
  int pair, cnt = 0, held = 0;
  E d0 = E::zero(), m0 = E::zero(), d1 = E::zero(), m1 = E::zero(), sum_f = E::zero();
  template <int D>
  E denom(const E& idx, const VD<E, D>& v) const {
    E d = prefix + beta_pow[0] * idx;
    for (int j = 0; j < D; ++j) d += beta_pow[j + 1] * v.c[j];
    return d;
  }
  template <int D>
  void add(const E& idx, const VD<E, D>& v, const E& mult) {
    const E d = denom(idx, v);
    ++cnt;
    if (!pair) {
      const E f = aux.at(cnt);
      fold.ext(f * d - mult);
      sum_f += f;
    } else if (held == 0) {
      d0 = d; m0 = mult; held = 1;
    } else if (pair == 1) {
      const E f = aux.at(cnt / 2);
      fold.ext(f * d0 * d - (d * m0 + d0 * mult));
      sum_f += f;
      held = 0;
    } else if (held == 1) {
      d1 = d; m1 = mult; held = 2;
    } else {   // triples (the budget of a ZK configuration)
      const E f = aux.at(cnt / 3);
      fold.ext(f * d0 * d1 * d - (m0 * d1 * d + m1 * d0 * d + mult * d0 * d1));
      sum_f += f;
      held = 0;
    }
  }
  void finish() {
    if (!held) return;
    const int G = pair + 1;
    const E f = aux.at((cnt + G - 1) / G);
    if (held == 1) fold.ext(f * d0 - m0);
    else fold.ext(f * d0 * d1 - (m0 * d1 + m1 * d0));
    sum_f += f;
  }
};

// ---- the out-of-domain identity of one instance: folded constraints(zeta) / Z_H(zeta) == quotient(zeta)
// (recursion/src/verifier/batch_stark.rs:886-1017, verifier/quotient.rs:60-140).  Shared by the
// verifier and by the prover's self-check before it serialises a proof (prove_impl.hip.h): the
// counterpart of prove_batch's debug constraint check, at the cost of one evaluation per table.
template <class PP, int DC = 4>
struct ZetaInstance {
  using E = typename Chal<PP, DC>::type;
  const std::vector<E>* main_local;
  const std::vector<E>* main_next;  // null when the AIR reads no next row
  const std::vector<E>* prep_local;
  const std::vector<E>* prep_next;
  const std::vector<E>* perm_local;
  const std::vector<E>* perm_next;
  const std::vector<std::vector<E>>* chunks;
  const E* terminal;  // null without lookups
};
// log_n_i: the BASE trace degree bits; is_zk: the quotient domain has 2^(log_chunks + is_zk) chunk cosets of the base
// trace size (batch_stark.rs:701-717).
template <class PP, int DC = 4>
void check_instance_at_zeta(const AirParams& air, const LookupLayout& L, int log_n_i, const ZetaInstance<PP, DC>& in,
                            typename Chal<PP, DC>::type alpha, typename Chal<PP, DC>::type zeta,
                            typename Chal<PP, DC>::type l_prefix, const typename Chal<PP, DC>::type* l_beta_pow,
                            const uint32_t* rc_mont, size_t i, int is_zk = 0) {
  using F = Fp<PP>;
  using E = typename Chal<PP, DC>::type;
  const F gen = F::generator();
  {
    const size_t n = size_t(1) << log_n_i;
    const F g = F::two_adic_generator(log_n_i), g_inv = g.inv();
    // selectors on the (unshifted) trace domain: Z_H = zeta^n - 1 (pcs/fri/targets.rs:868-908)
    const E zh = zeta.pow(n) - E::one();
    if (zh.is_zero()) vfail("zeta lies in the trace domain");
    const E is_transition = zeta - E::from_base(g_inv);
    const E is_first = zh * (zeta - E::one()).inv();
    const E is_last = zh * is_transition.inv();
    static const std::vector<E> none;
    ZetaView<PP, DC> v{in.main_local, in.main_next ? in.main_next : &none, in.prep_local, in.prep_next};
    ZetaFold<PP, DC> fold;
    fold.alpha = alpha;
    const bool generic = ext_degree_is_binomial_generic((uint32_t)air.ext_d);
    if (!(air.ext_d == 1 || air.ext_d == 4 || (air.ext_d == 5 && kHasQuintic<PP>) || (generic && air.kind != AIR_POSEIDON2)))
      vfail("instance %zu: no AIR of kind %d for circuit extension degree %d", i, air.kind, air.ext_d);
    if (air.kind == AIR_ALU) {
      dispatch_air_degree<PP>(air.ext_d, [&](auto dc) { alu_constraints<PP, decltype(dc)::value>(air, v, fold); });
    } else if (air.kind == AIR_POSEIDON2) {
      if (air.ext_d != 4) poseidon2_d1_constraints<PP>(v, is_transition, rc_mont, fold);
      else poseidon2_constraints<PP>(v, is_transition, rc_mont, fold);
    } else if (air.kind == AIR_POSEIDON2_W32) {
      if (air.ext_d != 4) vfail("instance %zu: the width-32 Poseidon2 table belongs to D = 4 circuits", i);
      poseidon2w_constraints<PP>(v, is_transition, rc_mont + p2_num_constants<PP>(), fold);
    }
    if (fold.count != air_num_base_constraints<PP>(air)) vfail("instance %zu: constraint count mismatch", i);
    if (L.n_groups) {
      // EF aux columns from their 4 base-column openings: sum_k x^k * col_k(zeta)
      auto ef_cols = [&](const std::vector<E>& flat) {
        std::vector<E> out(flat.size() / DC, E::zero());
        for (size_t c = 0; c < out.size(); ++c)
          for (int k = 0; k < DC; ++k) {
            E basis = E::zero();
            basis.c[k] = F::one();
            out[c] += basis * flat[c * DC + k];
          }
        return out;
      };
      const std::vector<E> aux_l = ef_cols(*in.perm_local), aux_n = ef_cols(*in.perm_next);
      ZetaLookupSink<PP, DC> sink{l_prefix, {l_beta_pow[0], l_beta_pow[1], l_beta_pow[2], l_beta_pow[3], l_beta_pow[4],
                                         l_beta_pow[5], l_beta_pow[6], l_beta_pow[7], l_beta_pow[8]},
                              aux_l, fold, L.pair};
      dispatch_air_degree<PP>(air.ext_d, [&](auto dc) { air_interactions<PP, decltype(dc)::value>(air, v, sink); });
      sink.finish();
      if (sink.cnt != L.n_interactions) vfail("instance %zu: interaction count mismatch", i);
      const E s = aux_l[0], s_next = aux_n[0], terminal = *in.terminal;
      fold.ext(s * is_first);
      fold.ext((s_next - s - sink.sum_f) * is_transition);
      fold.ext((s + sink.sum_f - terminal) * is_last);
    }
    // quotient(zeta) = sum_c L_c(zeta) * Q_c(zeta) over the 2^log_chunks cosets of the quotient domain
    // (recursion/src/verifier/quotient.rs:60-)
    const int lq = L.log_chunks + is_zk;
    const size_t C = size_t(1) << lq;
    if (in.chunks->size() != C) vfail("instance %zu: %zu quotient chunks, expected %zu", i, in.chunks->size(), C);
    const F wq = F::two_adic_generator(log_n_i + lq);
    std::vector<F> shifts(C);
    for (size_t c = 0; c < C; ++c) shifts[c] = gen * wq.pow(c);
    E quotient = E::zero();
    for (size_t c = 0; c < C; ++c) {
      // vanishing polynomial of coset c' at x: (x / shift_c')^n - 1
      E num = E::one();
      F den = F::one();
      for (size_t o = 0; o < C; ++o) {
        if (o == c) continue;
        num *= (zeta * shifts[o].inv()).pow(n) - E::one();
        den *= (shifts[c] * shifts[o].inv()).pow(n) - F::one();
      }
      E qc = E::zero();
      for (int k = 0; k < DC; ++k) {
        E basis = E::zero();
        basis.c[k] = F::one();
        qc += basis * (*in.chunks)[c][k];
      }
      quotient += num * den.inv() * qc;
    }
    if (!(fold.acc * zh.inv() == quotient)) vfail("instance %zu: constraints do not match the quotient at zeta (OodEvaluationMismatch)", i);
  }
}

// ---- the whole verification
struct VerifyParams {
  int log_blowup, max_log_arity, cap_height, log_final_poly_len, commit_pow_bits, query_pow_bits, num_queries;
  std::vector<uint8_t> fri_log_arities;  // explicit folding schedule (p3r_config), empty: the rule
  ProofLayout layout;                    // field order of the serialised structs (p3r_config.proof_layout)
  int mmcs_arity = 2;                    // 4: the arity-4 MMCS over the width-32 permutation (p3r_config.mmcs_arity)
  int zk = 0;                            // HidingFriPcs (p3r_config.zk)
  int num_random_codewords = 0;          // random codeword columns per committed matrix (p3r_config.num_random_codewords)
  int mmcs_salt_elems = 0;               // MerkleTreeHidingMmcs: salt elements per committed row (p3r_config.mmcs_salt_elems)
};

// The verifier's state and its phases, named after prove_batch's (prove_impl.hip.h): the members are what crosses a
// phase boundary, everything else is a local of its phase.
template <class PP, int DC = 4>
struct BatchVerifier {
  using F = Fp<PP>;
  using E = typename Chal<PP, DC>::type;
  using Digest = std::array<F, P2_DIGEST>;
  // a committed matrix of an input batch: log LDE height, width, opening points and the values claimed there
  struct Mat { int log_h; int w; std::vector<E> z; std::vector<std::vector<E>> vals; };

  const VerifyParams& prm;
  const std::vector<AirParams>& airs;
  const size_t ni;
  const int zk, R, lb, cap_h;
  const ParsedProof<PP, DC> P;
  const std::vector<uint32_t> rc;
  const MmcsChecker<PP> mmcs;
  std::vector<Digest> prep_cap;
  std::vector<LookupLayout> layouts;
  std::vector<int> log_n, log_e, width, prep_w;   // base / extended (committed) degree bits
  std::vector<int> perm_insts;                    // the instances with lookups
  HostChallenger<PP, DC> ch;
  E alpha, zeta, l_prefix = E::zero(), l_beta_pow[kMaxExtD + 1];
  std::vector<std::vector<Mat>> rounds;
  std::vector<const std::vector<Digest>*> round_caps;
  const FriVerifyParams fri_prm;
  FriVerifier<PP, DC> fri;
  std::vector<E> fa_pow;
  int log_max = 0;

  BatchVerifier(const VerifyParams& prm_, const std::vector<uint32_t>& rc_canonical, const std::vector<AirParams>& airs_,
                const std::vector<uint32_t>& prep_cap_canonical, const uint8_t* bytes, size_t n_bytes, bool canonical)
      : prm(prm_), airs(airs_), ni(airs_.size()), zk(prm_.zk ? 1 : 0), R(zk ? prm_.num_random_codewords : 0), lb(prm_.log_blowup),
        cap_h(prm_.cap_height), P(parse(prm_, bytes, n_bytes, canonical)), rc(montgomery_constants<PP>(rc_canonical)),
        mmcs{prm_.mmcs_arity, prm_.mmcs_salt_elems, rc.data()}, prep_cap(size_t(1) << cap_h), ch(rc.data()),
        fri_prm{prm_.log_blowup, prm_.max_log_arity, prm_.cap_height, prm_.log_final_poly_len, prm_.commit_pow_bits, prm_.query_pow_bits,
                prm_.num_queries, &prm_.fri_log_arities},
        fri(fri_prm, mmcs) {
    if (P.insts.size() != ni || P.degree_bits.size() != ni || P.terminals.size() != ni)
      vfail("proof has %zu instances, the verifier was given %zu AIRs", P.insts.size(), ni);
    if (prep_cap_canonical.size() != prep_cap.size() * P2_DIGEST) vfail("preprocessed commitment has the wrong size");
    for (size_t j = 0; j < prep_cap.size(); ++j)
      for (int k = 0; k < P2_DIGEST; ++k) prep_cap[j][k] = F::from_canonical(prep_cap_canonical[j * P2_DIGEST + k]);
    for (auto& b : l_beta_pow) b = E::zero();
  }
  static ParsedProof<PP, DC> parse(const VerifyParams& prm, const uint8_t* bytes, size_t n_bytes, bool canonical) {
    ProofBuilder<PP, DC> B(bytes, n_bytes, canonical);
    walk_batch_proof(B, prm.layout, prm.zk != 0, prm.mmcs_salt_elems != 0, false);
    return std::move(B.P);
  }
  bool any_lookup() const { return !perm_insts.empty(); }
  void observe_cap(const std::vector<Digest>& cap) { for (auto& d : cap) for (auto x : d) ch.observe(x); }

  void shapes(const std::vector<uint32_t>& expected_degree_bits) {
    // randomisation must match the PCS's ZK setting (batch_stark.rs:424-428: RandomizationError)
    if (P.rand_cap.has_value() != (zk != 0)) vfail("RandomizationError: random commitment presence does not match the ZK setting");
    for (auto& in : P.insts)
      if (in.random.has_value() != (zk != 0)) vfail("RandomizationError: random opened values presence does not match the ZK setting");
    layouts.resize(ni); log_n.resize(ni); log_e.resize(ni); width.resize(ni); prep_w.resize(ni);
    const int p2w = p2_perm_cols<PP>() + 2;
    for (size_t i = 0; i < ni; ++i) {
      const auto& in = P.insts[i];
      layouts[i] = lookup_layout(airs[i], zk);
      log_e[i] = P.degree_bits[i];
      // the domains are the verifier's, not the prover's: recursion/src/verifier/batch_stark.rs:793 (ZK: the preprocessed
      // metadata holds the EXTENDED degree bits, recursion.rs:374)
      if (expected_degree_bits.size() != ni || (uint32_t)log_e[i] != expected_degree_bits[i])
        vfail("InvalidProofShape: instance %zu declares degree_bits %d, the preprocessed metadata has %u", i, log_e[i],
              i < expected_degree_bits.size() ? expected_degree_bits[i] : 0u);
      if (log_e[i] < zk) vfail("InvalidProofShape: extended degree bits smaller than the ZK adjustment");   // :536
      log_n[i] = log_e[i] - zk;
      if (log_e[i] + lb > PP::TWO_ADICITY) vfail("instance %zu: degree too large", i);
      width[i] = air_width_of(airs[i], p2w, p2w_perm_cols<PP>() + 4);
      prep_w[i] = air_prep_width_of(airs[i]);
      // quotient_degree = 1 << (log_qd + is_zk) (:487-496)
      const size_t aw = (size_t)layouts[i].aux_width() * DC, C = size_t(1) << (layouts[i].log_chunks + zk);
      if (in.random && in.random->size() != (size_t)DC) vfail("RandomizationError: instance %zu: %zu random opened values", i, in.random->size());
      if (in.main_local.size() != (size_t)width[i]) vfail("instance %zu: %zu main openings, the AIR has %d columns", i, in.main_local.size(), width[i]);
      if (air_uses_next(airs[i]) != in.main_next.has_value()) vfail("instance %zu: main next-row openings do not match the AIR", i);
      if (in.main_next && in.main_next->size() != (size_t)width[i]) vfail("instance %zu: bad main next width", i);
      if (in.prep_local.size() != (size_t)prep_w[i] || in.prep_next.size() != (size_t)prep_w[i]) vfail("instance %zu: bad preprocessed opening width", i);
      if (in.perm_local.size() != aw || in.perm_next.size() != aw) vfail("instance %zu: bad permutation opening width", i);
      if (in.chunks.size() != C) vfail("instance %zu: %zu quotient chunks, expected %zu", i, in.chunks.size(), C);
      for (auto& c : in.chunks) if (c.size() != (size_t)DC) vfail("instance %zu: bad quotient chunk width", i);
      if ((layouts[i].n_groups > 0) != P.terminals[i].has_value()) vfail("instance %zu: lookup terminal presence mismatch", i);
      if (layouts[i].n_groups) perm_insts.push_back((int)i);
    }
    if (any_lookup() != P.perm_cap.has_value()) vfail("permutation commitment presence mismatch");
  }

  // same order as prove_batch: instance shapes, main and preprocessed commitments, the lookup challenges, alpha, zeta
  void transcript_head() {
    ch.observe_base_as_ext(ni);
    for (size_t i = 0; i < ni; ++i) {
      ch.observe_base_as_ext(log_e[i]);
      ch.observe_base_as_ext(log_n[i]);
      ch.observe_base_as_ext(width[i]);
      ch.observe_base_as_ext(uint64_t(1) << (layouts[i].log_chunks + zk));
    }
    observe_cap(P.main_cap);
    for (size_t i = 0; i < ni; ++i) ch.observe_base_as_ext(prep_w[i]);
    observe_cap(prep_cap);
    if (any_lookup()) {
      const E alpha_l = ch.sample_ext(), beta_l = ch.sample_ext();
      E bp = E::one();
      // gamma = beta^W, W = the widest bus tuple = 1 + circuit extension degree (get_perm_challenges,
      // recursion/src/verifier/batch_stark.rs:1086-1100)
      int tuple_w = 2;
      for (auto& a : airs) tuple_w = std::max(tuple_w, std::min(a.ext_d, kMaxExtD) + 1);
      for (int j = 0; j < tuple_w; ++j) { l_beta_pow[j] = bp; bp *= beta_l; }
      l_prefix = alpha_l + bp;
      observe_cap(*P.perm_cap);
      for (int i : perm_insts) ch.observe_ext(*P.terminals[i]);
    }
    alpha = ch.sample_ext();
    observe_cap(P.quot_cap);
    if (zk) observe_cap(*P.rand_cap);   // :623-625
    zeta = ch.sample_ext();
  }

  // input batches in round order ([random,] main, quotient, preprocessed, permutation): matrices (log LDE height,
  // width), points and claimed values.  ZK: every committed matrix has R more columns - the random codewords - whose
  // values at each point are the opening proof's first item; they are appended to the point's values before anything
  // is observed or reduced (merge_hiding_random_openings, pcs/fri/targets.rs:1076-1130; batch_stark.rs:1116-1260).
  void opening_rounds() {
    if (zk) {
      rounds.emplace_back();
      round_caps.push_back(&*P.rand_cap);
      for (size_t i = 0; i < ni; ++i) rounds.back().push_back({log_e[i] + lb, DC, {zeta}, {*P.insts[i].random}});   // :645-661
    }
    rounds.emplace_back();
    round_caps.push_back(&P.main_cap);
    for (size_t i = 0; i < ni; ++i) {
      Mat m{log_e[i] + lb, width[i], {zeta}, {P.insts[i].main_local}};
      // zeta * g of the BASE trace domain (:663-700)
      if (P.insts[i].main_next) { m.z.push_back(zeta * F::two_adic_generator(log_n[i])); m.vals.push_back(*P.insts[i].main_next); }
      rounds.back().push_back(m);
    }
    rounds.emplace_back();
    round_caps.push_back(&P.quot_cap);
    for (size_t i = 0; i < ni; ++i)   // randomized_quotient_domains: natural_domain_for_degree(size << is_zk) (:719-727)
      for (auto& c : P.insts[i].chunks) rounds.back().push_back({log_e[i] + lb, DC, {zeta}, {c}});
    rounds.emplace_back();
    round_caps.push_back(&prep_cap);
    for (size_t i = 0; i < ni; ++i)
      rounds.back().push_back({log_e[i] + lb, prep_w[i], {zeta, zeta * F::two_adic_generator(log_n[i])},
                               {P.insts[i].prep_local, P.insts[i].prep_next}});
    if (any_lookup()) {
      rounds.emplace_back();
      round_caps.push_back(&*P.perm_cap);
      for (int i : perm_insts)
        rounds.back().push_back({log_e[i] + lb, layouts[i].aux_width() * DC, {zeta, zeta * F::two_adic_generator(log_n[i])},
                                 {P.insts[i].perm_local, P.insts[i].perm_next}});
    }
    if (zk) {
      if (P.fri_random.size() != rounds.size()) vfail("InvalidProofShape: hiding FRI proof: random rounds count does not match commitments");
      for (size_t r = 0; r < rounds.size(); ++r) {
        if (P.fri_random[r].size() != rounds[r].size()) vfail("InvalidProofShape: hiding FRI proof: random matrices count does not match (round %zu)", r);
        for (size_t m = 0; m < rounds[r].size(); ++m) {
          Mat& M = rounds[r][m];
          if (P.fri_random[r][m].size() != M.z.size()) vfail("InvalidProofShape: hiding FRI proof: random points count does not match (round %zu matrix %zu)", r, m);
          for (size_t p = 0; p < M.z.size(); ++p) {
            const auto& extra = P.fri_random[r][m][p];
            if (extra.size() != (size_t)R) vfail("InvalidProofShape: hiding FRI proof: %zu random codeword values, expected %d", extra.size(), R);
            M.vals[p].insert(M.vals[p].end(), extra.begin(), extra.end());
          }
          M.w += R;
        }
      }
    }
    for (auto& r : rounds) for (auto& m : r) for (auto& pv : m.vals) for (auto& v : pv) ch.observe_ext(v);
  }

  void constraints_at_zeta() {
    E terminal_sum = E::zero();
    for (size_t i = 0; i < ni; ++i) {
      const auto& in = P.insts[i];
      ZetaInstance<PP, DC> zi{&in.main_local, in.main_next ? &*in.main_next : nullptr, &in.prep_local, &in.prep_next,
                          &in.perm_local, &in.perm_next, &in.chunks, P.terminals[i] ? &*P.terminals[i] : nullptr};
      check_instance_at_zeta<PP, DC>(airs[i], layouts[i], log_n[i], zi, alpha, zeta, l_prefix, l_beta_pow, rc.data(), i, zk);
      if (layouts[i].n_groups) terminal_sum += *P.terminals[i];
    }
    if (any_lookup() && !terminal_sum.is_zero()) vfail("global lookup sum is not zero");
  }

  // the FRI transcript (fri_verify.h): the arity schedule the prover must have used, the commit caps with their proofs
  // of work and betas, the final polynomial, the query proof of work
  void fri_commit_phase() {
    const E fri_alpha = ch.sample_ext();
    size_t max_w = 1;
    std::vector<int> heights;
    for (auto& r : rounds) for (auto& m : r) { heights.push_back(m.log_h); max_w = std::max(max_w, (size_t)m.w); }
    fa_pow.assign(max_w + 1, E::one());
    for (size_t c = 1; c <= max_w; ++c) fa_pow[c] = fa_pow[c - 1] * fri_alpha;
    fri.schedule(heights);
    log_max = fri.log_max;
    fri.commit_phase(ch, P.commit_caps, P.commit_pow, P.final_poly, P.query_pow, P.queries.size());
  }

  void queries() {
    for (size_t qi = 0; qi < P.queries.size(); ++qi) {
      const size_t index = ch.sample_bits(log_max);
      const Reduced ro = input_openings(qi, index);
      fri.fold_chain(qi, index, P.queries[qi].phases, P.commit_caps, P.final_poly, [&](int log_h) -> const E* {
        auto it = ro.find(log_h);
        return it == ro.end() ? nullptr : &it->second.second;
      });
    }
  }

  // the input batches of one query against their commitments, and its reduced openings per height: log_h -> (next
  // alpha power, value), alpha powers restart per height (pcs/fri/verifier.rs:1068-1356)
  using Reduced = std::map<int, std::pair<E, E>>;
  Reduced input_openings(size_t qi, size_t index) const {
    const auto& Q = P.queries[qi];
    const F gen = F::generator();
    if (Q.rounds.size() != rounds.size()) vfail("query %zu: %zu input batches, expected %zu", qi, Q.rounds.size(), rounds.size());
    Reduced ro;
    for (size_t r = 0; r < rounds.size(); ++r) {
      std::vector<int> lhs;
      for (auto& m : rounds[r]) lhs.push_back(m.log_h);
      int r_max = 0;
      for (int x : lhs) r_max = std::max(r_max, x);
      const auto& qr = Q.rounds[r];
      if (qr.rows.size() != rounds[r].size()) vfail("query %zu: batch %zu opens %zu matrices, expected %zu", qi, r, qr.rows.size(), rounds[r].size());
      for (size_t m = 0; m < rounds[r].size(); ++m)
        if (qr.rows[m].size() != (size_t)rounds[r][m].w) vfail("query %zu: batch %zu matrix %zu has the wrong width", qi, r, m);
      mmcs.check_opening(*round_caps[r], cap_h, lhs, qr.rows, qr.salts, index >> (log_max - r_max), qr.path, "input batch");
      for (size_t m = 0; m < rounds[r].size(); ++m) {
        const Mat& M = rounds[r][m];
        auto it = ro.find(M.log_h);
        if (it == ro.end()) it = ro.emplace(M.log_h, std::make_pair(E::one(), E::zero())).first;
        const size_t ridx = index >> (log_max - M.log_h);
        const F x = gen * F::two_adic_generator(M.log_h).pow(bit_reverse((uint32_t)ridx, M.log_h));  // verifier.rs:921-981
        E S = E::zero();
        for (int c = 0; c < M.w; ++c) S += fa_pow[c] * qr.rows[m][c];
        for (size_t p = 0; p < M.z.size(); ++p) {
          E Vp = E::zero();
          for (int c = 0; c < M.w; ++c) Vp += fa_pow[c] * M.vals[p][c];
          it->second.second += it->second.first * (Vp - S) * (M.z[p] - E::from_base(x)).inv();
          it->second.first *= fa_pow[M.w];
        }
      }
    }
    return ro;
  }
};

template <class PP, int DC = 4>
void verify_batch(const VerifyParams& prm, const std::vector<uint32_t>& rc_canonical, const std::vector<AirParams>& airs,
                  const std::vector<uint32_t>& prep_cap_canonical, const std::vector<uint32_t>& expected_degree_bits,
                  const uint8_t* bytes, size_t n_bytes, bool canonical) {
  if (prm.zk && (prm.num_random_codewords < 1 || prm.num_random_codewords > 8)) vfail("num_random_codewords must be in 1..8");
  if (prm.mmcs_salt_elems < 0 || prm.mmcs_salt_elems > 16) vfail("mmcs_salt_elems must be in 0..16");
  BatchVerifier<PP, DC> V(prm, rc_canonical, airs, prep_cap_canonical, bytes, n_bytes, canonical);
  V.shapes(expected_degree_bits);
  V.transcript_head();
  V.opening_rounds();
  V.constraints_at_zeta();
  V.fri_commit_phase();
  V.queries();
}

}  // namespace p3r
