// p3_fri::verifier::verify_fri on the host, free of HIP: the part of a FRI verification that knows nothing of the input
// batches.  One statement, two callers: the native batch verifier (verify_impl.h: BatchVerifier's FRI phases) and the
// public seam (p3r_fri_verify / p3r_fri_verify_transcript, include/p3r.h), whose inputs are the caller's reduced openings.
//   fold schedule, commit caps, proofs of work, betas     recursion/src/pcs/fri/verifier.rs:1371-1520
//   fold chain of a query, roll-ins, commit-phase MMCS    recursion/src/pcs/fri/verifier.rs:562-781
//   final polynomial at the query's point                 recursion/src/pcs/fri/verifier.rs:887-915
// A refusal is a VerifyFailure whose text names the rule and the place.
#pragma once
#include <map>

#include "host_mmcs.h"

namespace p3r {

struct FriVerifyParams {
  int log_blowup, max_log_arity, cap_height, log_final_poly_len, commit_pow_bits, query_pow_bits, num_queries;
  const std::vector<uint8_t>* schedule;   // the explicit folding schedule (p3r_config.fri_log_arities), empty: the rule
};

template <class PP, int DC = 4>
struct FriVerifier {
  using F = Fp<PP>;
  using E = typename Chal<PP, DC>::type;
  using Digest = std::array<F, P2_DIGEST>;
  using Cap = std::vector<Digest>;

  const FriVerifyParams prm;
  const MmcsChecker<PP>& mmcs;
  int log_max = 0;
  std::vector<int> las;    // the schedule the prover must have followed
  std::vector<E> betas;

  FriVerifier(const FriVerifyParams& prm_, const MmcsChecker<PP>& mmcs_) : prm(prm_), mmcs(mmcs_) {}

  // The arity schedule for these input heights (any order, repeats allowed): the FRI prover's rule (prove_impl.hip.h
  // step 7, Context.prove_fri), or the explicit schedule where it is legal.
  void schedule(std::vector<int> heights) {
    log_max = 0;
    for (int h : heights) log_max = std::max(log_max, h);
    std::sort(heights.rbegin(), heights.rend());
    heights.erase(std::unique(heights.begin(), heights.end()), heights.end());
    const int log_final = prm.log_final_poly_len + prm.log_blowup;
    size_t next_h = 1;
    int cur = log_max;
    las.clear();
    while (cur > log_final) {
      int log_next = next_h < heights.size() ? heights[next_h] : -1;
      const int la = fri_log_arity(*prm.schedule, las.size(), prm.max_log_arity, cur, log_final, log_next);
      if (la < 0) vfail("FRI: the configured folding schedule does not fit the proof (phase %zu)", las.size());
      if (next_h < heights.size() && heights[next_h] == cur - la) ++next_h;
      cur -= la;
      las.push_back(la);
    }
    if (next_h != heights.size()) vfail("FRI: an input height is never rolled in");
    if (cur != log_final) vfail("FRI: fold schedule does not end at the final polynomial length");
  }

  // The FRI transcript up to the query indices: every cap observed, its proof of work checked, its beta sampled; the
  // final polynomial and the log arities observed; the query proof of work checked.  `las` is set (schedule()).
  template <class Ch>
  void commit_phase(Ch& ch, const std::vector<Cap>& caps, const std::vector<F>& commit_pow, const std::vector<E>& final_poly, F query_pow,
                    size_t n_queries) {
    if (caps.size() != las.size() || commit_pow.size() != las.size()) vfail("FRI: %zu commit phases, expected %zu", caps.size(), las.size());
    if (final_poly.size() != (size_t(1) << prm.log_final_poly_len)) vfail("FRI: final polynomial has the wrong length");
    betas.clear();
    for (size_t p = 0; p < las.size(); ++p) {
      for (auto& d : caps[p]) for (auto x : d) ch.observe(x);
      if (!ch.check_witness(prm.commit_pow_bits, commit_pow[p])) vfail("FRI: invalid commit-phase proof of work (commit proof-of-work of phase %zu)", p);
      betas.push_back(ch.sample_ext());
    }
    for (auto& c : final_poly) ch.observe_ext(c);
    for (int la : las) ch.observe(F::from_canonical((uint32_t)la));
    if (!ch.check_witness(prm.query_pow_bits, query_pow)) vfail("FRI: invalid query proof of work");
    if ((int)n_queries != prm.num_queries) vfail("FRI: %zu queries, expected %d", n_queries, prm.num_queries);
  }

  // The fold chain of one query down to the final polynomial (pcs/fri/verifier.rs:562-781).  `phases`: per commit phase
  // an object with la, sibs (the opened row without the queried element), salts and path; `reduced(log_h)`: the reduced
  // opening of that height at index >> (log_max - log_h), or NULL where no input has it.
  template <class Phases, class Reduced>
  void fold_chain(size_t qi, size_t index, const Phases& phases, const std::vector<Cap>& caps, const std::vector<E>& final_poly,
                  Reduced&& reduced) const {
    if (phases.size() != las.size()) vfail("query %zu: %zu commit-phase openings, expected %zu", qi, phases.size(), las.size());
    const E* top = reduced(log_max);
    if (!top) vfail("query %zu: no reduced opening at the maximum height", qi);
    E folded = *top;
    size_t idx = index;
    int cur = log_max;
    const F neg_half = -(F::from_canonical(2).inv());
    for (size_t p = 0; p < las.size(); ++p) {
      const auto& ph = phases[p];
      const int la = las[p];
      const size_t arity = size_t(1) << la, pos = idx & (arity - 1), row = idx >> la;
      if (ph.la != la || ph.sibs.size() != arity - 1) vfail("query %zu phase %zu: wrong arity", qi, p);
      std::vector<E> e(arity);
      for (size_t j = 0, s = 0; j < arity; ++j) e[j] = j == pos ? folded : ph.sibs[s++];
      // the leaf is the row of 2^la sibling evaluations, extension elements flattened
      std::vector<F> leaf;
      for (auto& x : e) for (int k = 0; k < DC; ++k) leaf.push_back(x.c[k]);
      char what[64];
      snprintf(what, sizeof what, "FRI commit phase %zu of query %zu", p, qi);
      mmcs.check_opening(caps[p], prm.cap_height, {cur - la}, {leaf}, ph.salts, row, ph.path, what);
      F ss_inv = F::two_adic_generator(cur).inv().pow(bit_reverse((uint32_t)row, cur - la));
      E b = betas[p];
      const F omega = F::two_adic_generator(la);
      size_t len = arity;
      for (int s = 0; s < la; ++s) {
        const F om_s = omega.pow(uint64_t(1) << s);
        for (size_t j = 0; j < len / 2; ++j) {
          const F x0_inv = ss_inv * om_s.pow(bit_reverse((uint32_t)(2 * j), la - s)).inv();
          const E t = b * x0_inv - E::one();  // arity2_fold_at_point: e0 + (beta - x0)(e1 - e0)(-1/2)/x0
          e[j] = e[2 * j] + t * (e[2 * j + 1] - e[2 * j]) * neg_half;
        }
        len /= 2;
        ss_inv = ss_inv.sqr();
        b = b.sqr();
      }
      folded = e[0];
      cur -= la;
      idx = row;
      const E* in = cur != log_max ? reduced(cur) : nullptr;
      if (in) folded += betas[p].pow(arity) * *in;  // roll-in
    }
    // final polynomial at x = w^{bitrev(idx)} of the size-2^cur domain (verifier.rs:887-915)
    const F x = F::two_adic_generator(cur).pow(bit_reverse((uint32_t)idx, cur));
    E eval = E::zero();
    for (size_t k = final_poly.size(); k-- > 0;) eval = eval * x + final_poly[k];
    if (!(eval == folded)) vfail("query %zu: final polynomial mismatch", qi);
  }
};

// One commit-phase opening of a query, as the public seam's views are read into it
template <class PP, int DC = 4>
struct FriPhaseOpening {
  int la;
  std::vector<typename Chal<PP, DC>::type> sibs;
  std::vector<std::array<Fp<PP>, P2_DIGEST>> path;
  std::vector<std::vector<Fp<PP>>> salts;
};

}  // namespace p3r
