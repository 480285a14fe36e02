// The host-only entries of the FRI verifier seam and what they share with the other host-only entries (host_abi.h):
// the permutation constants of a configuration, the frame that turns a refusal into a code and a text, the challenger
// handle.  Free of HIP: a plain C++ compiler builds this header, which is how tests/fri_verify_san_main.cpp runs
// p3r_fri_verify under the address and undefined-behaviour sanitizers.  Included once per library.
#pragma once
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>

#include "../../include/p3r.h"
#include "error.h"
#include "poseidon2_rc_default.inc"
#include "poseidon2_w32_default.inc"
#include "fri_verify.h"

using namespace p3r;

namespace {

// The permutation constants of a configuration, canonical: the width-16 round constants, then the width-32 table
// (round constants | diagonal, poseidon2.h) - the layout of p3r_ctx::rc and of the verifier's table.  NULL pointers
// select the self-generated defaults.  `bad`: reports a length mismatch.
template <class PP, class Bad>
std::vector<uint32_t> constants_table(const p3r_config& cfg, Bad&& bad) {
  const size_t nrc = p2_num_constants<PP>(), nrcw = p2w_num_rc<PP>();
  const uint32_t* src = cfg.poseidon2_rc;
  if (src && cfg.poseidon2_rc_len != nrc) bad("poseidon2_rc_len", cfg.poseidon2_rc_len, nrc);
  if (!src) src = PP::FIELD_ID == 0 ? kDefaultRc_koala_bear : kDefaultRc_baby_bear;
  const uint32_t* w = cfg.poseidon2_w32_rc;
  if (w && cfg.poseidon2_w32_rc_len != nrcw) bad("poseidon2_w32_rc_len", cfg.poseidon2_w32_rc_len, nrcw);
  if (!w) w = PP::FIELD_ID == 0 ? kDefaultRcW32_koala_bear : kDefaultRcW32_baby_bear;
  const uint32_t* dg = cfg.poseidon2_w32_diag ? cfg.poseidon2_w32_diag : (PP::FIELD_ID == 0 ? kDefaultDiagW32_koala_bear : kDefaultDiagW32_baby_bear);
  std::vector<uint32_t> t(src, src + nrc);
  t.insert(t.end(), w, w + nrcw);
  t.insert(t.end(), dg, dg + P2W_WIDTH);
  for (size_t i = 0; i < t.size(); ++i)
    if (t[i] >= PP::P) p3r::vfail("%s constant %zu is not canonical (%u >= p)", i < nrc ? "poseidon2_rc" : "width-32 permutation", i < nrc ? i : i - nrc, t[i]);
  return t;
}

// p3r.h: P3R_EXT_UNPINNED_W32_DEFAULTS
inline bool w32_unacknowledged(const p3r_config& cfg) {
  return (!cfg.poseidon2_w32_rc || !cfg.poseidon2_w32_diag) && !(cfg.ext_choices & P3R_EXT_UNPINNED_W32_DEFAULTS);
}
constexpr const char* kW32Unpinned =
    "the width-32 permutation with poseidon2_w32_rc / poseidon2_w32_diag NULL: the built-in constants are self-generated, not "
    "upstream's - pass the caller's, or acknowledge with P3R_EXT_UNPINNED_W32_DEFAULTS";

template <class PP>
std::vector<uint32_t> host_constants_table(const p3r_config& cfg) {
  return constants_table<PP>(cfg, [](const char* what, uint32_t got, size_t want) {
    p3r::vfail("%s is %u, the field needs %zu constants", what, got, want);
  });
}

// ---- the frame of every entry point below: a refusal is a code and a text; anything thrown is P3R_EINVAL with its text
struct Refused { int code; const char* text; };
[[noreturn]] inline void refuse(int code, const char* text) { throw Refused{code, text}; }
template <class Body>
int guarded(char* err_buf, size_t err_cap, Body&& body) {
  auto report = [&](const char* msg) {
    if (err_buf && err_cap) snprintf(err_buf, err_cap, "%s", msg);
  };
  try {
    return body();
  } catch (const Refused& r) {
    report(r.text);
    return r.code;
  } catch (const std::exception& e) {
    report(e.what());
    return P3R_EINVAL;
  }
}
template <class Run>
void for_field(uint32_t field, Run&& run) {
  if (field == P3R_FIELD_KOALA_BEAR) run(p3r::KoalaBearParams{});
  else if (field == P3R_FIELD_BABY_BEAR) run(p3r::BabyBearParams{});
  else refuse(P3R_EINVAL, "unknown field");
}

// what p3r_mmcs_verify and p3r_verify_batch ask of a configuration's MMCS.  `uses_w32`: something of the call runs over
// the width-32 permutation (the arity-4 MMCS does; so does its AIR's table)
inline void check_mmcs_config(const p3r_config& cfg, bool uses_w32) {
  if (cfg.mmcs_arity != 0 && cfg.mmcs_arity != 2 && cfg.mmcs_arity != 4) refuse(P3R_EINVAL, "mmcs_arity must be 2 or 4");
  if (cfg.mmcs_arity == 4 && cfg.cap_height != 0) refuse(P3R_EUNSUPPORTED, "arity-4 MMCS: cap_height must be 0");
  if ((uses_w32 || cfg.mmcs_arity == 4) && w32_unacknowledged(cfg)) refuse(P3R_EINVAL, kW32Unpinned);
}
inline void check_salt_elems(const p3r_config& cfg) {
  if (cfg.mmcs_salt_elems > 16) refuse(P3R_EINVAL, "mmcs_salt_elems must be in 0..16");
}
inline void check_width(size_t w) {
  if (w > (size_t(1) << 24)) refuse(P3R_EINVAL, "matrix width out of range");
}

}  // namespace

// p3r_challenger: a thin handle around HostChallenger<PP, DC> (host_transcript.h), DC the context's challenge degree
struct p3r_challenger {
  p3r_ctx* ctx = nullptr;
  int tag = 0;                // 0: KoalaBear, DC = 4; 1: KoalaBear, DC = 5; 2: BabyBear, DC = 4
  std::vector<uint32_t> rc;   // the context's width-16 constants, Montgomery: what the HostChallenger points at
  std::shared_ptr<void> impl;
};
namespace {
template <class Fn>
void challenger_visit(const p3r_challenger* ch, Fn&& fn) {
  switch (ch->tag) {
    case 0: fn(*static_cast<HostChallenger<KoalaBearParams, 4>*>(ch->impl.get())); break;
    case 1: fn(*static_cast<HostChallenger<KoalaBearParams, 5>*>(ch->impl.get())); break;
    default: fn(*static_cast<HostChallenger<BabyBearParams, 4>*>(ch->impl.get())); break;
  }
}
// a fresh transcript, or a copy of src's (same tag), over ch's own copy of the constants
inline void challenger_make(p3r_challenger* ch, const p3r_challenger* src) {
  auto make = [&](auto tag) {
    using C = decltype(tag);
    auto c = std::make_shared<C>(ch->rc.data());
    if (src) {
      *c = *static_cast<const C*>(src->impl.get());
      c->rc = ch->rc.data();
    }
    ch->impl = c;
  };
  switch (ch->tag) {
    case 0: make(HostChallenger<KoalaBearParams, 4>(nullptr)); break;
    case 1: make(HostChallenger<KoalaBearParams, 5>(nullptr)); break;
    default: make(HostChallenger<BabyBearParams, 4>(nullptr)); break;
  }
}
}  // namespace

namespace {

// p3r_last_error(NULL): the text of the last refusal that had no context to keep it (a failed p3r_create, the host-only
// entries without an error buffer)
thread_local std::string g_create_error;

// The frame of the host-only entries that report through p3r_last_error(NULL).  A VerifyFailure is a rejected proof
// once `verifying` is set, and a malformed argument before.
template <class Body>
int host_guard(Body&& body) {
  bool verifying = false;
  try {
    body(verifying);
    return P3R_OK;
  } catch (const Error& e) {
    g_create_error = e.what();
    return e.code;
  } catch (const Refused& r) {
    g_create_error = r.text;
    return r.code;
  } catch (const VerifyFailure& e) {
    g_create_error = e.what();
    return verifying ? P3R_EVERIFY : P3R_EINVAL;
  } catch (const std::exception& e) {
    g_create_error = e.what();
    return P3R_EINVAL;
  }
}

// what every entry of the FRI verifier seam asks of a configuration; returns the challenger tag it implies
inline int check_fri_verify_config(const p3r_config* cfg) {
  if (!cfg) fail(P3R_EINVAL, "cfg is NULL");
  if (cfg->abi_version != P3R_ABI_VERSION) fail(P3R_EINVAL, "abi_version %u != %u", cfg->abi_version, P3R_ABI_VERSION);
  if (cfg->field != P3R_FIELD_KOALA_BEAR && cfg->field != P3R_FIELD_BABY_BEAR) fail(P3R_EINVAL, "unknown field %u", cfg->field);
  if (cfg->challenge_degree != 0 && cfg->challenge_degree != 4 && cfg->challenge_degree != 5)
    fail(P3R_EINVAL, "challenge_degree must be 4 or 5 (got %u)", cfg->challenge_degree);
  if (cfg->challenge_degree == 5 && cfg->field != P3R_FIELD_KOALA_BEAR)
    fail(P3R_EUNSUPPORTED, "UnsupportedChallengeDegree: the quintic challenge field is KoalaBear's");
  return cfg->field == P3R_FIELD_KOALA_BEAR ? (cfg->challenge_degree == 5 ? 1 : 0) : 2;
}

inline std::vector<uint8_t> config_schedule(const p3r_config& cfg) {
  if (!cfg.fri_log_arities) return {};
  return std::vector<uint8_t>(cfg.fri_log_arities, cfg.fri_log_arities + cfg.fri_log_arities_len);
}

// One run of p3r_fri_verify[_transcript]: the views are read into the verifier's own types (every read is inside the
// lengths given), then fri_verify.h decides.
template <class PP, int DC>
struct FriSeamRun {
  using F = Fp<PP>;
  using E = typename Chal<PP, DC>::type;
  using Digest = std::array<F, P2_DIGEST>;
  using Cap = std::vector<Digest>;

  const p3r_config& cfg;
  const p3r_fri_proof_view& pv;
  std::vector<uint8_t> sched;
  std::vector<uint32_t> rc;
  MmcsChecker<PP> mmcs;
  FriVerifier<PP, DC> fri;
  size_t n_phases, cap_len;
  std::vector<Cap> caps;
  std::vector<F> commit_pow;
  std::vector<E> final_poly;
  F query_pow;

  static F fe(uint32_t v, const char* what, size_t at) {
    if (v >= PP::P) fail(P3R_EINVAL, "non-canonical word %zu of %s", at, what);
    return F::from_canonical(v);
  }
  static void need(const void* p, size_t n, const char* what) {
    if (n && !p) fail(P3R_EINVAL, "%s is NULL", what);
  }

  FriSeamRun(const p3r_config& cfg_, const p3r_fri_proof_view& pv_)
      : cfg(cfg_), pv(pv_), sched(config_schedule(cfg_)), rc(montgomery_constants<PP>(host_constants_table<PP>(cfg_))),
        mmcs{cfg_.mmcs_arity == 4 ? 4 : 2, (int)cfg_.mmcs_salt_elems, rc.data()},
        fri(FriVerifyParams{(int)cfg_.log_blowup, (int)cfg_.max_log_arity, (int)cfg_.cap_height, (int)cfg_.log_final_poly_len,
                            (int)cfg_.commit_pow_bits, (int)cfg_.query_pow_bits, (int)cfg_.num_queries, &sched},
            mmcs),
        n_phases(pv_.log_arities_len), cap_len(size_t(1) << cfg_.cap_height) {
    // ---- the parts of the proof that do not depend on the query indices
    need(pv.log_arities, pv.log_arities_len, "log_arities");
    need(pv.commit_caps, pv.commit_caps_len, "commit_caps");
    need(pv.commit_pow, pv.commit_pow_len, "commit_pow");
    need(pv.final_poly, pv.final_poly_len, "final_poly");
    if (pv.log_max_height > (uint32_t)PP::TWO_ADICITY) fail(P3R_EINVAL, "log_max_height %u exceeds the field's two-adicity (%d)", pv.log_max_height, PP::TWO_ADICITY);
    if (n_phases > 32) fail(P3R_EINVAL, "%zu commit phases: more than any height has", n_phases);
    if (pv.commit_caps_len != n_phases * cap_len * P2_DIGEST)
      fail(P3R_EINVAL, "commit_caps holds %zu words, %zu phases of 2^%u digests need %zu", pv.commit_caps_len, n_phases, cfg.cap_height, n_phases * cap_len * P2_DIGEST);
    if (pv.commit_pow_len != n_phases) fail(P3R_EINVAL, "commit_pow holds %zu witnesses for %zu phases", pv.commit_pow_len, n_phases);
    if (pv.final_poly_len != ((size_t)DC << cfg.log_final_poly_len))
      fail(P3R_EINVAL, "final_poly holds %zu words, 2^%u coefficients of %d words need %zu", pv.final_poly_len, cfg.log_final_poly_len, DC, (size_t)DC << cfg.log_final_poly_len);
    caps.resize(n_phases);
    for (size_t p = 0, at = 0; p < n_phases; ++p) {
      caps[p].resize(cap_len);
      for (auto& d : caps[p]) for (auto& x : d) { x = fe(pv.commit_caps[at], "commit_caps", at); ++at; }
    }
    commit_pow.resize(n_phases);
    for (size_t p = 0; p < n_phases; ++p) commit_pow[p] = fe(pv.commit_pow[p], "commit_pow", p);
    final_poly.resize(size_t(1) << cfg.log_final_poly_len);
    for (size_t i = 0; i < final_poly.size(); ++i)
      for (int k = 0; k < DC; ++k) final_poly[i].c[k] = fe(pv.final_poly[i * DC + k], "final_poly", i * DC + k);
    query_pow = fe(pv.query_pow, "query_pow", 0);
  }

  // The schedule as far as it can be judged without the input heights: every arity within the configuration's bound,
  // the explicit schedule's entries where there is one, and the sum the distance to the final height.
  void adopt_proof_schedule() {
    const int log_final = (int)(cfg.log_final_poly_len + cfg.log_blowup);
    int cur = (int)pv.log_max_height;
    fri.log_max = cur;
    fri.las.clear();
    for (size_t p = 0; p < n_phases; ++p) {
      const int la = pv.log_arities[p];
      if (la < 1 || la > (int)cfg.max_log_arity || la > cur - log_final || (!sched.empty() && (p >= sched.size() || sched[p] != la)))
        vfail("FRI: log arity %d of phase %zu is not one the folding schedule allows", la, p);
      cur -= la;
      fri.las.push_back(la);
    }
    if (cur > log_final) vfail("FRI: %zu commit phases end at height 2^%d, above the final height 2^%d", n_phases, cur, log_final);
    if (cur != log_final) vfail("FRI: fold schedule does not end at the final polynomial length");
  }
  // With the input heights: exactly the schedule the prover follows
  void check_schedule(const std::vector<int>& heights) {
    fri.schedule(heights);
    if (fri.las.size() != n_phases) vfail("FRI: %zu commit phases, expected %zu", n_phases, fri.las.size());
    for (size_t p = 0; p < n_phases; ++p)
      if (fri.las[p] != (int)pv.log_arities[p])
        vfail("FRI: log arity %u of phase %zu, the folding schedule gives %d", (unsigned)pv.log_arities[p], p, fri.las[p]);
  }

  template <class Ch>
  std::vector<uint32_t> transcript(Ch& ch) {
    fri.commit_phase(ch, caps, commit_pow, final_poly, query_pow, pv.n_queries);
    std::vector<uint32_t> indices(pv.n_queries);
    for (auto& i : indices) i = ch.sample_bits(fri.log_max);
    return indices;
  }

  // the commit-phase openings of query q; every length is the schedule's (P3R_EINVAL otherwise)
  std::vector<FriPhaseOpening<PP, DC>> read_query(size_t q) const {
    std::vector<FriPhaseOpening<PP, DC>> out(n_phases);
    int cur = fri.log_max;
    for (size_t p = 0; p < n_phases; ++p) {
      const p3r_fri_phase_opening_view& o = pv.openings[q * n_phases + p];
      const int la = fri.las[p];
      cur -= la;
      if (mmcs.arity != 4 && cur < (int)cfg.cap_height) fail(P3R_EINVAL, "phase %zu commits 2^%d rows, fewer than the cap's 2^%u digests", p, cur, cfg.cap_height);
      const size_t row_len = ((size_t(1) << la) - 1) * DC, S = cfg.mmcs_salt_elems;
      const size_t depth = mmcs.arity == 4 ? mmcs_proof_len(mmcs4_schedule({size_t(1) << cur})) : (size_t)(cur - (int)cfg.cap_height);
      if (o.row_len != row_len) fail(P3R_EINVAL, "query %zu phase %zu: the opened row holds %zu words, %zu siblings of %d words need %zu", q, p, o.row_len, (size_t(1) << la) - 1, DC, row_len);
      if (o.salts_len != S) fail(P3R_EINVAL, "query %zu phase %zu: %zu salt words, the MMCS has %zu", q, p, o.salts_len, S);
      if (o.siblings_len != depth * P2_DIGEST) fail(P3R_EINVAL, "query %zu phase %zu: %zu sibling words, %zu digests need %zu", q, p, o.siblings_len, depth, depth * P2_DIGEST);
      need(o.row, o.row_len, "an opened row");
      need(o.salts, o.salts_len, "a salt");
      need(o.siblings, o.siblings_len, "a sibling array");
      FriPhaseOpening<PP, DC>& ph = out[p];
      ph.la = la;
      ph.sibs.resize((size_t(1) << la) - 1);
      for (size_t j = 0; j < ph.sibs.size(); ++j)
        for (int k = 0; k < DC; ++k) ph.sibs[j].c[k] = fe(o.row[j * DC + k], "an opened row", j * DC + k);
      if (S) {
        ph.salts.assign(1, std::vector<F>(S));
        for (size_t j = 0; j < S; ++j) ph.salts[0][j] = fe(o.salts[j], "a salt", j);
      }
      ph.path.resize(depth);
      for (size_t j = 0; j < depth; ++j)
        for (int k = 0; k < P2_DIGEST; ++k) ph.path[j][k] = fe(o.siblings[j * P2_DIGEST + k], "a sibling array", j * P2_DIGEST + k);
    }
    return out;
  }
};

// the checks the two entries share, then `run` with the field, the challenge degree and the challenger of `ch`
template <class Run>
void fri_seam_dispatch(const p3r_config* cfg, p3r_challenger* ch, const p3r_fri_proof_view* proof, Run&& run) {
  const int tag = check_fri_verify_config(cfg);
  if (!ch) fail(P3R_EINVAL, "challenger is NULL");
  if (!proof) fail(P3R_EINVAL, "proof is NULL");
  if (cfg->zk) fail(P3R_EUNSUPPORTED, "zk configurations: the hiding PCS's opening proof is out of scope of the FRI verifier seam");
  check_mmcs_config(*cfg, false);
  check_salt_elems(*cfg);
  if (cfg->cap_height >= 32 || cfg->log_final_poly_len >= 32 || cfg->log_blowup >= 32) fail(P3R_EINVAL, "cap_height, log_final_poly_len and log_blowup must be below 32");
  if (cfg->max_log_arity < 1 || cfg->max_log_arity > 30) fail(P3R_EINVAL, "max_log_arity must be in 1..30");
  if (cfg->commit_pow_bits > 30 || cfg->query_pow_bits > 30) fail(P3R_EINVAL, "proof-of-work bits must be <= 30");
  if (cfg->num_queries > (1u << 20)) fail(P3R_EINVAL, "num_queries out of range");
  if (cfg->fri_log_arities_len && !cfg->fri_log_arities) fail(P3R_EINVAL, "fri_log_arities is NULL");
  if (ch->tag != tag) fail(P3R_EINVAL, "the challenger is of another field or challenge degree than the configuration");
  if (proof->n_queries > (1u << 20)) fail(P3R_EINVAL, "n_queries out of range");
  if (proof->log_max_height < cfg->cap_height) fail(P3R_EINVAL, "log_max_height %u is below cap_height %u", proof->log_max_height, cfg->cap_height);
  challenger_visit(ch, run);
}

}  // namespace

extern "C" {

p3r_challenger* p3r_challenger_create_host(const p3r_config* cfg) {
  p3r_challenger* out = nullptr;
  host_guard([&](bool&) {
    auto ch = std::make_unique<p3r_challenger>();
    ch->tag = check_fri_verify_config(cfg);
    for_field(cfg->field, [&](auto tag) {
      using PP = decltype(tag);
      ch->rc = montgomery_constants<PP>(host_constants_table<PP>(*cfg));
    });
    challenger_make(ch.get(), nullptr);
    out = ch.release();
  });
  return out;
}

int p3r_fri_log_arity_cfg(const p3r_config* cfg, size_t phase, int log_cur, int log_final, int log_next_input) {
  if (!cfg || (cfg->fri_log_arities_len && !cfg->fri_log_arities)) return -1;
  return fri_log_arity(config_schedule(*cfg), phase, (int)cfg->max_log_arity, log_cur, log_final, log_next_input);
}

int p3r_fri_verify_transcript(const p3r_config* cfg, p3r_challenger* ch, const p3r_fri_proof_view* proof, uint32_t* betas_out,
                              uint32_t* indices_out) {
  return host_guard([&](bool& verifying) {
    fri_seam_dispatch(cfg, ch, proof, [&](auto& c) {
      using C = std::decay_t<decltype(c)>;
      using PP = typename C::F::Params;
      constexpr int DC = (int)(sizeof(typename C::E) / sizeof(typename C::F));
      FriSeamRun<PP, DC> run(*cfg, *proof);
      if (run.n_phases && !betas_out) fail(P3R_EINVAL, "betas_out is NULL");
      if (proof->n_queries && !indices_out) fail(P3R_EINVAL, "indices_out is NULL");
      verifying = true;
      run.adopt_proof_schedule();
      C work = c;   // the caller's transcript moves only when the replay is accepted
      const std::vector<uint32_t> indices = run.transcript(work);
      for (size_t p = 0; p < run.n_phases; ++p)
        for (int k = 0; k < DC; ++k) betas_out[p * DC + k] = run.fri.betas[p].c[k].to_canonical();
      std::copy(indices.begin(), indices.end(), indices_out);
      c = work;
    });
  });
}

int p3r_fri_verify(const p3r_config* cfg, p3r_challenger* ch, const p3r_fri_proof_view* proof, const p3r_fri_input_view* inputs,
                   size_t n_inputs) {
  return host_guard([&](bool& verifying) {
    fri_seam_dispatch(cfg, ch, proof, [&](auto& c) {
      using C = std::decay_t<decltype(c)>;
      using PP = typename C::F::Params;
      using E = typename C::E;
      constexpr int DC = (int)(sizeof(E) / sizeof(typename C::F));
      FriSeamRun<PP, DC> run(*cfg, *proof);
      // ---- the inputs: one per height, tallest first, the tallest at log_max_height
      if (!n_inputs || !inputs) fail(P3R_EINVAL, "no input: a proof has a reduced opening at its maximum height");
      if (n_inputs > 32) fail(P3R_EINVAL, "%zu inputs: more than there are heights", n_inputs);
      const size_t nq = proof->n_queries;
      std::vector<int> heights;
      std::vector<std::vector<E>> values(n_inputs);
      for (size_t i = 0; i < n_inputs; ++i) {
        const p3r_fri_input_view& in = inputs[i];
        if (in.log_height > proof->log_max_height) fail(P3R_EINVAL, "input %zu: height 2^%u is above log_max_height %u", i, in.log_height, proof->log_max_height);
        if (i == 0 && in.log_height != proof->log_max_height) fail(P3R_EINVAL, "input 0 has height 2^%u: the tallest input comes first and has log_max_height %u", in.log_height, proof->log_max_height);
        if (i && (int)in.log_height >= heights.back()) fail(P3R_EINVAL, "input %zu: height 2^%u after 2^%d - one input per height, tallest first", i, in.log_height, heights.back());
        if (in.values_len != nq * DC) fail(P3R_EINVAL, "input %zu holds %zu words, %zu queries of %d words need %zu", i, in.values_len, nq, DC, nq * DC);
        FriSeamRun<PP, DC>::need(in.values, in.values_len, "an input's values");
        values[i].resize(nq);
        for (size_t q = 0; q < nq; ++q)
          for (int k = 0; k < DC; ++k) values[i][q].c[k] = FriSeamRun<PP, DC>::fe(in.values[q * DC + k], "an input's values", q * DC + k);
        heights.push_back((int)in.log_height);
      }
      if (nq * run.n_phases != proof->openings_len) fail(P3R_EINVAL, "openings holds %zu entries, %zu queries of %zu phases need %zu", proof->openings_len, nq, run.n_phases, nq * run.n_phases);
      FriSeamRun<PP, DC>::need(proof->openings, proof->openings_len, "openings");
      verifying = true;
      run.check_schedule(heights);
      std::vector<std::vector<FriPhaseOpening<PP, DC>>> queries(nq);
      for (size_t q = 0; q < nq; ++q) queries[q] = run.read_query(q);
      C work = c;
      const std::vector<uint32_t> indices = run.transcript(work);
      for (size_t q = 0; q < nq; ++q)
        run.fri.fold_chain(q, indices[q], queries[q], run.caps, run.final_poly, [&](int log_h) -> const E* {
          for (size_t i = 0; i < n_inputs; ++i)
            if (heights[i] == log_h) return &values[i][q];
          return nullptr;
        });
      c = work;
    });
  });
}

}  // extern "C"
