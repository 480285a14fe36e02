// p3r_fri_verify under the address and undefined-behaviour sanitizers: a stand-alone program over the HIP-free headers
// (csrc/fri_verify_abi.h), compiled by tests/test_fri_verify_san.py with g++.  It reads one accepted proof from the
// file the test wrote (a stream of u32 words, layout below), checks that it is accepted, then applies structure-aware
// mutations - words changed, lengths shortened, counts raised - and requires P3R_OK, P3R_EINVAL or P3R_EVERIFY from every
// one.  Every array the view points at is a heap copy of exactly the length the view states, so a read past a stated
// length is a read past an allocation.
//
// words: field dc log_blowup max_log_arity cap_height log_final_poly_len commit_pow_bits query_pow_bits num_queries
//        mmcs_arity salt_elems | n_observed observed.. | log_max_height query_pow | n_phases arities.. | n caps.. | n pow.. |
//        n final_poly.. | n_queries | per query and phase: n row.. n salts.. n siblings.. | n_inputs | per input: log_height n values..
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "fri_verify_abi.h"

namespace {

struct Words {
  std::vector<uint32_t> w;
  size_t at = 0;
  uint32_t next() {
    if (at >= w.size()) { fprintf(stderr, "input truncated\n"); exit(2); }
    return w[at++];
  }
  std::vector<uint32_t> vec() {
    std::vector<uint32_t> v(next());
    for (auto& x : v) x = next();
    return v;
  }
};

struct Opening { std::vector<uint32_t> row, salts, sibs; };
struct Case {
  p3r_config cfg{};
  std::vector<uint32_t> observed, caps, pow, final_poly;
  std::vector<uint8_t> arities;
  uint32_t log_max = 0, query_pow = 0;
  size_t n_queries = 0;
  std::vector<Opening> openings;
  struct In { uint32_t log_h; std::vector<uint32_t> values; };
  std::vector<In> inputs;
};

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return rng_state;
}

// exact-size heap copies: what the views point at
template <class T>
const T* exact(std::vector<std::unique_ptr<T[]>>& keep, const std::vector<T>& v) {
  keep.emplace_back(new T[v.size() ? v.size() : 1]);
  std::copy(v.begin(), v.end(), keep.back().get());
  return v.empty() ? nullptr : keep.back().get();
}

int run(const Case& c) {
  std::vector<std::unique_ptr<uint32_t[]>> k32;
  std::vector<std::unique_ptr<uint8_t[]>> k8;
  std::vector<p3r_fri_phase_opening_view> ops(c.openings.size());
  for (size_t i = 0; i < ops.size(); ++i)
    ops[i] = {exact(k32, c.openings[i].row), c.openings[i].row.size(), exact(k32, c.openings[i].salts), c.openings[i].salts.size(),
              exact(k32, c.openings[i].sibs), c.openings[i].sibs.size()};
  std::unique_ptr<p3r_fri_phase_opening_view[]> ops_exact(new p3r_fri_phase_opening_view[ops.size() ? ops.size() : 1]);
  std::copy(ops.begin(), ops.end(), ops_exact.get());
  p3r_fri_proof_view v{};
  v.log_max_height = c.log_max;
  v.query_pow = c.query_pow;
  v.commit_caps = exact(k32, c.caps); v.commit_caps_len = c.caps.size();
  v.commit_pow = exact(k32, c.pow); v.commit_pow_len = c.pow.size();
  v.log_arities = exact(k8, c.arities); v.log_arities_len = c.arities.size();
  v.final_poly = exact(k32, c.final_poly); v.final_poly_len = c.final_poly.size();
  v.openings = ops.empty() ? nullptr : ops_exact.get(); v.openings_len = ops.size();
  v.n_queries = c.n_queries;
  std::vector<p3r_fri_input_view> ins(c.inputs.size());
  for (size_t i = 0; i < ins.size(); ++i) ins[i] = {c.inputs[i].log_h, exact(k32, c.inputs[i].values), c.inputs[i].values.size()};
  // the handle's own pieces (the other p3r_challenger_* entries live next to the device code)
  std::unique_ptr<p3r_challenger> ch(p3r_challenger_create_host(&c.cfg));
  if (!ch) return P3R_EINVAL;
  challenger_visit(ch.get(), [&](auto& t) {
    using F = typename std::decay_t<decltype(t)>::F;
    for (uint32_t w : c.observed) t.observe(F::from_canonical(w % F::P));
  });
  p3r_challenger probe;
  probe.tag = ch->tag;
  probe.rc = ch->rc;
  challenger_make(&probe, ch.get());
  std::vector<uint32_t> betas(c.arities.size() * 5 + 1), idx((c.n_queries < (1u << 21) ? c.n_queries : 0) + 1);
  const int rt = p3r_fri_verify_transcript(&c.cfg, &probe, &v, betas.data(), idx.data());
  if (rt != P3R_OK && rt != P3R_EINVAL && rt != P3R_EVERIFY && rt != P3R_EUNSUPPORTED) { fprintf(stderr, "transcript gave %d\n", rt); exit(3); }
  return p3r_fri_verify(&c.cfg, ch.get(), &v, ins.data(), ins.size());
}

void mutate_words(std::vector<uint32_t>& v) {
  if (v.empty()) return;
  const size_t at = rnd() % v.size();
  switch (rnd() % 4) {
    case 0: v[at] ^= 1u << (rnd() % 31); break;
    case 1: v[at] = (uint32_t)rnd(); break;          // often not canonical
    case 2: v.resize(rnd() % v.size()); break;       // shortened
    default: v[at] = 0x7F000001u; break;             // a modulus
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s proof.u32 n_mutants\n", argv[0]); return 2; }
  Words in;
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  uint32_t x;
  while (fread(&x, 4, 1, f) == 1) in.w.push_back(x);
  fclose(f);
  Case base;
  base.cfg.abi_version = P3R_ABI_VERSION;
  base.cfg.field = in.next();
  base.cfg.challenge_degree = in.next();
  base.cfg.ext_degree = 4;
  base.cfg.log_blowup = in.next();
  base.cfg.max_log_arity = in.next();
  base.cfg.cap_height = in.next();
  base.cfg.log_final_poly_len = in.next();
  base.cfg.commit_pow_bits = in.next();
  base.cfg.query_pow_bits = in.next();
  base.cfg.num_queries = in.next();
  base.cfg.mmcs_arity = in.next();
  base.cfg.mmcs_salt_elems = in.next();
  base.cfg.ext_choices = P3R_EXT_UNPINNED_W32_DEFAULTS;
  base.observed = in.vec();
  base.log_max = in.next();
  base.query_pow = in.next();
  for (uint32_t a : in.vec()) base.arities.push_back((uint8_t)a);
  base.caps = in.vec();
  base.pow = in.vec();
  base.final_poly = in.vec();
  base.n_queries = in.next();
  base.openings.resize(base.n_queries * base.arities.size());
  for (auto& o : base.openings) { o.row = in.vec(); o.salts = in.vec(); o.sibs = in.vec(); }
  base.inputs.resize(in.next());
  for (auto& i : base.inputs) { i.log_h = in.next(); i.values = in.vec(); }

  if (run(base) != P3R_OK) { fprintf(stderr, "the unmutated proof is not accepted: %s\n", g_create_error.c_str()); return 1; }
  const long n = atol(argv[2]);
  long count[3] = {0, 0, 0};
  for (long m = 0; m < n; ++m) {
    Case c = base;
    const int rounds = 1 + (int)(rnd() % 2);
    for (int r = 0; r < rounds; ++r) {
      switch (rnd() % 14) {
        case 0: mutate_words(c.caps); break;
        case 1: mutate_words(c.pow); break;
        case 2: mutate_words(c.final_poly); break;
        case 3: if (!c.openings.empty()) mutate_words(c.openings[rnd() % c.openings.size()].row); break;
        case 4: if (!c.openings.empty()) mutate_words(c.openings[rnd() % c.openings.size()].sibs); break;
        case 5: if (!c.openings.empty()) mutate_words(c.openings[rnd() % c.openings.size()].salts); break;
        case 6: if (!c.inputs.empty()) mutate_words(c.inputs[rnd() % c.inputs.size()].values); break;
        case 7: if (!c.arities.empty()) c.arities[rnd() % c.arities.size()] = (uint8_t)(rnd() % 40); break;
        case 8: if (rnd() & 1) c.arities.push_back((uint8_t)(1 + rnd() % 4)); else if (!c.arities.empty()) c.arities.pop_back(); break;
        case 9: c.n_queries = (rnd() & 1) ? c.n_queries + 1 + rnd() % 3 : (size_t)rnd(); break;                  // counts raised
        case 10: c.log_max = (rnd() & 1) ? c.log_max + 1 + (uint32_t)(rnd() % 40) : (uint32_t)(rnd() % 12); break;
        case 11: if (!c.inputs.empty()) c.inputs[rnd() % c.inputs.size()].log_h = (uint32_t)(rnd() % 40); break;
        case 12: if (!c.openings.empty()) c.openings.pop_back(); else c.inputs.clear(); break;
        default: {
          uint32_t* knobs[] = {&c.cfg.log_blowup, &c.cfg.max_log_arity, &c.cfg.cap_height, &c.cfg.log_final_poly_len, &c.cfg.commit_pow_bits,
                               &c.cfg.query_pow_bits, &c.cfg.num_queries, &c.cfg.mmcs_arity, &c.cfg.mmcs_salt_elems, &c.query_pow};
          *knobs[rnd() % 10] = (rnd() & 1) ? (uint32_t)(rnd() % 8) : (uint32_t)rnd();
        }
      }
    }
    const int rc = run(c);
    if (rc == P3R_OK) ++count[0];
    else if (rc == P3R_EINVAL || rc == P3R_EUNSUPPORTED) ++count[1];
    else if (rc == P3R_EVERIFY) ++count[2];
    else { fprintf(stderr, "mutant %ld: unexpected result %d (%s)\n", m, rc, g_create_error.c_str()); return 1; }
  }
  printf("mutants %ld accepted %ld refused %ld rejected %ld\n", n, count[0], count[1], count[2]);
  return 0;
}
