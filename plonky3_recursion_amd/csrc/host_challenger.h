// The pieces of the transcript a verifier shares with the prover, free of HIP so that host-only programs compile them
// with a plain C++ compiler: how a verifier refuses (vfail), the DuplexChallenger and the FRI folding schedule.
//
//   DuplexChallenger<F, Perm, 16, 8> + 0.6 prefix-free padding
//        recursion/src/challenger/circuit.rs:97-156 (duplexing), :337-364 (observe / sample),
//        :366-386 (extension elements), :388-430 (sample_bits, PoW check)
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "field.h"
#include "host_poseidon2_simd.h"

namespace p3r {

struct VerifyFailure : std::runtime_error {
  using std::runtime_error::runtime_error;
};
[[noreturn]] inline void vfail(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  throw VerifyFailure(buf);
}

template <class PP, int DC = 4>
struct HostChallenger {
  using F = Fp<PP>;
  using E = typename Chal<PP, DC>::type;   // the challenge field: DC sampled / observed coefficients per element
  const uint32_t* rc;  // Montgomery
  F state[P2_WIDTH];
  std::vector<F> in_buf, out_buf;
  explicit HostChallenger(const uint32_t* rc_) : rc(rc_) {
    for (auto& s : state) s = F::zero();
  }
  void duplexing() {
    size_t n = in_buf.size();
    for (size_t i = 0; i < n; ++i) state[i] = in_buf[i];
    in_buf.clear();
    if (n > 0) {
      for (size_t i = n; i < (size_t)P2_RATE; ++i) state[i] = F::zero();
      state[P2_RATE] += F::from_canonical((uint32_t)n);
    }
    host_permute<PP>(state, rc);
    out_buf.assign(state, state + P2_RATE);
  }
  void observe(F x) {
    out_buf.clear();
    in_buf.push_back(x);
    if (in_buf.size() == (size_t)P2_RATE) duplexing();
  }
  void observe_ext(const E& e) { for (int i = 0; i < DC; ++i) observe(e.c[i]); }
  void observe_base_as_ext(uint64_t v) { observe_ext(E::from_base(F::from_u64(v))); }
  void observe_digest_canonical(const uint32_t* d) { for (int i = 0; i < P2_DIGEST; ++i) observe(F::from_canonical(d[i])); }
  F sample() {
    if (!in_buf.empty() || out_buf.empty()) duplexing();
    F x = out_buf.back();
    out_buf.pop_back();
    return x;
  }
  E sample_ext() {
    E e;
    for (int i = 0; i < DC; ++i) e.c[i] = sample();
    return e;
  }
  uint32_t sample_bits(int bits) { return sample().to_canonical() & ((1u << bits) - 1); }
  bool check_witness(int bits, F w) {
    if (bits == 0) return true;
    observe(w);
    return sample_bits(bits) == 0;
  }
};

// FRI folding schedule: log2 arity of commit phase `phase` at height 2^log_cur.  Rule (no override):
// fold as far as max_log_arity allows without passing the next roll-in height or the final height.
// With an explicit schedule (p3r_config.fri_log_arities) the entry is used if it is legal; -1 otherwise.
inline int fri_log_arity(const std::vector<uint8_t>& schedule, size_t phase, int max_log_arity, int log_cur, int log_final,
                         int log_next_input) {
  int limit = log_cur - log_final;
  if (log_next_input >= 0 && log_next_input < log_cur) limit = std::min(limit, log_cur - log_next_input);
  if (schedule.empty()) return std::max(std::min(max_log_arity, limit), 1);
  if (phase >= schedule.size()) return -1;
  const int la = schedule[phase];
  return (la >= 1 && la <= limit && la <= max_log_arity) ? la : -1;
}

}  // namespace p3r
