// Host check of the FP64 Poseidon2 permutation (csrc/poseidon2_f64.hip.h: p2f_permute) against the integer Montgomery
// one (csrc/poseidon2.h: p2_permute): random and edge-value states, both fields, every CARRIED mask the kernels use.
// The FP64 path is exact integer (and dyadic) arithmetic, so IEEE doubles on the host compute the same values as
// gfx950 does; fused multiply-adds are the ones the header writes, nothing else may be contracted.
//   g++ -O2 -std=c++17 -ffp-contract=off -I plonky3_recursion_amd/csrc tools/microbench/host_p2f_check.cpp -o /tmp/hp2f
//   /tmp/hp2f [random states per field and mask, default 131072]
// Prints one line per field and mask; exit code 0 = no mismatching state.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "poseidon2_f64.hip.h"
using namespace p3r;

template <class PP, unsigned CARRIED>
long run(const char* name, long n_random) {
  using F = Fp<PP>;
  constexpr int64_t P = PP::P;
  std::mt19937_64 g(PP::FIELD_ID * 1000 + CARRIED);
  std::vector<uint32_t> rc(p2_num_constants<PP>());
  std::vector<double> rcd(rc.size());
  for (size_t i = 0; i < rc.size(); ++i) {
    rc[i] = (uint32_t)(g() % PP::P);                      // Montgomery, as the context keeps them
    rcd[i] = (double)F::raw(rc[i]).to_canonical();         // canonical doubles, as p3r_ctx::rc_f64
  }
  // the inputs a kernel hands over: fresh lanes are integers in [0, P] (p2f_load), carried lanes are the unreduced
  // outputs of a previous permutation, |x| < 2^36
  const int64_t C = (int64_t(1) << 36) - 1;
  auto edge = [&](int t, int i) -> int64_t {
    const bool carried = CARRIED >> i & 1u;
    switch (t) {
      case 0: return 0;
      case 1: return P - 1;
      case 2: return P;
      case 3: return carried ? C : P - 1;
      case 4: return carried ? -C : 0;
      case 5: return carried ? (i & 1 ? C : -C) : (i & 1 ? P : 0);
      default: return carried ? -C : P;
    }
  };
  const long n_edge = 7;
  long bad = 0;
  for (long t = 0; t < n_edge + n_random; ++t) {
    int64_t v[P2_WIDTH];
    for (int i = 0; i < P2_WIDTH; ++i) {
      if (t < n_edge) v[i] = edge((int)t, i);
      else if (CARRIED >> i & 1u) v[i] = (int64_t)(g() % (uint64_t)(2 * C + 1)) - C;
      else v[i] = (int64_t)(g() % (uint64_t)(P + 1));
    }
    F a[P2_WIDTH];
    double s[P2_WIDTH];
    for (int i = 0; i < P2_WIDTH; ++i) {
      a[i] = F::from_canonical((uint32_t)(((v[i] % P) + P) % P));
      s[i] = (double)v[i];
    }
    p2_permute<PP>(a, rc.data());
    p2f_permute<PP, CARRIED>(s, rcd.data());
    for (int i = 0; i < P2_WIDTH; ++i)
      if (p2f_store<PP>(s[i]) != a[i].v) {
        if (bad < 4) printf("  %s carried=0x%04x state %ld lane %d: fp64 %08x, integer %08x\n", name, CARRIED, t, i,
                            p2f_store<PP>(s[i]), a[i].v);
        ++bad;
        break;
      }
  }
  printf("%s carried=0x%04x: mismatches %ld of %ld\n", name, CARRIED, bad, n_edge + n_random);
  return bad;
}

template <class PP>
long field(const char* name, long n) {
  return run<PP, 0x0000u>(name, n) + run<PP, 0x00FFu>(name, n) + run<PP, 0xFF00u>(name, n) + run<PP, 0xFFFFu>(name, n);
}

int main(int argc, char** argv) {
  const long n = argc > 1 ? atol(argv[1]) : 131072;
  const long bad = field<KoalaBearParams>("koala-bear", n) + field<BabyBearParams>("baby-bear", n);
  return bad ? 1 : 0;
}
