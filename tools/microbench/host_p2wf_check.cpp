// Host check of the width-32 FP64 Poseidon2 permutation (csrc/poseidon2_w32_f64.hip.h: p2wf_permute) against the integer
// Montgomery one (csrc/poseidon2.h: p2w_permute_traced with a null sink): random and edge-value states, both fields, every
// CARRIED mask the kernels use, the built-in diagonal's compile-time forms (BUILTIN) and the general path with the built-in
// diagonal as data, a random diagonal and three adversarial ones (every entry (P-1)/2, every entry (P+1)/2, alternating
// 1 / P-1).  Sibling of host_p2f_check.cpp: the FP64 path is exact integer (and dyadic) arithmetic, so IEEE doubles on
// the host compute the same values as gfx950 does; fused multiply-adds are the ones the header writes, nothing else may be
// contracted.  The header's static_asserts (p2wf_partial_walk, p2wf_general_check) are compiled on the way.
//   g++ -O2 -std=c++17 -ffp-contract=off -I plonky3_recursion_amd/csrc tools/microbench/host_p2wf_check.cpp -o /tmp/hp2wf
//   /tmp/hp2wf [random states per field, mask and diagonal, default 8192]
// Prints one line per field, mask and diagonal; exit code 0 = no mismatching state.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "poseidon2_w32_f64.hip.h"
using namespace p3r;

enum Diag : int { BUILTIN, GENERAL_BUILTIN, GENERAL_RANDOM, GENERAL_HALF_LO, GENERAL_HALF_HI, GENERAL_PLUS_MINUS_ONE, N_DIAG };
static const char* const kDiagName[N_DIAG] = {"builtin", "general(builtin)", "general(random)", "general((P-1)/2)",
                                              "general((P+1)/2)", "general(1,P-1)"};

template <class PP, unsigned CARRIED>
long run(const char* name, int diag, long n_random) {
  using F = Fp<PP>;
  constexpr int64_t P = PP::P;
  std::mt19937_64 g(PP::FIELD_ID * 1000003ull + CARRIED * 7ull + (unsigned)diag);
  const int nrc = p2w_num_rc<PP>();
  std::vector<uint32_t> rcw(p2w_num_constants<PP>());   // Montgomery, as the context keeps them: constants | diagonal
  std::vector<double> tab(rcw.size());                  // canonical doubles | centred diagonal, as p3r_ctx::rcd_w32
  for (int i = 0; i < nrc; ++i) {
    rcw[i] = (uint32_t)(g() % PP::P);
    tab[i] = (double)F::raw(rcw[i]).to_canonical();
  }
  const uint32_t* builtin = PP::FIELD_ID == 0 ? kDefaultDiagW32_koala_bear : kDefaultDiagW32_baby_bear;
  for (int i = 0; i < P2W_WIDTH; ++i) {
    uint32_t d;
    switch (diag) {
      case BUILTIN: case GENERAL_BUILTIN: d = builtin[i]; break;
      case GENERAL_RANDOM: d = (uint32_t)(g() % PP::P); break;
      case GENERAL_HALF_LO: d = (PP::P - 1) / 2; break;
      case GENERAL_HALF_HI: d = (PP::P + 1) / 2; break;
      default: d = i & 1 ? PP::P - 1 : 1u; break;
    }
    rcw[nrc + i] = F::from_canonical(d).v;
    tab[nrc + i] = d > PP::P / 2 ? (double)d - (double)PP::P : (double)d;
  }
  // the inputs a kernel hands over: fresh lanes are integers in [0, P] (p2f_load), carried lanes are the unreduced
  // outputs of a previous permutation, |x| <= p2wf_out_bound
  const int64_t C = (int64_t)p2wf_out_bound<PP>();
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
    int64_t v[P2W_WIDTH];
    for (int i = 0; i < P2W_WIDTH; ++i) {
      if (t < n_edge) v[i] = edge((int)t, i);
      else if (CARRIED >> i & 1u) v[i] = (int64_t)(g() % (uint64_t)(2 * C + 1)) - C;
      else v[i] = (int64_t)(g() % (uint64_t)(P + 1));
    }
    F a[P2W_WIDTH];
    double s[P2W_WIDTH];
    for (int i = 0; i < P2W_WIDTH; ++i) {
      a[i] = F::from_canonical((uint32_t)(((v[i] % P) + P) % P));
      s[i] = (double)v[i];
    }
    P2NullSink sink;
    p2w_permute_traced<PP>(a, rcw.data(), sink);
    if (diag == BUILTIN) p2wf_permute<PP, true, CARRIED>(s, tab.data());
    else p2wf_permute<PP, false, CARRIED>(s, tab.data());
    for (int i = 0; i < P2W_WIDTH; ++i) {
      const double lim = (double)C;
      if (!(s[i] <= lim && s[i] >= -lim) || p2f_store<PP>(s[i]) != a[i].v) {
        if (bad < 4) printf("  %s carried=0x%08x %s state %ld lane %d: fp64 %.1f -> %08x, integer %08x\n", name, CARRIED,
                            kDiagName[diag], t, i, s[i], p2f_store<PP>(s[i]), a[i].v);
        ++bad;
        break;
      }
    }
  }
  printf("%s carried=0x%08x %s: mismatches %ld of %ld\n", name, CARRIED, kDiagName[diag], bad, n_edge + n_random);
  return bad;
}

template <class PP>
long field(const char* name, long n) {
  long bad = 0;
  for (int d = 0; d < N_DIAG; ++d)
    bad += run<PP, 0x00000000u>(name, d, n) + run<PP, 0x000000FFu>(name, d, n) + run<PP, 0xFF000000u>(name, d, n) +
           run<PP, 0xFFFFFFFFu>(name, d, n);
  return bad;
}

int main(int argc, char** argv) {
  const long n = argc > 1 ? atol(argv[1]) : 8192;
  const long bad = field<KoalaBearParams>("koala-bear", n) + field<BabyBearParams>("baby-bear", n);
  return bad ? 1 : 0;
}
