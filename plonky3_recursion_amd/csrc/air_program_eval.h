// The verifier's side of a constraint program (p3r_air_program_eval; include/p3r.h): VerifierConstraintFolder for the
// p3r_air_insn programs p3r_quotient_program_dmat takes, at one out-of-domain point, from opened values.  Host only, no HIP
// and no context, next to air_program.h, whose air_plan validates the program.  Every value is held as a challenge-field
// element and all of them are kept: there is no slot file here, so no P3R_AIR_MAX_LIVE.
#pragma once
#include "air_program.h"

namespace p3r {

// local / next: sum(widths) x DC canonical words, the opened values at zeta and zeta * w_h, matrices in order.
template <class PP, int DC>
void air_program_eval(const p3r_air_insn* prog, size_t n, const size_t* widths, size_t n_mats, const uint32_t* local, const uint32_t* next,
                      uint32_t log_height, const uint32_t* zeta_w, const uint32_t* publics, size_t n_public, const uint32_t* challenges,
                      size_t n_challenges, const uint32_t* alpha_w, uint32_t* folded_out, uint32_t* inv_zh_out) {
  using F = Fp<PP>;
  using E = typename Chal<PP, DC>::type;
  // ---- everything that is refused, before anything is evaluated
  (void)air_plan(prog, n, widths, n_mats, DC, PP::P, n_public, n_challenges, 0xffffffffu);
  if (!zeta_w || !alpha_w || !folded_out || !inv_zh_out) fail(P3R_EINVAL, "NULL argument");
  if (log_height > (uint32_t)PP::TWO_ADICITY) fail(P3R_EINVAL, "2^%u rows exceed the field's two-adicity (%d)", log_height, PP::TWO_ADICITY);
  if (n_public && !publics) fail(P3R_EINVAL, "public_values is NULL");
  if (n_challenges && !challenges) fail(P3R_EINVAL, "challenges is NULL");
  size_t total_w = 0;
  std::vector<size_t> col0(n_mats + 1, 0);
  for (size_t m = 0; m < n_mats; ++m) {
    if (widths[m] > (size_t(1) << 24)) fail(P3R_EINVAL, "matrix %zu: width %zu is too large", m, widths[m]);
    total_w += widths[m];
    col0[m + 1] = total_w;
  }
  if (total_w && (!local || !next)) fail(P3R_EINVAL, "the opened values are NULL");
  auto canonical = [](const uint32_t* w, size_t count, const char* what) {
    for (size_t i = 0; i < count; ++i)
      if (w[i] >= PP::P) fail(P3R_EINVAL, "non-canonical word %zu of %s", i, what);
  };
  canonical(zeta_w, DC, "zeta");
  canonical(alpha_w, DC, "alpha");
  canonical(publics, n_public, "the public values");
  canonical(challenges, n_challenges * DC, "the challenges");
  canonical(local, total_w * DC, "the opened values at zeta");
  canonical(next, total_w * DC, "the opened values at zeta * w_h");
  auto ext = [](const uint32_t* w) {
    E e;
    for (int k = 0; k < DC; ++k) e.c[k] = F::from_canonical(w[k]);
    return e;
  };
  const E zeta = ext(zeta_w), alpha = ext(alpha_w);
  // the selectors at zeta (p3r.h): division by zero is refused, no wrong value is returned
  const E zh = zeta.pow(uint64_t(1) << log_height) - E::one();
  const E z_m1 = zeta - E::one(), z_mg = zeta - E::from_base(F::two_adic_generator((int)log_height).inv());
  if (z_m1.is_zero()) fail(P3R_EINVAL, "zeta == 1: is_first_row divides by zero there");
  if (z_mg.is_zero()) fail(P3R_EINVAL, "zeta == w_h^-1: is_last_row divides by zero there");
  if (zh.is_zero()) fail(P3R_EINVAL, "zeta lies in the trace domain (zeta^h == 1): the vanishing polynomial is zero there");
  const E is_first = zh * z_m1.inv(), is_last = zh * z_mg.inv();

  std::vector<E> v(n, E::zero());
  E acc = E::zero();
  auto cell_ext = [&](const uint32_t* rows, size_t col) {   // sum_k X^k * opened[col + k]: a product in the challenge field
    E out = E::zero();
    for (int k = 0; k < DC; ++k) {
      E basis = E::zero();
      basis.c[k] = F::one();
      out += basis * ext(rows + (col + k) * DC);
    }
    return out;
  };
  for (size_t i = 0; i < n; ++i) {
    const p3r_air_insn& in = prog[i];
    switch (in.op) {
      case P3R_AIR_CONST: v[i] = E::from_base(F::from_canonical(in.a)); break;
      case P3R_AIR_PUBLIC: v[i] = E::from_base(F::from_canonical(publics[in.a])); break;
      case P3R_AIR_CHALLENGE: v[i] = ext(challenges + (size_t)in.a * DC); break;
      case P3R_AIR_LOCAL: v[i] = ext(local + (col0[in.a] + in.b) * DC); break;
      case P3R_AIR_NEXT: v[i] = ext(next + (col0[in.a] + in.b) * DC); break;
      case P3R_AIR_LOCAL_EXT: v[i] = cell_ext(local, col0[in.a] + in.b); break;
      case P3R_AIR_NEXT_EXT: v[i] = cell_ext(next, col0[in.a] + in.b); break;
      case P3R_AIR_IS_FIRST_ROW: v[i] = is_first; break;
      case P3R_AIR_IS_LAST_ROW: v[i] = is_last; break;
      case P3R_AIR_IS_TRANSITION: v[i] = z_mg; break;
      case P3R_AIR_ADD: v[i] = v[in.a] + v[in.b]; break;
      case P3R_AIR_SUB: v[i] = v[in.a] - v[in.b]; break;
      case P3R_AIR_MUL: v[i] = v[in.a] * v[in.b]; break;
      case P3R_AIR_NEG: v[i] = E::zero() - v[in.a]; break;
      case P3R_AIR_ASSERT_ZERO: acc = acc * alpha + v[in.a]; break;   // Horner in program order
    }
  }
  const E inv_zh = zh.inv();
  for (int k = 0; k < DC; ++k) {
    folded_out[k] = acc.c[k].to_canonical();
    inv_zh_out[k] = inv_zh.c[k].to_canonical();
  }
}

}  // namespace p3r
