// The value half of TwoAdicFriPcs::open at the public seam (p3r_open_points / p3r_open_points_dmat): every column of a
// committed matrix evaluated at any number of extension-field points, straight from the low coset of its bit-reversed
// LDE (or from a natural-order matrix).  Own translation unit (tu_api.h).  The kernels (K9, kernels_open.hip.h) and the
// host planner (OpenPlan, open_impl.hip.h) are the ones the prover's Opener uses; what is the seam's own is below: what
// is refused, the split of a matrix's points into passes of at most P3R_OPEN_POINTS_PER_PASS, the strides of the two row
// orders, and canonical values copied into the caller's buffer.
//
// The value is the unique interpolant's (upstream: interpolate_coset, fri/src/two_adic_pcs.rs `open`), by the barycentric
// formula over the coset s<w_h>, with u = z / s:
//     f(z) = sum_j y_j L_j(u),   L_j(u) = w^j (u^h - 1) / (h (u - w^j)).
// Three launches per call, whatever the number of matrices: the weights (one vector per distinct (height, point), stored
// under the ROW index of the evaluation, so that bit-reversed rows and their weights are both read contiguously), the
// dot pass (a matrix element is read once for up to P3R_OPEN_POINTS_PER_PASS points) and the reduction of the row
// chunks, which also leaves Montgomery form.
#include "open_impl.hip.h"

namespace p3r {

namespace {

template <class PP, int DC>
void open_points_dc(p3r_ctx* ctx, const std::vector<OpenPointsItem>& items, int added_bits, uint32_t shift_word, bool bit_reversed,
                    const uint32_t* points, uint32_t* values_out) {
  using F = Fp<PP>;
  using E = typename Chal<PP, DC>::type;
  // ---- everything that is refused, before anything is allocated or launched
  if (added_bits < 0 || added_bits > PP::TWO_ADICITY) fail(P3R_EINVAL, "added_bits (%d) out of range", added_bits);
  if (shift_word >= PP::P) fail(P3R_EINVAL, "coset shift must be a canonical element (0: the field's generator)");
  const F shift = shift_word ? F::from_canonical(shift_word) : F::generator();
  const F inv_shift = shift.inv();
  struct Plan { size_t n; int log_n; };
  std::vector<Plan> plans(items.size());
  std::vector<E> us;   // u = z / shift per point of the call, in the order of `points`
  size_t first = items.empty() ? 0 : items[0].p0, last = first;
  for (size_t i = 0; i < items.size(); ++i) {
    const OpenPointsItem& it = items[i];
    const int log_h = log2_exact(it.h, "matrix height");
    if (log_h < added_bits) fail(P3R_EINVAL, "matrix %zu: height %zu is smaller than 2^added_bits (%d)", i, it.h, added_bits);
    const int log_n = log_h - added_bits;
    if (log_n > PP::TWO_ADICITY) fail(P3R_EINVAL, "matrix %zu: 2^%d evaluations exceed the field's two-adicity (%d)", i, log_n, PP::TWO_ADICITY);
    if (it.p0 != last || it.p1 < it.p0) fail(P3R_EINVAL, "point_offsets must be monotone (matrix %zu: %zu .. %zu after %zu)", i, it.p0, it.p1, last);
    last = it.p1;
    plans[i] = {size_t(1) << log_n, log_n};
  }
  if (last > first && (!points || !values_out)) fail(P3R_EINVAL, "NULL argument");
  for (size_t q = first * DC; q < last * DC; ++q)
    if (points[q] >= PP::P) fail(P3R_EINVAL, "non-canonical word %zu of point %zu", q % DC, q / DC);
  us.resize(last - first);
  for (size_t q = first; q < last; ++q) {
    E z;
    for (int k = 0; k < DC; ++k) z.c[k] = F::from_canonical(points[q * DC + k]);
    us[q - first] = z * inv_shift;
  }
  for (size_t i = 0; i < items.size(); ++i)
    for (size_t q = items[i].p0; q < items[i].p1; ++q)
      // z^h == shift^h: the interpolant's formula divides by zero there (upstream's interpolate_coset does too)
      if (us[q - first].pow(plans[i].n) == E::one())
        fail(P3R_EINVAL, "matrix %zu: point %zu lies in the evaluation coset (z^%zu == shift^%zu)", i, q - items[i].p0, plans[i].n, plans[i].n);

  // ---- the passes: a matrix element is read once for up to kPtsMax points
  OpenPlan<PP, DC> plan(ctx);
  for (size_t i = 0; i < items.size(); ++i) {
    const OpenPointsItem& it = items[i];
    const Plan& pl = plans[i];
    if (it.w == 0) continue;   // contributes nothing
    if (it.w > (size_t)INT32_MAX / (kPtsMax * kPtsColsMax)) fail(P3R_EINVAL, "matrix %zu: width %zu is too large", i, it.w);
    for (size_t q0 = it.p0; q0 < it.p1; q0 += kPtsMax) {
      const int P = (int)std::min<size_t>(kPtsMax, it.p1 - q0);
      const uint32_t* wt[kPtsMax];
      for (int p = 0; p < P; ++p) wt[p] = plan.weights(pl.n, pl.log_n, us[q0 + p - first], bit_reversed);
      plan.add_pass(it.d, pl.n, it.h, bit_reversed ? 1 : (size_t(1) << added_bits), (int)it.w, wt, P, pts_cols(P), kBlock);
    }
  }
  if (plan.djobs.empty()) return;
  if (plan.used > (uint64_t)0x7fffffffu * kBlock) fail(P3R_EINVAL, "too many opened values for one call");

  // ---- three launches and one wait
  DevBuf out((size_t)plan.used);
  plan.launch("open_points_weights", "open_points_dot", "open_points_reduce", k_points_dot<PP, DC>, k_open_reduce<PP, DC, true>, out.p);
  P3R_HIP(copy_sync(ctx->stream, values_out, out.p, (size_t)plan.used * 4, hipMemcpyDeviceToHost));
}

}  // namespace

template <class PP>
void open_points(p3r_ctx* ctx, const std::vector<OpenPointsItem>& items, int added_bits, uint32_t shift, bool bit_reversed,
                 const uint32_t* points, uint32_t* values_out) {
  with_challenge_degree<PP>(ctx, [&](auto dc) { open_points_dc<PP, decltype(dc)::value>(ctx, items, added_bits, shift, bit_reversed, points, values_out); });
}

template void open_points<KoalaBearParams>(p3r_ctx*, const std::vector<OpenPointsItem>&, int, uint32_t, bool, const uint32_t*, uint32_t*);
template void open_points<BabyBearParams>(p3r_ctx*, const std::vector<OpenPointsItem>&, int, uint32_t, bool, const uint32_t*, uint32_t*);

}  // namespace p3r
