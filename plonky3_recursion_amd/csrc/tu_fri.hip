// The two deterministic steps of the FRI half of TwoAdicFriPcs::open at the public seam (p3r_fri_reduce_dmat,
// p3r_fri_fold_dmat): the per-height reduced openings of committed LDEs, and FriFoldingStrategy::fold_matrix with the
// roll-in of the next height.  Own translation unit (tu_api.h).  No transcript, no randomness, no proof bytes: alpha and
// beta are the caller's challenger's.
//
// Reduce: three launches per call, whatever the number of matrices, heights and points - the inverse vectors (one per
// distinct (height, point), k_fri_inv_points), the column sums of the opened values (k_fri_vsum) and the pass
// (k_fri_reduce_points, kernels_fri_points.hip.h), which reads every matrix element once.  The walk - matrices in call
// order, a matrix's points in order, one running alpha power per height - is TwoAdicFriPcs::open's and
// prove_impl.hip.h::fri_reduce's.
// Fold: one launch of k_fri_fold (kernels_stark.hip.h), the kernel of the prover's commit phase.
// Leaf view (p3r_fri_leaf_view_dmat): one launch of k_fri_leaf_view (kernels_fri_points.hip.h), a copy of the folded
// vector into the matrix ExtensionMmcs commits in a commit phase, so that the public MMCS calls serve it as they are.
#include <algorithm>
#include <array>
#include <map>

#include "kernels_fri_points.hip.h"
#include "profile.h"
#include "tu_api.h"

namespace p3r {

namespace {

inline unsigned fri_blocks_for(size_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

template <class PP, int DC>
std::vector<std::unique_ptr<p3r_dmat>> fri_reduce_dc(p3r_ctx* ctx, const std::vector<FriReduceItem>& items, uint32_t shift_word,
                                                     const uint32_t* points, const uint32_t* values, const uint32_t* alpha_words) {
  using F = Fp<PP>;
  using E = typename Chal<PP, DC>::type;
  // ---- everything that is refused, before anything is allocated or launched
  if (items.empty()) fail(P3R_EINVAL, "n_mats == 0: no matrix to reduce");
  if (!alpha_words) fail(P3R_EINVAL, "alpha is NULL");
  if (shift_word >= PP::P) fail(P3R_EINVAL, "coset shift must be a canonical element (0: the field's generator)");
  const F shift = shift_word ? F::from_canonical(shift_word) : F::generator();
  for (int k = 0; k < DC; ++k)
    if (alpha_words[k] >= PP::P) fail(P3R_EINVAL, "non-canonical word %d of alpha", k);
  std::vector<int> log_h(items.size());
  size_t last = items[0].p0, n_values = 0, max_w = 1;
  const size_t first = last;
  for (size_t i = 0; i < items.size(); ++i) {
    const FriReduceItem& it = items[i];
    log_h[i] = log2_exact(it.h, "matrix height");
    if (log_h[i] > PP::TWO_ADICITY) fail(P3R_EINVAL, "matrix %zu: 2^%d rows exceed the field's two-adicity (%d)", i, log_h[i], PP::TWO_ADICITY);
    if (it.p0 != last || it.p1 < it.p0) fail(P3R_EINVAL, "point_offsets must be monotone (matrix %zu: %zu .. %zu after %zu)", i, it.p0, it.p1, last);
    last = it.p1;
    if (it.w > (size_t)INT32_MAX / DC) fail(P3R_EINVAL, "matrix %zu: width %zu is too large", i, it.w);
    n_values += (it.p1 - it.p0) * it.w;
    max_w = std::max(max_w, it.w);
  }
  if (last > first && !points) fail(P3R_EINVAL, "points is NULL");
  if (n_values && !values) fail(P3R_EINVAL, "values is NULL while a matrix has both points and columns");
  for (size_t q = first * DC; q < last * DC; ++q)
    if (points[q] >= PP::P) fail(P3R_EINVAL, "non-canonical word %zu of point %zu", q % DC, q / DC);
  for (size_t q = 0; q < n_values * DC; ++q)
    if (values[q] >= PP::P) fail(P3R_EINVAL, "non-canonical word %zu of the opened values", q);
  if (last - first > 0x7fffffffu) fail(P3R_EINVAL, "too many points for one call");
  std::vector<E> zs(last - first);
  for (size_t q = first; q < last; ++q)
    for (int k = 0; k < DC; ++k) zs[q - first].c[k] = F::from_canonical(points[q * DC + k]);
  for (size_t i = 0; i < items.size(); ++i) {
    const E sh = E::from_base(shift.pow(items[i].h));
    for (size_t q = items[i].p0; q < items[i].p1; ++q)
      // z^H == shift^H: z is a row's point and the quotient divides by zero there (as p3r_open_points refuses it)
      if (zs[q - first].pow(items[i].h) == sh)
        fail(P3R_EINVAL, "matrix %zu: point %zu lies in the evaluation coset (z^%zu == shift^%zu)", i, q - items[i].p0, items[i].h, items[i].h);
  }
  uint64_t blocks64 = 0, inv_blocks64 = 0;
  for (size_t i = 0; i < items.size(); ++i) {   // an upper bound of both grids: every matrix its own height, every point its own vector
    blocks64 += fri_blocks_for(items[i].h);
    inv_blocks64 += (uint64_t)(items[i].p1 - items[i].p0) * fri_blocks_for((items[i].h + 3) / 4);
  }
  if (blocks64 > 0x7fffffffu || inv_blocks64 > 0x7fffffffu) fail(P3R_EINVAL, "too many rows and points for one call");

  // ---- the walk: one running alpha power per height, one inverse vector per distinct (height, point)
  E alpha;
  for (int k = 0; k < DC; ++k) alpha.c[k] = F::from_canonical(alpha_words[k]);
  std::vector<E> apow(max_w + 1);
  apow[0] = E::one();
  for (size_t c = 1; c <= max_w; ++c) apow[c] = apow[c - 1] * alpha;
  struct Height { E a = E::one(); std::vector<FriPointsMat> mats; };
  std::map<int, Height, std::greater<int>> heights;   // tallest first
  std::vector<DevBuf> keep;                            // inverse vectors and the uploads: alive until everything is enqueued
  std::map<std::array<uint64_t, 6>, const uint32_t*> inv_cache;
  std::vector<FriInvJobT<DC>> inv_jobs;
  std::vector<FriPointT<DC>> pts;
  std::vector<FriVsumJob> vsum_jobs;
  std::vector<uint32_t> vals_mont(n_values * DC);
  for (size_t q = 0; q < vals_mont.size(); ++q) vals_mont[q] = F::from_canonical(values[q]).v;
  if (last == first) return {};   // no matrix has a point: no height has a vector
  size_t n_terms = 0;
  for (const FriReduceItem& it : items)
    if (it.w) n_terms += it.p1 - it.p0;
  DevBuf d_vals(vals_mont.size()), d_vsums(n_terms * DC);
  uint32_t inv_blocks = 0;
  size_t val0 = 0;
  for (size_t i = 0; i < items.size(); ++i) {
    const FriReduceItem& it = items[i];
    const size_t np = it.p1 - it.p0;
    if (np == 0) continue;   // adds nothing and does not advance the running power
    Height& H = heights[log_h[i]];
    if (it.w == 0) continue;   // its height has a vector (all zero if nothing else is added); alpha^0 = 1 leaves the power as it is
    FriPointsMat a{};
    a.mat = it.d;
    a.w = (int)it.w;
    a.p0 = (uint32_t)pts.size();
    a.n_points = (uint32_t)np;
    for (size_t p = 0; p < np; ++p) {
      const E& z = zs[it.p0 + p - first];
      std::array<uint64_t, 6> key{(uint64_t)log_h[i], 0, 0, 0, 0, 0};
      for (int k = 0; k < DC; ++k) key[1 + k] = z.c[k].v;
      auto hit = inv_cache.find(key);
      if (hit == inv_cache.end()) {
        keep.emplace_back((size_t)DC * it.h);
        FriInvJobT<DC> j{};
        j.inv = keep.back().p;
        j.h = it.h;
        j.log_h = log_h[i];
        j.w_h = F::two_adic_generator(log_h[i]).v;
        j.w_4 = F::two_adic_generator(2).v;
        j.z = e4_store<PP, DC>(z);
        j.block0 = inv_blocks;
        inv_blocks += fri_blocks_for((it.h + 3) / 4);   // a lane owns four consecutive rows
        inv_jobs.push_back(j);
        hit = inv_cache.emplace(key, j.inv).first;
      }
      FriPointT<DC> q{};
      q.inv = hit->second;
      q.v = d_vsums.p + DC * vsum_jobs.size();
      q.off = e4_store<PP, DC>(H.a);
      vsum_jobs.push_back({d_vals.p + (val0 + p * it.w) * DC, d_vsums.p + DC * vsum_jobs.size(), (int)it.w});
      pts.push_back(q);
      H.a *= apow[it.w];
    }
    val0 += np * it.w;
    H.mats.push_back(a);
  }
  std::vector<std::unique_ptr<p3r_dmat>> outs;
  std::vector<FriPointsMat> mats;
  std::vector<FriReduceJob> jobs;
  uint32_t blocks = 0;
  for (auto& kv : heights) {
    outs.push_back(dmat_alloc(size_t(1) << kv.first, DC));   // [DC][h]: column k is coefficient k
    FriReduceJob j{};
    j.ro = outs.back()->d;
    j.h = uint64_t(1) << kv.first;
    j.mat0 = (uint32_t)mats.size();
    j.n_mats = (uint32_t)kv.second.mats.size();
    j.block0 = blocks;
    blocks += fri_blocks_for(size_t(1) << kv.first);
    jobs.push_back(j);
    mats.insert(mats.end(), kv.second.mats.begin(), kv.second.mats.end());
  }

  // ---- uploads through the staging ring, three launches
  auto upload = [&](const auto& v) {
    using T = typename std::decay_t<decltype(v)>::value_type;
    keep.emplace_back((v.size() * sizeof(T) + 3) / 4);
    P3R_HIP(ctx->stage.upload(ctx->stream, keep.back().p, v.data(), v.size() * sizeof(T)));
    return reinterpret_cast<const T*>(keep.back().p);
  };
  std::vector<uint32_t> apow_words(max_w * DC);
  for (size_t c = 0; c < max_w; ++c)
    for (int k = 0; k < DC; ++k) apow_words[c * DC + k] = apow[c].c[k].v;
  P3R_HIP(ctx->stage.upload(ctx->stream, d_vals.p, vals_mont.data(), vals_mont.size() * 4));
  const uint32_t* d_apow = upload(apow_words);
  const auto* d_inv = upload(inv_jobs);
  const auto* d_vsum = upload(vsum_jobs);
  const auto* d_pts = upload(pts);
  const auto* d_mats = upload(mats);
  const auto* d_jobs = upload(jobs);
  if (!inv_jobs.empty()) {
    ProfScope ps(ctx, "fri_seam_inv_points");
    hipLaunchKernelGGL((k_fri_inv_points<PP, DC>), dim3(inv_blocks), dim3(kBlock), 0, ctx->stream, d_inv, (int)inv_jobs.size(), shift.v);
  }
  {
    ProfScope ps(ctx, "fri_seam_reduce");
    if (!vsum_jobs.empty())
      hipLaunchKernelGGL((k_fri_vsum<PP, DC>), dim3((unsigned)vsum_jobs.size()), dim3(kBlock), 0, ctx->stream, d_vsum, d_apow);
    hipLaunchKernelGGL((k_fri_reduce_points<PP, DC>), dim3(blocks), dim3(kBlock), 0, ctx->stream, d_jobs, (int)jobs.size(), d_mats,
                       d_pts, d_apow);
  }
  P3R_HIP(hipGetLastError());
  // everything is enqueued on the context's stream, like the results' later readers; the buffers of `keep` go back to
  // the context's pool, which is ordered by that stream (context.h)
  return outs;
}

template <class PP, int DC>
std::unique_ptr<p3r_dmat> fri_fold_dc(p3r_ctx* ctx, const p3r_dmat* in, uint32_t la, const uint32_t* beta_words, const p3r_dmat* roll_in) {
  using F = Fp<PP>;
  // ---- everything that is refused, before anything is allocated or launched
  if (la == 0) fail(P3R_EINVAL, "log_arity must be at least 1");
  if (la > 4) fail(P3R_EUNSUPPORTED, "log_arity > 4 is not supported");
  const int log_n = log2_exact(in->h, "height of the vector to fold");
  if (log_n > PP::TWO_ADICITY) fail(P3R_EINVAL, "2^%d rows exceed the field's two-adicity (%d)", log_n, PP::TWO_ADICITY);
  if ((uint32_t)log_n < la) fail(P3R_EINVAL, "a vector of %zu rows cannot be folded by %u", in->h, 1u << la);
  if (in->w != (size_t)DC) fail(P3R_EINVAL, "the vector to fold must be %d words wide (it is %zu)", DC, in->w);
  const size_t rows = in->h >> la;
  if (roll_in && roll_in->w != (size_t)DC) fail(P3R_EINVAL, "roll_in must be %d words wide (it is %zu)", DC, roll_in->w);
  if (roll_in && roll_in->h != rows) fail(P3R_EINVAL, "roll_in has %zu rows, the folded vector %zu", roll_in->h, rows);
  uint32_t bw[DC];
  for (int k = 0; k < DC; ++k) {
    if (beta_words[k] >= PP::P) fail(P3R_EINVAL, "non-canonical word %d of beta", k);
    bw[k] = F::from_canonical(beta_words[k]).v;
  }

  auto out = dmat_alloc(rows, DC);
  DevBuf d_beta(DC);
  P3R_HIP(ctx->stage.upload(ctx->stream, d_beta.p, bw, sizeof bw));
  // k_fri_fold reads a lane's 2^la siblings of one plane with 16-byte loads (one 8-byte load at la = 1) at
  // in + k * n + (r << la) words.  For a caller's p3r_dmat that address is aligned: every handle owns a pool allocation
  // (p3r_dmat::d is DevBuf::p, from hipMalloc at a multiple of 256 bytes - there are no borrowed views behind the
  // ABI), a plane is n = 2^L >= 2^la words, so k * n and r << la are both multiples of 2^la words: of 16 bytes for
  // la >= 2 and of 8 bytes for la = 1.  The last lane's load ends at the plane's end, never past the allocation.
  FriFoldArgs fa{};
  fa.in = in->d; fa.out = out->d; fa.rows = rows; fa.log_rows = log_n - (int)la;
  fa.beta = d_beta.p;
  fa.roll = roll_in ? roll_in->d : nullptr;
  fa.w_inv = F::two_adic_generator(log_n).inv().v;
  const F omega = F::two_adic_generator((int)la);
  for (int s = 0; s < (int)la; ++s) {
    const F om_s = omega.pow(uint64_t(1) << s);
    for (int j = 0; j < (int)((size_t(1) << la) >> (s + 1)); ++j) fa.tw_inv[s][j] = om_s.pow(bit_reverse(2 * j, (int)la - s)).inv().v;
  }
  fa.neg_half = (-(F::from_canonical(2).inv())).v;
  {
    ProfScope ps(ctx, "fri_seam_fold");
    static constexpr void (*kFold[4])(FriFoldArgs) = {k_fri_fold<PP, DC, 1>, k_fri_fold<PP, DC, 2>, k_fri_fold<PP, DC, 3>,
                                                      k_fri_fold<PP, DC, 4>};
    hipLaunchKernelGGL(kFold[la - 1], dim3(fri_blocks_for(rows)), dim3(kBlock), 0, ctx->stream, fa);
  }
  P3R_HIP(hipGetLastError());
  return out;
}

template <class PP, int DC>
std::unique_ptr<p3r_dmat> fri_leaf_view_dc(p3r_ctx* ctx, const p3r_dmat* vec, uint32_t la) {
  // ---- everything that is refused, before anything is allocated or launched (the refusals of fri_fold_dc)
  if (la == 0) fail(P3R_EINVAL, "log_arity must be at least 1");
  if (la > 4) fail(P3R_EUNSUPPORTED, "log_arity > 4 is not supported");
  const int log_n = log2_exact(vec->h, "height of the folded vector");
  if (log_n > PP::TWO_ADICITY) fail(P3R_EINVAL, "2^%d rows exceed the field's two-adicity (%d)", log_n, PP::TWO_ADICITY);
  if ((uint32_t)log_n < la) fail(P3R_EINVAL, "a vector of %zu rows has no rows of %u elements", vec->h, 1u << la);
  if (vec->w != (size_t)DC) fail(P3R_EINVAL, "the folded vector must be %d words wide (it is %zu)", DC, vec->w);
  const size_t rows = vec->h >> la;

  auto out = dmat_alloc(rows, (size_t)DC << la);
  // k_fri_leaf_view reads a lane's 2^la adjacent words of one plane with 16-byte loads (one 8-byte load at la = 1) at
  // vec + k * n + (r << la) words.  For a caller's p3r_dmat that address is aligned: every handle owns a pool allocation
  // (p3r_dmat::d is DevBuf::p, from hipMalloc at a multiple of 256 bytes - there are no borrowed views behind the
  // ABI), a plane is n = 2^L >= 2^la words, so k * n and r << la are both multiples of 2^la words: of 16 bytes for
  // la >= 2 and of 8 bytes for la = 1.  The last lane's load ends at the plane's end, never past the allocation; its
  // last store is word (2^la * DC - 1) * rows + rows - 1, the last of the rows x (DC << la) result.
  {
    ProfScope ps(ctx, "fri_seam_leaf_view");
    static constexpr void (*kView[4])(const uint32_t*, uint32_t*, size_t) = {k_fri_leaf_view<DC, 1>, k_fri_leaf_view<DC, 2>,
                                                                             k_fri_leaf_view<DC, 3>, k_fri_leaf_view<DC, 4>};
    hipLaunchKernelGGL(kView[la - 1], dim3(fri_blocks_for(rows), DC), dim3(kBlock), 0, ctx->stream, vec->d, out->d, rows);
  }
  P3R_HIP(hipGetLastError());
  return out;
}

}  // namespace

template <class PP>
std::vector<std::unique_ptr<p3r_dmat>> fri_reduce(p3r_ctx* ctx, const std::vector<FriReduceItem>& items, uint32_t shift,
                                                  const uint32_t* points, const uint32_t* values, const uint32_t* alpha) {
  return with_challenge_degree<PP>(ctx, [&](auto dc) { return fri_reduce_dc<PP, decltype(dc)::value>(ctx, items, shift, points, values, alpha); });
}
template <class PP>
std::unique_ptr<p3r_dmat> fri_fold(p3r_ctx* ctx, const p3r_dmat* in, uint32_t log_arity, const uint32_t* beta, const p3r_dmat* roll_in) {
  return with_challenge_degree<PP>(ctx, [&](auto dc) { return fri_fold_dc<PP, decltype(dc)::value>(ctx, in, log_arity, beta, roll_in); });
}

template <class PP>
std::unique_ptr<p3r_dmat> fri_leaf_view(p3r_ctx* ctx, const p3r_dmat* vec, uint32_t log_arity) {
  return with_challenge_degree<PP>(ctx, [&](auto dc) { return fri_leaf_view_dc<PP, decltype(dc)::value>(ctx, vec, log_arity); });
}

template std::vector<std::unique_ptr<p3r_dmat>> fri_reduce<KoalaBearParams>(p3r_ctx*, const std::vector<FriReduceItem>&, uint32_t,
                                                                            const uint32_t*, const uint32_t*, const uint32_t*);
template std::vector<std::unique_ptr<p3r_dmat>> fri_reduce<BabyBearParams>(p3r_ctx*, const std::vector<FriReduceItem>&, uint32_t,
                                                                           const uint32_t*, const uint32_t*, const uint32_t*);
template std::unique_ptr<p3r_dmat> fri_fold<KoalaBearParams>(p3r_ctx*, const p3r_dmat*, uint32_t, const uint32_t*, const p3r_dmat*);
template std::unique_ptr<p3r_dmat> fri_fold<BabyBearParams>(p3r_ctx*, const p3r_dmat*, uint32_t, const uint32_t*, const p3r_dmat*);
template std::unique_ptr<p3r_dmat> fri_leaf_view<KoalaBearParams>(p3r_ctx*, const p3r_dmat*, uint32_t);
template std::unique_ptr<p3r_dmat> fri_leaf_view<BabyBearParams>(p3r_ctx*, const p3r_dmat*, uint32_t);

}  // namespace p3r
