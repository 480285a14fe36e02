// The value half of TwoAdicFriPcs::open at the public seam (p3r_open_points / p3r_open_points_dmat): every column of a
// committed matrix evaluated at any number of extension-field points, straight from the low coset of its bit-reversed
// LDE (or from a natural-order matrix).  Own translation unit (tu_api.h): the prover's Opener (open_impl.hip.h, K9) takes
// trace-domain matrices in natural order and at most two points, and stays as it is.
//
// The value is the unique interpolant's (upstream: interpolate_coset, fri/src/two_adic_pcs.rs `open`), by the barycentric
// formula over the coset s<w_h>, with u = z / s:
//     f(z) = sum_j y_j L_j(u),   L_j(u) = w^j (u^h - 1) / (h (u - w^j)).
// Three launches per call, whatever the number of matrices: the weights (one vector per distinct (height, point), stored
// under the ROW index of the evaluation, so that bit-reversed rows and their weights are both read contiguously), the
// dot pass (a matrix element is read once for up to P3R_OPEN_POINTS_PER_PASS points) and the reduction of the row
// chunks, which also leaves Montgomery form.
#include <array>
#include <map>

#include "tu_api.h"
#include "profile.h"

namespace p3r {

// matrix columns sharing one pass over the weights: eight for one or two points (the prover's k_open_dot), four for three
// or four, so that the accumulators (P x columns x DC words per lane) never exceed 4 x 4 x 5 = 80 registers
constexpr int kPtsColsMax = 8;
constexpr int pts_cols(int P) { return P <= 2 ? 8 : 4; }
constexpr int kPtsMax = P3R_OPEN_POINTS_PER_PASS;    // points sharing one pass over the matrix
constexpr int kPtsRows = 8192;                       // rows per block for tall matrices (the host shrinks it for short ones)

// weights[r] = L_{e(r)}(u) for evaluation row r, e(r) = r (natural) or bitrev(r) (bit-reversed rows).  A lane owns four
// consecutive rows: w^e(i0 + m) = w^e(i0) * tw[m] (i0 is a multiple of four, so the exponents add in both orders), and
// the four inversions share one base-field inversion (inv4).  `scale` = (u^h - 1) / h is the host's.
template <int DC>
struct PtWeightJob {
  uint32_t* out;  // [DC][n]
  uint64_t n;
  uint32_t w_n;
  uint32_t tw[4];
  int log_n, bitrev;
  EW<DC> u, scale;
  uint32_t block0;
};
template <class PP, int DC>
__global__ void __launch_bounds__(kBlock) k_point_weights(const PtWeightJob<DC>* __restrict__ jobs, int n_jobs) {
  using F = Fp<PP>;
  using E = typename Chal<PP, DC>::type;
  const int j = find_job(jobs, n_jobs);
  const PtWeightJob<DC>& b = jobs[j];
  const size_t i0 = ((size_t)(blockIdx.x - b.block0) * kBlock + threadIdx.x) * 4;
  if (i0 >= b.n) return;
  const E u = e4_load<PP, DC>(b.u), scale = e4_load<PP, DC>(b.scale);
  const F base = F::raw(b.w_n).pow(b.bitrev ? bit_reverse((uint32_t)i0, b.log_n) : (uint32_t)i0);
  F wi[4];
  E x[4], inv[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) wi[m] = base * F::raw(b.tw[m]);
#pragma unroll
  for (int m = 0; m < 4; ++m) x[m] = u - E::from_base(wi[m]);   // never zero: the host refuses points in the coset
  inv4<PP>(x, inv);
  const gptr<uint32_t> out = as_global(b.out);
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    if (i0 + m < b.n) {
      const E r = inv[m] * scale * wi[m];
#pragma unroll
      for (int k = 0; k < DC; ++k) out[(size_t)k * b.n + i0 + m] = r.c[k].v;
    }
  }
}

// One pass of one matrix: P <= kPtsMax points.  Evaluation row r of column c is mat[c * col_stride + r * row_stride]
// (row_stride 1: the first n rows of a bit-reversed LDE; 2^added_bits: every 2^added_bits-th row of a natural one).
struct PtDotJob {
  const uint32_t* mat;
  const uint32_t* wt[kPtsMax];  // weights per point ([DC][n]); the first P are set
  uint32_t* partial;            // [P][n_chunks][w][DC]
  uint64_t n, col_stride, row_stride;
  uint64_t out0;                // first output word of this pass ([P][w][DC]) in the reduce launch
  int w, P, n_chunks, rows_per_block, col_groups;
  uint32_t block0;              // first block of this pass in the dot launch
};
// COPIES: pts_dot_block / k_points_dot / k_points_reduce follow open_dot_block / k_open_dot / k_open_reduce of
// kernels_stark.hip.h (the prover's K9, which must not change) line for line; k_point_weights follows k_bary_weights.
// What differs: the row and column strides, the wt[] array of up to kPtsMax weight vectors, the P-dependent column
// group, 64-bit output offsets and the canonical store of the reduce.  A fix to one of the pair belongs in both.
// partial[p][chunk][col] = sum over the chunk's rows of weights_p[row] * M[col][row].  Accumulators (P x pts_cols(P) x DC
// words) are indexed at compile time; the block reduction is a wave shuffle tree followed by a 4-wave LDS combine, as in
// k_open_dot.
template <class PP, int P, int DC>
__device__ __forceinline__ void pts_dot_block(const PtDotJob& job, int col_group, int chunk,
                                              uint32_t (*sh)[kPtsMax * pts_cols(kPtsMax) * DC]) {
  using F = Fp<PP>;
  using E = typename Chal<PP, DC>::type;
  constexpr int kPtsCols = pts_cols(P);
  constexpr int NV = P * kPtsCols * DC;
  const gptr<const uint32_t> mat = as_global(job.mat);
  gptr<const uint32_t> wt[P];
#pragma unroll
  for (int p = 0; p < P; ++p) wt[p] = as_global(job.wt[p]);
  const size_t n = job.n, cs = job.col_stride, rs = job.row_stride;
  const int w = job.w, c0 = col_group * kPtsCols;
  const size_t r0 = (size_t)chunk * job.rows_per_block, r1 = r0 + job.rows_per_block < n ? r0 + job.rows_per_block : n;
  E acc[P][kPtsCols];
#pragma unroll
  for (int p = 0; p < P; ++p)
#pragma unroll
    for (int c = 0; c < kPtsCols; ++c) acc[p][c] = E::zero();
  // two rows per step: their products share one reduction per coefficient
  for (size_t r = r0 + threadIdx.x; r < r1; r += 2 * kBlock) {
    const size_t rb = r + kBlock;
    const bool has_b = rb < r1;
    E wa[P], wb[P];
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
      for (int k = 0; k < DC; ++k) {
        wa[p].c[k] = F::raw(wt[p][(size_t)k * n + r]);
        wb[p].c[k] = has_b ? F::raw(wt[p][(size_t)k * n + rb]) : F::zero();
      }
#pragma unroll
    for (int c = 0; c < kPtsCols; ++c) {
      const bool col = c0 + c < w;
      const F ma = col ? F::raw(mat[(size_t)(c0 + c) * cs + r * rs]) : F::zero();
      const F mb = col && has_b ? F::raw(mat[(size_t)(c0 + c) * cs + rb * rs]) : F::zero();
#pragma unroll
      for (int p = 0; p < P; ++p) acc[p][c] += E::dot2_base(wa[p], ma, wb[p], mb);
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int p = 0; p < P; ++p)
#pragma unroll
    for (int c = 0; c < kPtsCols; ++c)
#pragma unroll
      for (int k = 0; k < DC; ++k) {
        F v = acc[p][c].c[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += F::raw(__shfl_down(v.v, off));
        if (lane == 0) sh[wave][(p * kPtsCols + c) * DC + k] = v.v;
      }
  __syncthreads();
  if ((int)threadIdx.x < NV) {
    F s = F::zero();
#pragma unroll
    for (int wv = 0; wv < kBlock / 64; ++wv) s += F::raw(sh[wv][threadIdx.x]);
    const int p = threadIdx.x / (kPtsCols * DC), rem = threadIdx.x % (kPtsCols * DC), c = rem / DC, k = rem % DC;
    if (c0 + c < w) as_global(job.partial)[(((size_t)p * job.n_chunks + chunk) * w + c0 + c) * DC + k] = s.v;
  }
}
template <class PP, int DC>
__global__ void __launch_bounds__(kBlock) k_points_dot(const PtDotJob* __restrict__ jobs, int n_jobs) {
  static_assert(kPtsMax == 4 && pts_cols(kPtsMax) * kPtsMax == pts_cols(2) * 2 && kPtsMax * pts_cols(kPtsMax) * 5 <= kBlock,
                "one lane per partial sum in the LDS combine; the widest combine is that of kPtsMax points");
  __shared__ uint32_t sh[kBlock / 64][kPtsMax * pts_cols(kPtsMax) * DC];
  const int j = find_job(jobs, n_jobs);
  const PtDotJob job = jobs[j];
  const int local = (int)(blockIdx.x - job.block0);
  const int col_group = local % job.col_groups, chunk = local / job.col_groups;
  switch (job.P) {   // uniform over the workgroup
    case 1: pts_dot_block<PP, 1, DC>(job, col_group, chunk, sh); break;
    case 2: pts_dot_block<PP, 2, DC>(job, col_group, chunk, sh); break;
    case 3: pts_dot_block<PP, 3, DC>(job, col_group, chunk, sh); break;
    default: pts_dot_block<PP, 4, DC>(job, col_group, chunk, sh); break;
  }
}
// out[out0 + (p*w + c)*DC + k] = sum over chunks of partial[p][chunk][c][k], canonical
template <class PP, int DC>
__global__ void __launch_bounds__(kBlock)
k_points_reduce(const PtDotJob* __restrict__ jobs, int n_jobs, uint64_t total, uint32_t* __restrict__ out) {
  using F = Fp<PP>;
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= total) return;
  int j = 0, hi = n_jobs - 1;   // the last pass whose first output is not past t
  while (j < hi) {
    const int mid = (j + hi + 1) >> 1;
    if (t >= jobs[mid].out0) j = mid; else hi = mid - 1;
  }
  const PtDotJob& job = jobs[j];
  const uint64_t local = t - job.out0;
  const uint64_t per_point = (uint64_t)job.w * DC, p = local / per_point, rem = local % per_point;
  F s = F::zero();
  const gptr<const uint32_t> partial = as_global(job.partial);
  for (int ch = 0; ch < job.n_chunks; ++ch) s += F::raw(partial[((size_t)p * job.n_chunks + ch) * per_point + rem]);
  out[t] = s.to_canonical();
}

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

  // ---- the job lists
  std::vector<DevBuf> keep;   // weights and partial sums
  std::vector<PtWeightJob<DC>> wjobs;
  std::vector<PtDotJob> djobs;
  std::map<std::array<uint64_t, 6>, const uint32_t*> wcache;
  uint32_t wblocks = 0, dblocks = 0;
  uint64_t used = 0;   // output words so far
  auto weights = [&](const Plan& pl, const E& u) -> const uint32_t* {
    std::array<uint64_t, 6> key{pl.n, 0, 0, 0, 0, 0};
    for (int k = 0; k < DC; ++k) key[1 + k] = u.c[k].v;
    auto hit = wcache.find(key);
    if (hit != wcache.end()) return hit->second;
    keep.emplace_back((size_t)DC * pl.n);
    PtWeightJob<DC> b{};
    b.out = keep.back().p;
    b.n = pl.n;
    const F w_n = F::two_adic_generator(pl.log_n);
    b.w_n = w_n.v;
    for (uint32_t m = 0; m < 4; ++m) {
      const uint32_t row = (uint32_t)(m % pl.n);   // rows past a height below four: any point of the coset (never stored)
      b.tw[m] = w_n.pow(bit_reversed ? bit_reverse(row, pl.log_n) : row).v;
    }
    b.log_n = pl.log_n;
    b.bitrev = bit_reversed ? 1 : 0;
    b.u = e4_store<PP, DC>(u);
    b.scale = e4_store<PP, DC>((u.pow(pl.n) - E::one()) * F::from_u64(pl.n).inv());
    b.block0 = wblocks;
    wblocks += (uint32_t)((((pl.n + 3) / 4) + kBlock - 1) / kBlock);
    wjobs.push_back(b);
    return wcache.emplace(key, b.out).first->second;
  };
  for (size_t i = 0; i < items.size(); ++i) {
    const OpenPointsItem& it = items[i];
    const Plan& pl = plans[i];
    if (it.w == 0) continue;   // contributes nothing
    if (it.w > (size_t)INT32_MAX / (kPtsMax * kPtsColsMax)) fail(P3R_EINVAL, "matrix %zu: width %zu is too large", i, it.w);
    for (size_t q0 = it.p0; q0 < it.p1; q0 += kPtsMax) {
      PtDotJob j{};
      j.P = (int)std::min<size_t>(kPtsMax, it.p1 - q0);
      for (int p = 0; p < j.P; ++p) j.wt[p] = weights(pl, us[q0 + p - first]);
      j.mat = it.d;
      j.n = pl.n;
      j.col_stride = it.h;
      j.row_stride = bit_reversed ? 1 : (uint64_t(1) << added_bits);
      j.w = (int)it.w;
      j.col_groups = (j.w + pts_cols(j.P) - 1) / pts_cols(j.P);
      // rows per block: 8192 for tall matrices, fewer for short ones so that the pass still has ~1000 workgroups; not
      // below one row per lane
      size_t rows_per_block = kPtsRows;
      while (rows_per_block > (size_t)kBlock && (pl.n + rows_per_block - 1) / rows_per_block < 64 &&
             j.col_groups * ((pl.n + rows_per_block - 1) / rows_per_block) < 1024)
        rows_per_block /= 2;
      j.rows_per_block = (int)rows_per_block;
      j.n_chunks = (int)((pl.n + rows_per_block - 1) / rows_per_block);
      keep.emplace_back((size_t)j.P * j.n_chunks * it.w * DC);
      j.partial = keep.back().p;
      j.block0 = dblocks;
      const uint64_t nb = (uint64_t)j.col_groups * j.n_chunks;
      if (dblocks + nb > 0x7fffffffu) fail(P3R_EINVAL, "too many matrices, columns and points for one call");
      dblocks += (uint32_t)nb;
      j.out0 = used;
      used += (uint64_t)j.P * it.w * DC;
      djobs.push_back(j);
    }
  }
  if (djobs.empty()) return;
  if (used > (uint64_t)0x7fffffffu * kBlock) fail(P3R_EINVAL, "too many opened values for one call");

  // ---- three launches and one wait
  auto upload_jobs = [&](const void* data, size_t bytes) -> const void* {
    keep.emplace_back((bytes + 3) / 4);
    P3R_HIP(ctx->stage.upload(ctx->stream, keep.back().p, data, bytes));
    return keep.back().p;
  };
  DevBuf out((size_t)used);
  const auto* d_w = static_cast<const PtWeightJob<DC>*>(upload_jobs(wjobs.data(), wjobs.size() * sizeof(PtWeightJob<DC>)));
  const auto* d_j = static_cast<const PtDotJob*>(upload_jobs(djobs.data(), djobs.size() * sizeof(PtDotJob)));
  {
    ProfScope ps(ctx, "open_points_weights");
    hipLaunchKernelGGL((k_point_weights<PP, DC>), dim3(wblocks), dim3(kBlock), 0, ctx->stream, d_w, (int)wjobs.size());
  }
  {
    ProfScope ps(ctx, "open_points_dot");
    hipLaunchKernelGGL((k_points_dot<PP, DC>), dim3(dblocks), dim3(kBlock), 0, ctx->stream, d_j, (int)djobs.size());
  }
  {
    ProfScope ps(ctx, "open_points_reduce");
    hipLaunchKernelGGL((k_points_reduce<PP, DC>), dim3((unsigned)((used + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, d_j,
                       (int)djobs.size(), used, out.p);
  }
  P3R_HIP(hipGetLastError());
  P3R_HIP(copy_sync(ctx->stream, values_out, out.p, (size_t)used * 4, hipMemcpyDeviceToHost));
}

}  // namespace

template <class PP>
void open_points(p3r_ctx* ctx, const std::vector<OpenPointsItem>& items, int added_bits, uint32_t shift, bool bit_reversed,
                 const uint32_t* points, uint32_t* values_out) {
  if (ctx->cfg.challenge_degree == 5) {
    if constexpr (kHasQuintic<PP>) open_points_dc<PP, 5>(ctx, items, added_bits, shift, bit_reversed, points, values_out);
    else fail(P3R_EUNSUPPORTED, "UnsupportedChallengeDegree: the quintic challenge field is KoalaBear's");
    return;
  }
  open_points_dc<PP, 4>(ctx, items, added_bits, shift, bit_reversed, points, values_out);
}

template void open_points<KoalaBearParams>(p3r_ctx*, const std::vector<OpenPointsItem>&, int, uint32_t, bool, const uint32_t*, uint32_t*);
template void open_points<BabyBearParams>(p3r_ctx*, const std::vector<OpenPointsItem>&, int, uint32_t, bool, const uint32_t*, uint32_t*);

}  // namespace p3r
