// K9: every column of a matrix evaluated at extension-field points, by the barycentric formula over the coset s<w_n> with
// u = z / s:
//     f(z) = sum_j y_j L_j(u),   L_j(u) = w^j (u^n - 1) / (n (u - w^j)).
// One kernel family for its two callers (open_impl.hip.h plans both): the prover's Opener (trace-domain matrices in
// natural order, one or two points) and the public seam p3r_open_points (tu_open.hip: the low coset of a bit-reversed
// LDE or every 2^added_bits-th row of a natural-order matrix, any number of points).  All openings of one call run as
// three launches over job lists (a recursion layer opens ~20 matrices at 1-2 points each; per-matrix launches are
// latency-bound for 2^14..2^16-row layers): the weights (one vector per distinct (height, point)), the dot pass and the
// reduction of the row chunks.  Included by kernels_stark.hip.h after inv4, which k_fri_inv_points shares.
#pragma once
#include "kernels_stark.hip.h"

namespace p3r {

constexpr int kPtsMax = P3R_OPEN_POINTS_PER_PASS;    // points sharing one pass over the matrix
// matrix columns sharing one pass over the weights: eight for one or two points, four for three or four, so that the
// accumulators (P x columns x DC words per lane) never exceed 4 x 4 x 5 = 80 registers
constexpr int kPtsColsMax = 8;
constexpr int pts_cols(int P) { return P <= 2 ? 8 : 4; }
constexpr int kOpenRows = 8192;                      // rows per block for tall matrices (the host shrinks it for short ones)
constexpr int kOpenSums = 2 * pts_cols(2);           // partial sums of a block per coefficient: P x pts_cols(P) at its widest

// weights[r] = L_{e(r)}(u) for evaluation row r, e(r) = r (natural) or bitrev(r) (bit-reversed rows): stored under the
// ROW index, so that rows and their weights are both read contiguously.  A lane owns four consecutive rows:
// w^e(i0 + m) = w^e(i0) * tw[m] (i0 is a multiple of four, so the exponents add in both orders), and the four inversions
// share one base-field inversion (inv4).  `scale` = (u^n - 1) / n is the host's.
template <int DC>
struct OpenWeightJob {
  uint32_t* out;  // [DC][n]
  uint64_t n;
  uint32_t w_n;
  uint32_t tw[4];
  int log_n, bitrev;
  EW<DC> u, scale;
  uint32_t block0;  // first block of this job
};
template <class PP, int DC>
__global__ void __launch_bounds__(kBlock) k_bary_weights(const OpenWeightJob<DC>* __restrict__ jobs, int n_jobs) {
  using F = Fp<PP>;
  using E = typename Chal<PP, DC>::type;
  const int j = find_job(jobs, n_jobs);
  const OpenWeightJob<DC>& b = jobs[j];
  const size_t i0 = ((size_t)(blockIdx.x - b.block0) * kBlock + threadIdx.x) * 4;
  if (i0 >= b.n) return;
  const E u = e4_load<PP, DC>(b.u), scale = e4_load<PP, DC>(b.scale);
  const F base = F::raw(b.w_n).pow(b.bitrev ? bit_reverse((uint32_t)i0, b.log_n) : (uint32_t)i0);
  F wi[4];
  E x[4], inv[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) wi[m] = base * F::raw(b.tw[m]);
#pragma unroll
  for (int m = 0; m < 4; ++m) x[m] = u - E::from_base(wi[m]);   // never zero: a point in the coset is refused (the prover's are outside the base field)
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
// (the prover: n and 1; the seam: row_stride 1 for the first n rows of a bit-reversed LDE, 2^added_bits for every
// 2^added_bits-th row of a natural one).
struct OpenJob {
  const uint32_t* mat;
  const uint32_t* wt[kPtsMax];  // weights per point ([DC][n]); the first P are set
  uint32_t* partial;            // [P][n_chunks][w][DC]
  uint64_t n, col_stride, row_stride;
  uint64_t out0;                // first output word of this pass ([P][w][DC]) in the reduce launch
  int w, P, n_chunks, rows_per_block, col_groups;
  uint32_t block0;              // first block of this pass in the dot launch
};
// partial[p][chunk][col] = sum over the chunk's rows of weights_p[row] * M[col][row].  Accumulators (P x COLS x DC words)
// are indexed at compile time (register resident); the block reduction is a wave shuffle tree followed by a 4-wave LDS
// combine.  UNIT: the matrix is read as mat[c * n + r] - the prover's addressing (col_stride = n, row_stride = 1), known
// to the compiler so that its instance carries no stride arithmetic.
template <class PP, int P, int COLS, int DC, bool UNIT>
__device__ __forceinline__ void open_dot_block(const OpenJob& job, int col_group, int chunk, uint32_t (*sh)[kOpenSums * DC]) {
  using F = Fp<PP>;
  using E = typename Chal<PP, DC>::type;
  constexpr int NV = P * COLS * DC;
  static_assert(P * COLS <= kOpenSums && NV <= kBlock, "one lane per partial sum in the LDS combine");
  const gptr<const uint32_t> mat = as_global(job.mat);
  gptr<const uint32_t> wt[P];
#pragma unroll
  for (int p = 0; p < P; ++p) wt[p] = as_global(job.wt[p]);
  const size_t n = job.n, cs = UNIT ? n : job.col_stride, rs = UNIT ? 1 : job.row_stride;
  const int w = job.w, c0 = col_group * COLS;
  const size_t r0 = (size_t)chunk * job.rows_per_block, r1 = r0 + job.rows_per_block < n ? r0 + job.rows_per_block : n;
  E acc[P][COLS];
#pragma unroll
  for (int p = 0; p < P; ++p)
#pragma unroll
    for (int c = 0; c < COLS; ++c) acc[p][c] = E::zero();
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
    for (int c = 0; c < COLS; ++c) {
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
    for (int c = 0; c < COLS; ++c)
#pragma unroll
      for (int k = 0; k < DC; ++k) {
        F v = acc[p][c].c[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += F::raw(__shfl_down(v.v, off));
        if (lane == 0) sh[wave][(p * COLS + c) * DC + k] = v.v;
      }
  __syncthreads();
  if ((int)threadIdx.x < NV) {
    F s = F::zero();
#pragma unroll
    for (int wv = 0; wv < kBlock / 64; ++wv) s += F::raw(sh[wv][threadIdx.x]);
    const int p = threadIdx.x / (COLS * DC), rem = threadIdx.x % (COLS * DC), c = rem / DC, k = rem % DC;
    if (c0 + c < w) as_global(job.partial)[(((size_t)p * job.n_chunks + chunk) * w + c0 + c) * DC + k] = s.v;
  }
}
// Two entry points over that one body, and they stay two: all passes of a launch share the kernel's register footprint,
// so a single entry with the four-point switch would run the prover's one- and two-point passes at the seam's 152 (DC =
// 4) / 172 (DC = 5) VGPRs ("The cap is 4") instead of at their own.
// The prover's: one or two points, eight columns, unit strides.
template <class PP, int DC>
__global__ void __launch_bounds__(kBlock) k_open_dot(const OpenJob* __restrict__ jobs, int n_jobs) {
  __shared__ uint32_t sh[kBlock / 64][kOpenSums * DC];
  const int j = find_job(jobs, n_jobs);
  const OpenJob job = jobs[j];
  const int local = (int)(blockIdx.x - job.block0);
  const int col_group = local % job.col_groups, chunk = local / job.col_groups;
  if (job.P == 2) open_dot_block<PP, 2, pts_cols(2), DC, true>(job, col_group, chunk, sh);
  else open_dot_block<PP, 1, pts_cols(1), DC, true>(job, col_group, chunk, sh);
}
// The seam's: one to kPtsMax points, pts_cols(P) columns, the job's strides.
template <class PP, int DC>
__global__ void __launch_bounds__(kBlock) k_points_dot(const OpenJob* __restrict__ jobs, int n_jobs) {
  static_assert(kPtsMax == 4 && pts_cols(kPtsMax) * kPtsMax == pts_cols(2) * 2 && kPtsMax * pts_cols(kPtsMax) * 5 <= kBlock,
                "one lane per partial sum in the LDS combine; the widest combine is that of kPtsMax points");
  __shared__ uint32_t sh[kBlock / 64][kOpenSums * DC];
  const int j = find_job(jobs, n_jobs);
  const OpenJob job = jobs[j];
  const int local = (int)(blockIdx.x - job.block0);
  const int col_group = local % job.col_groups, chunk = local / job.col_groups;
  switch (job.P) {   // uniform over the workgroup
    case 1: open_dot_block<PP, 1, pts_cols(1), DC, false>(job, col_group, chunk, sh); break;
    case 2: open_dot_block<PP, 2, pts_cols(2), DC, false>(job, col_group, chunk, sh); break;
    case 3: open_dot_block<PP, 3, pts_cols(3), DC, false>(job, col_group, chunk, sh); break;
    default: open_dot_block<PP, 4, pts_cols(4), DC, false>(job, col_group, chunk, sh); break;
  }
}
// out[out0 + (p*w + c)*DC + k] = sum over chunks of partial[p][chunk][c][k]: Montgomery words for the prover (they feed
// values_dev and the reduced openings), CANONICAL ones for the seam (copied straight into the caller's buffer)
template <class PP, int DC, bool CANONICAL>
__global__ void __launch_bounds__(kBlock)
k_open_reduce(const OpenJob* __restrict__ jobs, int n_jobs, uint64_t total, uint32_t* __restrict__ out) {
  using F = Fp<PP>;
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= total) return;
  int j = 0, hi = n_jobs - 1;   // the last pass whose first output is not past t (bisection: field.h::find_job)
  while (j < hi) {
    const int mid = (j + hi + 1) >> 1;
    if (t >= jobs[mid].out0) j = mid; else hi = mid - 1;
  }
  const OpenJob& job = jobs[j];
  const uint64_t local = t - job.out0;
  const uint64_t per_point = (uint64_t)job.w * DC, p = local / per_point, rem = local % per_point;
  F s = F::zero();
  const gptr<const uint32_t> partial = as_global(job.partial);
  for (int ch = 0; ch < job.n_chunks; ++ch) s += F::raw(partial[((size_t)p * job.n_chunks + ch) * per_point + rem]);
  out[t] = CANONICAL ? s.to_canonical() : s.v;
}

}  // namespace p3r
