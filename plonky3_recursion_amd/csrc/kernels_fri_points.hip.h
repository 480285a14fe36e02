// FRI reduced openings at the public seam (p3r_fri_reduce_dmat, tu_fri.hip): any number of opening points per matrix and
// any power-of-two height, where the prover's k_fri_reduce_pre (kernels_fri_reduce.hip.h) carries exactly two point
// slots per matrix and its host side refuses LDEs of fewer than four rows.
//   inv_{z}[r] = 1 / (z - x_r),  x_r = shift * w_h^{bitrev(r)}                          (k_fri_inv_points, shared)
//   V_p = sum_c alpha^c value_{p,c}                                                       (k_fri_vsum, shared)
//   ro[r] = sum_m sum_{p of m} off_{m,p} * (V_{m,p} - S_m[r]) * inv_{z_{m,p}}[r],  S_m[r] = sum_c alpha^c M_m[c][r]
// S_m does not depend on the point: lane r forms it once per matrix and then walks that matrix's points, so a matrix
// element is read once per call however many points its matrix has.
//
// Heights below four.  k_fri_inv_points gives a lane the rows r0 .. r0 + 3 and their points x, -x, ix, -ix.  At h = 2 the
// rows are x_0 = shift and x_1 = shift * w_2 = -shift, at h = 1 the one row is x_0 = shift (bit_reverse(0, 0) = 0): the
// first h of the lane's four points are the right ones, the others are formed, inverted and never stored (the stores are
// guarded by r0 + m < h), and a zero among them - z = -shift is a legal point at h = 1 - takes inv4's separate-inversion
// path instead of poisoning the shared one.  So the kernel serves every height as it is; what refuses h < 4 in the
// prover is its host side.
#pragma once
#include "kernels_fri_reduce.hip.h"

namespace p3r {

// One (matrix, point) of the call.
template <int DC>
struct FriPointT {
  const uint32_t* inv;  // [DC][h]: the vector of this height and point
  const uint32_t* v;    // [DC]: the k_fri_vsum result of this matrix and point
  EW<DC> off;           // the running alpha power of the height when the walk reaches this (matrix, point)
};
// One matrix with at least one column and one point.
struct FriPointsMat {
  const uint32_t* mat;  // bit-reversed LDE [w][h]
  int w;
  uint32_t p0, n_points;  // range in the point list
};
// The heights are FriReduceJob's (kernels_fri_reduce.hip.h): lane r owns ro[r] and adds every term to it, so ro is
// written once and needs no zero fill.
template <class PP, int DC = 4>
__global__ void __launch_bounds__(kBlock)
k_fri_reduce_points(const FriReduceJob* __restrict__ jobs, int n_jobs, const FriPointsMat* __restrict__ mats,
                    const FriPointT<DC>* __restrict__ pts, const uint32_t* __restrict__ apow_tab /* alpha^c, DC words each */) {
  using F = Fp<PP>;
  using E = typename Chal<PP, DC>::type;
  const int j = find_job(jobs, n_jobs);
  const FriReduceJob job = jobs[j];
  const size_t h = job.h, r = (size_t)(blockIdx.x - job.block0) * kBlock + threadIdx.x;
  if (r >= h) return;
  auto apow = [&](int c) {
    E ap;
#pragma unroll
    for (int k = 0; k < DC; ++k) ap.c[k] = F::raw(apow_tab[DC * c + k]);
    return ap;
  };
  E acc = E::zero();
  for (uint32_t m = 0; m < job.n_mats; ++m) {
    const FriPointsMat a = mats[job.mat0 + m];
    const gptr<const uint32_t> mat = as_global(a.mat);
    const int w = a.w;
    E S = E::zero(), S2 = E::zero();
    int c = 0;
    // four column loads in flight, two columns per reduction, two accumulators (the shape k_fri_reduce_pre measured)
    for (; c + 3 < w; c += 4) {
      const F m0 = F::raw(mat[(size_t)c * h + r]), m1 = F::raw(mat[(size_t)(c + 1) * h + r]);
      const F m2 = F::raw(mat[(size_t)(c + 2) * h + r]), m3 = F::raw(mat[(size_t)(c + 3) * h + r]);
      S += E::dot2_base(apow(c), m0, apow(c + 1), m1);
      S2 += E::dot2_base(apow(c + 2), m2, apow(c + 3), m3);
    }
    for (; c + 1 < w; c += 2)
      S += E::dot2_base(apow(c), F::raw(mat[(size_t)c * h + r]), apow(c + 1), F::raw(mat[(size_t)(c + 1) * h + r]));
    if (c < w) S += apow(c) * F::raw(mat[(size_t)c * h + r]);
    S += S2;
    for (uint32_t p = 0; p < a.n_points; ++p) {
      const FriPointT<DC>& q = pts[a.p0 + p];
      E inv, V;
#pragma unroll
      for (int k = 0; k < DC; ++k) inv.c[k] = F::raw(as_global(q.inv)[(size_t)k * h + r]);
#pragma unroll
      for (int k = 0; k < DC; ++k) V.c[k] = F::raw(as_global(q.v)[k]);
      acc += e4_load<PP, DC>(q.off) * (V - S) * inv;
    }
  }
#pragma unroll
  for (int k = 0; k < DC; ++k) as_global(job.ro)[(size_t)k * h + r] = acc.c[k].v;
}

// The commit-phase leaf view of a folded vector (p3r_fri_leaf_view_dmat): the (rows) x (DC << LA) matrix whose row r is
// the flattened extension elements r << LA .. (r + 1) << LA of the n = rows << LA element vector - what
// ExtensionMmcs::commit_matrix commits in commit_phase, and what the prover's commit_phase_leaves hashes through a
// strided view.  A pure copy of Montgomery words, no arithmetic:
//   out[(j * DC + k) * rows + r] = in[k * n + (r << LA) + j],   j < 2^LA, k < DC.
// One lane owns row r of plane k = blockIdx.y.  It reads its 2^LA adjacent words as k_fri_fold does (16-byte loads, one
// 8-byte load at LA = 1; the alignment argument is at the launch) and stores one word into each of the 2^LA columns
// j * DC + k: in every one of those stores consecutive lanes write consecutive words.  No LDS.
template <int DC, int LA>
__global__ void __launch_bounds__(kBlock) k_fri_leaf_view(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, size_t rows) {
  static_assert(LA >= 1 && LA <= 4, "rows of 2, 4, 8 or 16 elements");
  constexpr int ARITY = 1 << LA;
  const size_t r = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const int k = (int)blockIdx.y;
  if (r >= rows) return;
  const size_t n_in = rows << LA;
  const gptr<const uint32_t> src = as_global(in) + (size_t)k * n_in + (r << LA);
  uint32_t e[ARITY];
  if constexpr (LA == 1) {
    const fri_u32x2 v = *(gptr<const fri_u32x2>)src;
    e[0] = v.x;
    e[1] = v.y;
  } else {
#pragma unroll
    for (int q = 0; q < ARITY / 4; ++q) {
      const fri_u32x4 v = ((gptr<const fri_u32x4>)src)[q];
      e[4 * q] = v.x;
      e[4 * q + 1] = v.y;
      e[4 * q + 2] = v.z;
      e[4 * q + 3] = v.w;
    }
  }
  const gptr<uint32_t> dst = as_global(out) + (size_t)k * rows + r;
#pragma unroll
  for (int j = 0; j < ARITY; ++j) dst[(size_t)j * DC * rows] = e[j];
}

}  // namespace p3r
