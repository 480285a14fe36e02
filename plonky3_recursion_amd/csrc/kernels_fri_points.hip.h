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

}  // namespace p3r
