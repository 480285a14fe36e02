// K9 sequencing (kernels_open.hip.h).  OpenPlan is the host planner of both callers: the weight cache (one vector per
// distinct (height, point)), the job lists of the passes and the three launches.  Opener is the prover's use of it: all
// openings of one proof, back on the host in ONE transfer; included into p3r_core.hip.  The public seam's is
// open_points (tu_open.hip).
//
// Opening points and their order: recursion/src/verifier/batch_stark.rs:645-852 (rounds),
// :1114-1276 (observation order).  Values are the unique interpolants, so any exact evaluation
// method matches upstream's `interpolate_coset`.
#pragma once
#include <array>
#include <map>
#include <optional>

#include "tu_api.h"
#include "profile.h"

namespace p3r {

template <class PP, int DC>
struct OpenPlan {
  using F = Fp<PP>;
  using E = typename Chal<PP, DC>::type;
  p3r_ctx* ctx;
  std::vector<DevBuf> keep;  // weights, partial sums and the uploaded job lists: alive until the caller has its values
  std::vector<OpenWeightJob<DC>> wjobs;
  std::vector<OpenJob> djobs;
  std::map<std::array<uint64_t, 6>, const uint32_t*> wcache;
  uint32_t wblocks = 0, dblocks = 0;
  uint64_t used = 0;  // output words so far

  explicit OpenPlan(p3r_ctx* c) : ctx(c) {}

  // L_e(r)(u) = w^e(r) (u^n - 1) / (n (u - w^e(r))) for the n = 2^log_n rows of an evaluation over u's coset of <w_n>,
  // e(r) = bitrev(r) for bit-reversed rows
  const uint32_t* weights(size_t n, int log_n, const E& u, bool bit_reversed) {
    std::array<uint64_t, 6> key{2 * n + bit_reversed, 0, 0, 0, 0, 0};
    for (int k = 0; k < DC; ++k) key[1 + k] = u.c[k].v;
    auto hit = wcache.find(key);
    if (hit != wcache.end()) return hit->second;
    keep.emplace_back((size_t)DC * n);
    OpenWeightJob<DC> b{};
    b.out = keep.back().p;
    b.n = n;
    const F w_n = F::two_adic_generator(log_n);
    b.w_n = w_n.v;
    for (uint32_t m = 0; m < 4; ++m) {
      const uint32_t row = (uint32_t)(m % n);   // rows past a height below four: any point of the coset (never stored)
      b.tw[m] = w_n.pow(bit_reversed ? bit_reverse(row, log_n) : row).v;
    }
    b.log_n = log_n;
    b.bitrev = bit_reversed ? 1 : 0;
    b.u = e4_store<PP, DC>(u);
    b.scale = e4_store<PP, DC>((u.pow(n) - E::one()) * F::from_u64(n).inv());
    b.block0 = wblocks;
    wblocks += (uint32_t)((((n + 3) / 4) + kBlock - 1) / kBlock);  // a lane owns four consecutive rows
    wjobs.push_back(b);
    return wcache.emplace(key, b.out).first->second;
  }

  // One pass over one matrix: its w columns (`cols` per workgroup) at the P points whose weight vectors are wt[0 .. P).
  // Returns the first word of the pass's values ([P][w][DC]) in the output of launch().
  uint64_t add_pass(const uint32_t* mat, size_t n, size_t col_stride, size_t row_stride, int w, const uint32_t* const* wt, int P,
                    int cols, size_t rows_floor) {
    OpenJob j{};
    j.mat = mat;
    for (int p = 0; p < P; ++p) j.wt[p] = wt[p];
    j.P = P;
    j.n = n;
    j.col_stride = col_stride;
    j.row_stride = row_stride;
    j.w = w;
    j.col_groups = (w + cols - 1) / cols;
    // rows per block: 8192 for tall matrices, fewer for short ones so that the pass still has ~1000 workgroups (a
    // 2^16-row table would otherwise occupy a third of the chip); at most 64 chunks, which the reduction walks serially;
    // not below the caller's floor
    size_t rows_per_block = kOpenRows;
    while (rows_per_block > rows_floor && (n + rows_per_block - 1) / rows_per_block < 64 &&
           j.col_groups * ((n + rows_per_block - 1) / rows_per_block) < 1024)
      rows_per_block /= 2;
    j.rows_per_block = (int)rows_per_block;
    j.n_chunks = (int)((n + rows_per_block - 1) / rows_per_block);
    keep.emplace_back((size_t)P * j.n_chunks * w * DC);
    j.partial = keep.back().p;
    j.block0 = dblocks;
    const uint64_t nb = (uint64_t)j.col_groups * j.n_chunks;
    if (dblocks + nb > 0x7fffffffu) fail(P3R_EINVAL, "too many matrices, columns and points for one call");
    dblocks += (uint32_t)nb;
    j.out0 = used;
    used += (uint64_t)P * w * DC;
    djobs.push_back(j);
    return j.out0;
  }

  // Three launches: the weights, the dot passes and the reduction of the row chunks into out[0 .. used).  The reduction
  // is timed with the dot passes when it has no name of its own.
  void launch(const char* weights_name, const char* dot_name, const char* reduce_name, void (*dot)(const OpenJob*, int),
              void (*reduce)(const OpenJob*, int, uint64_t, uint32_t*), uint32_t* out) {
    auto upload_jobs = [&](const auto& v) {
      using T = typename std::decay_t<decltype(v)>::value_type;
      keep.emplace_back((v.size() * sizeof(T) + 3) / 4);
      P3R_HIP(ctx->stage.upload(ctx->stream, keep.back().p, v.data(), v.size() * sizeof(T)));
      return reinterpret_cast<const T*>(keep.back().p);
    };
    const OpenWeightJob<DC>* d_w = upload_jobs(wjobs);
    const OpenJob* d_j = upload_jobs(djobs);
    std::optional<ProfScope> ps;
    ps.emplace(ctx, weights_name);
    hipLaunchKernelGGL((k_bary_weights<PP, DC>), dim3(wblocks), dim3(kBlock), 0, ctx->stream, d_w, (int)wjobs.size());
    ps.emplace(ctx, dot_name);
    hipLaunchKernelGGL(dot, dim3(dblocks), dim3(kBlock), 0, ctx->stream, d_j, (int)djobs.size());
    if (reduce_name) ps.emplace(ctx, reduce_name);
    hipLaunchKernelGGL(reduce, dim3((unsigned)((used + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, d_j, (int)djobs.size(),
                       used, out);
    ps.reset();
    P3R_HIP(hipGetLastError());
  }
};

// The prover's openings.
template <class PP, int DC = 4>
struct Opener {
  using F = Fp<PP>;
  using E = typename Chal<PP, DC>::type;
  p3r_ctx* ctx;
  OpenPlan<PP, DC> plan;
  struct Job { size_t off; int P, w; };  // off: the job's first value in `out`, in extension-field elements
  std::vector<Job> jobs;
  DevBuf out;  // the opened values on the device: [job][point][col][DC]

  explicit Opener(p3r_ctx* c) : ctx(c), plan(c) {}

  // `mat`: n x w evaluations over dshift*<w_n> (natural order), at one or two points.  Returns a job id; nothing is
  // launched before finish().
  size_t open(const uint32_t* mat, size_t n, int w, F dshift, const std::vector<E>& points) {
    const int P = (int)points.size(), log_n = log2_exact(n, "trace height");
    const F inv_shift = dshift.inv();
    const uint32_t* wt[2];
    for (int p = 0; p < P; ++p) wt[p] = plan.weights(n, log_n, points[p] * inv_shift, false);
    const uint64_t out0 = plan.add_pass(mat, n, n, 1, w, wt, P, pts_cols(P), 2 * kBlock);
    jobs.push_back({(size_t)(out0 / DC), P, w});
    return jobs.size() - 1;
  }

  // device address of the opened values of one job and point ([w][DC]), valid after finish()
  const uint32_t* values_dev(size_t job, int point) const {
    return out.p + (jobs[job].off + (size_t)point * jobs[job].w) * DC;
  }

  // values[job][point][col]
  std::vector<std::vector<std::vector<E>>> finish() {
    if (jobs.empty()) return {};
    const size_t words = (size_t)plan.used;
    out.alloc(words);
    plan.launch("open_weights", "open_dot", nullptr, k_open_dot<PP, DC>, k_open_reduce<PP, DC, false>, out.p);
    // the opened values (4 800 words for a recursion layer) travel like a commitment root: posted by a one-workgroup
    // kernel and polled for - the copy engine's round trip is 30 - 40 us longer (profiles/r06/host_gaps.txt); read in
    // place, before the next post
    const uint32_t* raw = nullptr;
    if (words <= HostPost::kWords) P3R_HIP(ctx->post.post(ctx->stream, out.p, words, &raw));
    else P3R_HIP(ctx->landing.fetch(ctx->stream, out.p, words * 4, &raw));
    plan.keep.clear();  // `out` stays for the reduced openings (values_dev)
    std::vector<std::vector<std::vector<E>>> res(jobs.size());
    for (size_t j = 0; j < jobs.size(); ++j) {
      res[j].resize(jobs[j].P);
      for (int p = 0; p < jobs[j].P; ++p) {
        res[j][p].resize(jobs[j].w);
        for (int c = 0; c < jobs[j].w; ++c)
          for (int k = 0; k < DC; ++k)
            res[j][p][c].c[k] = F::raw(raw[(jobs[j].off + (size_t)p * jobs[j].w + c) * DC + k]);
      }
    }
    return res;
  }
};

}  // namespace p3r
