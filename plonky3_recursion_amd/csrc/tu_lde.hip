// K5: NTT tables, the passes of kernels_ntt.hip.h / kernels_ntt2.hip.h, the coset LDE of a batch of matrices
// (TwoAdicSubgroupDft::coset_lde_batch as TwoAdicFriPcs::commit uses it, circuit-prover/src/config.rs:55,131) and its
// two halves on their own (dft_batch / idft_batch / coset_dft_batch / coset_idft_batch of the same trait).
// What is decided per height - the split into two passes, lean or generic kernels, tile sizes, workgroups - is
// ntt_plan.h; here are the device tables, the job lists (a group per kernel instance) and their launches.
// Own translation unit (tu_api.h).
#include "tu_api.h"
#include "kernels_ntt2.hip.h"
#include "profile.h"

#include <algorithm>
#include <map>

namespace p3r {
namespace {

// ------------------------------------------------------------------ NTT tables
// Two-level power tables, built on the host and cached on the device (p3r_ctx::ntt_tables): lo[i] = x^i for i < n_lo,
// hi[j] = lead * (x^n_lo)^j for j < n_hi, Montgomery form; x^(j * n_lo + i) = hi[j] * lo[i] (times lead).
enum NttTableKind { NTT_TW_SUB, NTT_TW4, NTT_PRE, NTT_INV_POW };
struct PowTable {
  const uint32_t *lo, *hi;
};
template <class F>
void append_powers(std::vector<uint32_t>& lo, std::vector<uint32_t>& hi, F x, size_t n_lo, size_t n_hi, F lead) {
  F v = F::one();
  for (size_t i = 0; i < n_lo; ++i) {
    lo.push_back(v.v);
    v *= x;
  }
  const F step = v;  // x^n_lo
  v = lead;
  for (size_t j = 0; j < n_hi; ++j) {
    hi.push_back(v.v);
    v *= step;
  }
}
// The table under `key`; fill(lo, hi) builds it the first time.
template <class Fill>
PowTable power_table(p3r_ctx* ctx, NttTableKind kind, int a, int b, uint32_t shift, Fill fill) {
  const auto key = std::make_tuple((int)kind, a, b, shift);
  auto it = ctx->ntt_tables.find(key);
  if (it == ctx->ntt_tables.end()) {
    std::vector<uint32_t> lo, hi;
    fill(lo, hi);
    p3r_ctx::NttTable t{DevBuf(lo.size()), DevBuf(hi.size())};
    P3R_HIP(copy_sync(ctx->stream, t.lo.p, lo.data(), lo.size() * 4, hipMemcpyHostToDevice));
    if (!hi.empty()) P3R_HIP(copy_sync(ctx->stream, t.hi.p, hi.data(), hi.size() * 4, hipMemcpyHostToDevice));
    it = ctx->ntt_tables.emplace(key, std::move(t)).first;
  }
  return {it->second.lo.p, it->second.hi.p};
}
template <class PP>
Fp<PP> ntt_root(int log_n, int inverse) {
  const Fp<PP> root = Fp<PP>::two_adic_generator(log_n);
  return inverse ? root.inv() : root;
}

// w_R^(+-i), i < R/2: the twiddles of a size-R sub-transform (one level).
template <class PP>
const uint32_t* get_tw_sub(p3r_ctx* ctx, int log_r, int inverse) {
  return power_table(ctx, NTT_TW_SUB, log_r, inverse, 0, [&](auto& lo, auto& hi) {
    append_powers(lo, hi, ntt_root<PP>(log_r, inverse), log_r ? size_t(1) << (log_r - 1) : 1, 0, Fp<PP>::one());
  }).lo;
}
// The four-step twiddles w_N^(+-x) = hi[x >> 10] * lo[x & 1023].
template <class PP>
PowTable get_tw4(p3r_ctx* ctx, int log_n, int inverse) {
  return power_table(ctx, NTT_TW4, log_n, inverse, 0, [&](auto& lo, auto& hi) {
    append_powers(lo, hi, ntt_root<PP>(log_n, inverse), 1024, log_n > 10 ? size_t(1) << (log_n - 10) : 1, Fp<PP>::one());
  });
}
// Per-coset input scaling for the forward pass: output block z of the bit-reversed LDE is
// the coset shift * w_{N<<b}^{bitrev_b(z)} * <w_N>, so cell k of the coefficient vector is
// multiplied by s_z^k = s_z^{N2*n1} * s_z^{n2}: hi = [cosets][N1] (the jobs' pre_a), lo = [cosets][N2] (pre_b).
// (The split is not in the key: it is a function of log_n and of tuning values that are fixed for the process.)
template <class PP>
PowTable get_pre(p3r_ctx* ctx, int log_n, int log_n1, int log_n2, int added_bits, uint32_t shift) {
  using F = Fp<PP>;
  return power_table(ctx, NTT_PRE, log_n, added_bits, shift, [&](auto& lo, auto& hi) {
    const F wbig = F::two_adic_generator(log_n + added_bits);
    for (uint32_t z = 0; z < (1u << added_bits); ++z)
      append_powers(lo, hi, F::from_canonical(shift) * wbig.pow(bit_reverse(z, added_bits)), size_t(1) << log_n2,
                    size_t(1) << log_n1, F::one());
  });
}
// Coefficient scaling of a coset inverse transform: coefficient k = j * 2^log_lo + i of an N-point inverse over
// shift * <w_N> is the plain inverse's times shift^-k / N = hi[j] * lo[i] (hi carries the 1/N).  Its own kind of table,
// keyed by (log_n, shift): the split is a function of log_n alone (ntt_inv_pow_log_lo), and nothing the LDE reads
// (NTT_PRE) is touched.
template <class PP>
PowTable get_inv_pow(p3r_ctx* ctx, int log_n, uint32_t shift) {
  using F = Fp<PP>;
  return power_table(ctx, NTT_INV_POW, log_n, 0, shift, [&](auto& lo, auto& hi) {
    const int log_lo = ntt_inv_pow_log_lo(log_n);
    append_powers(lo, hi, F::from_canonical(shift).inv(), size_t(1) << log_lo, size_t(1) << (log_n - log_lo),
                  F::from_canonical((uint32_t)((size_t(1) << log_n) % PP::P)).inv());
  });
}

// ------------------------------------------------------------------ job lists and their launches
// The jobs of one launch: a job owns `tiles` consecutive workgroups from its block0.
template <class JOB>
struct JobGroup {
  std::vector<JOB> jobs;
  uint64_t blocks = 0;
  void add(JOB j, uint64_t tiles) {
    j.block0 = (uint32_t)blocks;
    blocks += tiles;
    jobs.push_back(j);
  }
};
// The lean passes (kernels_ntt2.hip.h) are instantiated per sub-transform size and tile size: a group per instance,
// launched in this order.
struct GroupKey {
  int log_r, log_tile;
  bool operator<(const GroupKey& o) const { return log_r != o.log_r ? log_r < o.log_r : log_tile < o.log_tile; }
};
template <class JOB>
using JobGroups = std::map<GroupKey, JobGroup<JOB>>;
template <class JOB>
using JobKernel = void (*)(const JOB*, int);

// One launch of a job list (its device copy: const_table), a workgroup per tile.
template <class JOB>
void launch_jobs(p3r_ctx* ctx, const char* name, JobKernel<JOB> kernel, const JobGroup<JOB>& g, unsigned lanes, size_t lds = 0) {
  if (g.jobs.empty()) return;
  if (g.blocks >= (uint64_t(1) << 31)) fail(P3R_EUNSUPPORTED, "%s: launch of %llu tiles", name, (unsigned long long)g.blocks);
  const auto* d = static_cast<const JOB*>(const_table(ctx, g.jobs.data(), g.jobs.size() * sizeof(JOB)));
  ProfScope ps(ctx, name);
  hipLaunchKernelGGL(kernel, dim3((unsigned)g.blocks), dim3(lanes), lds, ctx->stream, d, (int)g.jobs.size());
  P3R_HIP(hipGetLastError());
}
// The groups of one pass: a launch per group, `pick(key)` the instance.  Two groups or more, all of them on the mixed
// kernel's tile size and at most kNtt2MixedMaxBlocks workgroups in total (the tables of a small layer): one launch of
// the mixed-size kernel, the groups one after the other, instead of one per size.
// A lane per 16 cells of the tile, at most kNtt2Lanes (2^14-cell column tiles: two items per lane and stage group).
template <class JOB, class Pick>
void launch_groups(p3r_ctx* ctx, const char* name, const JobGroups<JOB>& groups, int mixed_log_tile, JobKernel<JOB> mixed,
                   Pick pick) {
  auto lanes = [](int log_tile) { return std::min<unsigned>(kNtt2Lanes, 1u << (log_tile - 4)); };
  uint64_t total = 0;
  bool merge = groups.size() >= 2;
  for (const auto& kv : groups) {
    merge = merge && kv.first.log_tile == mixed_log_tile;
    total += kv.second.blocks;
  }
  if (merge && total <= kNtt2MixedMaxBlocks) {
    JobGroup<JOB> all;
    for (const auto& kv : groups) {
      const uint32_t base = (uint32_t)all.blocks;
      for (JOB j : kv.second.jobs) {
        j.block0 += base;
        all.jobs.push_back(j);
      }
      all.blocks += kv.second.blocks;
    }
    return launch_jobs(ctx, name, mixed, all, lanes(mixed_log_tile));
  }
  for (const auto& kv : groups) launch_jobs(ctx, name, pick(kv.first), kv.second, lanes(kv.first.log_tile));
}

template <class PP, int MODE>
void launch_col(p3r_ctx* ctx, const JobGroups<NttColJob>& groups) {
  const char* name = MODE == NTT2_FWD ? "ntt_forward_1" : MODE == NTT2_INV1 ? "ntt_inverse_1" : "ntt_inverse_2";
  launch_groups(ctx, name, groups, kNtt2LogTile, k_ntt_col_mixed<PP, MODE>, [](GroupKey k) -> JobKernel<NttColJob> {
#define P3R_COL_CASE(R) case R: return k.log_tile == 14 ? k_ntt_col<PP, R, MODE, 14> : k_ntt_col<PP, R, MODE, 13>;
    switch (k.log_r) {  // kNtt2MinLogR .. kNtt2MaxLogR
      P3R_COL_CASE(5) P3R_COL_CASE(6) P3R_COL_CASE(7) P3R_COL_CASE(8) P3R_COL_CASE(9) P3R_COL_CASE(10) P3R_COL_CASE(11)
      P3R_COL_CASE(12)
      default: fail(P3R_EUNSUPPORTED, "NTT column pass of 2^%d rows", k.log_r);
    }
#undef P3R_COL_CASE
  });
}
template <class PP>
void launch_fwd_line(p3r_ctx* ctx, const JobGroups<NttLineJob>& groups) {
  launch_groups(ctx, "ntt_forward_2", groups, 12, k_ntt_fwd_line_mixed<PP>, [](GroupKey k) -> JobKernel<NttLineJob> {
#define P3R_LINE_CASE(R) case R: return k.log_tile == 12 ? k_ntt_fwd_line<PP, R, 12> : k_ntt_fwd_line<PP, R, 13>;
    switch (k.log_r) {  // kNtt2MinLogR .. kNtt2MaxLineLogR
      P3R_LINE_CASE(5) P3R_LINE_CASE(6) P3R_LINE_CASE(7) P3R_LINE_CASE(8) P3R_LINE_CASE(9) P3R_LINE_CASE(10)
      P3R_LINE_CASE(11) P3R_LINE_CASE(12)
      case 13: return k_ntt_fwd_line<PP, 13, 13>;
      default: fail(P3R_EUNSUPPORTED, "forward NTT line pass of 2^%d cells", k.log_r);
    }
#undef P3R_LINE_CASE
  });
}

// The generic passes (k_ntt_tile, kernels_ntt.hip.h): the listed passes in ONE launch (they must be independent of
// each other); the tile of each is chosen here.
struct NttJob {
  NttPass pass;
  size_t ncols, ncosets;
};
template <class PP>
void launch_ntt(p3r_ctx* ctx, const std::vector<NttJob>& jobs, const char* name) {
  static const int log_tile = tuning_knob("P3R_NTT_LOG_TILE") ? atoi(tuning_knob("P3R_NTT_LOG_TILE")) : 13;
  JobGroup<NttPass> g;
  size_t lds_max = 0;
  unsigned threads_max = 64;
  for (const NttJob& j : jobs) {
    NttPass a = j.pass;
    const int log_r = a.sub_dim == 0 ? a.log_n1 : a.log_n2;
    const int log_lines = a.sub_dim == 0 ? a.log_n2 : a.log_n1;
    a.log_t = ntt_generic_log_t(log_r, log_lines, a.sub_dim == 0, log_tile);
    lds_max = std::max(lds_max, ntt_generic_lds_bytes(log_r, a.log_t));
    threads_max = std::max(threads_max, (unsigned)std::min<size_t>(kNttBlock, (size_t(1) << (log_r + a.log_t)) >> 4));
    a.log_gx = log_lines - a.log_t;
    a.log_gz = log2_exact(j.ncosets, "coset count");
    g.add(a, ntt_pass_blocks(j.ncols, a.log_n1 + a.log_n2 + a.log_gz, log_r + a.log_t));
  }
  launch_jobs<NttPass>(ctx, name, k_ntt_tile<PP>, g, threads_max, lds_max);
}

// The launches of one batch.  plan_inverse / plan_forward / plan_bitrev add the passes of one matrix to the lists,
// run_plan launches every list once: pass k of all matrices of the batch is one launch.
struct NttPlan {
  // phase 0/1: inverse transform (matrices of one tile: 0 = inverse, 1 = forward); 2/3: forward of the rest
  std::vector<NttJob> phase[4];
  JobGroups<NttColJob> fwd_col, inv1, inv2, inv2c;
  JobGroups<NttLineJob> fwd_line;
  JobGroup<BitrevJob> rev_in, rev_out;  // row bit-reversals before / after the transforms
  std::vector<DevBuf> scratch;          // coefficient vectors and transposition buffers
  uint32_t* temp(size_t cells) {
    scratch.emplace_back(cells);
    return scratch.back().p;
  }
};

// Inverse half: `in` = N x w evaluations over shift * <w_N>, natural order -> `coef` = coefficients, natural order.
// shift = 1 (the LDE's inverse: a subgroup) takes the scalar 1/N; any other shift the power table of get_inv_pow.
template <class PP>
void plan_inverse(p3r_ctx* ctx, NttPlan& pl, const uint32_t* in, uint32_t* coef, int log_n, size_t w, uint32_t shift) {
  using F = Fp<PP>;
  const size_t N = size_t(1) << log_n;
  const uint32_t inv_n = F::from_canonical((uint32_t)(N % PP::P)).inv().v;
  const bool coset = shift != 1;
  const PowTable ip = coset ? get_inv_pow<PP>(ctx, log_n, shift) : PowTable{nullptr, nullptr};
  const NttSplit s = ntt_inverse_split(log_n);
  const int la = s.la, lb = s.lb;
  // the last pass of the generic kernel: scaled, natural order
  auto last_pass = [&](NttPass& p) {
    p.out = coef;
    p.in_col_stride = N; p.out_col_stride = N;
    p.out_mode = 1; p.inverse = 1;
    if (coset) { p.post_a = ip.hi; p.post_b = ip.lo; p.post_log = ntt_inv_pow_log_lo(log_n); }
    else { p.scale = inv_n; p.use_scale = 1; }
  };
  NttPass p{};
  if (s.single) {
    // single pass: whole polynomial in one LDS tile
    p.in = in;
    p.log_n1 = 0; p.log_n2 = log_n; p.sub_dim = 1;
    p.tw_sub = get_tw_sub<PP>(ctx, log_n, 1);
    last_pass(p);
    pl.phase[0].push_back({p, w, 1});
    return;
  }
  uint32_t* tmp = pl.temp(N * w);
  const PowTable tw4i = get_tw4<PP>(ctx, log_n, 1);
  if (s.lean) {
    NttColJob j1{};
    j1.in = in; j1.out = tmp;
    j1.tw = get_tw_sub<PP>(ctx, la, 1);
    j1.tw4_lo = tw4i.lo; j1.tw4_hi = tw4i.hi;
    j1.in_col_stride = N; j1.out_col_stride = N;
    j1.log_n2 = lb; j1.log_r = la;
    pl.inv1[{la, s.log_tile1}].add(j1, ntt_pass_blocks(w, log_n, s.log_tile1));
    NttColJob j2{};   // tmp viewed as [N2 rows][N1]: size-N2 transforms along the rows
    j2.in = tmp; j2.out = coef;
    j2.tw = get_tw_sub<PP>(ctx, lb, 1);
    j2.in_col_stride = N; j2.out_col_stride = N;
    j2.log_n2 = la; j2.log_r = lb;
    if (coset) { j2.pre_a = ip.hi; j2.pre_b = ip.lo; }  // ntt_inv_pow_log_lo(log_n) = la: [N2] x [N1]
    else j2.scale = inv_n;
    (coset ? pl.inv2c : pl.inv2)[{lb, s.log_tile2}].add(j2, ntt_pass_blocks(w, log_n, s.log_tile2));
    return;
  }
  // inverse pass 1: size-N1 transforms along n1, twiddle, transposed store tmp[n2*N1 + k1]
  p.in = in; p.out = tmp;
  p.in_col_stride = N; p.out_col_stride = N;
  p.log_n1 = la; p.log_n2 = lb; p.sub_dim = 0; p.out_mode = 2;
  p.tw_sub = get_tw_sub<PP>(ctx, la, 1); p.inverse = 1;
  p.tw4_lo = tw4i.lo; p.tw4_hi = tw4i.hi;
  pl.phase[0].push_back({p, w, 1});
  // inverse pass 2: tmp viewed as [N2][N1]; size-N2 transforms along its first dim,
  // natural row order -> coefficient k1 + N1*k2 lands at k2*N1 + k1
  p = NttPass{};
  p.in = tmp;
  p.log_n1 = lb; p.log_n2 = la; p.sub_dim = 0;
  p.tw_sub = get_tw_sub<PP>(ctx, lb, 1);
  last_pass(p);
  pl.phase[1].push_back({p, w, 1});
}

// Forward half: `coef` = N x w coefficients, natural order -> `out` = (N << added_bits) x w evaluations over
// shift * <w_{N << added_bits}>, rows in bit-reversed order.
template <class PP>
void plan_forward(p3r_ctx* ctx, NttPlan& pl, const uint32_t* coef, uint32_t* out, int log_n, size_t w, int added_bits,
                  uint32_t shift) {
  static const int fwd_la_cap = tuning_knob("P3R_NTT_FWD_LOG_N1") ? atoi(tuning_knob("P3R_NTT_FWD_LOG_N1")) : 8;
  static const int line_log_tile = tuning_knob("P3R_NTT_LINE_LOG_TILE") ? atoi(tuning_knob("P3R_NTT_LINE_LOG_TILE")) : 12;
  const size_t N = size_t(1) << log_n, B = size_t(1) << added_bits;
  const NttSplit s = ntt_forward_split(log_n, fwd_la_cap, line_log_tile);
  const int la_f = s.la, lb_f = s.lb;
  const PowTable pre = get_pre<PP>(ctx, log_n, la_f, lb_f, added_bits, shift);
  // pass 1 (all cosets): scale by s_z^k, size-N1 transforms along n1, twiddle, in place rows
  // (single: the whole transform, N1 = 1)
  NttPass p{};
  p.in = coef; p.out = out;
  p.in_col_stride = N; p.out_col_stride = N * B; p.out_coset_stride = N;
  p.log_n1 = la_f; p.log_n2 = lb_f; p.sub_dim = s.single ? 1 : 0; p.out_mode = 0;
  p.tw_sub = get_tw_sub<PP>(ctx, s.single ? log_n : la_f, 0);
  p.pre_a = pre.hi; p.pre_b = pre.lo;
  if (s.single) {
    pl.phase[1].push_back({p, w, B});
    return;
  }
  const PowTable tw4f = get_tw4<PP>(ctx, log_n, 0);
  if (s.lean) {
    // lean kernels (kernels_ntt2.hip.h): the same two passes with compile-time geometry
    NttColJob cj{};
    cj.in = coef; cj.out = out;
    cj.tw = p.tw_sub;
    cj.tw4_lo = tw4f.lo; cj.tw4_hi = tw4f.hi;
    cj.pre_a = pre.hi; cj.pre_b = pre.lo;
    cj.in_col_stride = N; cj.out_col_stride = N * B; cj.out_coset_stride = N;
    cj.log_n2 = lb_f; cj.log_cosets = added_bits; cj.log_r = la_f;
    JobGroup<NttColJob>& fc = pl.fwd_col[{la_f, s.log_tile1}];
    const uint64_t tiles = ntt_pass_blocks(w, log_n, s.log_tile1);  // of one coset
    cj.xcd_map = (added_bits > 0 && (fc.blocks & 7) == 0 && (tiles & 7) == 0) ? 1 : 0;
    fc.add(cj, tiles << added_bits);
    NttLineJob lj{};
    lj.data = out;
    lj.tw = get_tw_sub<PP>(ctx, lb_f, 0);
    lj.log_r = (uint32_t)lb_f;
    pl.fwd_line[{lb_f, s.log_tile2}].add(lj, ntt_pass_blocks(w, log_n + added_bits, s.log_tile2));
    return;
  }
  p.tw4_lo = tw4f.lo; p.tw4_hi = tw4f.hi;
  pl.phase[2].push_back({p, w, B});
  // forward pass 2: contiguous size-N2 transforms, in place, bit-reversed rows kept.
  // The B cosets of a column are contiguous, so they are just B*N1 lines of N2 cells.
  p = NttPass{};
  p.in = out; p.out = out;
  p.in_col_stride = N * B; p.out_col_stride = N * B;
  p.log_n1 = la_f + added_bits; p.log_n2 = lb_f; p.sub_dim = 1; p.out_mode = 0;
  p.tw_sub = get_tw_sub<PP>(ctx, lb_f, 0);
  pl.phase[3].push_back({p, w, 1});
}

// Row bit-reversal of an N x w matrix, `in` -> `out` (two different matrices; k_bitrev_rows), before the transforms
// (`after` = false: the input of an inverse transform) or after them (the output of a forward one).
inline void plan_bitrev(NttPlan& pl, bool after, const uint32_t* in, uint32_t* out, int log_n, size_t w) {
  BitrevJob j{};
  j.in = in; j.out = out;
  j.log_n = (uint32_t)log_n;
  j.log_t = (uint32_t)ntt_bitrev_log_t(log_n);
  (after ? pl.rev_out : pl.rev_in).add(j, ntt_pass_blocks(w, log_n, ntt_bitrev_log_tile(log_n)));
}

template <class PP>
void run_plan(p3r_ctx* ctx, NttPlan& pl) {
  launch_jobs<BitrevJob>(ctx, "ntt_bitrev_rows", k_bitrev_rows, pl.rev_in, kBitrevLanes);
  launch_ntt<PP>(ctx, pl.phase[0], "ntt_inverse_1");
  launch_col<PP, NTT2_INV1>(ctx, pl.inv1);
  launch_ntt<PP>(ctx, pl.phase[1], "ntt_inverse_2");
  launch_col<PP, NTT2_INV2>(ctx, pl.inv2);
  launch_col<PP, NTT2_INV2C>(ctx, pl.inv2c);
  launch_ntt<PP>(ctx, pl.phase[2], "ntt_forward_1");
  launch_col<PP, NTT2_FWD>(ctx, pl.fwd_col);
  launch_ntt<PP>(ctx, pl.phase[3], "ntt_forward_2");
  launch_fwd_line<PP>(ctx, pl.fwd_line);
  launch_jobs<BitrevJob>(ctx, "ntt_bitrev_rows", k_bitrev_rows, pl.rev_out, kBitrevLanes);
}

}  // namespace

// K5 for a batch of matrices (all tables of a commit): every matrix goes through the same passes,
// and pass k of all of them is one launch.
// in: h x w evaluations over the subgroup (natural order, column-major Montgomery).
// Returns (h << added_bits) x w, rows in bit-reversed order over shift * <w_{h<<added_bits}>.
// The composition of the two halves: the inverse transform to a coefficient vector, the forward transform of it.
template <class PP>
std::vector<std::unique_ptr<p3r_dmat>> coset_lde_batch(p3r_ctx* ctx, const std::vector<LdeItem>& items,
                                                       int added_bits) {
  const size_t B = size_t(1) << added_bits;
  std::vector<std::unique_ptr<p3r_dmat>> outs;
  NttPlan pl;
  for (const LdeItem& it : items) {
    const p3r_dmat* in = it.in;
    const int log_n = log2_exact(in->h, "LDE input height");
    if (log_n + added_bits > PP::TWO_ADICITY)
      fail(P3R_EINVAL, "LDE of 2^%d rows exceeds the field's two-adicity (%d)", log_n + added_bits,
           PP::TWO_ADICITY);
    if (it.shift == 0 || it.shift >= PP::P) fail(P3R_EINVAL, "coset shift must be a non-zero canonical element");
    const size_t N = in->h, w = in->w;
    outs.push_back(dmat_alloc(N * B, w));
    uint32_t* coef = pl.temp(N * w);
    plan_inverse<PP>(ctx, pl, in->d, coef, log_n, w, 1);
    plan_forward<PP>(ctx, pl, coef, outs.back()->d, log_n, w, added_bits, it.shift);
  }
  run_plan<PP>(ctx, pl);
  return outs;
}

// TwoAdicSubgroupDft::dft_batch / idft_batch / coset_dft_batch / coset_idft_batch (tu_api.h): one half each.
template <class PP>
std::vector<std::unique_ptr<p3r_dmat>> dft_batch(p3r_ctx* ctx, const std::vector<LdeItem>& items, bool inverse,
                                                 bool bit_reversed) {
  for (const LdeItem& it : items) dft_check<PP>(it.in->h, it.in->w, it.shift);  // before anything is allocated
  std::vector<std::unique_ptr<p3r_dmat>> outs;
  NttPlan pl;
  for (const LdeItem& it : items) {
    const int log_n = log2_exact(it.in->h, "DFT height");
    const size_t N = it.in->h, w = it.in->w;
    outs.push_back(dmat_alloc(N, w));
    uint32_t* out = outs.back()->d;
    if (inverse) {
      const uint32_t* evals = it.in->d;
      if (bit_reversed && log_n >= 2) {  // (rows of a 1- or 2-row matrix are their own bit-reversal)
        uint32_t* nat = pl.temp(N * w);
        plan_bitrev(pl, false, evals, nat, log_n, w);
        evals = nat;
      }
      plan_inverse<PP>(ctx, pl, evals, out, log_n, w, it.shift);
    } else if (bit_reversed || log_n < 2) {
      plan_forward<PP>(ctx, pl, it.in->d, out, log_n, w, 0, it.shift);
    } else {
      uint32_t* rev = pl.temp(N * w);
      plan_forward<PP>(ctx, pl, it.in->d, rev, log_n, w, 0, it.shift);
      plan_bitrev(pl, true, rev, out, log_n, w);
    }
  }
  run_plan<PP>(ctx, pl);
  return outs;
}

template <class PP>
void lde_init(p3r_ctx*) {
  P3R_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ntt_tile<PP>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kNttMaxLdsBytes));
}

template std::vector<std::unique_ptr<p3r_dmat>> coset_lde_batch<KoalaBearParams>(p3r_ctx*, const std::vector<LdeItem>&, int);
template std::vector<std::unique_ptr<p3r_dmat>> coset_lde_batch<BabyBearParams>(p3r_ctx*, const std::vector<LdeItem>&, int);
template std::vector<std::unique_ptr<p3r_dmat>> dft_batch<KoalaBearParams>(p3r_ctx*, const std::vector<LdeItem>&, bool, bool);
template std::vector<std::unique_ptr<p3r_dmat>> dft_batch<BabyBearParams>(p3r_ctx*, const std::vector<LdeItem>&, bool, bool);
template void lde_init<KoalaBearParams>(p3r_ctx*);
template void lde_init<BabyBearParams>(p3r_ctx*);

}  // namespace p3r
