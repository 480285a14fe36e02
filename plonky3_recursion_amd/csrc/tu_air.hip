// The constraint-program seam (p3r_quotient_program_dmat): quotient_values + split_evals of p3_uni_stark::prove for an
// AIR the caller brings as data.  Own translation unit (tu_api.h).  The host half - validation, typing, degrees,
// liveness, slots, the instruction stream, the per-chunk constants - is air_program.h; the interpreter is
// k_quotient_program (kernels_air.hip.h).  One launch per call, whatever the program; the call only enqueues.
// The lookup-program seam (p3r_logup_program_dmat) lives here too: the same host half in its lookup mode, the same
// interpreter with the lookup sinks (k_logup_program), and the prover's scan for the running sum.
#include "kernels_air.hip.h"
#include "profile.h"
#include "tu_api.h"

namespace p3r {

namespace {

template <class PP, int DC>
std::vector<std::unique_ptr<p3r_dmat>> quotient_program_dc(p3r_ctx* ctx, const p3r_air_insn* prog, size_t n_insns,
                                                           const std::vector<const p3r_dmat*>& mats, uint32_t added_bits, uint32_t shift,
                                                           uint32_t log_q, const uint32_t* publics, size_t n_public,
                                                           const uint32_t* challenges, size_t n_challenges, const uint32_t* alpha_words) {
  using F = Fp<PP>;
  // ---- everything that is refused, before anything is allocated or launched
  if (ctx->cfg.zk) fail(P3R_EUNSUPPORTED, "the constraint-program seam does not serve zk contexts (their quotient domains are doubled)");
  if (log_q > (uint32_t)kAirMaxLogChunks) fail(P3R_EUNSUPPORTED, "log_quotient_degree > %d is not supported", kAirMaxLogChunks);
  if (added_bits > 31) fail(P3R_EINVAL, "added_bits (%u) out of range", added_bits);
  if (added_bits < log_q) fail(P3R_EINVAL, "added_bits (%u) is below log_quotient_degree (%u): the LDEs do not hold the quotient domain", added_bits, log_q);
  if (mats.empty()) fail(P3R_EINVAL, "n_mats == 0: no trace to evaluate the program on");
  if (!alpha_words) fail(P3R_EINVAL, "alpha is NULL");
  if ((n_public && !publics) || (n_challenges && !challenges)) fail(P3R_EINVAL, "public_values or challenges is NULL");
  const size_t H = mats[0]->h;
  const int log_H = log2_exact(H, "matrix height");
  if (log_H > PP::TWO_ADICITY) fail(P3R_EINVAL, "2^%d rows exceed the field's two-adicity (%d)", log_H, PP::TWO_ADICITY);
  if ((uint32_t)log_H < added_bits) fail(P3R_EINVAL, "a matrix of %zu rows is no LDE of blow-up 2^%u", H, added_bits);
  std::vector<size_t> widths(mats.size());
  size_t n_cols = 0;
  for (size_t m = 0; m < mats.size(); ++m) {
    if (mats[m]->h != H) fail(P3R_EINVAL, "matrix %zu has %zu rows, matrix 0 has %zu: the traces of one AIR share a height", m, mats[m]->h, H);
    widths[m] = mats[m]->w;
    n_cols += widths[m];
  }
  if (n_cols > 0x7fffffffu) fail(P3R_EINVAL, "too many columns");
  for (size_t k = 0; k < n_public; ++k)
    if (publics[k] >= PP::P) fail(P3R_EINVAL, "non-canonical public value %zu", k);
  for (size_t k = 0; k < n_challenges * DC; ++k)
    if (challenges[k] >= PP::P) fail(P3R_EINVAL, "non-canonical word %zu of challenge %zu", k % DC, k / DC);
  for (int k = 0; k < DC; ++k)
    if (alpha_words[k] >= PP::P) fail(P3R_EINVAL, "non-canonical word %d of alpha", k);
  const AirPlan plan = air_plan(prog, n_insns, widths.data(), widths.size(), DC, PP::P, n_public, n_challenges, P3R_AIR_MAX_LIVE);
  if (log_q < plan.info.log_quotient_degree)
    fail(P3R_EINVAL, "log_quotient_degree %u is below what the program needs (%u: its largest constraint degree is %u)", log_q,
         plan.info.log_quotient_degree, plan.info.max_degree);
  const int log_h = log_H - (int)added_bits, log_n = log_h + (int)log_q;
  const AirDomain dom = air_domain<PP>(shift, log_h, (int)log_q);
  const size_t lds = plan.lds_bytes(DC);
  if (lds > kAirMaxLdsBytes) fail(P3R_EUNSUPPORTED, "the program's slot file (%zu bytes) does not fit the LDS", lds);

  // ---- the launch
  const AirCompiled code = air_compile<PP>(plan, prog, n_insns, widths.data(), widths.size(), DC, publics, challenges);
  std::vector<const uint32_t*> cols;
  cols.reserve(n_cols);
  for (const p3r_dmat* m : mats)
    for (size_t c = 0; c < m->w; ++c) cols.push_back(m->d + c * m->h);
  const size_t h = size_t(1) << log_h, n_chunks = size_t(1) << log_q;
  std::vector<std::unique_ptr<p3r_dmat>> outs;
  for (size_t c = 0; c < n_chunks; ++c) outs.push_back(dmat_alloc(h, DC));   // [DC][h]: column k is coefficient k
  // one upload: the per-chunk tables, then the instruction stream, the challenge table and the column pointers
  const size_t off_insns = (sizeof(AirChunkTables) + 15) / 16 * 16;
  const size_t off_consts = off_insns + code.insns.size() * sizeof(AirDevInsn);
  const size_t off_cols = (off_consts + code.ext_consts.size() * 4 + 7) / 8 * 8;
  std::vector<unsigned char> blob(off_cols + cols.size() * sizeof(void*));
  DevBuf d_blob((blob.size() + 3) / 4);
  unsigned char* base = reinterpret_cast<unsigned char*>(d_blob.p);
  AirProgArgs a{};
  a.insns = reinterpret_cast<const AirDevInsn*>(base + off_insns);
  a.ext_consts = reinterpret_cast<const uint32_t*>(base + off_consts);
  a.cols = reinterpret_cast<const uint32_t* const*>(base + off_cols);
  a.chunks = reinterpret_cast<const AirChunkTables*>(base);
  AirChunkTables t{};
  for (size_t c = 0; c < n_chunks; ++c) {
    t.zh[c] = dom.zh[c];
    t.zh_inv[c] = dom.zh_inv[c];
    t.out[c] = outs[c]->d;
  }
  a.n_insns = (uint32_t)code.insns.size();
  a.log_n = log_n;
  a.log_q = (int)log_q;
  a.flags = (plan.uses_x ? 1u : 0u) | (plan.uses_inv ? 2u : 0u);
  a.shift = dom.shift;
  a.w_n = dom.w_n;
  a.g_inv = dom.g_inv;
  for (int k = 0; k < DC; ++k) a.alpha[k] = F::from_canonical(alpha_words[k]).v;
  memcpy(blob.data(), &t, sizeof t);
  memcpy(blob.data() + off_insns, code.insns.data(), code.insns.size() * sizeof(AirDevInsn));
  if (!code.ext_consts.empty()) memcpy(blob.data() + off_consts, code.ext_consts.data(), code.ext_consts.size() * 4);
  if (!cols.empty()) memcpy(blob.data() + off_cols, cols.data(), cols.size() * sizeof(void*));
  P3R_HIP(ctx->stage.upload(ctx->stream, d_blob.p, blob.data(), blob.size()));
  {
    ProfScope ps(ctx, "quotient_program");
    // rows j < N = 2^log_n <= H of every column are read, words k * h + r < DC * h of every chunk written: all inside
    // the matrices' allocations
    const unsigned blocks = (unsigned)(((size_t(1) << log_n) + kAirLanes - 1) / kAirLanes);
    // a slot file above the 48 KiB a kernel gets without asking (the worst P3R_AIR_MAX_LIVE admits is 72 KiB)
    if (lds > 48 * 1024)
      P3R_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_quotient_program<PP, DC>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)kAirMaxLdsBytes));
    hipLaunchKernelGGL((k_quotient_program<PP, DC>), dim3(blocks), dim3(kAirLanes), lds, ctx->stream,
                       a);
  }
  P3R_HIP(hipGetLastError());
  // the blob goes back to the context's pool, which is ordered by the stream the launch is on (context.h)
  return outs;
}

// The lookup-program seam (p3r_logup_program_dmat): the LogUp gadget of p3_lookup for interactions the caller brings as
// data.  k_logup_program writes the fraction columns and each row's total; the running sum and the table's sum are the
// prover's own three-mode scan k_ef_scan over a LogupJob of one job.  The call waits for the stream: the sum goes to the
// caller's challenger, and with it comes the word that says whether a denominator vanished.
template <class PP, int DC>
std::unique_ptr<p3r_dmat> logup_program_dc(p3r_ctx* ctx, const p3r_air_insn* prog, size_t n_insns, const std::vector<const p3r_dmat*>& mats,
                                           const uint32_t* publics, size_t n_public, const uint32_t* challenges, size_t n_challenges,
                                           uint32_t* sum_out) {
  using F = Fp<PP>;
  // ---- everything that is refused, before anything is allocated or launched
  if (ctx->cfg.zk) fail(P3R_EUNSUPPORTED, "the lookup-program seam does not serve zk contexts (their traces are randomised and their domains doubled)");
  if (!sum_out) fail(P3R_EINVAL, "sum_out is NULL");
  if (mats.empty()) fail(P3R_EINVAL, "n_mats == 0: no trace to evaluate the program on");
  if ((n_public && !publics) || (n_challenges && !challenges)) fail(P3R_EINVAL, "public_values or challenges is NULL");
  const size_t h = mats[0]->h;
  const int log_h = air_trace_log_height(h, PP::TWO_ADICITY);   // a power of two within the field's two-adicity
  std::vector<size_t> widths(mats.size());
  size_t n_cols = 0;
  for (size_t m = 0; m < mats.size(); ++m) {
    if (mats[m]->h != h) fail(P3R_EINVAL, "matrix %zu has %zu rows, matrix 0 has %zu: the traces of one table share a height", m, mats[m]->h, h);
    widths[m] = mats[m]->w;
    n_cols += widths[m];
  }
  if (n_cols > 0x7fffffffu) fail(P3R_EINVAL, "too many columns");
  for (size_t k = 0; k < n_public; ++k)
    if (publics[k] >= PP::P) fail(P3R_EINVAL, "non-canonical public value %zu", k);
  for (size_t k = 0; k < n_challenges * DC; ++k)
    if (challenges[k] >= PP::P) fail(P3R_EINVAL, "non-canonical word %zu of challenge %zu", k % DC, k / DC);
  const AirPlan plan = air_plan(prog, n_insns, widths.data(), widths.size(), DC, PP::P, n_public, n_challenges, P3R_AIR_MAX_LIVE, AIR_MODE_LOOKUP);
  const size_t lds = plan.lds_bytes(DC);
  if (lds > kAirMaxLdsBytes) fail(P3R_EUNSUPPORTED, "the program's slot file (%zu bytes) does not fit the LDS", lds);
  const size_t G = plan.lookup.n_columns;
  if (G > (0x7fffffffu / DC) - 1) fail(P3R_EINVAL, "too many auxiliary columns");

  // ---- the launches
  const AirCompiled code = air_compile<PP>(plan, prog, n_insns, widths.data(), widths.size(), DC, publics, challenges);
  std::vector<const uint32_t*> cols;
  cols.reserve(n_cols);
  for (const p3r_dmat* m : mats)
    for (size_t c = 0; c < m->w; ++c) cols.push_back(m->d + c * m->h);
  std::unique_ptr<p3r_dmat> out = dmat_alloc(h, (size_t)DC * (1 + G));   // [DC * (1 + G)][h]
  const size_t n_tiles = (h + kScanTile - 1) / kScanTile;
  DevBuf rowsum((size_t)DC * h), agg((size_t)DC * n_tiles);
  // one upload: the scan's job, the words the device answers in (bad row, then the table's sum), the instruction stream,
  // the challenge table and the column pointers
  const size_t off_answer = (sizeof(LogupJob) + 15) / 16 * 16;
  const size_t off_insns = off_answer + 16 * ((4 * (1 + DC) + 15) / 16);
  const size_t off_consts = off_insns + code.insns.size() * sizeof(AirDevInsn);
  const size_t off_cols = (off_consts + code.ext_consts.size() * 4 + 7) / 8 * 8;
  std::vector<unsigned char> blob(off_cols + cols.size() * sizeof(void*));
  DevBuf d_blob((blob.size() + 3) / 4);
  unsigned char* base = reinterpret_cast<unsigned char*>(d_blob.p);
  uint32_t* d_answer = reinterpret_cast<uint32_t*>(base + off_answer);
  AirLogupArgs a{};
  a.insns = reinterpret_cast<const AirDevInsn*>(base + off_insns);
  a.ext_consts = reinterpret_cast<const uint32_t*>(base + off_consts);
  a.cols = reinterpret_cast<const uint32_t* const*>(base + off_cols);
  a.out = out->d;
  a.rowsum = rowsum.p;
  a.bad_row = d_answer;
  a.n_insns = (uint32_t)code.insns.size();
  a.log_h = log_h;
  LogupJob job{};   // what k_ef_scan reads of it
  job.aux = out->d;
  job.rowsum = rowsum.p;
  job.agg = agg.p;
  job.total = d_answer + 1;
  job.n = h;
  job.n_tiles = (uint32_t)n_tiles;
  const uint32_t answer0[1 + kMaxAirDC] = {0xffffffffu};   // no bad row; the sum is written by the scan
  memcpy(blob.data(), &job, sizeof job);
  memcpy(blob.data() + off_answer, answer0, 4 * (1 + DC));
  memcpy(blob.data() + off_insns, code.insns.data(), code.insns.size() * sizeof(AirDevInsn));
  if (!code.ext_consts.empty()) memcpy(blob.data() + off_consts, code.ext_consts.data(), code.ext_consts.size() * 4);
  if (!cols.empty()) memcpy(blob.data() + off_cols, cols.data(), cols.size() * sizeof(void*));
  P3R_HIP(ctx->stage.upload(ctx->stream, d_blob.p, blob.data(), blob.size()));
  {
    ProfScope ps(ctx, "logup_program");
    // rows r < h of every input column are read; words (col * DC + k) * h + r with 1 <= col <= G, so below
    // DC * (1 + G) * h, of the output and k * h + r < DC * h of rowsum are written by k_logup_program; k_ef_scan writes
    // words k * h + r < DC * h of the output, DC * tile + k < DC * n_tiles of agg and the DC words of the sum: all inside
    // the allocations above
    const unsigned blocks = (unsigned)((h + kAirLanes - 1) / kAirLanes);
    if (lds > 48 * 1024)
      P3R_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_logup_program<PP, DC>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)kAirMaxLdsBytes));
    hipLaunchKernelGGL((k_logup_program<PP, DC>), dim3(blocks), dim3(kAirLanes), lds, ctx->stream, a);
    const auto* d_job = reinterpret_cast<const LogupJob*>(base);
    hipLaunchKernelGGL((k_ef_scan<PP, DC>), dim3((unsigned)n_tiles), dim3(kBlock), 0, ctx->stream, 0, d_job, 1);
    hipLaunchKernelGGL((k_ef_scan<PP, DC>), dim3(1), dim3(kBlock), 0, ctx->stream, 1, d_job, 1);
    hipLaunchKernelGGL((k_ef_scan<PP, DC>), dim3((unsigned)n_tiles), dim3(kBlock), 0, ctx->stream, 2, d_job, 1);
  }
  P3R_HIP(hipGetLastError());
  uint32_t answer[1 + kMaxAirDC];
  P3R_HIP(fetch_small(ctx, d_answer, 1 + DC, answer));   // waits for the stream
  if (answer[0] != 0xffffffffu) fail(P3R_EINVAL, "zero denominator in row %u: the fraction of an auxiliary column is not defined there", answer[0]);
  for (int k = 0; k < DC; ++k) sum_out[k] = F::raw(answer[1 + k]).to_canonical();
  return out;
}

}  // namespace

template <class PP>
std::unique_ptr<p3r_dmat> logup_program(p3r_ctx* ctx, const p3r_air_insn* prog, size_t n_insns, const std::vector<const p3r_dmat*>& mats,
                                        const uint32_t* publics, size_t n_public, const uint32_t* challenges, size_t n_challenges,
                                        uint32_t* sum_out) {
  if (ctx->cfg.challenge_degree == 5) {
    if constexpr (kHasQuintic<PP>) return logup_program_dc<PP, 5>(ctx, prog, n_insns, mats, publics, n_public, challenges, n_challenges, sum_out);
    else fail(P3R_EUNSUPPORTED, "UnsupportedChallengeDegree: the quintic challenge field is KoalaBear's");
  }
  return logup_program_dc<PP, 4>(ctx, prog, n_insns, mats, publics, n_public, challenges, n_challenges, sum_out);
}

template <class PP>
std::vector<std::unique_ptr<p3r_dmat>> quotient_program(p3r_ctx* ctx, const p3r_air_insn* prog, size_t n_insns,
                                                        const std::vector<const p3r_dmat*>& mats, uint32_t added_bits, uint32_t shift,
                                                        uint32_t log_quotient_degree, const uint32_t* publics, size_t n_public,
                                                        const uint32_t* challenges, size_t n_challenges, const uint32_t* alpha) {
  if (ctx->cfg.challenge_degree == 5) {
    if constexpr (kHasQuintic<PP>)
      return quotient_program_dc<PP, 5>(ctx, prog, n_insns, mats, added_bits, shift, log_quotient_degree, publics, n_public, challenges,
                                        n_challenges, alpha);
    else fail(P3R_EUNSUPPORTED, "UnsupportedChallengeDegree: the quintic challenge field is KoalaBear's");
  }
  return quotient_program_dc<PP, 4>(ctx, prog, n_insns, mats, added_bits, shift, log_quotient_degree, publics, n_public, challenges,
                                    n_challenges, alpha);
}

#define P3R_AIR_INSTANCE(PP)                                                                                                     \
  template std::vector<std::unique_ptr<p3r_dmat>> quotient_program<PP>(p3r_ctx*, const p3r_air_insn*, size_t,                    \
                                                                       const std::vector<const p3r_dmat*>&, uint32_t, uint32_t, \
                                                                       uint32_t, const uint32_t*, size_t, const uint32_t*, size_t, \
                                                                       const uint32_t*);
P3R_AIR_INSTANCE(KoalaBearParams)
P3R_AIR_INSTANCE(BabyBearParams)
#undef P3R_AIR_INSTANCE
#define P3R_LOGUP_INSTANCE(PP)                                                                                                              \
  template std::unique_ptr<p3r_dmat> logup_program<PP>(p3r_ctx*, const p3r_air_insn*, size_t, const std::vector<const p3r_dmat*>&,          \
                                                       const uint32_t*, size_t, const uint32_t*, size_t, uint32_t*);
P3R_LOGUP_INSTANCE(KoalaBearParams)
P3R_LOGUP_INSTANCE(BabyBearParams)
#undef P3R_LOGUP_INSTANCE

}  // namespace p3r
