// The constraint-program seam (p3r_quotient_program_dmat): quotient_values + split_evals of p3_uni_stark::prove for an
// AIR the caller brings as data.  Own translation unit (tu_api.h).  The host half - validation, typing, degrees,
// liveness, slots, the instruction stream, the per-chunk constants - is air_program.h; the interpreter is
// k_quotient_program (kernels_air.hip.h).  One launch per call, whatever the program; the call only enqueues.
// The seams that run a program on TRACES live here too, all of them k_trace_program with a sink of their own:
// the lookup-program seam (p3r_logup_program_dmat: the same host half in its lookup mode, LogupProgSink, and the prover's
// scan for the running sum); the two checks of a caller's traces, p3r_check_program_dmat (CheckProgSink: the constraints
// on the trace domain, a first failing row and a count per constraint) and p3r_lookup_check_dmat (RecordSink, then the
// stable radix sort and the sums of device_prims.hip.h: the keys of the bus whose multiplicities do not cancel);
// p3r_lookup_multiplicities_dmat, the same pass (LookupPass) with another end: k_lookup_scatter gives every key's first
// table slot the sum its queries ask for - the multiplicity column of a table - and reports the keys no table slot offers;
// and the witness seam (p3r_witness_program_dmat: the witness mode, WitnessSink): the values a program stores become the
// columns of a new trace.  One launch; the call only enqueues.
// What they share is written once: the refusals about tables and matrices, the upload (ProgramBlob) and the launch
// (launch_program: the grid, the opt-in to a slot file above 48 KiB, the error check).
// The recurrence seam (p3r_affine_scan_dmat) is the one entry here that runs no program: the accumulator columns
// s[r + 1] = a[r] s[r] + b[r] of resident traces, validated by scan_plan.h and scanned by k_affine_scan (kernels_scan.hip.h).
#include <algorithm>

#include "device_prims.hip.h"
#include "kernels_air.hip.h"
#include "kernels_scan.hip.h"
#include "profile.h"
#include "tu_api.h"

namespace p3r {

namespace {

// ---- what the entries that run a program refuse about its tables and matrices, each written once.  The entries call them
// in their own order, between refusals of their own: which refusal comes first is part of what an entry promises.
inline void refuse_null_tables(const uint32_t* publics, size_t n_public, const uint32_t* challenges, size_t n_challenges) {
  if ((n_public && !publics) || (n_challenges && !challenges)) fail(P3R_EINVAL, "public_values or challenges is NULL");
}
template <class PP, int DC>
void refuse_non_canonical(const uint32_t* publics, size_t n_public, const uint32_t* challenges, size_t n_challenges) {
  for (size_t k = 0; k < n_public; ++k)
    if (publics[k] >= PP::P) fail(P3R_EINVAL, "non-canonical public value %zu", k);
  for (size_t k = 0; k < n_challenges * DC; ++k)
    if (challenges[k] >= PP::P) fail(P3R_EINVAL, "non-canonical word %zu of challenge %zu", k % DC, k / DC);
}
// What an entry keeps of one program and its matrices: the plan, and the figures of the launch.  h and log_h are the height
// of the MATRICES: of the traces, or in the quotient seam of their LDEs - the trace height there is a local of the entry.
struct TraceProgram {
  AirPlan plan;
  std::vector<size_t> widths;
  size_t h = 0, n_cols = 0, lds = 0;
  int log_h = 0;
  // the widths of `mats`, which share the height h; `whose` ("AIR", "table") is how the refusal names them
  void columns(const std::vector<const p3r_dmat*>& mats, const char* whose) {
    widths.resize(mats.size());
    for (size_t m = 0; m < mats.size(); ++m) {
      if (mats[m]->h != h)
        fail(P3R_EINVAL, "matrix %zu has %zu rows, matrix 0 has %zu: the traces of one %s share a height", m, mats[m]->h, h, whose);
      widths[m] = mats[m]->w;
      n_cols += widths[m];
    }
    if (n_cols > 0x7fffffffu) fail(P3R_EINVAL, "too many columns");
  }
  // the plan's slot file against the LDS
  void slot_file(int dc) {
    lds = plan.lds_bytes(dc);
    if (lds > kAirMaxLdsBytes) fail(P3R_EUNSUPPORTED, "the program's slot file (%zu bytes) does not fit the LDS", lds);
  }
};
// What the entries that run a program on TRACES (the lookup-program seam, the two checks, the witness seam) refuse, in one
// order for all of them.
// `height`: the witness seam's, which takes a program with no input matrix and then needs it; 0 with matrices: theirs.
template <class PP, int DC>
TraceProgram trace_program(const p3r_air_insn* prog, size_t n_insns, const std::vector<const p3r_dmat*>& mats, const uint32_t* publics,
                           size_t n_public, const uint32_t* challenges, size_t n_challenges, AirMode mode, size_t height = 0) {
  TraceProgram tp;
  if (mats.empty() && mode != AIR_MODE_WITNESS) fail(P3R_EINVAL, "n_mats == 0: no trace to evaluate the program on");
  refuse_null_tables(publics, n_public, challenges, n_challenges);
  const size_t h = tp.h = mats.empty() ? height : mats[0]->h;
  if (!mats.empty() && height && height != h)
    fail(P3R_EINVAL, "height (%zu) is not the matrices' (%zu): pass 0, or the height of the traces", height, h);
  tp.log_h = air_trace_log_height(h, PP::TWO_ADICITY);   // a power of two within the field's two-adicity
  tp.columns(mats, "table");
  refuse_non_canonical<PP, DC>(publics, n_public, challenges, n_challenges);
  tp.plan = air_plan(prog, n_insns, tp.widths.data(), tp.widths.size(), DC, PP::P, n_public, n_challenges, P3R_AIR_MAX_LIVE, mode);
  tp.slot_file(DC);
  return tp;
}

// The one place that knows the upload of a launch: `head` bytes the caller fills (answer words, a job, the chunk tables),
// then the instruction stream (16-aligned), the challenge table and the column pointers (8-aligned).
struct ProgramBlob {
  size_t off_insns, off_consts, off_cols, n_insns;
  std::vector<unsigned char> host;
  DevBuf dev;
  ProgramBlob(size_t head, const AirCompiled& code, const std::vector<const p3r_dmat*>& mats, size_t n_cols) : n_insns(code.insns.size()) {
    std::vector<const uint32_t*> cols;
    cols.reserve(n_cols);
    for (const p3r_dmat* m : mats)
      for (size_t c = 0; c < m->w; ++c) cols.push_back(m->d + c * m->h);
    off_insns = (head + 15) / 16 * 16;
    off_consts = off_insns + code.insns.size() * sizeof(AirDevInsn);
    off_cols = (off_consts + code.ext_consts.size() * 4 + 7) / 8 * 8;
    host.assign(off_cols + cols.size() * sizeof(void*), 0);
    memcpy(host.data() + off_insns, code.insns.data(), code.insns.size() * sizeof(AirDevInsn));
    if (!code.ext_consts.empty()) memcpy(host.data() + off_consts, code.ext_consts.data(), code.ext_consts.size() * 4);
    if (!cols.empty()) memcpy(host.data() + off_cols, cols.data(), cols.size() * sizeof(void*));
    dev.alloc((host.size() + 3) / 4);
  }
  unsigned char* base() const { return reinterpret_cast<unsigned char*>(dev.p); }
  AirStream stream() const {
    return AirStream{reinterpret_cast<const AirDevInsn*>(base() + off_insns), reinterpret_cast<const uint32_t*>(base() + off_consts),
                     reinterpret_cast<const uint32_t* const*>(base() + off_cols), (uint32_t)n_insns};
  }
  // the blob goes back to the context's pool when it dies; the pool is ordered by the stream the launch is on (context.h)
  void upload(p3r_ctx* ctx) { P3R_HIP(ctx->stage.upload(ctx->stream, dev.p, host.data(), host.size())); }
};

// One launch of an interpreter: one lane per row, one wave per workgroup, `lds` bytes of slot file.  Above the 48 KiB a
// kernel gets without asking (the worst P3R_AIR_MAX_LIVE admits is 72 KiB) the kernel is opted in, every time.
template <class Args>
void launch_program(p3r_ctx* ctx, void (*kernel)(Args), size_t n_rows, size_t lds, const Args& a) {
  const unsigned blocks = (unsigned)((n_rows + kAirLanes - 1) / kAirLanes);
  if (lds > 48 * 1024)
    P3R_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAirMaxLdsBytes));
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kAirLanes), lds, ctx->stream, a);
  P3R_HIP(hipGetLastError());
}

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
  refuse_null_tables(publics, n_public, challenges, n_challenges);
  TraceProgram tp;   // of the LDEs: tp.h and tp.log_h are their height H; h and log_h below are the trace's
  const size_t H = tp.h = mats[0]->h;
  const int log_H = log2_exact(H, "matrix height");
  if (log_H > PP::TWO_ADICITY) fail(P3R_EINVAL, "2^%d rows exceed the field's two-adicity (%d)", log_H, PP::TWO_ADICITY);
  if ((uint32_t)log_H < added_bits) fail(P3R_EINVAL, "a matrix of %zu rows is no LDE of blow-up 2^%u", H, added_bits);
  tp.log_h = log_H;
  tp.columns(mats, "AIR");
  refuse_non_canonical<PP, DC>(publics, n_public, challenges, n_challenges);
  for (int k = 0; k < DC; ++k)
    if (alpha_words[k] >= PP::P) fail(P3R_EINVAL, "non-canonical word %d of alpha", k);
  tp.plan = air_plan(prog, n_insns, tp.widths.data(), tp.widths.size(), DC, PP::P, n_public, n_challenges, P3R_AIR_MAX_LIVE);
  const AirPlan& plan = tp.plan;
  if (log_q < plan.info.log_quotient_degree)
    fail(P3R_EINVAL, "log_quotient_degree %u is below what the program needs (%u: its largest constraint degree is %u)", log_q,
         plan.info.log_quotient_degree, plan.info.max_degree);
  const int log_h = log_H - (int)added_bits, log_n = log_h + (int)log_q;
  const AirDomain dom = air_domain<PP>(shift, log_h, (int)log_q);
  tp.slot_file(DC);

  // ---- the launch
  const AirCompiled code = air_compile<PP>(plan, prog, n_insns, tp.widths.data(), tp.widths.size(), DC, publics, challenges);
  const size_t h = size_t(1) << log_h, n_chunks = size_t(1) << log_q;
  std::vector<std::unique_ptr<p3r_dmat>> outs;
  for (size_t c = 0; c < n_chunks; ++c) outs.push_back(dmat_alloc(h, DC));   // [DC][h]: column k is coefficient k
  AirChunkTables t{};   // leads the upload
  for (size_t c = 0; c < n_chunks; ++c) {
    t.zh[c] = dom.zh[c];
    t.zh_inv[c] = dom.zh_inv[c];
    t.out[c] = outs[c]->d;
  }
  ProgramBlob blob(sizeof t, code, mats, tp.n_cols);
  memcpy(blob.host.data(), &t, sizeof t);
  blob.upload(ctx);
  AirProgArgs a{};
  a.prog = blob.stream();
  a.chunks = reinterpret_cast<const AirChunkTables*>(blob.base());
  a.log_n = log_n;
  a.log_q = (int)log_q;
  a.flags = (plan.uses_x ? 1u : 0u) | (plan.uses_inv ? 2u : 0u);
  a.shift = dom.shift;
  a.w_n = dom.w_n;
  a.g_inv = dom.g_inv;
  for (int k = 0; k < DC; ++k) a.alpha[k] = F::from_canonical(alpha_words[k]).v;
  ProfScope ps(ctx, "quotient_program");
  // rows j < N = 2^log_n <= H of every column are read, words k * h + r < DC * h of every chunk written: all inside
  // the matrices' allocations
  launch_program(ctx, k_quotient_program<PP, DC>, size_t(1) << log_n, tp.lds, a);
  return outs;
}

// The lookup-program seam (p3r_logup_program_dmat): the LogUp gadget of p3_lookup for interactions the caller brings as
// data.  k_trace_program with the LogUp sink writes the fraction columns and each row's total; the running sum and the
// table's sum are the prover's own three-mode scan k_ef_scan over a LogupJob of one job.  The call waits for the stream: the
// sum goes to the caller's challenger, and with it comes the word that says whether a denominator vanished.
template <class PP, int DC>
std::unique_ptr<p3r_dmat> logup_program_dc(p3r_ctx* ctx, const p3r_air_insn* prog, size_t n_insns, const std::vector<const p3r_dmat*>& mats,
                                           const uint32_t* publics, size_t n_public, const uint32_t* challenges, size_t n_challenges,
                                           uint32_t* sum_out) {
  using F = Fp<PP>;
  // ---- everything that is refused, before anything is allocated or launched
  if (ctx->cfg.zk) fail(P3R_EUNSUPPORTED, "the lookup-program seam does not serve zk contexts (their traces are randomised and their domains doubled)");
  if (!sum_out) fail(P3R_EINVAL, "sum_out is NULL");
  const TraceProgram tp = trace_program<PP, DC>(prog, n_insns, mats, publics, n_public, challenges, n_challenges, AIR_MODE_LOOKUP);
  const size_t h = tp.h, G = tp.plan.lookup.n_columns;
  if (G > (0x7fffffffu / DC) - 1) fail(P3R_EINVAL, "too many auxiliary columns");

  // ---- the launches
  const AirCompiled code = air_compile<PP>(tp.plan, prog, n_insns, tp.widths.data(), tp.widths.size(), DC, publics, challenges);
  std::unique_ptr<p3r_dmat> out = dmat_alloc(h, (size_t)DC * (1 + G));   // [DC * (1 + G)][h]
  const size_t n_tiles = (h + kScanTile - 1) / kScanTile;
  DevBuf rowsum((size_t)DC * h), agg((size_t)DC * n_tiles);
  // the upload is led by the scan's job and the words the device answers in: the bad row, then the table's sum
  const size_t off_answer = (sizeof(LogupJob) + 15) / 16 * 16;
  ProgramBlob blob(off_answer + 16 * ((4 * (1 + DC) + 15) / 16), code, mats, tp.n_cols);
  uint32_t* d_answer = reinterpret_cast<uint32_t*>(blob.base() + off_answer);
  AirLogupArgs a{};
  a.prog = blob.stream();
  a.log_h = tp.log_h;
  a.out = out->d;
  a.rowsum = rowsum.p;
  a.bad_row = d_answer;
  LogupJob job{};   // what k_ef_scan reads of it
  job.aux = out->d;
  job.rowsum = rowsum.p;
  job.agg = agg.p;
  job.total = d_answer + 1;
  job.n = h;
  job.n_tiles = (uint32_t)n_tiles;
  const uint32_t answer0[1 + kMaxAirDC] = {0xffffffffu};   // no bad row; the sum is written by the scan
  memcpy(blob.host.data(), &job, sizeof job);
  memcpy(blob.host.data() + off_answer, answer0, 4 * (1 + DC));
  blob.upload(ctx);
  {
    ProfScope ps(ctx, "logup_program");
    // rows r < h of every input column are read; words (col * DC + k) * h + r with 1 <= col <= G, so below
    // DC * (1 + G) * h, of the output and k * h + r < DC * h of rowsum are written by the interpreter; k_ef_scan writes
    // words k * h + r < DC * h of the output, DC * tile + k < DC * n_tiles of agg and the DC words of the sum: all inside
    // the allocations above
    launch_program(ctx, k_trace_program<PP, DC, LogupProgSink>, h, tp.lds, a);
    const auto* d_job = reinterpret_cast<const LogupJob*>(blob.base());
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

// The witness seam (p3r_witness_program_dmat): the values a witness program stores, as the columns of a fresh trace.  One
// launch of k_trace_program with the witness sink; nothing is read back and the call does not wait.
template <class PP, int DC>
std::unique_ptr<p3r_dmat> witness_program_dc(p3r_ctx* ctx, const p3r_air_insn* prog, size_t n_insns, const std::vector<const p3r_dmat*>& mats,
                                             size_t height, const uint32_t* publics, size_t n_public, const uint32_t* challenges,
                                             size_t n_challenges) {
  // ---- everything that is refused, before anything is allocated or launched
  if (ctx->cfg.zk) fail(P3R_EUNSUPPORTED, "the witness seam does not serve zk contexts (their traces are randomised and their domains doubled)");
  const TraceProgram tp = trace_program<PP, DC>(prog, n_insns, mats, publics, n_public, challenges, n_challenges, AIR_MODE_WITNESS, height);
  const size_t W = tp.plan.witness.n_out_columns;

  // ---- the launch
  const AirCompiled code = air_compile<PP>(tp.plan, prog, n_insns, tp.widths.data(), tp.widths.size(), DC, publics, challenges);
  std::unique_ptr<p3r_dmat> out = dmat_alloc(tp.h, W);   // [W][h]
  ProgramBlob blob(0, code, mats, tp.n_cols);
  blob.upload(ctx);
  AirWitnessArgs a{};
  a.prog = blob.stream();
  a.log_h = tp.log_h;
  a.out = out->d;
  ProfScope ps(ctx, "witness_program");
  // rows r < h of every input column are read (with no input matrix the stream has no load); a STORE writes words
  // col * h + r with col < W - air_plan took W as one past the highest stored column - and r < h: all inside the
  // allocation above.  Every column below W is stored: nothing of the output stays uninitialised.
  launch_program(ctx, k_trace_program<PP, DC, WitnessSink>, tp.h, tp.lds, a);
  return out;
}

// The recurrence seam (p3r_affine_scan_dmat): the columns s[r + 1] = a[r] s[r] + b[r] of resident traces.  Three launches
// of k_affine_scan (kernels_scan.hip.h) whatever the number of recurrences; with `last_out` the call waits for the stream
// and hands back s[h] of each, otherwise it only enqueues.
template <class PP, int DC>
std::unique_ptr<p3r_dmat> affine_scan_dc(p3r_ctx* ctx, const p3r_recurrence* recs, size_t n_recs, const std::vector<const p3r_dmat*>& mats,
                                         uint32_t* last_out) {
  using F = Fp<PP>;
  // ---- everything that is refused, before anything is allocated or launched
  if (ctx->cfg.zk) fail(P3R_EUNSUPPORTED, "the recurrence seam does not serve zk contexts (their traces are randomised and their domains doubled)");
  std::vector<size_t> widths(mats.size());
  for (size_t m = 0; m < mats.size(); ++m) widths[m] = mats[m]->w;
  const ScanPlan plan = scan_plan(recs, n_recs, widths.data(), widths.size(), DC, PP::P);   // n_mats == 0 is refused here
  const size_t h = mats[0]->h;
  scan_log_height(h, PP::TWO_ADICITY);
  for (size_t m = 0; m < mats.size(); ++m)
    if (mats[m]->h != h) fail(P3R_EINVAL, "matrix %zu has %zu rows, matrix 0 has %zu: the traces of one table share a height", m, mats[m]->h, h);
  const size_t W = plan.info.n_out_columns, n_tiles = scan_tiles(h);

  // ---- the launches
  std::unique_ptr<p3r_dmat> out = dmat_alloc(h, W);   // [W][h]
  const size_t agg_words = (size_t)3 * DC * n_tiles;  // per recurrence: the tiles' A, B and entering state
  DevBuf agg(n_recs * agg_words), d_last(n_recs * kAffMaxDC);
  std::vector<AffRec> host(n_recs);
  auto aligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  for (size_t i = 0; i < n_recs; ++i) {
    const p3r_recurrence& r = recs[i];
    AffRec& d = host[i];
    d = AffRec{};
    d.form = plan.form[i];
    if (d.form & AFF_MUL) d.a = mats[r.mul_mat]->d + (size_t)r.mul_col * h;
    if (d.form & AFF_ADD) d.b = mats[r.add_mat]->d + (size_t)r.add_col * h;
    d.out = out->d + (size_t)r.out_col * h;
    d.agg = agg.p + i * agg_words;
    d.last = d_last.p + i * kAffMaxDC;
    for (int k = 0; k < ((d.form & AFF_EXT) ? DC : 1); ++k) d.init[k] = F::from_canonical(r.init[k]).v;
    d.inclusive = (r.flags & P3R_SCAN_INCLUSIVE) ? 1u : 0u;
    d.vec = h % kAffItems == 0 && aligned(d.a) && aligned(d.b) && aligned(d.out);
  }
  DevBuf d_recs((n_recs * sizeof(AffRec) + 3) / 4);
  P3R_HIP(ctx->stage.upload(ctx->stream, d_recs.p, host.data(), n_recs * sizeof(AffRec)));
  {
    ProfScope ps(ctx, "affine_scan");
    // Rows i < h of columns [col, col + D) of the inputs are read and of the output written, col + D within the matrix's
    // width (scan_plan); a 16-byte access covers rows [i, i + 4) with i + 4 <= h.  Words word * n_tiles + tile with
    // word < 3 D <= 3 DC and tile < n_tiles of a recurrence's scratch and the kAffMaxDC words of its total are written:
    // all inside the allocations above.  Every column below W has one writer: nothing of the output stays uninitialised.
    const auto* dr = reinterpret_cast<const AffRec*>(d_recs.p);
    const dim3 tiles((unsigned)n_tiles, (unsigned)n_recs), one(1, (unsigned)n_recs);
    hipLaunchKernelGGL((k_affine_scan<PP, DC, 0>), tiles, dim3(kAffBlock), 0, ctx->stream, dr, h, n_tiles);
    hipLaunchKernelGGL((k_affine_scan<PP, DC, 1>), one, dim3(kAffBlock), 0, ctx->stream, dr, h, n_tiles);
    hipLaunchKernelGGL((k_affine_scan<PP, DC, 2>), tiles, dim3(kAffBlock), 0, ctx->stream, dr, h, n_tiles);
  }
  P3R_HIP(hipGetLastError());
  if (last_out) {
    std::vector<uint32_t> raw(n_recs * kAffMaxDC);
    P3R_HIP(fetch_small(ctx, d_last.p, raw.size(), raw.data()));   // waits for the stream
    for (size_t i = 0; i < n_recs; ++i)
      for (int k = 0; k < kAffMaxDC; ++k)
        last_out[i * kAffMaxDC + k] = k < ((plan.form[i] & AFF_EXT) ? DC : 1) ? F::raw(raw[i * kAffMaxDC + k]).to_canonical() : 0u;
  }
  // the scratch and the descriptors go back to the context's pool, which is ordered by the stream the launches are on
  return out;
}

// The constraint check (p3r_check_program_dmat): DebugConstraintBuilder / check_air_satisfies for constraints the caller
// brings as data.  One launch of k_trace_program<CheckProgSink>; the device answers with a first failing row and a count per constraint,
// from which the report is derived here.  A trace that fails is a result, not an error.  Waits for the stream.
template <class PP, int DC>
void check_program_dc(p3r_ctx* ctx, const p3r_air_insn* prog, size_t n_insns, const std::vector<const p3r_dmat*>& mats,
                      const uint32_t* publics, size_t n_public, const uint32_t* challenges, size_t n_challenges, p3r_check_report* report,
                      uint32_t* first_row_out, uint64_t* n_failed_out) {
  // ---- everything that is refused, before anything is allocated or launched
  if (ctx->cfg.zk) fail(P3R_EUNSUPPORTED, "the constraint check does not serve zk contexts (their traces are randomised and their domains doubled)");
  if (!report) fail(P3R_EINVAL, "report is NULL");
  const TraceProgram tp = trace_program<PP, DC>(prog, n_insns, mats, publics, n_public, challenges, n_challenges, AIR_MODE_CONSTRAINTS);
  const size_t nc = tp.plan.info.n_constraints;

  // ---- the launch
  const AirCompiled code = air_compile<PP>(tp.plan, prog, n_insns, tp.widths.data(), tp.widths.size(), DC, publics, challenges);
  // the answer leads the upload: a count (two words) per constraint, zero, then a first row per constraint, "none"
  ProgramBlob blob(12 * nc, code, mats, tp.n_cols);
  memset(blob.host.data() + 8 * nc, 0xff, 4 * nc);
  blob.upload(ctx);
  AirCheckArgs a{};
  a.prog = blob.stream();
  a.log_h = tp.log_h;
  a.n_failed = reinterpret_cast<unsigned long long*>(blob.base());
  a.first_row = blob.dev.p + 2 * nc;
  {
    ProfScope ps(ctx, "check_program");
    // rows r < h of every input column are read; constraint k < nc - the ASSERTs of the stream, which air_plan counted -
    // touches n_failed[k] and first_row[k]: all inside the allocations above
    launch_program(ctx, k_trace_program<PP, DC, CheckProgSink>, tp.h, tp.lds, a);
  }
  std::vector<uint32_t> answer(3 * nc);
  P3R_HIP(fetch_small(ctx, blob.dev.p, answer.size(), answer.data()));   // waits for the stream
  *report = p3r_check_report{0, 0xffffffffu, 0xffffffffu};
  for (size_t k = 0; k < nc; ++k) {
    const uint64_t failed = answer[2 * k] | ((uint64_t)answer[2 * k + 1] << 32);
    const uint32_t first = answer[2 * nc + k];
    report->n_failures += failed;
    if (first < report->first_row) {   // constraints in ascending order: the smallest of the row stays
      report->first_row = first;
      report->first_constraint = (uint32_t)k;
    }
    if (first_row_out) first_row_out[k] = first;
    if (n_failed_out) n_failed_out[k] = failed;
  }
}

// ---- the lookup check (p3r_lookup_check_dmat): p3_lookup::debug_util::check_lookups over lookup programs.
// Slots: term t of row r of instance p is slot base_p + r * n_terms_p + t; a slot whose multiplicity is not zero is a
// record, and ascending slots are record order.  After k_trace_program<RecordSink> the pass is the primitives of
// device_prims.hip.h and the few kernels below, which index by what those wrote.

// words [DC][n_slots] of the records at sorted positions i - 1 and i differ: i opens a key's run
template <int DC>
__global__ void __launch_bounds__(prims::kPB) k_lookup_heads(const uint32_t* __restrict__ den, size_t n_slots, const uint32_t* __restrict__ order,
                                                             size_t n, uint32_t* __restrict__ head) {
  const size_t i = (size_t)blockIdx.x * prims::kPB + threadIdx.x;
  if (i >= n) return;
  uint32_t differ = i == 0;
  if (i) {
    const size_t s = order[i], s_prev = order[i - 1];
#pragma unroll
    for (int k = 0; k < DC; ++k) differ |= den[(size_t)k * n_slots + s] != den[(size_t)k * n_slots + s_prev];
  }
  head[i] = differ ? 1u : 0u;
}
// the multiplicity word of coefficient k at a sorted position: what the exclusive sums run over
struct SortedWord {
  const uint32_t* words;   // one coefficient's [n_slots]
  const uint32_t* order;
  __device__ uint64_t operator()(size_t i) const { return words[order[i]]; }
};
// A key's run in the sorted records: head_rank[i] = the heads before position i and heads[j] = position of head j
// (select_marked over the head marks; the number of heads stands at head_rank[n]); prefix[k][i] = the canonical words of
// coefficient k before position i, n + 1 of them (ranks_of).
template <int DC>
struct LookupRuns {
  const uint32_t* head_rank;
  const uint32_t* heads;
  const uint64_t* prefix[DC];
  size_t n;
  // position one past the run that position `i` opens
  __device__ size_t end_of(size_t i) const {
    const uint32_t j = head_rank[i];
    return j + 1 < head_rank[n] ? heads[j + 1] : n;
  }
  // at most 2^28 words below 2^31 per coefficient: the sums stay below 2^59
  __device__ uint32_t net(int k, size_t i, size_t end, uint32_t p) const { return (uint32_t)((prefix[k][end] - prefix[k][i]) % p); }
};
template <int DC>
__global__ void __launch_bounds__(prims::kPB) k_lookup_flag(LookupRuns<DC> runs, const uint32_t* __restrict__ head, uint32_t p,
                                                            uint32_t* __restrict__ flag) {
  const size_t i = (size_t)blockIdx.x * prims::kPB + threadIdx.x;
  if (i >= runs.n) return;
  uint32_t unbalanced = 0;
  if (head[i]) {
    const size_t end = runs.end_of(i);
#pragma unroll
    for (int k = 0; k < DC; ++k) unbalanced |= runs.net(k, i, end, p);
  }
  flag[i] = unbalanced ? 1u : 0u;
}
constexpr int kImbalanceWords = 2 + 2 * kMaxAirDC;   // first slot, records, denominator, net
// entry j < n_out of the answer: the unbalanced key whose first record is slot first_slot[j], at sorted position pos[j]
template <int DC>
__global__ void __launch_bounds__(prims::kPB) k_lookup_report(LookupRuns<DC> runs, const uint32_t* __restrict__ den, size_t n_slots,
                                                              const uint32_t* __restrict__ first_slot, const uint32_t* __restrict__ pos,
                                                              size_t n_out, uint32_t p, uint32_t* __restrict__ out) {
  const size_t j = (size_t)blockIdx.x * prims::kPB + threadIdx.x;
  if (j >= n_out) return;
  const size_t i = pos[j], s = first_slot[j], end = runs.end_of(i);
  uint32_t* o = out + j * kImbalanceWords;
  o[0] = (uint32_t)s;
  o[1] = (uint32_t)(end - i);
#pragma unroll
  for (int k = 0; k < DC; ++k) {
    o[2 + k] = den[(size_t)k * n_slots + s];
    o[2 + kMaxAirDC + k] = runs.net(k, i, end, p);
  }
#pragma unroll
  for (int k = DC; k < kMaxAirDC; ++k) o[2 + k] = o[2 + kMaxAirDC + k] = 0u;
}

// the marked items of marks[0 .. n): their number (one blocking read) and their indices in ascending order
inline DevBuf marked_list(p3r_ctx* ctx, const uint32_t* marks, size_t n, DevBuf& rank /* n + 1 */, size_t* count) {
  *count = prims::select_marked_count(ctx->stream, marks, n, rank.p);
  DevBuf list(*count);
  if (*count) hipLaunchKernelGGL(prims::k_compact_marked, dim3(prims::blocks_of(n)), dim3(prims::kPB), 0, ctx->stream, marks, rank.p, n, list.p);
  P3R_HIP(hipGetLastError());
  return list;
}

// the same word with the slots below `floor` - the table's, in the join - counted as zero
struct SortedWordFrom {
  const uint32_t* words;
  const uint32_t* order;
  uint32_t floor;
  __device__ uint64_t operator()(size_t i) const {
    const uint32_t s = order[i];
    return s >= floor ? words[s] : 0u;
  }
};

// What the lookup check and the multiplicity join share: the instances validated and their slots numbered (plan), every
// term recorded, the records among the slots ordered by key (sorted_records), the head of every key's run marked and the
// exclusive sums of the multiplicity words taken over the sorted records (run_sums).  The entries differ in what they
// refuse about their own arguments, in what a run's head then does, and in their words.
struct LookupPassWords {
  const char *first, *rest;   // "instance" / "instance", or "table" / "query": how a refused instance is named
  const char* too_many;
  const char *scope_records, *scope_sort;
};
template <class PP, int DC>
struct LookupPass {
  std::vector<TraceProgram> tps;
  std::vector<size_t> base{0};   // first slot of every instance, and the total
  size_t S = 0, n = 0;           // slots, records
  DevBuf den, mul, order;        // [DC][S], [DC][S]; order[i]: the slot of the record at sorted position i
  DevBuf head, head_rank, heads, prefix[DC], no_sums;
  LookupRuns<DC> runs{};

  // ---- the refusals about the instances, before anything is allocated or launched
  void plan(const std::vector<LookupCheckInstance>& insts, const uint32_t* challenges, size_t n_challenges, const LookupPassWords& w,
            bool first_is_table) {
    for (size_t p = 0; p < insts.size(); ++p) {
      const LookupCheckInstance& in = insts[p];
      try {
        tps.push_back(trace_program<PP, DC>(in.prog, in.n_insns, in.mats, in.publics, in.n_public, challenges, n_challenges, AIR_MODE_LOOKUP));
      } catch (const Error& e) {
        if (first_is_table && p == 0) fail(e.code, "%s: %s", w.first, e.what());
        fail(e.code, "%s %zu: %s", w.rest, first_is_table ? p - 1 : p, e.what());
      }
      const size_t slots = tps[p].h * tps[p].plan.lookup.n_terms;   // below 2^27 * 2^31
      if (slots > P3R_LOOKUP_CHECK_MAX_RECORDS || base[p] + slots > P3R_LOOKUP_CHECK_MAX_RECORDS) fail(P3R_EUNSUPPORTED, "%s", w.too_many);
      base.push_back(base[p] + slots);
    }
    S = base.back();
  }

  // ---- the records (one launch per instance), then the records among the slots, ordered by key; n: their number
  void sorted_records(p3r_ctx* ctx, const std::vector<LookupCheckInstance>& insts, const uint32_t* challenges, const LookupPassWords& w) {
    hipStream_t s = ctx->stream;
    den.alloc((size_t)DC * S);
    mul.alloc((size_t)DC * S);
    DevBuf mark(S);
    {
      ProfScope ps(ctx, w.scope_records);
      for (size_t p = 0; p < insts.size(); ++p) {
        const LookupCheckInstance& in = insts[p];
        const TraceProgram& tp = tps[p];
        const AirCompiled code = air_compile<PP>(tp.plan, in.prog, in.n_insns, tp.widths.data(), tp.widths.size(), DC, in.publics, challenges);
        ProgramBlob blob(0, code, in.mats, tp.n_cols);
        blob.upload(ctx);
        AirRecordArgs a{};
        a.prog = blob.stream();
        a.log_h = tp.log_h;
        a.den = den.p;
        a.mul = mul.p;
        a.mark = mark.p;
        a.n_slots = S;
        a.base = base[p];
        a.n_terms = tp.plan.lookup.n_terms;
        // rows r < h of every input column are read; slot base + r * n_terms + t with r < h and t < n_terms - the TERMs of
        // the stream, which air_plan counted - lies in [base_p, base_p+1), so below S: words k * S + slot < DC * S of den and
        // mul and word slot of mark.  Every slot of the instance is written: nothing is read uninitialised afterwards.
        launch_program(ctx, k_trace_program<PP, DC, RecordSink>, tp.h, tp.lds, a);
      }
    }
    {
      DevBuf slot_rank(S + 1);
      order = marked_list(ctx, mark.p, S, slot_rank, &n);
    }
    mark.release();
    if (!n) return;
    const unsigned blocks_n = prims::blocks_of(n);
    ProfScope ps(ctx, w.scope_sort);
    // least significant word first, every word a canonical residue below 2^31; the sort is stable, so records of one key
    // stay in record order and the first of a run is the key's first record
    DevBuf keys(n), keys_sorted(n), order_next(n);
    for (int k = 0; k < DC; ++k) {
      hipLaunchKernelGGL(prims::k_gather_u32, dim3(blocks_n), dim3(prims::kPB), 0, s, den.p + (size_t)k * S, order.p, n, keys.p);
      prims::sort_pairs(s, keys.p, keys_sorted.p, order.p, order_next.p, n, 31);
      std::swap(order, order_next);
    }
    P3R_HIP(hipGetLastError());
  }

  // ---- the runs of equal keys and their sums (n > 0): the multiplicity words of coefficients k < n_words, with the slots
  // below `floor` counted as zero; the other coefficients sum to zero (their multiplicities are base values)
  void run_sums(p3r_ctx* ctx, int n_words, uint32_t floor) {
    hipStream_t s = ctx->stream;
    head.alloc(n);
    head_rank.alloc(n + 1);
    heads.alloc(n);
    hipLaunchKernelGGL((k_lookup_heads<DC>), dim3(prims::blocks_of(n)), dim3(prims::kPB), 0, s, den.p, S, order.p, n, head.p);
    prims::select_marked(s, head.p, n, head_rank.p, heads.p);   // as many heads as keys: the first of them are written
    runs.head_rank = head_rank.p;
    runs.heads = heads.p;
    runs.n = n;
    if (n_words < DC) {
      no_sums.alloc(2 * (n + 1));
      P3R_HIP(hipMemsetAsync(no_sums.p, 0, 8 * (n + 1), s));
    }
    for (int k = 0; k < DC; ++k) {
      if (k >= n_words) {
        runs.prefix[k] = reinterpret_cast<const uint64_t*>(no_sums.p);
        continue;
      }
      prefix[k].alloc(2 * (n + 1));
      uint64_t* pk = reinterpret_cast<uint64_t*>(prefix[k].p);
      if (floor) prims::ranks_of<uint64_t>(s, SortedWordFrom{mul.p + (size_t)k * S, order.p, floor}, n, pk);
      else prims::ranks_of<uint64_t>(s, SortedWord{mul.p + (size_t)k * S, order.p}, n, pk);
      runs.prefix[k] = pk;
    }
    P3R_HIP(hipGetLastError());
  }

  // ---- the keys at the marked heads flag[0 .. n), ordered by their first record: their number, and the first `cap` of them
  // as k_lookup_report writes them (waits for the stream)
  uint64_t report(p3r_ctx* ctx, const uint32_t* flag, size_t cap, std::vector<uint32_t>& answer) {
    hipStream_t s = ctx->stream;
    size_t nu = 0;
    DevBuf flag_rank(n + 1);
    DevBuf pos = marked_list(ctx, flag, n, flag_rank, &nu);   // sorted positions of the marked heads
    const size_t n_out = std::min(cap, nu);
    if (n_out) {
      DevBuf first_slot(nu), first_sorted(nu), pos_sorted(nu), d_answer(n_out * kImbalanceWords);
      hipLaunchKernelGGL(prims::k_gather_u32, dim3(prims::blocks_of(nu)), dim3(prims::kPB), 0, s, order.p, pos.p, nu, first_slot.p);
      prims::sort_pairs(s, first_slot.p, first_sorted.p, pos.p, pos_sorted.p, nu, 32);
      // j < n_out <= nu entries of first_sorted / pos_sorted are read, n_out * kImbalanceWords words written
      hipLaunchKernelGGL((k_lookup_report<DC>), dim3(prims::blocks_of(n_out)), dim3(prims::kPB), 0, s, runs, den.p, S, first_sorted.p,
                         pos_sorted.p, n_out, PP::P, d_answer.p);
      P3R_HIP(hipGetLastError());
      answer.resize(n_out * kImbalanceWords);
      P3R_HIP(fetch_small(ctx, d_answer.p, answer.size(), answer.data()));   // waits for the stream
    }
    return nu;
  }

  // the host's half of the report: slots back to (instance, row, term); first_instance: what instance 0 of the report is
  void entries(const std::vector<uint32_t>& answer, size_t first_instance, p3r_lookup_imbalance* out) const {
    for (size_t j = 0; j * kImbalanceWords < answer.size(); ++j) {   // at most `cap` entries: no loop over records
      const uint32_t* o = answer.data() + j * kImbalanceWords;
      const size_t p = (size_t)(std::upper_bound(base.begin(), base.end(), (size_t)o[0]) - base.begin()) - 1;
      const uint32_t n_terms = tps[p].plan.lookup.n_terms;
      p3r_lookup_imbalance& e = out[j];
      e.instance = (uint32_t)(p - first_instance);
      e.row = (uint32_t)((o[0] - base[p]) / n_terms);
      e.term = (uint32_t)((o[0] - base[p]) % n_terms);
      e.n_records = o[1];
      for (int k = 0; k < kMaxAirDC; ++k) {
        e.denominator[k] = o[2 + k];
        e.net[k] = o[2 + kMaxAirDC + k];
      }
    }
  }
};

template <class PP, int DC>
void lookup_check_dc(p3r_ctx* ctx, const std::vector<LookupCheckInstance>& insts, const uint32_t* challenges, size_t n_challenges,
                     p3r_lookup_imbalance* out, size_t cap, uint64_t* n_unbalanced_out) {
  // ---- everything that is refused, before anything is allocated or launched
  if (ctx->cfg.zk) fail(P3R_EUNSUPPORTED, "the lookup check does not serve zk contexts (their traces are randomised and their domains doubled)");
  if (insts.empty()) fail(P3R_EINVAL, "n_inst == 0: no table on the bus");
  if (!n_unbalanced_out) fail(P3R_EINVAL, "n_unbalanced_out is NULL");
  if (cap && !out) fail(P3R_EINVAL, "out is NULL with cap > 0");
  const LookupPassWords words{"instance", "instance",
                              "more than P3R_LOOKUP_CHECK_MAX_RECORDS (2^28) term slots: rows x terms, summed over the instances",
                              "lookup_check_records", "lookup_check_sort"};
  LookupPass<PP, DC> pass;
  pass.plan(insts, challenges, n_challenges, words, false);

  pass.sorted_records(ctx, insts, challenges, words);
  *n_unbalanced_out = 0;
  const size_t n = pass.n;
  if (!n) return;
  uint64_t n_unbalanced = 0;
  std::vector<uint32_t> answer;
  {
    ProfScope ps(ctx, "lookup_check_sums");
    pass.run_sums(ctx, DC, 0);
    DevBuf flag(n);
    hipLaunchKernelGGL((k_lookup_flag<DC>), dim3(prims::blocks_of(n)), dim3(prims::kPB), 0, ctx->stream, pass.runs, pass.head.p, PP::P, flag.p);
    P3R_HIP(hipGetLastError());
    n_unbalanced = pass.report(ctx, flag.p, cap, answer);   // the unbalanced heads, ordered by their first record
  }
  *n_unbalanced_out = n_unbalanced;
  pass.entries(answer, 0, out);
}

// ---- the multiplicity join (p3r_lookup_multiplicities_dmat): the column that balances a table against its queries.
// The table's slots are numbered first, and its enable flag is the record mark: the sort is stable, so the first table
// slot that offers a key heads the key's run, and a run headed by a query slot has no table slot in it.

// Sorted position i, if it heads a run: a table slot (below n_table) takes the run's sum - the table's own words count as
// zero in it - into its cell of the zeroed h x n_terms output (Montgomery, [term][row]); one head per run and one cell
// per slot, so every cell has at most one writer.  A query slot whose run does not cancel is flagged as a miss.
template <class PP, int DC>
__global__ void __launch_bounds__(prims::kPB) k_lookup_scatter(LookupRuns<DC> runs, const uint32_t* __restrict__ head,
                                                               const uint32_t* __restrict__ order, uint32_t n_table, uint32_t n_terms,
                                                               size_t h, uint32_t* __restrict__ out, uint32_t* __restrict__ flag) {
  const size_t i = (size_t)blockIdx.x * prims::kPB + threadIdx.x;
  if (i >= runs.n) return;
  uint32_t missing = 0;
  if (head[i]) {
    const uint32_t s = order[i];
    const uint32_t net = runs.net(0, i, runs.end_of(i), PP::P);
    if (s < n_table) out[(size_t)(s % n_terms) * h + s / n_terms] = Fp<PP>::from_canonical(net).v;   // s < n_table = h * n_terms
    else missing = net != 0;
  }
  flag[i] = missing;
}

template <class PP, int DC>
std::unique_ptr<p3r_dmat> lookup_multiplicities_dc(p3r_ctx* ctx, const std::vector<LookupCheckInstance>& insts, const uint32_t* challenges,
                                                   size_t n_challenges, p3r_lookup_imbalance* missing, size_t cap, uint64_t* n_missing_out) {
  // ---- everything that is refused, before anything is allocated or launched.  insts[0] is the table.
  if (ctx->cfg.zk)
    fail(P3R_EUNSUPPORTED, "the multiplicity join does not serve zk contexts (their traces are randomised and their domains doubled)");
  if (!n_missing_out) fail(P3R_EINVAL, "n_missing_out is NULL");
  if (cap && !missing) fail(P3R_EINVAL, "missing is NULL with cap > 0");
  const LookupPassWords words{"table", "query",
                              "more than P3R_LOOKUP_CHECK_MAX_RECORDS (2^28) term slots: rows x terms, summed over the table and the queries",
                              "lookup_mult_records", "lookup_mult_sort"};
  LookupPass<PP, DC> pass;
  pass.plan(insts, challenges, n_challenges, words, true);
  for (size_t q = 1; q < insts.size(); ++q)
    for (size_t i = 0; i < insts[q].n_insns; ++i)
      if (insts[q].prog[i].op == P3R_AIR_LOOKUP && pass.tps[q].plan.is_ext[insts[q].prog[i].a])
        fail(P3R_EUNSUPPORTED, "query %zu: instruction %zu: a multiplicity of extension type; the column of counts is a base column", q - 1, i);
  const size_t h = pass.tps[0].h, n_terms = pass.tps[0].plan.lookup.n_terms, n_table = pass.base[1];

  hipStream_t s = ctx->stream;
  std::unique_ptr<p3r_dmat> out = dmat_alloc(h, n_terms);   // [n_terms][h]
  P3R_HIP(hipMemsetAsync(out->d, 0, 4 * h * n_terms, s));
  *n_missing_out = 0;
  pass.sorted_records(ctx, insts, challenges, words);
  const size_t n = pass.n;
  if (!n) {
    P3R_HIP(hipStreamSynchronize(s));
    return out;
  }
  uint64_t n_missing = 0;
  std::vector<uint32_t> answer;
  {
    ProfScope ps(ctx, "lookup_mult_sums");
    pass.run_sums(ctx, 1, (uint32_t)n_table);
  }
  {
    ProfScope ps(ctx, "lookup_mult_scatter");
    DevBuf flag(n);
    // order[i] < S; a head below n_table = h * n_terms writes word (s % n_terms) * h + s / n_terms < n_terms * h of the output
    hipLaunchKernelGGL((k_lookup_scatter<PP, DC>), dim3(prims::blocks_of(n)), dim3(prims::kPB), 0, s, pass.runs, pass.head.p, pass.order.p,
                       (uint32_t)n_table, (uint32_t)n_terms, h, out->d, flag.p);
    P3R_HIP(hipGetLastError());
    n_missing = pass.report(ctx, flag.p, cap, answer);   // the misses, ordered by their first record; waits for the stream
  }
  *n_missing_out = n_missing;
  pass.entries(answer, 1, missing);
  return out;
}

}  // namespace

template <class PP>
std::unique_ptr<p3r_dmat> logup_program(p3r_ctx* ctx, const p3r_air_insn* prog, size_t n_insns, const std::vector<const p3r_dmat*>& mats,
                                        const uint32_t* publics, size_t n_public, const uint32_t* challenges, size_t n_challenges,
                                        uint32_t* sum_out) {
  return with_challenge_degree<PP>(ctx, [&](auto dc) {
    return logup_program_dc<PP, decltype(dc)::value>(ctx, prog, n_insns, mats, publics, n_public, challenges, n_challenges, sum_out);
  });
}

template <class PP>
std::vector<std::unique_ptr<p3r_dmat>> quotient_program(p3r_ctx* ctx, const p3r_air_insn* prog, size_t n_insns,
                                                        const std::vector<const p3r_dmat*>& mats, uint32_t added_bits, uint32_t shift,
                                                        uint32_t log_quotient_degree, const uint32_t* publics, size_t n_public,
                                                        const uint32_t* challenges, size_t n_challenges, const uint32_t* alpha) {
  return with_challenge_degree<PP>(ctx, [&](auto dc) {
    return quotient_program_dc<PP, decltype(dc)::value>(ctx, prog, n_insns, mats, added_bits, shift, log_quotient_degree, publics, n_public,
                                                        challenges, n_challenges, alpha);
  });
}

template <class PP>
void check_program(p3r_ctx* ctx, const p3r_air_insn* prog, size_t n_insns, const std::vector<const p3r_dmat*>& mats, const uint32_t* publics,
                   size_t n_public, const uint32_t* challenges, size_t n_challenges, p3r_check_report* report, uint32_t* first_row_out,
                   uint64_t* n_failed_out) {
  with_challenge_degree<PP>(ctx, [&](auto dc) {
    check_program_dc<PP, decltype(dc)::value>(ctx, prog, n_insns, mats, publics, n_public, challenges, n_challenges, report, first_row_out,
                                              n_failed_out);
  });
}

template <class PP>
void lookup_check(p3r_ctx* ctx, const std::vector<LookupCheckInstance>& insts, const uint32_t* challenges, size_t n_challenges,
                  p3r_lookup_imbalance* out, size_t cap, uint64_t* n_unbalanced_out) {
  with_challenge_degree<PP>(ctx, [&](auto dc) { lookup_check_dc<PP, decltype(dc)::value>(ctx, insts, challenges, n_challenges, out, cap, n_unbalanced_out); });
}

template <class PP>
std::unique_ptr<p3r_dmat> lookup_multiplicities(p3r_ctx* ctx, const std::vector<LookupCheckInstance>& insts, const uint32_t* challenges,
                                                size_t n_challenges, p3r_lookup_imbalance* missing, size_t cap, uint64_t* n_missing_out) {
  return with_challenge_degree<PP>(ctx, [&](auto dc) {
    return lookup_multiplicities_dc<PP, decltype(dc)::value>(ctx, insts, challenges, n_challenges, missing, cap, n_missing_out);
  });
}

template <class PP>
std::unique_ptr<p3r_dmat> witness_program(p3r_ctx* ctx, const p3r_air_insn* prog, size_t n_insns, const std::vector<const p3r_dmat*>& mats,
                                          size_t height, const uint32_t* publics, size_t n_public, const uint32_t* challenges,
                                          size_t n_challenges) {
  return with_challenge_degree<PP>(ctx, [&](auto dc) {
    return witness_program_dc<PP, decltype(dc)::value>(ctx, prog, n_insns, mats, height, publics, n_public, challenges, n_challenges);
  });
}

template <class PP>
std::unique_ptr<p3r_dmat> affine_scan(p3r_ctx* ctx, const p3r_recurrence* recs, size_t n_recs, const std::vector<const p3r_dmat*>& mats,
                                      uint32_t* last_out) {
  return with_challenge_degree<PP>(ctx, [&](auto dc) { return affine_scan_dc<PP, decltype(dc)::value>(ctx, recs, n_recs, mats, last_out); });
}

#define P3R_AIR_INSTANCE(PP)                                                                                                               \
  template std::vector<std::unique_ptr<p3r_dmat>> quotient_program<PP>(p3r_ctx*, const p3r_air_insn*, size_t,                              \
                                                                       const std::vector<const p3r_dmat*>&, uint32_t, uint32_t, uint32_t,  \
                                                                       const uint32_t*, size_t, const uint32_t*, size_t, const uint32_t*); \
  template std::unique_ptr<p3r_dmat> logup_program<PP>(p3r_ctx*, const p3r_air_insn*, size_t, const std::vector<const p3r_dmat*>&,         \
                                                       const uint32_t*, size_t, const uint32_t*, size_t, uint32_t*);                       \
  template void check_program<PP>(p3r_ctx*, const p3r_air_insn*, size_t, const std::vector<const p3r_dmat*>&, const uint32_t*, size_t,     \
                                  const uint32_t*, size_t, p3r_check_report*, uint32_t*, uint64_t*);                                       \
  template void lookup_check<PP>(p3r_ctx*, const std::vector<LookupCheckInstance>&, const uint32_t*, size_t, p3r_lookup_imbalance*,        \
                                 size_t, uint64_t*);                                                                                       \
  template std::unique_ptr<p3r_dmat> lookup_multiplicities<PP>(p3r_ctx*, const std::vector<LookupCheckInstance>&, const uint32_t*, size_t, \
                                                               p3r_lookup_imbalance*, size_t, uint64_t*);                                  \
  template std::unique_ptr<p3r_dmat> witness_program<PP>(p3r_ctx*, const p3r_air_insn*, size_t, const std::vector<const p3r_dmat*>&,       \
                                                         size_t, const uint32_t*, size_t, const uint32_t*, size_t);                        \
  template std::unique_ptr<p3r_dmat> affine_scan<PP>(p3r_ctx*, const p3r_recurrence*, size_t, const std::vector<const p3r_dmat*>&,         \
                                                     uint32_t*);
P3R_AIR_INSTANCE(KoalaBearParams)
P3R_AIR_INSTANCE(BabyBearParams)
#undef P3R_AIR_INSTANCE

}  // namespace p3r
