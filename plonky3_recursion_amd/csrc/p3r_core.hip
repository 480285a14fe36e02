// C ABI (include/p3r.h): context, device matrices, Poseidon2 (K3), coset LDE (K5), MMCS (K6: mmcs_impl.hip.h).
// Host orchestration only; all arithmetic on data runs in the gfx950 kernels of kernels.hip.h.
#include "context.h"
#include "kernels.hip.h"
#include "kernels_stark.hip.h"
#include "kernels_coop.hip.h"
#include "tu_api.h"
#include "air_program.h"
#include "scan_plan.h"
#include "air_program_eval.h"
#include "profile.h"
#include "run_schedule.h"
#include "prep_device.h"
#include "host_abi.h"

#include <sys/random.h>

#include <algorithm>
#include <cerrno>
#include <future>
#include <numeric>
#include <unordered_map>

using namespace p3r;

namespace {

template <class Fn>
int guard(p3r_ctx* ctx, Fn&& fn) {
  try {
    // the calling thread's current device may have been changed by the embedding framework
    if (ctx) {
      (void)hipSetDevice(ctx->cfg.device);
      tls_pool() = ctx->pool;
      // the table cache is only trimmed here, between API calls: a call keeps device pointers into
      // it while it assembles its launches (e.g. column tables referenced from a job list)
      if (ctx->const_tables.size() > 4096) ctx->const_tables.clear();
    }
    fn();
    return P3R_OK;
  } catch (const Error& e) {
    if (ctx) ctx->err = e.what(); else g_create_error = e.what();
    return e.code;
  } catch (const std::exception& e) {
    if (ctx) ctx->err = e.what(); else g_create_error = e.what();
    return P3R_EINVAL;
  }
}

// the width-32 permutation is about to be used: its constants must be the caller's, or acknowledged as unpinned (p3r.h)
inline void require_w32_constants(const p3r_ctx* ctx) {
  if (ctx->w32_unacknowledged)
    fail(P3R_EINVAL, "the width-32 permutation with poseidon2_w32_rc / poseidon2_w32_diag NULL: the built-in constants are self-generated, "
                     "not upstream's - pass the caller's, or acknowledge with P3R_EXT_UNPINNED_W32_DEFAULTS");
}

#define P3R_FIELD_CALL(ctx, fn, ...)                                              \
  ((ctx)->cfg.field == P3R_FIELD_KOALA_BEAR ? fn<KoalaBearParams>(__VA_ARGS__)    \
                                            : fn<BabyBearParams>(__VA_ARGS__))

inline unsigned blocks_for(size_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// ------------------------------------------------------------------ matrices
template <class PP>
std::unique_ptr<p3r_dmat> upload(p3r_ctx* ctx, const uint32_t* rowmajor, size_t h, size_t w) {
  log2_exact(h, "matrix height");
  if (w == 0) fail(P3R_EINVAL, "matrix width must be positive");
  auto m = std::make_unique<p3r_dmat>();
  m->buf.alloc(h * w);
  m->d = m->buf.p;
  m->h = h;
  m->w = w;
  DevBuf stage(h * w);
  P3R_HIP(hipMemcpyAsync(stage.p, rowmajor, h * w * 4, hipMemcpyHostToDevice, ctx->stream));
  dim3 grid((unsigned)((h + 63) / 64), (unsigned)((w + 63) / 64));
  hipLaunchKernelGGL(k_rowmajor_to_colmajor<PP>, grid, dim3(kBlock), 0, ctx->stream, stage.p,
                     m->d, (uint32_t)h, (uint32_t)w, 1);
  P3R_HIP(hipGetLastError());
  // the caller's (pageable) host buffer must be fully consumed before we return
  P3R_HIP(hipStreamSynchronize(ctx->stream));
  return m;
}

template <class PP>
void download(p3r_ctx* ctx, const p3r_dmat* m, uint32_t* rowmajor_out) {
  DevBuf stage(m->h * m->w);
  dim3 grid((unsigned)((m->h + 63) / 64), (unsigned)((m->w + 63) / 64));
  hipLaunchKernelGGL(k_colmajor_to_rowmajor<PP>, grid, dim3(kBlock), 0, ctx->stream, m->d,
                     stage.p, (uint32_t)m->h, (uint32_t)m->w, 1);
  P3R_HIP(hipGetLastError());
  P3R_HIP(hipMemcpyAsync(rowmajor_out, stage.p, m->h * m->w * 4, hipMemcpyDeviceToHost,
                         ctx->stream));
  P3R_HIP(hipStreamSynchronize(ctx->stream));
}


// ------------------------------------------------------------------ Poseidon2
template <class PP>
void permute_dmat(p3r_ctx* ctx, p3r_dmat* s) {
  if (s->w != P2_WIDTH) fail(P3R_EINVAL, "state matrix must have width 16, got %zu", s->w);
  ProfScope ps(ctx, "p2_permute_batch");
  hipLaunchKernelGGL(k_p2_permute_batch<PP>, dim3(blocks_for(s->h)), dim3(kBlock), 0, ctx->stream,
                     s->d, s->d, s->h, ctx->rcd());
  P3R_HIP(hipGetLastError());
}

// Device-resident Poseidon2CircuitRow batch (inputs column-major Montgomery, flags as bytes).
template <class PP>
std::unique_ptr<p3r_p2_dev> p2_rows_upload(p3r_ctx* ctx, const p3r_p2_rows* rows) {
  const size_t n = rows->n;
  log2_exact(n, "Poseidon2 row count (callers pad to a power of two)");
  if (!rows->input_values || !rows->new_start || !rows->merkle_path || !rows->mmcs_bit ||
      !rows->mmcs_index_sum)
    fail(P3R_EINVAL, "p3r_p2_rows has a NULL field");
  auto d = std::make_unique<p3r_p2_dev>();
  d->n = n;
  d->flags.alloc((3 * n + 3) / 4 + 1);
  uint8_t* f8 = reinterpret_cast<uint8_t*>(d->flags.p);
  P3R_HIP(hipMemcpyAsync(f8, rows->new_start, n, hipMemcpyHostToDevice, ctx->stream));
  P3R_HIP(hipMemcpyAsync(f8 + n, rows->merkle_path, n, hipMemcpyHostToDevice, ctx->stream));
  P3R_HIP(hipMemcpyAsync(f8 + 2 * n, rows->mmcs_bit, n, hipMemcpyHostToDevice, ctx->stream));
  d->seed.alloc(n);
  P3R_HIP(hipMemcpyAsync(d->seed.p, rows->mmcs_index_sum, n * 4, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_convert_inplace<PP>, dim3(blocks_for(n)), dim3(kBlock), 0, ctx->stream,
                     d->seed.p, n, 1);
  P3R_HIP(hipGetLastError());
  d->inputs = upload<PP>(ctx, rows->input_values, n, P2_WIDTH);  // syncs the stream
  return d;
}

template <class PP>
std::unique_ptr<p3r_dmat> trace_fill(p3r_ctx* ctx, const p3r_p2_dev* rows) {
  const size_t n = rows->n;
  const uint8_t* f8 = reinterpret_cast<const uint8_t*>(rows->flags.p);
  DevBuf acc(n);
  const size_t n_blocks = (n + kScanTile - 1) / kScanTile;
  DevBuf agg(2 * n_blocks);
  {
    ProfScope ps(ctx, "p2_acc_scan");
    hipLaunchKernelGGL(k_p2_acc_scan<PP>, dim3((unsigned)n_blocks), dim3(kBlock), 0, ctx->stream, 0,
                       n, f8, f8 + n, f8 + 2 * n, rows->seed.p, agg.p, n_blocks, acc.p);
    hipLaunchKernelGGL(k_p2_acc_scan<PP>, dim3(1), dim3(kBlock), 0, ctx->stream, 1, n, f8, f8 + n,
                       f8 + 2 * n, rows->seed.p, agg.p, n_blocks, acc.p);
    hipLaunchKernelGGL(k_p2_acc_scan<PP>, dim3((unsigned)n_blocks), dim3(kBlock), 0, ctx->stream, 2,
                       n, f8, f8 + n, f8 + 2 * n, rows->seed.p, agg.p, n_blocks, acc.p);
  }
  const size_t width = p2_perm_cols<PP>() + 2;
  auto trace = dmat_alloc(n, width);
  {
    ProfScope ps(ctx, "p2_trace_fill");
    hipLaunchKernelGGL(k_p2_trace_fill<PP>, dim3(blocks_for(n)), dim3(kBlock), 0, ctx->stream,
                       rows->inputs->d, f8 + 2 * n, acc.p, trace->d, n, ctx->rc.p);
  }
  P3R_HIP(hipGetLastError());
  return trace;
}

// width-32 permutation over n row-major states (canonical in / out): the unit seam of p3r_poseidon2_w32_permute_batch
template <class PP>
__global__ void __launch_bounds__(kBlock) k_p2w_permute_rows(uint32_t* __restrict__ s, size_t n, const uint32_t* __restrict__ rcw) {
  using F = Fp<PP>;
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  F x[P2W_WIDTH];
#pragma unroll
  for (int k = 0; k < P2W_WIDTH; ++k) x[k] = F::from_canonical(s[i * P2W_WIDTH + k]);
  P2NullSink sink;
  p2w_permute_traced<PP>(x, rcw, sink);
#pragma unroll
  for (int k = 0; k < P2W_WIDTH; ++k) s[i * P2W_WIDTH + k] = x[k].to_canonical();
}
template <class PP>
void permute_w32_rows(p3r_ctx* ctx, uint32_t* d, size_t n) {
  hipLaunchKernelGGL(k_p2w_permute_rows<PP>, dim3(blocks_for(n)), dim3(kBlock), 0, ctx->stream, d, n, ctx->rc.p + p2_num_constants<PP>());
  P3R_HIP(hipGetLastError());
}

// ------------------------------------------------------------------ coset LDE (tu_lde.hip)
template <class PP>
std::unique_ptr<p3r_dmat> coset_lde(p3r_ctx* ctx, const p3r_dmat* in, int added_bits, uint32_t shift) {
  return std::move(coset_lde_batch<PP>(ctx, {{in, shift}}, added_bits)[0]);
}

// ------------------------------------------------------------------ context
template <class PP>
void init_ctx(p3r_ctx* ctx) {
  using F = Fp<PP>;
  const size_t nrc = p2_num_constants<PP>();
  const std::vector<uint32_t> table = constants_table<PP>(ctx->cfg, [](const char* what, uint32_t got, size_t want) {
    fail(P3R_EINVAL, "%s is %u, the field needs %zu constants", what, got, want);
  });
  const uint32_t* src = table.data();
  ctx->rc_canonical = table;   // width-16 constants first (nrc of them), then the width-32 table
  std::vector<uint32_t> mont(table.size());
  for (size_t i = 0; i < table.size(); ++i) {
    if (table[i] >= PP::P) fail(P3R_EINVAL, "permutation constant %zu is not canonical", i);
    mont[i] = F::from_canonical(table[i]).v;
  }
  ctx->rc_mont_host = mont;
  ctx->rc.alloc(mont.size());
  P3R_HIP(copy_sync(ctx->stream, ctx->rc.p, mont.data(), mont.size() * 4, hipMemcpyHostToDevice));
  // FP64 tables: the width-16 round constants, then the width-32 table of poseidon2_w32_f64.hip.h (round constants |
  // the diagonal as centred integers | diagonal / P)
  std::vector<double> rcd(src, src + nrc);
  ctx->rcd_w32_at = nrc;
  {
    const size_t nrcw = p2w_num_rc<PP>();
    const uint32_t* w = src + nrc;
    rcd.insert(rcd.end(), w, w + nrcw);
    for (int i = 0; i < P2W_WIDTH; ++i) {
      const uint32_t d = w[nrcw + i];
      rcd.push_back(d > PP::P / 2 ? (double)d - (double)PP::P : (double)d);
    }
    // the kernels have the lane forms of the BUILT-IN diagonal compiled in: those instances are launched when the
    // configured diagonal is the built-in one, entry by entry (poseidon2_w32_f64.hip.h); any other diagonal is data
    const uint32_t* builtin = PP::FIELD_ID == 0 ? kDefaultDiagW32_koala_bear : kDefaultDiagW32_baby_bear;
    const bool is_builtin = std::equal(builtin, builtin + P2W_WIDTH, w + nrcw) && !tuning_knob("P3R_W32_GENERAL_DIAG");
    ctx->w32_diag_builtin = is_builtin;
  }
  ctx->rc_f64.alloc(2 * rcd.size());
  P3R_HIP(copy_sync(ctx->stream, ctx->rc_f64.p, rcd.data(), rcd.size() * 8, hipMemcpyHostToDevice));
  {
    auto inv2k = [](int k) { return F::from_u64(uint64_t(1) << k).inv(); };
    const F two = F::from_canonical(2), three = F::from_canonical(3), four = F::from_canonical(4);
    F d[16] = {-two, F::one(), two, inv2k(1), three, four, -inv2k(1), -three, -four, inv2k(8), inv2k(3), inv2k(24),
               -inv2k(8), -inv2k(3), -inv2k(4), -inv2k(24)};
    if (PP::FIELD_ID == 1) {
      F b[16] = {-two, F::one(), two, inv2k(1), three, four, -inv2k(1), -three, -four, inv2k(8), inv2k(2), inv2k(3),
                 inv2k(27), -inv2k(8), -inv2k(4), -inv2k(27)};
      for (int i = 0; i < 16; ++i) d[i] = b[i];
    }
    uint32_t dm[16];
    for (int i = 0; i < 16; ++i) dm[i] = d[i].v;
    ctx->p2_diag.alloc(16);
    P3R_HIP(copy_sync(ctx->stream, ctx->p2_diag.p, dm, sizeof dm, hipMemcpyHostToDevice));
  }
  ctx->partial_rounds = PP::PARTIAL_ROUNDS;
  ctx->cfg.poseidon2_rc = nullptr;  // caller's pointers are not retained
  ctx->w32_unacknowledged = (!ctx->cfg.poseidon2_w32_rc || !ctx->cfg.poseidon2_w32_diag) && !(ctx->cfg.ext_choices & P3R_EXT_UNPINNED_W32_DEFAULTS);
  if (ctx->w32_unacknowledged && ctx->cfg.mmcs_arity == 4)
    fail(P3R_EINVAL, "mmcs_arity = 4 with poseidon2_w32_rc / poseidon2_w32_diag NULL: the built-in width-32 constants are self-generated, "
                     "not upstream's - pass the caller's, or acknowledge with P3R_EXT_UNPINNED_W32_DEFAULTS");
  ctx->cfg.poseidon2_w32_rc = nullptr;
  ctx->cfg.poseidon2_w32_diag = nullptr;
  if (ctx->cfg.fri_log_arities) ctx->fri_log_arities.assign(ctx->cfg.fri_log_arities, ctx->cfg.fri_log_arities + ctx->cfg.fri_log_arities_len);
  ctx->cfg.fri_log_arities = nullptr;
  if (!ctx->proof_layout.set(ctx->cfg.proof_layout, ctx->cfg.proof_layout_len))
    fail(P3R_EINVAL, "proof_layout must be 18 bytes: three permutations batch[5] | fri[5] | opened[8]");
  ctx->cfg.proof_layout = nullptr;
  lde_init<PP>(ctx);
}

}  // namespace

#include "mmcs_impl.hip.h"
#include "prove_impl.hip.h"
#include "layer_impl.hip.h"
#include "circuit_impl.hip.h"

namespace {
// MMCS commit as the ABI hands the cap out: canonical.  Under a hiding MMCS (p3r_config.mmcs_salt_elems > 0) the tree
// commits [M0, S0, M1, S1, ..] as the prover's trees do (commit_dmats), with salts of its own: the key of the next proof
// counter value - a public commit takes one, as a proof does - on a stream round no proof draws from.
template <class PP>
void mmcs_commit_canonical(p3r_ctx* ctx, p3r_tree* tree, uint32_t* cap_out) {
  const size_t S = ctx->cfg.mmcs_salt_elems, n_mats = tree->mats.size();
  if (S) {
    const std::vector<const p3r_dmat*> mats = tree->mats;
    for (const p3r_dmat* m : mats) log2_exact(m->h, "matrix height");
    const ZkKey key = zk_key_of(ctx, ctx->zk_nonce++);
    tree->salt_elems = (int)S;
    tree->salt_owned = draw_salts<PP>(ctx, mats, kSaltRound + ZK_ROUND_PUBLIC_COMMIT, key);
    tree->mats.clear();
    for (size_t i = 0; i < n_mats; ++i) { tree->mats.push_back(mats[i]); tree->mats.push_back(tree->salt_owned[i].get()); }
  }
  const std::vector<uint32_t> cap = mmcs_commit<PP>(ctx, tree);
  tree->total_width -= n_mats * S;  // words of opened_values per index: the caller's widths, without the salts
  for (size_t i = 0; i < cap.size(); ++i) cap_out[i] = Fp<PP>::raw(cap[i]).to_canonical();
}

// p3r_fri_final_poly_dmat: the prover's final polynomial of a caller's last folded vector, canonical
template <class PP, int DC>
void fri_final_poly_dc(p3r_ctx* ctx, const p3r_dmat* vec, uint32_t lf, uint32_t* coeffs_out) {
  if (vec->w != (size_t)DC) fail(P3R_EINVAL, "the folded vector must be %d words wide (it is %zu)", DC, vec->w);
  const int log_m = log2_exact(vec->h, "height of the last folded vector");
  if (log_m > 16) fail(P3R_EINVAL, "the last folded vector has 2^%d rows: the final polynomial is formed on the host, from at most 2^16", log_m);
  if (lf > (uint32_t)log_m) fail(P3R_EINVAL, "the last folded vector has 2^%d rows, fewer than the 2^%u coefficients asked for", log_m, lf);
  std::vector<uint32_t> raw((size_t)DC << log_m);
  P3R_HIP(fetch_small(ctx, vec->d, raw.size(), raw.data()));
  const auto coeffs = fri_final_poly<PP, DC>(raw.data(), log_m, lf);
  for (size_t i = 0; i < coeffs.size(); ++i)
    for (int k = 0; k < DC; ++k) coeffs_out[i * DC + k] = coeffs[i].c[k].to_canonical();
}
template <class PP>
void fri_final_poly_canonical(p3r_ctx* ctx, const p3r_dmat* vec, uint32_t lf, uint32_t* coeffs_out) {
  if (ctx->cfg.challenge_degree == 5) {
    if constexpr (kHasQuintic<PP>) return fri_final_poly_dc<PP, 5>(ctx, vec, lf, coeffs_out);
    else fail(P3R_EUNSUPPORTED, "UnsupportedChallengeDegree: the quintic challenge field is KoalaBear's");
  }
  fri_final_poly_dc<PP, 4>(ctx, vec, lf, coeffs_out);
}
}  // namespace

// =============================================================================== C ABI
extern "C" {

p3r_ctx* p3r_create(const p3r_config* cfg) {
  p3r_ctx* ctx = nullptr;
  int rc = guard(nullptr, [&] {
    if (!cfg) fail(P3R_EINVAL, "cfg is NULL");
    if (cfg->abi_version != P3R_ABI_VERSION)
      fail(P3R_EINVAL, "abi_version %u != %u", cfg->abi_version, P3R_ABI_VERSION);
    if (cfg->field != P3R_FIELD_KOALA_BEAR && cfg->field != P3R_FIELD_BABY_BEAR)
      fail(P3R_EUNSUPPORTED, "unsupported field id %u", cfg->field);
    // circuit extension degree: 4 (binomial) on both fields; 5 = the KoalaBear quintic trinomial extension, proved
    // under the same D = 4 STARK configuration (batch_stark_prover/tests.rs:844-1029), primitive tables only
    if (cfg->mmcs_arity != 0 && cfg->mmcs_arity != 2 && cfg->mmcs_arity != 4)
      fail(P3R_EINVAL, "mmcs_arity must be 2 or 4 (got %u)", cfg->mmcs_arity);
    // the cap of an arity-4 tree strips whole compression steps (recursion/src/pcs/mmcs.rs:1143-1156); the reference's
    // arity-4 configurations run with the default cap_height 0 (recursive_aggregation.rs:77), and only that is built
    if (cfg->mmcs_arity == 4 && cfg->cap_height != 0) fail(P3R_EUNSUPPORTED, "arity-4 MMCS: cap_height must be 0");
    if (cfg->zk > 1) fail(P3R_EINVAL, "zk must be 0 or 1 (got %u)", cfg->zk);
    if (cfg->zk && cfg->num_random_codewords > 8) fail(P3R_EINVAL, "num_random_codewords must be in 1..8 (0 selects 2)");
    if (cfg->challenge_degree != 0 && cfg->challenge_degree != 4 &&
        !(cfg->challenge_degree == 5 && cfg->field == P3R_FIELD_KOALA_BEAR))
      fail(P3R_EUNSUPPORTED, "UnsupportedChallengeDegree(%u): 4, or 5 over KoalaBear", cfg->challenge_degree);
    if (p3r::ext_degree_is_binomial_generic(cfg->ext_degree)) {
      // binomial extension x^D = W of degree 2 / 6 / 8: W is the caller's (BinomiallyExtendable<D>::W of its field
      // crate; the proof carries it as w_binomial)
      const uint32_t P = cfg->field == P3R_FIELD_KOALA_BEAR ? p3r::KoalaBearParams::P : p3r::BabyBearParams::P;
      if (cfg->ext_w == 0 || cfg->ext_w >= P) fail(P3R_EINVAL, "MissingWForExtension: ext_degree %u needs ext_w in 1..p-1", cfg->ext_degree);
    } else if (cfg->ext_degree != 1 && cfg->ext_degree != 4 && !(cfg->ext_degree == 5 && cfg->field == P3R_FIELD_KOALA_BEAR))
      fail(P3R_EUNSUPPORTED, "UnsupportedExtDegree(%u): 1, 2, 4, 6, 8, or 5 over KoalaBear", cfg->ext_degree);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
      fail(P3R_ENODEV, "no HIP device available (%s); this library has no CPU fallback",
           e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (cfg->device < 0 || cfg->device >= ndev)
      fail(P3R_ENODEV, "device %d out of range (%d devices)", cfg->device, ndev);
    P3R_HIP(hipSetDevice(cfg->device));
    auto c = std::make_unique<p3r_ctx>();
    c->cfg = *cfg;
    tls_pool() = c->pool;
    P3R_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    {
      int cus = 0;
      if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg->device) == hipSuccess && cus > 0) c->n_cus = cus;
    }
    if (cfg->mmcs_salt_elems > 16) fail(P3R_EINVAL, "mmcs_salt_elems must be in 0..16 (got %u)", cfg->mmcs_salt_elems);
    if (cfg->zk || cfg->mmcs_salt_elems) {
      // the key the context draws its masks (and the salts of a hiding MMCS) with (zk_rand.h): the caller's, mixed with 128 bits of operating-system
      // entropy unless reproducible proofs were asked for
      uint32_t entropy[4] = {0, 0, 0, 0};
      const bool deterministic = cfg->ext_choices & P3R_EXT_ZK_DETERMINISTIC;
      if (!deterministic) {
        size_t got = 0;
        while (got < sizeof entropy) {
          const ssize_t r = getrandom(reinterpret_cast<uint8_t*>(entropy) + got, sizeof entropy - got, 0);
          if (r < 0) { if (errno == EINTR) continue; fail(P3R_EHIP, "getrandom failed (errno %d): no entropy for the ZK key", errno); }
          got += (size_t)r;
        }
      }
      zk_context_key(cfg->zk_key, entropy, deterministic, c->zk_key);
    }
    P3R_FIELD_CALL(c, init_ctx, c.get());
    ctx = c.release();
  });
  return rc == P3R_OK ? ctx : nullptr;
}

void p3r_destroy(p3r_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->cfg.device);
  (void)hipStreamSynchronize(ctx->stream);
  prof_clear(ctx);
  (void)hipStreamDestroy(ctx->stream);
  std::shared_ptr<DevPool> pool = ctx->pool;
  delete ctx;
  pool->trim();  // cached blocks go back to the driver; blocks still owned by live objects follow later
  if (tls_pool() == pool) tls_pool().reset();
}

const char* p3r_last_error(const p3r_ctx* ctx) {
  return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

uint32_t p3r_poseidon2_trace_width(const p3r_ctx* ctx) {
  return ctx->cfg.field == P3R_FIELD_KOALA_BEAR ? p2_perm_cols<KoalaBearParams>() + 2
                                                : p2_perm_cols<BabyBearParams>() + 2;
}
uint32_t p3r_poseidon2_num_constants(const p3r_ctx* ctx) {
  return ctx->cfg.field == P3R_FIELD_KOALA_BEAR ? p2_num_constants<KoalaBearParams>()
                                                : p2_num_constants<BabyBearParams>();
}
int p3r_poseidon2_round_constants(const p3r_ctx* ctx, uint32_t* out) {
  if (!ctx || !out) return P3R_EINVAL;
  std::copy(ctx->rc_canonical.begin(), ctx->rc_canonical.begin() + p3r_poseidon2_num_constants(ctx), out);   // the width-16 table
  return P3R_OK;
}

uint64_t p3r_zk_nonce(const p3r_ctx* ctx) { return ctx ? ctx->zk_nonce : 0; }
int p3r_zk_set_nonce(p3r_ctx* ctx, uint64_t nonce) {
  if (!ctx) return P3R_EINVAL;
  if (!(ctx->cfg.ext_choices & P3R_EXT_ZK_DETERMINISTIC)) {
    ctx->err = "p3r_zk_set_nonce needs P3R_EXT_ZK_DETERMINISTIC: replaying a nonce repeats the masks of an earlier proof";
    return P3R_EINVAL;
  }
  ctx->zk_nonce = nonce;
  return P3R_OK;
}

int p3r_trim(p3r_ctx* ctx, uint64_t* freed_bytes) {
  if (!ctx) return P3R_EINVAL;
  return guard(ctx, [&] {
    P3R_HIP(hipStreamSynchronize(ctx->stream));
    if (freed_bytes) {
      std::lock_guard<std::mutex> g(ctx->pool->mu);  // a sibling's out-of-memory path may be trimming this pool
      *freed_bytes = ctx->pool->cached_bytes;
    }
    ctx->pool->trim();
    ctx->const_tables.clear();  // the job lists were keyed to the addresses the pool handed out
  });
}

int p3r_sync(p3r_ctx* ctx) {
  return guard(ctx, [&] { P3R_HIP(hipStreamSynchronize(ctx->stream)); });
}

p3r_dmat* p3r_dmat_upload(p3r_ctx* ctx, const uint32_t* rowmajor, size_t h, size_t w) {
  p3r_dmat* out = nullptr;
  guard(ctx, [&] {
    if (!rowmajor) fail(P3R_EINVAL, "rowmajor is NULL");
    out = P3R_FIELD_CALL(ctx, upload, ctx, rowmajor, h, w).release();
  });
  return out;
}
p3r_dmat* p3r_dmat_alloc(p3r_ctx* ctx, size_t h, size_t w) {
  p3r_dmat* out = nullptr;
  guard(ctx, [&] { out = dmat_alloc(h, w).release(); });
  return out;
}
int p3r_dmat_download(p3r_ctx* ctx, const p3r_dmat* m, uint32_t* out) {
  return guard(ctx, [&] {
    if (!m || !out) fail(P3R_EINVAL, "NULL argument");
    P3R_FIELD_CALL(ctx, download, ctx, m, out);
  });
}
size_t p3r_dmat_height(const p3r_dmat* m) { return m->h; }
size_t p3r_dmat_width(const p3r_dmat* m) { return m->w; }
void p3r_dmat_free(p3r_ctx* ctx, p3r_dmat* m) {
  if (ctx) (void)hipStreamSynchronize(ctx->stream);
  delete m;
}

int p3r_poseidon2_permute_dmat(p3r_ctx* ctx, p3r_dmat* states) {
  return guard(ctx, [&] {
    if (!states) fail(P3R_EINVAL, "states is NULL");
    P3R_FIELD_CALL(ctx, permute_dmat, ctx, states);
  });
}

int p3r_poseidon2_permute_batch(p3r_ctx* ctx, const uint32_t* in, uint32_t* out, size_t n) {
  return guard(ctx, [&] {
    if (!in || !out) fail(P3R_EINVAL, "NULL argument");
    if (n == 0) return;
    // pad the batch to a power of two of lanes; the tail rows are zeros and are dropped
    size_t np = 1;
    while (np < n) np <<= 1;
    std::vector<uint32_t> padded;
    const uint32_t* src = in;
    if (np != n) {
      padded.assign(np * P2_WIDTH, 0);
      memcpy(padded.data(), in, n * P2_WIDTH * 4);
      src = padded.data();
    }
    auto m = P3R_FIELD_CALL(ctx, upload, ctx, src, np, (size_t)P2_WIDTH);
    P3R_FIELD_CALL(ctx, permute_dmat, ctx, m.get());
    if (np != n) {
      P3R_FIELD_CALL(ctx, download, ctx, m.get(), padded.data());
      memcpy(out, padded.data(), n * P2_WIDTH * 4);
    } else {
      P3R_FIELD_CALL(ctx, download, ctx, m.get(), out);
    }
  });
}

p3r_p2_dev* p3r_p2_rows_upload(p3r_ctx* ctx, const p3r_p2_rows* rows) {
  p3r_p2_dev* out = nullptr;
  guard(ctx, [&] {
    if (!rows) fail(P3R_EINVAL, "rows is NULL");
    out = P3R_FIELD_CALL(ctx, p2_rows_upload, ctx, rows).release();
  });
  return out;
}
void p3r_p2_rows_free(p3r_ctx* ctx, p3r_p2_dev* rows) {
  if (ctx) (void)hipStreamSynchronize(ctx->stream);
  delete rows;
}
p3r_dmat* p3r_poseidon2_trace_fill_dev(p3r_ctx* ctx, const p3r_p2_dev* rows) {
  p3r_dmat* out = nullptr;
  guard(ctx, [&] {
    if (!rows) fail(P3R_EINVAL, "rows is NULL");
    out = P3R_FIELD_CALL(ctx, trace_fill, ctx, rows).release();
  });
  return out;
}
p3r_dmat* p3r_poseidon2_trace_fill_dmat(p3r_ctx* ctx, const p3r_p2_rows* rows) {
  p3r_dmat* out = nullptr;
  guard(ctx, [&] {
    if (!rows) fail(P3R_EINVAL, "rows is NULL");
    auto d = P3R_FIELD_CALL(ctx, p2_rows_upload, ctx, rows);
    out = P3R_FIELD_CALL(ctx, trace_fill, ctx, d.get()).release();
  });
  return out;
}

int p3r_poseidon2_trace_fill(p3r_ctx* ctx, const p3r_p2_rows* rows, uint32_t* trace_out) {
  return guard(ctx, [&] {
    if (!rows || !trace_out) fail(P3R_EINVAL, "NULL argument");
    auto d = P3R_FIELD_CALL(ctx, p2_rows_upload, ctx, rows);
    auto t = P3R_FIELD_CALL(ctx, trace_fill, ctx, d.get());
    P3R_FIELD_CALL(ctx, download, ctx, t.get(), trace_out);
  });
}

// unit seams of the width-32 permutation (ABI 6): the permutation itself, and the table's trace fill
int p3r_poseidon2_w32_permute_batch(p3r_ctx* ctx, const uint32_t* in, uint32_t* out, size_t n) {
  return guard(ctx, [&] {
    require_w32_constants(ctx);
    if (!in || !out) fail(P3R_EINVAL, "NULL argument");
    if (n == 0) return;
    DevBuf d(n * P2W_WIDTH);
    P3R_HIP(hipMemcpyAsync(d.p, in, n * P2W_WIDTH * 4, hipMemcpyHostToDevice, ctx->stream));
    P3R_FIELD_CALL(ctx, permute_w32_rows, ctx, d.p, n);
    P3R_HIP(copy_sync(ctx->stream, out, d.p, n * P2W_WIDTH * 4, hipMemcpyDeviceToHost));
  });
}
int p3r_poseidon2_w32_trace_fill(p3r_ctx* ctx, const p3r_p2w_rows* rows, uint32_t* trace_out) {
  return guard(ctx, [&] {
    require_w32_constants(ctx);
    if (!rows || !trace_out || !rows->input_values || !rows->new_start || !rows->merkle_path || !rows->mmcs_bit || !rows->mmcs_bit2 ||
        !rows->mmcs_index_sum)
      fail(P3R_EINVAL, "NULL argument");
    const size_t n = rows->n;
    log2_exact(n, "width-32 Poseidon2 row count (callers pad to a power of two)");
    std::vector<uint8_t> f(4 * n);
    std::copy(rows->new_start, rows->new_start + n, f.begin());
    std::copy(rows->merkle_path, rows->merkle_path + n, f.begin() + n);
    std::copy(rows->mmcs_bit, rows->mmcs_bit + n, f.begin() + 2 * n);
    std::copy(rows->mmcs_bit2, rows->mmcs_bit2 + n, f.begin() + 3 * n);
    auto run = [&](auto tag) {
      using PP = decltype(tag);
      auto d = p2w_rows_upload<PP>(ctx, n, n, rows->input_values, f.data(), rows->mmcs_index_sum);
      auto t = trace_fill_w32<PP>(ctx, d.get());
      download<PP>(ctx, t.get(), trace_out);
    };
    if (ctx->cfg.field == P3R_FIELD_KOALA_BEAR) run(KoalaBearParams{}); else run(BabyBearParams{});
  });
}
uint32_t p3r_poseidon2_w32_trace_width(const p3r_ctx* ctx) {
  return (ctx->cfg.field == P3R_FIELD_KOALA_BEAR ? p2w_perm_cols<KoalaBearParams>() : p2w_perm_cols<BabyBearParams>()) + 4;
}

p3r_dmat* p3r_coset_lde_dmat(p3r_ctx* ctx, const p3r_dmat* evals, uint32_t added_bits,
                             uint32_t shift) {
  p3r_dmat* out = nullptr;
  guard(ctx, [&] {
    if (!evals) fail(P3R_EINVAL, "evals is NULL");
    out = P3R_FIELD_CALL(ctx, coset_lde, ctx, evals, (int)added_bits, shift).release();
  });
  return out;
}

int p3r_coset_lde(p3r_ctx* ctx, const uint32_t* evals, size_t h, size_t w, uint32_t added_bits,
                  uint32_t shift, uint32_t* out) {
  return guard(ctx, [&] {
    if (!evals || !out) fail(P3R_EINVAL, "NULL argument");
    auto in = P3R_FIELD_CALL(ctx, upload, ctx, evals, h, w);
    auto lde = P3R_FIELD_CALL(ctx, coset_lde, ctx, in.get(), (int)added_bits, shift);
    P3R_FIELD_CALL(ctx, download, ctx, lde.get(), out);
  });
}

// A caller's array of matrix handles, none of them NULL.  `who` leads the refusal where the array is one of several
// ("instance 2: ", "table: ").
static std::vector<const p3r_dmat*> checked_mats(const p3r_dmat* const* mats, size_t n_mats, const char* who = "") {
  if (n_mats && !mats) fail(P3R_EINVAL, "%smats is NULL", who);
  for (size_t i = 0; i < n_mats; ++i)
    if (!mats[i]) fail(P3R_EINVAL, "%smatrix %zu is NULL", who, i);
  return std::vector<const p3r_dmat*>(mats, mats + n_mats);
}

// TwoAdicSubgroupDft::dft_batch / idft_batch / coset_dft_batch / coset_idft_batch: one half of the LDE (tu_lde.hip)
static void dft_check_modes(uint32_t direction, uint32_t eval_order) {
  if (direction != P3R_DFT_FORWARD && direction != P3R_DFT_INVERSE) fail(P3R_EINVAL, "unknown DFT direction %u", direction);
  if (eval_order != P3R_DFT_NATURAL && eval_order != P3R_DFT_BITREV) fail(P3R_EINVAL, "unknown DFT evaluation order %u", eval_order);
}
int p3r_dft_batch_dmat(p3r_ctx* ctx, const p3r_dmat* const* mats, size_t n_mats, uint32_t direction, const uint32_t* shifts,
                       uint32_t eval_order, p3r_dmat** outs) {
  return guard(ctx, [&] {
    if (!mats || !shifts || !outs || n_mats == 0) fail(P3R_EINVAL, "bad arguments");
    dft_check_modes(direction, eval_order);
    const auto ms = checked_mats(mats, n_mats);
    std::vector<LdeItem> items(n_mats);
    for (size_t i = 0; i < n_mats; ++i) items[i] = {ms[i], shifts[i]};
    auto res = P3R_FIELD_CALL(ctx, dft_batch, ctx, items, direction == P3R_DFT_INVERSE, eval_order == P3R_DFT_BITREV);
    for (size_t i = 0; i < n_mats; ++i) outs[i] = res[i].release();
  });
}
int p3r_dft(p3r_ctx* ctx, const uint32_t* rowmajor_in, size_t h, size_t w, uint32_t direction, uint32_t shift,
            uint32_t eval_order, uint32_t* rowmajor_out) {
  return guard(ctx, [&] {
    if (!rowmajor_in || !rowmajor_out) fail(P3R_EINVAL, "NULL argument");
    dft_check_modes(direction, eval_order);
    P3R_FIELD_CALL(ctx, dft_check, h, w, shift);
    const uint32_t p = ctx->cfg.field == P3R_FIELD_KOALA_BEAR ? KoalaBearParams::P : BabyBearParams::P;
    for (size_t i = 0; i < h * w; ++i)
      if (rowmajor_in[i] >= p) fail(P3R_EINVAL, "non-canonical field element at word %zu", i);
    auto in = P3R_FIELD_CALL(ctx, upload, ctx, rowmajor_in, h, w);
    auto res = P3R_FIELD_CALL(ctx, dft_batch, ctx, {{in.get(), shift}}, direction == P3R_DFT_INVERSE, eval_order == P3R_DFT_BITREV);
    P3R_FIELD_CALL(ctx, download, ctx, res[0].get(), rowmajor_out);
  });
}

// The value half of Pcs::open (TwoAdicFriPcs::open's interpolate_coset loop): tu_open.hip
static void open_points_check_modes(uint32_t added_bits, uint32_t eval_order, const size_t* point_offsets) {
  if (eval_order != P3R_DFT_NATURAL && eval_order != P3R_DFT_BITREV) fail(P3R_EINVAL, "unknown evaluation order %u", eval_order);
  if (added_bits > 31) fail(P3R_EINVAL, "added_bits (%u) out of range", added_bits);
  if (!point_offsets) fail(P3R_EINVAL, "point_offsets is NULL");
}
int p3r_open_points_dmat(p3r_ctx* ctx, const p3r_dmat* const* mats, size_t n_mats, uint32_t added_bits, uint32_t shift,
                         uint32_t eval_order, const size_t* point_offsets, const uint32_t* points, uint32_t* values_out) {
  return guard(ctx, [&] {
    if (n_mats == 0) return;
    if (!mats) fail(P3R_EINVAL, "mats is NULL");
    open_points_check_modes(added_bits, eval_order, point_offsets);
    const auto ms = checked_mats(mats, n_mats);
    std::vector<OpenPointsItem> items(n_mats);
    for (size_t i = 0; i < n_mats; ++i) items[i] = {ms[i]->d, ms[i]->h, ms[i]->w, point_offsets[i], point_offsets[i + 1]};
    P3R_FIELD_CALL(ctx, open_points, ctx, items, (int)added_bits, shift, eval_order == P3R_DFT_BITREV, points, values_out);
  });
}
int p3r_open_points(p3r_ctx* ctx, const p3r_matrix* mats, size_t n_mats, uint32_t added_bits, uint32_t shift,
                    uint32_t eval_order, const size_t* point_offsets, const uint32_t* points, uint32_t* values_out) {
  return guard(ctx, [&] {
    if (n_mats == 0) return;
    if (!mats) fail(P3R_EINVAL, "mats is NULL");
    open_points_check_modes(added_bits, eval_order, point_offsets);
    const uint32_t p = ctx->cfg.field == P3R_FIELD_KOALA_BEAR ? KoalaBearParams::P : BabyBearParams::P;
    std::vector<OpenPointsItem> items(n_mats);
    for (size_t i = 0; i < n_mats; ++i) {
      items[i] = {nullptr, mats[i].height, mats[i].width, point_offsets[i], point_offsets[i + 1]};
      log2_exact(mats[i].height, "matrix height");
      if (mats[i].width && !mats[i].values) fail(P3R_EINVAL, "matrix %zu has no values", i);
      for (size_t k = 0; k < mats[i].height * mats[i].width; ++k)
        if (mats[i].values[k] >= p) fail(P3R_EINVAL, "matrix %zu: non-canonical field element at word %zu", i, k);
    }
    // what the device form refuses, before any matrix is uploaded (all widths 0: every check runs, nothing is launched)
    {
      std::vector<OpenPointsItem> dry = items;
      for (auto& it : dry) it.w = 0;
      P3R_FIELD_CALL(ctx, open_points, ctx, dry, (int)added_bits, shift, eval_order == P3R_DFT_BITREV, points, values_out);
    }
    std::vector<std::unique_ptr<p3r_dmat>> up(n_mats);
    for (size_t i = 0; i < n_mats; ++i) {
      if (mats[i].width == 0 || point_offsets[i] == point_offsets[i + 1]) {   // contributes nothing
        items[i].w = 0;
        continue;
      }
      up[i] = P3R_FIELD_CALL(ctx, upload, ctx, mats[i].values, mats[i].height, mats[i].width);
      items[i].d = up[i]->d;
    }
    P3R_FIELD_CALL(ctx, open_points, ctx, items, (int)added_bits, shift, eval_order == P3R_DFT_BITREV, points, values_out);
  });
}

// The reduced openings of Pcs::open and FriFoldingStrategy::fold_matrix with the roll-in: tu_fri.hip
int p3r_fri_reduce_dmat(p3r_ctx* ctx, const p3r_dmat* const* mats, size_t n_mats, uint32_t shift, const size_t* point_offsets,
                        const uint32_t* points, const uint32_t* values, const uint32_t* alpha, p3r_dmat** outs, size_t* n_outs) {
  return guard(ctx, [&] {
    if (n_outs) *n_outs = 0;
    if (n_mats == 0) fail(P3R_EINVAL, "n_mats == 0: no matrix to reduce");
    if (!mats || !point_offsets || !alpha || !outs || !n_outs) fail(P3R_EINVAL, "NULL argument");
    const auto ms = checked_mats(mats, n_mats);
    std::vector<FriReduceItem> items(n_mats);
    for (size_t i = 0; i < n_mats; ++i) items[i] = {ms[i]->d, ms[i]->h, ms[i]->w, point_offsets[i], point_offsets[i + 1]};
    auto res = P3R_FIELD_CALL(ctx, fri_reduce, ctx, items, shift, points, values, alpha);
    for (size_t i = 0; i < res.size(); ++i) outs[i] = res[i].release();
    *n_outs = res.size();
  });
}
int p3r_fri_fold_dmat(p3r_ctx* ctx, const p3r_dmat* in, uint32_t log_arity, const uint32_t* beta, const p3r_dmat* roll_in,
                      p3r_dmat** out) {
  return guard(ctx, [&] {
    if (out) *out = nullptr;
    if (!in || !beta || !out) fail(P3R_EINVAL, "NULL argument");
    *out = P3R_FIELD_CALL(ctx, fri_fold, ctx, in, log_arity, beta, roll_in).release();
  });
}

// The rest of prove_fri at the seam: the challenger (HostChallenger, host_transcript.h; grind_witness / k_grind for the
// proof of work), the commit-phase leaf view (tu_fri.hip), the final polynomial (fri_final_poly) and the schedule rule.
p3r_challenger* p3r_challenger_create(p3r_ctx* ctx) {
  p3r_challenger* out = nullptr;
  guard(ctx, [&] {
    if (!ctx) fail(P3R_EINVAL, "ctx is NULL");
    auto ch = std::make_unique<p3r_challenger>();
    ch->ctx = ctx;
    ch->rc = ctx->rc_mont_host;
    ch->tag = ctx->cfg.field == P3R_FIELD_KOALA_BEAR ? (ctx->cfg.challenge_degree == 5 ? 1 : 0) : 2;
    challenger_make(ch.get(), nullptr);
    out = ch.release();
  });
  return out;
}
p3r_challenger* p3r_challenger_clone(const p3r_challenger* src) {
  p3r_challenger* out = nullptr;
  guard(src ? src->ctx : nullptr, [&] {
    if (!src) fail(P3R_EINVAL, "challenger is NULL");
    auto ch = std::make_unique<p3r_challenger>();
    ch->ctx = src->ctx;
    ch->rc = src->rc;
    ch->tag = src->tag;
    challenger_make(ch.get(), src);
    out = ch.release();
  });
  return out;
}
void p3r_challenger_free(p3r_challenger* ch) { delete ch; }
int p3r_challenger_observe(p3r_challenger* ch, const uint32_t* words, size_t n) {
  return guard(ch ? ch->ctx : nullptr, [&] {
    if (!ch) fail(P3R_EINVAL, "challenger is NULL");
    if (n && !words) fail(P3R_EINVAL, "words is NULL");
    challenger_visit(ch, [&](auto& c) {
      using F = typename std::decay_t<decltype(c)>::F;
      for (size_t i = 0; i < n; ++i)   // all of them, before any is observed
        if (words[i] >= F::P) fail(P3R_EINVAL, "non-canonical word %zu observed", i);
      for (size_t i = 0; i < n; ++i) c.observe(F::from_canonical(words[i]));
    });
  });
}
int p3r_challenger_sample(p3r_challenger* ch, uint32_t* out, size_t n) {
  return guard(ch ? ch->ctx : nullptr, [&] {
    if (!ch) fail(P3R_EINVAL, "challenger is NULL");
    if (n && !out) fail(P3R_EINVAL, "out is NULL");
    challenger_visit(ch, [&](auto& c) {
      for (size_t i = 0; i < n; ++i) out[i] = c.sample().to_canonical();
    });
  });
}
int p3r_challenger_sample_ext(p3r_challenger* ch, uint32_t* out) {
  return guard(ch ? ch->ctx : nullptr, [&] {
    if (!ch) fail(P3R_EINVAL, "challenger is NULL");
    if (!out) fail(P3R_EINVAL, "out is NULL");
    challenger_visit(ch, [&](auto& c) {
      const auto e = c.sample_ext();
      for (size_t k = 0; k < sizeof e.c / sizeof e.c[0]; ++k) out[k] = e.c[k].to_canonical();
    });
  });
}
int p3r_challenger_sample_bits(p3r_challenger* ch, uint32_t bits, uint32_t* out) {
  return guard(ch ? ch->ctx : nullptr, [&] {
    if (!ch) fail(P3R_EINVAL, "challenger is NULL");
    if (!out) fail(P3R_EINVAL, "out is NULL");
    if (bits > 30) fail(P3R_EINVAL, "sample_bits: bits must be <= 30 (got %u)", bits);
    challenger_visit(ch, [&](auto& c) { *out = c.sample_bits((int)bits); });
  });
}
int p3r_challenger_check_witness(p3r_challenger* ch, uint32_t bits, uint32_t witness, int* ok_out) {
  return guard(ch ? ch->ctx : nullptr, [&] {
    if (!ch) fail(P3R_EINVAL, "challenger is NULL");
    if (!ok_out) fail(P3R_EINVAL, "ok_out is NULL");
    if (bits > 30) fail(P3R_EINVAL, "proof-of-work bits must be <= 30");
    challenger_visit(ch, [&](auto& c) {
      using F = typename std::decay_t<decltype(c)>::F;
      if (witness >= F::P) fail(P3R_EINVAL, "non-canonical proof-of-work witness");
      *ok_out = c.check_witness((int)bits, F::from_canonical(witness)) ? 1 : 0;
    });
  });
}
int p3r_challenger_grind(p3r_ctx* ctx, p3r_challenger* ch, uint32_t bits, uint32_t* witness_out) {
  return guard(ctx, [&] {
    if (ch && !ch->ctx) fail(P3R_EINVAL, "a host challenger (p3r_challenger_create_host) cannot grind: the search runs on a device");
    if (!ctx || !ch) fail(P3R_EINVAL, "ctx or challenger is NULL");
    if (!witness_out) fail(P3R_EINVAL, "witness_out is NULL");
    if (ch->ctx != ctx) fail(P3R_EINVAL, "the challenger belongs to another context");
    if (bits > 30) fail(P3R_EINVAL, "proof-of-work bits must be <= 30");
    challenger_visit(ch, [&](auto& c) {
      using PP = typename std::decay_t<decltype(c)>::F::Params;
      *witness_out = grind_witness<PP>(ctx, c, (int)bits).to_canonical();
    });
  });
}
int p3r_fri_leaf_view_dmat(p3r_ctx* ctx, const p3r_dmat* vec, uint32_t log_arity, p3r_dmat** out) {
  return guard(ctx, [&] {
    if (out) *out = nullptr;
    if (!vec || !out) fail(P3R_EINVAL, "NULL argument");
    *out = P3R_FIELD_CALL(ctx, fri_leaf_view, ctx, vec, log_arity).release();
  });
}
int p3r_fri_final_poly_dmat(p3r_ctx* ctx, const p3r_dmat* vec, uint32_t log_final_poly_len, uint32_t* coeffs_out) {
  return guard(ctx, [&] {
    if (!vec || !coeffs_out) fail(P3R_EINVAL, "NULL argument");
    P3R_FIELD_CALL(ctx, fri_final_poly_canonical, ctx, vec, log_final_poly_len, coeffs_out);
  });
}
int p3r_fri_log_arity(const p3r_ctx* ctx, size_t phase, int log_cur, int log_final, int log_next_input) {
  if (!ctx) return -1;
  return fri_log_arity(ctx->fri_log_arities, phase, (int)ctx->cfg.max_log_arity, log_cur, log_final, log_next_input);
}

// The field and the challenge degree of a host-only entry's configuration: what is refused of them, the modulus and DC.
struct HostField {
  uint32_t p;
  int dc;
};
static HostField host_field(const p3r_config* cfg) {
  if (cfg->field != P3R_FIELD_KOALA_BEAR && cfg->field != P3R_FIELD_BABY_BEAR) fail(P3R_EINVAL, "unknown field %u", cfg->field);
  if (cfg->challenge_degree != 0 && cfg->challenge_degree != 4 && cfg->challenge_degree != 5)
    fail(P3R_EINVAL, "challenge_degree must be 4 or 5 (got %u)", cfg->challenge_degree);
  return {cfg->field == P3R_FIELD_KOALA_BEAR ? KoalaBearParams::P : BabyBearParams::P, cfg->challenge_degree == 5 ? 5 : 4};
}
// The caller's AIR as a constraint program: air_program.h (the host half), tu_air.hip (the launch)
int p3r_air_program_info(const p3r_config* cfg, const p3r_air_insn* prog, size_t n_insns, const size_t* widths, size_t n_mats,
                         p3r_air_info* out) {
  return guard(nullptr, [&] {
    if (!cfg || !out) fail(P3R_EINVAL, "NULL argument");
    const HostField f = host_field(cfg);
    *out = air_plan(prog, n_insns, widths, n_mats, f.dc, f.p, kAirUnknownCount, kAirUnknownCount,
                    P3R_AIR_MAX_LIVE).info;
  });
}
// The verifier's side of a constraint program: air_program_eval.h (host only)
int p3r_air_program_eval(const p3r_config* cfg, const p3r_air_insn* prog, size_t n_insns, const size_t* widths, size_t n_mats,
                         const uint32_t* local, const uint32_t* next, uint32_t log_height, const uint32_t* zeta, const uint32_t* public_values,
                         size_t n_public, const uint32_t* challenges, size_t n_challenges, const uint32_t* alpha, uint32_t* folded_out,
                         uint32_t* inv_zh_out) {
  return guard(nullptr, [&] {
    if (!cfg) fail(P3R_EINVAL, "cfg is NULL");
    const HostField f = host_field(cfg);
    if (cfg->zk) fail(P3R_EUNSUPPORTED, "zk configurations: their doubled domains are out of scope of the program seams");
    if (cfg->field == P3R_FIELD_BABY_BEAR) {
      if (f.dc == 5) fail(P3R_EUNSUPPORTED, "UnsupportedChallengeDegree: the quintic challenge field is KoalaBear's");
      air_program_eval<BabyBearParams, 4>(prog, n_insns, widths, n_mats, local, next, log_height, zeta, public_values, n_public, challenges,
                                          n_challenges, alpha, folded_out, inv_zh_out);
    } else if (f.dc == 5) {
      air_program_eval<KoalaBearParams, 5>(prog, n_insns, widths, n_mats, local, next, log_height, zeta, public_values, n_public, challenges,
                                           n_challenges, alpha, folded_out, inv_zh_out);
    } else {
      air_program_eval<KoalaBearParams, 4>(prog, n_insns, widths, n_mats, local, next, log_height, zeta, public_values, n_public, challenges,
                                           n_challenges, alpha, folded_out, inv_zh_out);
    }
  });
}
int p3r_quotient_program_dmat(p3r_ctx* ctx, const p3r_air_insn* prog, size_t n_insns, const p3r_dmat* const* mats, size_t n_mats,
                              uint32_t added_bits, uint32_t shift, uint32_t log_quotient_degree, const uint32_t* public_values,
                              size_t n_public, const uint32_t* challenges, size_t n_challenges, const uint32_t* alpha, p3r_dmat** outs) {
  return guard(ctx, [&] {
    if (!ctx) fail(P3R_EINVAL, "ctx is NULL");
    if (!outs) fail(P3R_EINVAL, "outs is NULL");
    const auto ms = checked_mats(mats, n_mats);
    auto res = P3R_FIELD_CALL(ctx, quotient_program, ctx, prog, n_insns, ms, added_bits, shift, log_quotient_degree, public_values,
                              n_public, challenges, n_challenges, alpha);
    for (size_t i = 0; i < res.size(); ++i) outs[i] = res[i].release();
  });
}

// The caller's lookups as a lookup program: air_program.h in its lookup mode, tu_air.hip (the launches)
int p3r_lookup_program_info(const p3r_config* cfg, const p3r_air_insn* prog, size_t n_insns, const size_t* widths, size_t n_mats,
                            p3r_lookup_info* out) {
  return guard(nullptr, [&] {
    if (!cfg || !out) fail(P3R_EINVAL, "NULL argument");
    const HostField f = host_field(cfg);
    *out = air_plan(prog, n_insns, widths, n_mats, f.dc, f.p, kAirUnknownCount, kAirUnknownCount,
                    P3R_AIR_MAX_LIVE, AIR_MODE_LOOKUP).lookup;
  });
}
int p3r_logup_program_dmat(p3r_ctx* ctx, const p3r_air_insn* prog, size_t n_insns, const p3r_dmat* const* mats, size_t n_mats,
                           const uint32_t* public_values, size_t n_public, const uint32_t* challenges, size_t n_challenges,
                           p3r_dmat** out, uint32_t* sum_out) {
  return guard(ctx, [&] {
    if (out) *out = nullptr;
    if (!ctx) fail(P3R_EINVAL, "ctx is NULL");
    if (!out) fail(P3R_EINVAL, "out is NULL");
    const auto ms = checked_mats(mats, n_mats);
    *out = P3R_FIELD_CALL(ctx, logup_program, ctx, prog, n_insns, ms, public_values, n_public, challenges, n_challenges, sum_out).release();
  });
}

// Is the caller's trace right: the constraints on the trace domain and the balance of the bus (tu_air.hip)
int p3r_check_program_dmat(p3r_ctx* ctx, const p3r_air_insn* prog, size_t n_insns, const p3r_dmat* const* mats, size_t n_mats,
                           const uint32_t* public_values, size_t n_public, const uint32_t* challenges, size_t n_challenges,
                           p3r_check_report* report, uint32_t* first_row_out, uint64_t* n_failed_out) {
  return guard(ctx, [&] {
    if (!ctx) fail(P3R_EINVAL, "ctx is NULL");
    const auto ms = checked_mats(mats, n_mats);
    P3R_FIELD_CALL(ctx, check_program, ctx, prog, n_insns, ms, public_values, n_public, challenges, n_challenges, report, first_row_out,
                   n_failed_out);
  });
}
int p3r_lookup_check_dmat(p3r_ctx* ctx, const p3r_lookup_instance* inst, size_t n_inst, const uint32_t* challenges, size_t n_challenges,
                          p3r_lookup_imbalance* out, size_t cap, uint64_t* n_unbalanced_out) {
  return guard(ctx, [&] {
    if (!ctx) fail(P3R_EINVAL, "ctx is NULL");
    if (n_inst && !inst) fail(P3R_EINVAL, "inst is NULL");
    std::vector<LookupCheckInstance> is(n_inst);
    for (size_t p = 0; p < n_inst; ++p) {
      const std::string who = "instance " + std::to_string(p) + ": ";
      is[p] = LookupCheckInstance{inst[p].prog, inst[p].n_insns, checked_mats(inst[p].mats, inst[p].n_mats, who.c_str()), inst[p].public_values,
                                  inst[p].n_public};
    }
    P3R_FIELD_CALL(ctx, lookup_check, ctx, is, challenges, n_challenges, out, cap, n_unbalanced_out);
  });
}
int p3r_lookup_multiplicities_dmat(p3r_ctx* ctx, const p3r_lookup_instance* table, const p3r_lookup_instance* queries, size_t n_queries,
                                   const uint32_t* challenges, size_t n_challenges, p3r_dmat** out, p3r_lookup_imbalance* missing,
                                   size_t cap, uint64_t* n_missing_out) {
  return guard(ctx, [&] {
    if (out) *out = nullptr;
    if (!ctx) fail(P3R_EINVAL, "ctx is NULL");
    if (!table) fail(P3R_EINVAL, "table is NULL");
    if (!out) fail(P3R_EINVAL, "out is NULL");
    if (n_queries && !queries) fail(P3R_EINVAL, "queries is NULL");
    std::vector<LookupCheckInstance> is(1 + n_queries);   // the table first
    for (size_t p = 0; p <= n_queries; ++p) {
      const p3r_lookup_instance& in = p ? queries[p - 1] : *table;
      const std::string who = p ? "query " + std::to_string(p - 1) + ": " : std::string("table: ");
      is[p] = LookupCheckInstance{in.prog, in.n_insns, checked_mats(in.mats, in.n_mats, who.c_str()), in.public_values, in.n_public};
    }
    *out = P3R_FIELD_CALL(ctx, lookup_multiplicities, ctx, is, challenges, n_challenges, missing, cap, n_missing_out).release();
  });
}

// Derived trace columns as a witness program: air_program.h in its witness mode, tu_air.hip (the launch)
int p3r_witness_program_info(const p3r_config* cfg, const p3r_air_insn* prog, size_t n_insns, const size_t* widths, size_t n_mats,
                             p3r_witness_info* out) {
  return guard(nullptr, [&] {
    if (!cfg || !out) fail(P3R_EINVAL, "NULL argument");
    const HostField f = host_field(cfg);
    *out = air_plan(prog, n_insns, widths, n_mats, f.dc, f.p, kAirUnknownCount, kAirUnknownCount,
                    P3R_AIR_MAX_LIVE, AIR_MODE_WITNESS).witness;
  });
}
int p3r_witness_program_dmat(p3r_ctx* ctx, const p3r_air_insn* prog, size_t n_insns, const p3r_dmat* const* mats, size_t n_mats,
                             size_t height, const uint32_t* public_values, size_t n_public, const uint32_t* challenges,
                             size_t n_challenges, p3r_dmat** out) {
  return guard(ctx, [&] {
    if (out) *out = nullptr;
    if (!ctx) fail(P3R_EINVAL, "ctx is NULL");
    if (!out) fail(P3R_EINVAL, "out is NULL");
    const auto ms = checked_mats(mats, n_mats);
    *out = P3R_FIELD_CALL(ctx, witness_program, ctx, prog, n_insns, ms, height, public_values, n_public, challenges, n_challenges).release();
  });
}

// Accumulator columns as affine recurrences: scan_plan.h (the descriptors), tu_air.hip (the launches)
int p3r_affine_scan_info(const p3r_config* cfg, const p3r_recurrence* recs, size_t n_recs, const size_t* widths, size_t n_mats,
                         p3r_scan_info* out) {
  return guard(nullptr, [&] {
    if (!cfg || !out) fail(P3R_EINVAL, "NULL argument");
    const HostField f = host_field(cfg);
    *out = scan_plan(recs, n_recs, widths, n_mats, f.dc, f.p).info;
  });
}
int p3r_affine_scan_dmat(p3r_ctx* ctx, const p3r_recurrence* recs, size_t n_recs, const p3r_dmat* const* mats, size_t n_mats,
                         p3r_dmat** out, uint32_t* last_out) {
  return guard(ctx, [&] {
    if (out) *out = nullptr;
    if (!ctx) fail(P3R_EINVAL, "ctx is NULL");
    if (!out) fail(P3R_EINVAL, "out is NULL");
    const auto ms = checked_mats(mats, n_mats);
    *out = P3R_FIELD_CALL(ctx, affine_scan, ctx, recs, n_recs, ms, last_out).release();
  });
}

int p3r_mmcs_commit_dmat(p3r_ctx* ctx, const p3r_dmat* const* mats, size_t n_mats,
                         uint32_t* cap_out, p3r_tree** tree_out) {
  return guard(ctx, [&] {
    if (!mats || !cap_out || n_mats == 0) fail(P3R_EINVAL, "bad arguments");
    auto tree = std::make_unique<p3r_tree>();
    tree->mats.assign(mats, mats + n_mats);
    P3R_FIELD_CALL(ctx, mmcs_commit_canonical, ctx, tree.get(), cap_out);
    if (tree_out) *tree_out = tree.release();
  });
}

int p3r_mmcs_commit(p3r_ctx* ctx, const p3r_matrix* mats, size_t n_mats, uint32_t* cap_out,
                    p3r_tree** tree_out) {
  return guard(ctx, [&] {
    if (!mats || !cap_out || n_mats == 0) fail(P3R_EINVAL, "bad arguments");
    auto tree = std::make_unique<p3r_tree>();
    for (size_t i = 0; i < n_mats; ++i) {
      if (!mats[i].values) fail(P3R_EINVAL, "matrix %zu has NULL values", i);
      tree->owned.push_back(
          P3R_FIELD_CALL(ctx, upload, ctx, mats[i].values, mats[i].height, mats[i].width));
      tree->mats.push_back(tree->owned.back().get());
    }
    P3R_FIELD_CALL(ctx, mmcs_commit_canonical, ctx, tree.get(), cap_out);
    if (tree_out) *tree_out = tree.release();
  });
}

int p3r_mmcs_open(p3r_ctx* ctx, const p3r_tree* tree, size_t index, uint32_t* opened_values,
                  uint32_t* proof_out) {
  return guard(ctx, [&] {
    if (!tree || !opened_values || !proof_out) fail(P3R_EINVAL, "NULL argument");
    if (tree->salt_elems) fail(P3R_EINVAL, "p3r_mmcs_open has no salt output: open a hiding tree with p3r_mmcs_open_batch");
    P3R_FIELD_CALL(ctx, mmcs_open, ctx, tree, index, opened_values, proof_out);
  });
}
int p3r_mmcs_open_batch(p3r_ctx* ctx, const p3r_tree* tree, const size_t* indices, size_t n, uint32_t* opened_values,
                        uint32_t* salts, uint32_t* proofs) {
  return guard(ctx, [&] {
    if (!tree) fail(P3R_EINVAL, "tree is NULL");
    if (n == 0) return;
    if (!indices || !opened_values || !proofs) fail(P3R_EINVAL, "NULL argument");
    if (tree->salt_elems && !salts) fail(P3R_EINVAL, "salts is NULL: the openings of a hiding tree carry %d salt elements per matrix", tree->salt_elems);
    P3R_FIELD_CALL(ctx, mmcs_open_batch, ctx, tree, indices, n, opened_values, salts, proofs);
  });
}
size_t p3r_tree_salt_elems(const p3r_tree* t) { return (size_t)t->salt_elems; }
size_t p3r_tree_num_matrices(const p3r_tree* t) { return t->mats.size() / (t->salt_elems ? 2 : 1); }
size_t p3r_tree_log_max_height(const p3r_tree* t) { return (size_t)t->log_max_h; }
size_t p3r_tree_total_width(const p3r_tree* t) { return t->total_width; }
size_t p3r_tree_proof_len(const p3r_tree* t) { return p3r::mmcs_proof_len(t->levels); }
void p3r_tree_free(p3r_ctx* ctx, p3r_tree* tree) {
  if (ctx) (void)hipStreamSynchronize(ctx->stream);
  delete tree;
}

int p3r_time_permute_dmat(p3r_ctx* ctx, p3r_dmat* states, int iters, double* ms_per_launch) {
  return guard(ctx, [&] {
    if (!states || !ms_per_launch || iters <= 0) fail(P3R_EINVAL, "bad arguments");
    hipEvent_t a, b;
    P3R_HIP(hipEventCreate(&a));
    P3R_HIP(hipEventCreate(&b));
    P3R_FIELD_CALL(ctx, permute_dmat, ctx, states);  // warm-up
    P3R_HIP(hipEventRecord(a, ctx->stream));
    for (int i = 0; i < iters; ++i) P3R_FIELD_CALL(ctx, permute_dmat, ctx, states);
    P3R_HIP(hipEventRecord(b, ctx->stream));
    P3R_HIP(hipEventSynchronize(b));
    float ms = 0;
    P3R_HIP(hipEventElapsedTime(&ms, a, b));
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    *ms_per_launch = (double)ms / iters;
  });
}

p3r_prep* p3r_prep_create(p3r_ctx* ctx, const p3r_air_desc* airs, const p3r_matrix* prep_mats,
                          size_t n_instances, uint32_t* commit_out) {
  p3r_prep* out = nullptr;
  guard(ctx, [&] {
    if (!airs || !prep_mats || !commit_out || n_instances == 0) fail(P3R_EINVAL, "bad arguments");
    for (size_t i = 0; i < n_instances; ++i)
      if (!prep_mats[i].values) fail(P3R_EINVAL, "preprocessed matrix %zu has NULL values", i);
    auto prep = P3R_FIELD_CALL(ctx, prep_create, ctx, airs, prep_mats, n_instances);
    std::copy(prep->cap_canonical.begin(), prep->cap_canonical.end(), commit_out);
    out = prep.release();
  });
  return out;
}
void p3r_prep_free(p3r_ctx* ctx, p3r_prep* prep) {
  if (ctx) (void)hipStreamSynchronize(ctx->stream);
  delete prep;
}

// A proof that does not fit the caller's buffer is KEPT (p3r_take_proof): proving again to learn nothing but the size
// would double the call's cost, and under zk = 1 - or a hiding MMCS - the second proof is another one, of another length.
static int emit_proof(p3r_ctx* ctx, std::vector<uint8_t>&& bytes, uint8_t* buf, size_t cap, size_t* len) {
  *len = bytes.size();
  ctx->pending_proof.clear();
  if (bytes.size() > cap) {
    const size_t need = bytes.size();
    ctx->pending_proof = std::move(bytes);
    fail(P3R_EBUFFER, "proof needs %zu bytes, buffer holds %zu (p3r_take_proof hands it over)", need, cap);
  }
  memcpy(buf, bytes.data(), bytes.size());
  return 0;
}

int p3r_take_proof(p3r_ctx* ctx, uint8_t* proof_buf, size_t proof_cap, size_t* proof_len) {
  return guard(ctx, [&] {
    if (!proof_len || (!proof_buf && proof_cap)) fail(P3R_EINVAL, "bad arguments");
    if (ctx->pending_proof.empty()) fail(P3R_EINVAL, "no proof is waiting: the last prove call on this context did not return P3R_EBUFFER");
    *proof_len = ctx->pending_proof.size();
    if (ctx->pending_proof.size() > proof_cap)
      fail(P3R_EBUFFER, "proof needs %zu bytes, buffer holds %zu", ctx->pending_proof.size(), proof_cap);
    memcpy(proof_buf, ctx->pending_proof.data(), ctx->pending_proof.size());
    std::vector<uint8_t>().swap(ctx->pending_proof);
  });
}

int p3r_prove_batch(p3r_ctx* ctx, const p3r_prep* prep, const p3r_dmat* const* main_traces,
                    size_t n_instances, uint32_t flags, uint8_t* proof_buf, size_t proof_cap,
                    size_t* proof_len) {
  return guard(ctx, [&] {
    if (!prep || !main_traces || !proof_len || (!proof_buf && proof_cap)) fail(P3R_EINVAL, "bad arguments");
    for (size_t i = 0; i < n_instances; ++i)
      if (!main_traces[i]) fail(P3R_EINVAL, "main trace %zu is NULL", i);
    auto bytes = P3R_FIELD_CALL(ctx, prove_batch_any, ctx, prep, main_traces, n_instances,
                                (flags & P3R_PROVE_CANONICAL_FIELD_ENCODING) != 0);
    emit_proof(ctx, std::move(bytes), proof_buf, proof_cap, proof_len);
  });
}

int p3r_prove_batch_host(p3r_ctx* ctx, const p3r_prep* prep, const p3r_matrix* main_traces,
                         size_t n_instances, uint32_t flags, uint8_t* proof_buf, size_t proof_cap,
                         size_t* proof_len) {
  return guard(ctx, [&] {
    if (!prep || !main_traces || !proof_len || (!proof_buf && proof_cap)) fail(P3R_EINVAL, "bad arguments");
    std::vector<std::unique_ptr<p3r_dmat>> owned;
    std::vector<const p3r_dmat*> ptrs;
    for (size_t i = 0; i < n_instances; ++i) {
      if (!main_traces[i].values) fail(P3R_EINVAL, "main trace %zu has NULL values", i);
      owned.push_back(P3R_FIELD_CALL(ctx, upload, ctx, main_traces[i].values, main_traces[i].height,
                                     main_traces[i].width));
      ptrs.push_back(owned.back().get());
    }
    auto bytes = P3R_FIELD_CALL(ctx, prove_batch_any, ctx, prep, ptrs.data(), n_instances,
                                (flags & P3R_PROVE_CANONICAL_FIELD_ENCODING) != 0);
    emit_proof(ctx, std::move(bytes), proof_buf, proof_cap, proof_len);
  });
}

p3r_layer* p3r_layer_create(p3r_ctx* ctx, const p3r_layer_desc* desc, uint32_t* commit_out) {
  p3r_layer* out = nullptr;
  guard(ctx, [&] {
    if (!desc || !commit_out) fail(P3R_EINVAL, "NULL argument");
    out = P3R_FIELD_CALL(ctx, layer_create, ctx, desc, commit_out).release();
  });
  return out;
}
void p3r_layer_free(p3r_ctx* ctx, p3r_layer* layer) {
  if (ctx) (void)hipStreamSynchronize(ctx->stream);
  delete layer;
}
int p3r_layer_table_heights(const p3r_layer* L, size_t h[5]) {
  if (!L || !h) return P3R_EINVAL;
  h[0] = L->h_const; h[1] = L->h_public; h[2] = L->h_alu; h[3] = L->h_p2; h[4] = L->h_recompose;
  return P3R_OK;
}
int p3r_layer_p2w_height(const p3r_layer* L, size_t* h) {
  if (!L || !h) return P3R_EINVAL;
  *h = L->h_p2w;
  return P3R_OK;
}
int p3r_layer_recompose_coeff_height(const p3r_layer* L, size_t* h) {
  if (!L || !h) return P3R_EINVAL;
  *h = L->h_recompose_coeff;
  return P3R_OK;
}
int p3r_layer_recompose_kind(const p3r_layer* L, uint32_t* coeff_lookups) {
  if (!L || !coeff_lookups) return P3R_EINVAL;
  *coeff_lookups = L->recompose_coeff ? 1u : 0u;
  return P3R_OK;
}
int p3r_layer_effective_lanes(const p3r_layer* L, uint32_t* public_lanes, uint32_t* alu_lanes) {
  if (!L || !public_lanes || !alu_lanes) return P3R_EINVAL;
  *public_lanes = L->public_lanes;
  *alu_lanes = L->alu_lanes;
  return P3R_OK;
}
p3r_dtraces* p3r_traces_upload(p3r_ctx* ctx, const p3r_layer* layer, const p3r_traces* traces) {
  p3r_dtraces* out = nullptr;
  guard(ctx, [&] {
    if (!layer || !traces) fail(P3R_EINVAL, "NULL argument");
    out = P3R_FIELD_CALL(ctx, traces_upload, ctx, layer, traces).release();
  });
  return out;
}
void p3r_traces_free(p3r_ctx* ctx, p3r_dtraces* t) {
  if (ctx) (void)hipStreamSynchronize(ctx->stream);
  delete t;
}
int p3r_prove_all_tables_resident(p3r_ctx* ctx, const p3r_layer* layer, const p3r_dtraces* traces,
                                  uint32_t flags, uint8_t* proof_buf, size_t proof_cap, size_t* proof_len) {
  return guard(ctx, [&] {
    if (!layer || !traces || !proof_len || (!proof_buf && proof_cap)) fail(P3R_EINVAL, "bad arguments");
    auto bytes = P3R_FIELD_CALL(ctx, prove_all_tables, ctx, layer, traces,
                                (flags & P3R_PROVE_CANONICAL_FIELD_ENCODING) != 0);
    emit_proof(ctx, std::move(bytes), proof_buf, proof_cap, proof_len);
  });
}
int p3r_prove_all_tables(p3r_ctx* ctx, const p3r_layer* layer, const p3r_traces* traces, uint32_t flags,
                         uint8_t* proof_buf, size_t proof_cap, size_t* proof_len) {
  return guard(ctx, [&] {
    if (!layer || !traces || !proof_len || (!proof_buf && proof_cap)) fail(P3R_EINVAL, "bad arguments");
    auto d = P3R_FIELD_CALL(ctx, traces_upload, ctx, layer, traces);
    auto bytes = P3R_FIELD_CALL(ctx, prove_all_tables, ctx, layer, d.get(),
                                (flags & P3R_PROVE_CANONICAL_FIELD_ENCODING) != 0);
    emit_proof(ctx, std::move(bytes), proof_buf, proof_cap, proof_len);
  });
}
p3r_dmat* p3r_layer_build_main_trace(p3r_ctx* ctx, const p3r_layer* layer, const p3r_dtraces* traces,
                                     uint32_t table) {
  p3r_dmat* out = nullptr;
  guard(ctx, [&] {
    if (!layer || !traces || table > 6) fail(P3R_EINVAL, "bad arguments");
    if (layer->slot_of((int)table) < 0) fail(P3R_EINVAL, "table %u has no rows and is not part of the batch", table);
    auto m = P3R_FIELD_CALL(ctx, build_main_traces, ctx, layer, traces);
    P3R_HIP(hipStreamSynchronize(ctx->stream));
    out = m[table].release();
  });
  return out;
}

// ---- circuit boundary (circuit_impl.hip.h) ----
p3r_circuit* p3r_circuit_create(p3r_ctx* ctx, const p3r_circuit_desc* desc, uint32_t* commit_out) {
  p3r_circuit* out = nullptr;
  guard(ctx, [&] {
    if (!desc || !commit_out) fail(P3R_EINVAL, "NULL argument");
    if (p3r::ext_degree_is_binomial_generic(ctx->cfg.ext_degree))
      fail(P3R_EUNSUPPORTED, "UnsupportedDegree(%u): the device runner computes in degree 1, 4 and 5; hand the layer over as Traces",
           ctx->cfg.ext_degree);
    out = P3R_FIELD_CALL(ctx, circuit_create, ctx, desc, commit_out).release();
  });
  return out;
}
void p3r_circuit_free(p3r_ctx* ctx, p3r_circuit* circuit) {
  if (ctx) (void)hipStreamSynchronize(ctx->stream);
  delete circuit;
}
const p3r_layer* p3r_circuit_layer(const p3r_circuit* circuit) { return circuit ? circuit->layer.get() : nullptr; }
int p3r_circuit_counts(const p3r_circuit* circuit, p3r_layer_desc_counts* out) {
  if (!circuit || !out) return P3R_EINVAL;
  *out = circuit->counts;
  return P3R_OK;
}
int p3r_circuit_levels(const p3r_circuit* circuit, size_t* n_levels) {
  if (!circuit || !n_levels) return P3R_EINVAL;
  *n_levels = circuit->sched.levels;
  return P3R_OK;
}
int p3r_circuit_prepared_on_device(const p3r_circuit* circuit) { return circuit && circuit->prepared_on_device ? 1 : 0; }
p3r_dinputs* p3r_circuit_inputs_upload(p3r_ctx* ctx, const p3r_circuit* circuit, const p3r_circuit_inputs* inputs) {
  p3r_dinputs* out = nullptr;
  guard(ctx, [&] {
    if (!circuit || !inputs) fail(P3R_EINVAL, "NULL argument");
    out = P3R_FIELD_CALL(ctx, circuit_inputs_upload, ctx, circuit, inputs).release();
  });
  return out;
}
void p3r_circuit_inputs_free(p3r_ctx* ctx, p3r_dinputs* inputs) {
  if (ctx) (void)hipStreamSynchronize(ctx->stream);
  delete inputs;
}
p3r_dtraces* p3r_circuit_run_resident(p3r_ctx* ctx, const p3r_circuit* circuit, const p3r_dinputs* inputs) {
  p3r_dtraces* out = nullptr;
  guard(ctx, [&] {
    if (!circuit || !inputs) fail(P3R_EINVAL, "NULL argument");
    out = P3R_FIELD_CALL(ctx, circuit_run, ctx, circuit, inputs).release();
  });
  return out;
}
p3r_dtraces* p3r_circuit_run(p3r_ctx* ctx, const p3r_circuit* circuit, const p3r_circuit_inputs* inputs) {
  p3r_dtraces* out = nullptr;
  guard(ctx, [&] {
    if (!circuit || !inputs) fail(P3R_EINVAL, "NULL argument");
    auto d = P3R_FIELD_CALL(ctx, circuit_inputs_upload, ctx, circuit, inputs);
    out = P3R_FIELD_CALL(ctx, circuit_run, ctx, circuit, d.get()).release();
  });
  return out;
}
static void prove_next_layer_impl(p3r_ctx* ctx, const p3r_circuit* circuit, const p3r_dinputs* d, uint32_t flags,
                                  uint8_t* proof_buf, size_t proof_cap, size_t* proof_len) {
  // The run is enqueued, not awaited: proving starts behind it on the stream, and the run's error
  // word lands in a pinned host word that is read once the proof is done.  (A failed run leaves
  // garbage VALUES in the traces, never a bad address, so proving over them is harmless; its error
  // takes precedence over whatever the prover made of the garbage.)
  uint32_t* run_err = nullptr;
  P3R_HIP(ctx->stage.words(&run_err));
  *run_err = 0xFFFFFFFFu;
  auto t = P3R_FIELD_CALL(ctx, circuit_run, ctx, circuit, d, run_err);
  std::vector<uint8_t> bytes;
  try {
    bytes = P3R_FIELD_CALL(ctx, prove_all_tables, ctx, circuit->layer.get(), t.get(),
                           (flags & P3R_PROVE_CANONICAL_FIELD_ENCODING) != 0);
  } catch (...) {
    if (hipStreamSynchronize(ctx->stream) == hipSuccess) run_raise_error(*run_err);
    throw;
  }
  run_raise_error(*run_err);  // prove_all_tables returns with the stream drained
  emit_proof(ctx, std::move(bytes), proof_buf, proof_cap, proof_len);
}
int p3r_prove_next_layer(p3r_ctx* ctx, const p3r_circuit* circuit, const p3r_circuit_inputs* inputs,
                         uint32_t flags, uint8_t* proof_buf, size_t proof_cap, size_t* proof_len) {
  return guard(ctx, [&] {
    if (!circuit || !inputs || !proof_len || (!proof_buf && proof_cap)) fail(P3R_EINVAL, "bad arguments");
    auto d = P3R_FIELD_CALL(ctx, circuit_inputs_upload, ctx, circuit, inputs);
    prove_next_layer_impl(ctx, circuit, d.get(), flags, proof_buf, proof_cap, proof_len);
  });
}
int p3r_prove_next_layer_resident(p3r_ctx* ctx, const p3r_circuit* circuit, const p3r_dinputs* inputs,
                                  uint32_t flags, uint8_t* proof_buf, size_t proof_cap, size_t* proof_len) {
  return guard(ctx, [&] {
    if (!circuit || !inputs || !proof_len || (!proof_buf && proof_cap)) fail(P3R_EINVAL, "bad arguments");
    prove_next_layer_impl(ctx, circuit, inputs, flags, proof_buf, proof_cap, proof_len);
  });
}
int p3r_dtraces_get(p3r_ctx* ctx, const p3r_layer* layer, const p3r_dtraces* traces, uint32_t which,
                    uint32_t* out, size_t out_len) {
  return guard(ctx, [&] {
    if (!layer || !traces || (!out && out_len)) fail(P3R_EINVAL, "NULL argument");
    P3R_FIELD_CALL(ctx, dtraces_get, ctx, layer, traces, which, out, out_len);
  });
}

int p3r_profile_enable(p3r_ctx* ctx, int on) {
  return guard(ctx, [&] {
    P3R_HIP(hipStreamSynchronize(ctx->stream));
    prof_clear(ctx);
    ctx->prof_enabled = on != 0;
  });
}

int p3r_profile_read(p3r_ctx* ctx, p3r_profile_entry* out, size_t cap, size_t* n_out) {
  return guard(ctx, [&] {
    if (!out || !n_out) fail(P3R_EINVAL, "NULL argument");
    P3R_HIP(hipStreamSynchronize(ctx->stream));
    std::vector<p3r_profile_entry> acc;
    for (auto& r : ctx->prof) {
      float ms = 0;
      P3R_HIP(hipEventElapsedTime(&ms, r.a, r.b));
      auto it = std::find_if(acc.begin(), acc.end(),
                             [&](const p3r_profile_entry& e) { return !strcmp(e.name, r.name); });
      if (it == acc.end()) {
        p3r_profile_entry e{};
        strncpy(e.name, r.name, sizeof e.name - 1);
        acc.push_back(e);
        it = acc.end() - 1;
      }
      it->total_ms += ms;
      it->launches += 1;
    }
    for (auto& kv : ctx->stage_ms) {
      p3r_profile_entry e{};
      snprintf(e.name, sizeof e.name, "stage:%s", kv.first.c_str());
      e.total_ms = kv.second;
      acc.push_back(e);
    }
    if (acc.size() > cap) fail(P3R_EBUFFER, "need room for %zu profile entries", acc.size());
    std::copy(acc.begin(), acc.end(), out);
    *n_out = acc.size();
  });
}

}  // extern "C"
