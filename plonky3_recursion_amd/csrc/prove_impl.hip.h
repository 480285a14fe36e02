// prove_batch on the GPU: the body the reference delegates to p3_batch_stark::prove_batch
// (call site circuit-prover/src/batch_stark_prover.rs:1595).  Included into p3r_core.hip.
//
// Stage order and transcript are pinned by the in-tree circuit verifier:
//   transcript head, commitments, challenges   recursion/src/verifier/batch_stark.rs:521-627
//   rounds / opening points                     recursion/src/verifier/batch_stark.rs:645-852
//   opened-value observation order              recursion/src/verifier/batch_stark.rs:1114-1276
//   quotient domain / chunks                    recursion/src/verifier/batch_stark.rs:701-717,
//                                               recursion/src/verifier/quotient.rs:60-140
//   FRI challenges, arities, PoW, queries       recursion/src/pcs/fri/targets.rs:748-866
//   reduced openings / folding / final poly     recursion/src/pcs/fri/verifier.rs:562-781,887-915,1068-1356
//   ZK (p3r_config.zk, HidingFriPcs)            recursion/src/verifier/batch_stark.rs:424-428,487-490,536,623-661,701-735,
//                                               855-864,1116-1260; pcs/fri/targets.rs:1076-1130 - the prover side is
//                                               un-vendored and randomised: written from those acceptance conditions
// All matrices stay resident in HBM; only commitments, opened values, the final polynomial
// and the query answers cross to the host.
#include "host_transcript.h"
#include "kernels_stark.hip.h"
#include "kernels_fri_reduce.hip.h"
#include "kernels_zk.hip.h"
#include "open_impl.hip.h"

struct p3r_prep {
  std::vector<p3r::AirParams> airs;
  std::vector<std::unique_ptr<p3r_dmat>> traces;  // preprocessed traces (K7 and openings read them)
  std::vector<std::unique_ptr<p3r_dmat>> evals;   // ZK: the committed evaluations, 2h x (w + R), zero-padded (else empty)
  std::vector<std::unique_ptr<p3r_dmat>> ldes;    // their bit-reversed LDEs (K8, FRI)
  std::vector<size_t> heights;                    // BASE trace heights
  int zk_codewords = -1;                          // R the preparation was committed with (0: not ZK)
  const p3r_dmat* committed(size_t i) const { return evals.empty() ? traces[i].get() : evals[i].get(); }
  std::unique_ptr<p3r_tree> tree;
  std::vector<uint32_t> cap_canonical;
};

namespace {

template <class PP, int DC = 4>
EW<DC> to_e4(const typename Chal<PP, DC>::type& e) { return e4_store<PP, DC>(e); }

template <class PP, int DC = 4>
std::vector<typename Chal<PP, DC>::type> download_ef(p3r_ctx* ctx, const uint32_t* dev, size_t count) {
  std::vector<uint32_t> raw(count * DC);
  P3R_HIP(fetch_small(ctx, dev, raw.size(), raw.data()));
  std::vector<typename Chal<PP, DC>::type> out(count);
  for (size_t i = 0; i < count; ++i)
    for (int k = 0; k < DC; ++k) out[i].c[k] = Fp<PP>::raw(raw[i * DC + k]);
  return out;
}

// The context's generator key with a proof's nonce (zk_rand.h).
inline ZkKey zk_key_of(const p3r_ctx* ctx, uint64_t nonce) {
  ZkKey k{};
  for (int i = 0; i < 8; ++i) k.k[i] = ctx->zk_key[i];
  k.nonce_lo = (uint32_t)nonce; k.nonce_hi = (uint32_t)(nonce >> 32);
  return k;
}

// the tiled fills of kernels_zk.hip.h (one ChaCha block per eight cells)
template <class PP>
void launch_zk_tiles(p3r_ctx* ctx, std::vector<ZkTileJob>& jobs, const ZkKey& key, const char* family) {
  uint64_t blocks = 0;
  for (auto& j : jobs) {
    if (2 * (uint64_t)(j.w2 | 1u) > kZkTileWords) fail(P3R_EUNSUPPORTED, "ZK fill of a matrix of %u columns", j.w2);
    j.log_tr = zk_tile_log_rows(j.rows, j.w2);
    j.block0 = (uint32_t)blocks;
    blocks += j.rows >> j.log_tr;
  }
  if (blocks >= (uint64_t(1) << 31)) fail(P3R_EUNSUPPORTED, "ZK fill launch of %llu tiles", (unsigned long long)blocks);
  if (!blocks) return;
  DevBuf d_jobs((jobs.size() * sizeof(ZkTileJob) + 3) / 4);
  P3R_HIP(ctx->stage.upload(ctx->stream, d_jobs.p, jobs.data(), jobs.size() * sizeof(ZkTileJob)));
  ProfScope ps(ctx, family);
  hipLaunchKernelGGL(k_zk_fill_tiles<PP>, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, reinterpret_cast<const ZkTileJob*>(d_jobs.p),
                     (int)jobs.size(), key);
  P3R_HIP(hipGetLastError());
}

// Salt matrices of a hiding MMCS for the matrices of one batch (commit order): h x S each, one launch.
template <class PP>
std::vector<std::unique_ptr<p3r_dmat>> draw_salts(p3r_ctx* ctx, const std::vector<const p3r_dmat*>& mats, int salt_round, const ZkKey& key) {
  const uint32_t S = ctx->cfg.mmcs_salt_elems;
  std::vector<std::unique_ptr<p3r_dmat>> out;
  std::vector<ZkTileJob> tj;
  for (size_t i = 0; i < mats.size(); ++i) {
    out.push_back(dmat_alloc(mats[i]->h, S));
    ZkTileJob j{};
    j.dst = out.back()->d; j.rows = mats[i]->h; j.w2 = S; j.mode = 1; j.stride = 1;
    j.stream = zk_stream_id(salt_round, i);
    tj.push_back(j);
  }
  launch_zk_tiles<PP>(ctx, tj, key, "mmcs_salts");
  return out;
}

// `salt_round` >= 0 under a hiding MMCS (p3r_config.mmcs_salt_elems > 0): the stream round of this batch's salts.
template <class PP>
std::unique_ptr<p3r_tree> commit_dmats(p3r_ctx* ctx, const std::vector<const p3r_dmat*>& mats,
                                       std::vector<uint32_t>& cap_mont, int salt_round = -1, const ZkKey* key = nullptr) {
  auto tree = std::make_unique<p3r_tree>();
  tree->mats = mats;
  if (ctx->cfg.mmcs_salt_elems) {
    if (salt_round < 0 || !key) fail(P3R_EHIP, "internal: a commit without its salt stream under a hiding MMCS");
    tree->salt_elems = (int)ctx->cfg.mmcs_salt_elems;
    tree->salt_owned = draw_salts<PP>(ctx, mats, salt_round, *key);
    tree->mats.clear();
    for (size_t i = 0; i < mats.size(); ++i) { tree->mats.push_back(mats[i]); tree->mats.push_back(tree->salt_owned[i].get()); }
  }
  cap_mont = mmcs_commit<PP>(ctx, tree.get());
  return tree;
}

// Coset LDE + MMCS commitment of one round's matrices (TwoAdicFriPcs::commit), back to back on the ctx's one stream
// (a second stream for the leaf hashing gained too little: profiles/r05/commit_overlap_ab.txt).
template <class PP>
std::unique_ptr<p3r_tree> lde_and_commit(p3r_ctx* ctx, const std::vector<LdeItem>& items, int log_blowup,
                                         std::vector<std::unique_ptr<p3r_dmat>>& ldes, std::vector<uint32_t>& cap_mont,
                                         int salt_round = -1, const ZkKey* key = nullptr) {
  ldes.clear();
  ldes.resize(items.size());
  std::vector<const p3r_dmat*> ptrs(items.size());
  host_mark("lde: enqueue");
  auto out = coset_lde_batch<PP>(ctx, items, log_blowup);
  host_mark("lde: enqueued; commit: enqueue");
  for (size_t i = 0; i < items.size(); ++i) { ldes[i] = std::move(out[i]); ptrs[i] = ldes[i].get(); }
  return commit_dmats<PP>(ctx, ptrs, cap_mont, salt_round, key);
}

// Proof-of-work grinding on the device: the smallest witness w such that, after observing w, the
// low `bits` bits of the next sample are zero (recursion/src/challenger/circuit.rs:409-430).
// Leaves the host challenger in the post-check state.  bits == 0: witness 0, transcript untouched.
template <class PP, class Challenger>
Fp<PP> grind_witness(p3r_ctx* ctx, Challenger& ch, int bits) {
  using F = Fp<PP>;
  if (bits == 0) return F::zero();
  if (bits > 30) fail(P3R_EINVAL, "proof-of-work bits must be <= 30");
  GrindArgs g{};
  for (int k = 0; k < 16; ++k) g.state[k] = ch.state[k].v;
  g.n_pending = (int)ch.in_buf.size();
  for (int k = 0; k < g.n_pending; ++k) g.pending[k] = ch.in_buf[k].v;
  g.bits = bits;
  g.rc = ctx->rc.p;
  DevBuf res(1);
  g.result = res.p;
  uint32_t found = 0xFFFFFFFFu;
  // 4x the expected number of tries per launch: a miss (e^-4) costs one more round trip, while a
  // larger batch makes every proof pay for permutations past the witness
  const uint32_t batch = 1u << std::min<uint32_t>(std::max<uint32_t>(bits + 2, 12), 24);
  // 2^(bits+10) candidates all miss with probability e^-1024; stop there instead of sweeping the field
  const uint64_t limit = std::min<uint64_t>(PP::P, (uint64_t(1) << std::min<uint32_t>(bits + 10, 31)) + batch);
  for (uint64_t base = 0; base < limit && found == 0xFFFFFFFFu; base += batch) {
    P3R_HIP(fill_async(ctx->stream, res.p, 0xFF, 4));
    g.base = (uint32_t)base;
    ProfScope ps(ctx, "grind");
    hipLaunchKernelGGL(k_grind<PP>, dim3(batch / kBlock), dim3(kBlock), 0, ctx->stream, g);
    P3R_HIP(fetch_small(ctx, res.p, 1, &found));
  }
  if (found == 0xFFFFFFFFu) fail(P3R_EINVAL, "proof-of-work search found no witness");
  const F w = F::from_canonical(found);
  if (!ch.check_witness(bits, w)) fail(P3R_EHIP, "device PoW witness rejected on host");
  return w;
}

// The final polynomial of FRI (ProofState::final_polynomial, p3r_fri_final_poly_dmat): `raw` is the last folded vector as
// fetched, [DC][m] Montgomery planes, m = 2^log_m values over <w_m> in bit-reversed order.  Returns the 2^log_final_poly_len
// low coefficients in natural order; a non-zero coefficient above them is refused.
template <class PP, int DC>
std::vector<typename Chal<PP, DC>::type> fri_final_poly(const uint32_t* raw, int log_m, uint32_t log_final_poly_len) {
  using F = Fp<PP>;
  using E = typename Chal<PP, DC>::type;
  const size_t m = size_t(1) << log_m;
  // inverse DFT, decimation in time: the rows are already in bit-reversed order, the
  // coefficients come out in natural order
  std::vector<E> coeffs(m);
  for (size_t i = 0; i < m; ++i)
    for (int k = 0; k < DC; ++k) coeffs[i].c[k] = F::raw(raw[(size_t)k * m + i]);
  const F w_inv = F::two_adic_generator(log_m).inv(), m_inv = F::from_u64(m).inv();
  for (size_t len = 2; len <= m; len <<= 1) {
    const F w_len = w_inv.pow(m / len);
    for (size_t i = 0; i < m; i += len) {
      F x = F::one();
      for (size_t j = 0; j < len / 2; ++j) {
        const E u = coeffs[i + j], v = coeffs[i + j + len / 2] * x;
        coeffs[i + j] = u + v;
        coeffs[i + j + len / 2] = u - v;
        x *= w_len;
      }
    }
  }
  for (auto& c : coeffs) c = c * m_inv;
  const size_t flen = size_t(1) << log_final_poly_len;
  for (size_t i = flen; i < m; ++i)
    if (!coeffs[i].is_zero())
      fail(P3R_EINVAL, "FRI final polynomial has degree >= 2^%u: the traces do not satisfy the constraints", log_final_poly_len);
  coeffs.resize(flen);
  return coeffs;
}

inline int zk_codewords(const p3r_config& cfg) { return cfg.zk ? (cfg.num_random_codewords ? (int)cfg.num_random_codewords : 2) : 0; }

// HidingFriPcs::commit on a batch of matrices (kernels_zk.hip.h): h x w -> 2h x (w + R) each, one launch.
// src[i] == nullptr: a fully random 2 * h[i] x (w[i] + R) matrix (w[i] = the width before the codeword columns).
template <class PP>
std::vector<std::unique_ptr<p3r_dmat>> zk_randomize(p3r_ctx* ctx, const std::vector<const p3r_dmat*>& src, const std::vector<size_t>& h,
                                                    const std::vector<size_t>& w, int R, const std::vector<uint32_t>& streams, const ZkKey& key,
                                                    bool zero_fill) {
  std::vector<std::unique_ptr<p3r_dmat>> out;
  std::vector<ZkRandomizeJob> jobs;
  uint64_t blocks = 0;
  for (size_t i = 0; i < h.size(); ++i) {
    out.push_back(dmat_alloc(2 * h[i], w[i] + (size_t)R));
    ZkRandomizeJob j{};
    j.src = src[i] ? src[i]->d : nullptr;
    j.dst = out.back()->d;
    j.h2 = 2 * h[i];
    j.w = src[i] ? (uint32_t)w[i] : 0u;
    j.w2 = (uint32_t)(w[i] + (size_t)R);
    j.zero_fill = zero_fill ? 1u : 0u;
    j.stream = streams[i];
    if ((uint64_t)j.h2 * j.w2 >= (uint64_t(1) << 35)) fail(P3R_EUNSUPPORTED, "ZK: a matrix of 2^35 cells or more");
    j.block0 = (uint32_t)blocks;
    blocks += (uint64_t)j.w2 * ((j.h2 + kBlock - 1) / kBlock);
    jobs.push_back(j);
  }
  if (blocks >= (uint64_t(1) << 31)) fail(P3R_EUNSUPPORTED, "ZK randomisation launch of %llu tiles", (unsigned long long)blocks);
  if (jobs.empty()) return out;
  if (!zero_fill) {   // (a zero fill draws nothing: the per-cell kernel is the cheap one there)
    std::vector<ZkTileJob> tj;
    for (auto& j : jobs) {
      ZkTileJob t{};
      t.src = j.src; t.dst = j.dst; t.rows = j.h2; t.w = j.w; t.w2 = j.w2; t.stride = 1; t.stream = j.stream;
      t.mode = j.src ? 0u : 1u;   // no source matrix (the random round): every cell is random
      tj.push_back(t);
    }
    launch_zk_tiles<PP>(ctx, tj, key, "zk_randomize");
    return out;
  }
  DevBuf d_jobs((jobs.size() * sizeof(ZkRandomizeJob) + 3) / 4);
  P3R_HIP(ctx->stage.upload(ctx->stream, d_jobs.p, jobs.data(), jobs.size() * sizeof(ZkRandomizeJob)));
  ProfScope ps(ctx, "zk_randomize");
  hipLaunchKernelGGL(k_zk_randomize<PP>, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream,
                     reinterpret_cast<const ZkRandomizeJob*>(d_jobs.p), (int)jobs.size(), key);
  P3R_HIP(hipGetLastError());
  return out;
}

// `dev_traces`: the preprocessed traces already in HBM (column-major, Montgomery: the device-side preparation
// writes them there); otherwise they are uploaded from the host matrices `mats`.
template <class PP>
std::unique_ptr<p3r_prep> prep_create(p3r_ctx* ctx, const p3r_air_desc* airs, const p3r_matrix* mats, size_t n,
                                      std::vector<std::unique_ptr<p3r_dmat>>* dev_traces = nullptr) {
  using F = Fp<PP>;
  auto prep = std::make_unique<p3r_prep>();
  std::vector<LdeItem> items;
  for (size_t i = 0; i < n; ++i) {
    AirParams a{(int)airs[i].kind, (int)airs[i].lanes, (int)airs[i].horner_packed_steps, (int)airs[i].coeff_lookups,
                (ctx->cfg.ext_choices & P3R_EXT_LOOKUP_UNPACKED) ? 1 : 0, (int)ctx->cfg.ext_degree,
                ext_degree_is_binomial_generic(ctx->cfg.ext_degree) ? Fp<PP>::from_canonical(ctx->cfg.ext_w).v : 0u};
    if (ext_degree_is_binomial_generic(ctx->cfg.ext_degree) && a.kind == AIR_POSEIDON2)
      fail(P3R_EUNSUPPORTED, "instance %zu: UnsupportedDegree(%d): no Poseidon2 table for this circuit degree", i, a.ext_d);
    if (a.kind < 0 || a.kind > AIR_POSEIDON2_W32) fail(P3R_EINVAL, "instance %zu: unknown AIR kind %d", i, a.kind);
    if (a.kind == AIR_POSEIDON2_W32) require_w32_constants(ctx);
    if (a.kind == AIR_POSEIDON2_W32 && ctx->cfg.ext_degree != 4)
      fail(P3R_EUNSUPPORTED, "instance %zu: the width-32 Poseidon2 table belongs to D = 4 circuits", i);
    if (a.lanes < 1) fail(P3R_EINVAL, "instance %zu: lanes must be positive", i);
    if (a.kind == AIR_ALU && (a.horner_k < 2 || a.horner_k > 8))
      fail(P3R_EINVAL, "instance %zu: horner_packed_steps must be in 2..8", i);
    const size_t width = dev_traces ? (*dev_traces)[i]->w : mats[i].width, height = dev_traces ? (*dev_traces)[i]->h : mats[i].height;
    if ((int)width != air_prep_width_of(a))
      fail(P3R_EINVAL, "instance %zu: preprocessed width %zu, the AIR expects %d", i, width, air_prep_width_of(a));
    {
      // known at preparation time: a quotient of 2^(log_chunks) cosets (twice as many under ZK) is evaluated ON the
      // committed LDE here, so log_chunks must not exceed log_blowup.  Upstream re-evaluates on the larger domain
      // instead; that is a capability this prover lacks, not a caller error - said so, and said early
      const LookupLayout lay = lookup_layout(a, ctx->cfg.zk ? 1 : 0);
      if (lay.log_chunks > (int)ctx->cfg.log_blowup)
        fail(P3R_EUNSUPPORTED, "instance %zu: quotient domain larger than the LDE: constraint degree needs log_blowup >= %d%s, log_blowup is %u "
             "(upstream extends the traces to the quotient domain in this case; this prover does not)", i, lay.log_chunks,
             ctx->cfg.zk ? " under zk = 1" : "", ctx->cfg.log_blowup);
    }
    prep->airs.push_back(a);
    prep->heights.push_back(height);
    auto m = dev_traces ? std::move((*dev_traces)[i]) : upload<PP>(ctx, mats[i].values, mats[i].height, mats[i].width);
    items.push_back({m.get(), PP::GEN});
    prep->traces.push_back(std::move(m));
  }
  prep->zk_codewords = zk_codewords(ctx->cfg);
  if (ctx->cfg.zk) {
    // commit_preprocessing of a hiding PCS: the same extended domain and codeword columns, padded with ZEROS - public
    // data, and the commitment stays a function of the circuit shape (p3r.h: p3r_config.zk)
    std::vector<const p3r_dmat*> src;
    std::vector<size_t> hs, ws;
    for (auto& t : prep->traces) { src.push_back(t.get()); hs.push_back(t->h); ws.push_back(t->w); }
    prep->evals = zk_randomize<PP>(ctx, src, hs, ws, prep->zk_codewords, std::vector<uint32_t>(n, 0), ZkKey{}, true);
    for (size_t i = 0; i < n; ++i) items[i].in = prep->evals[i].get();
  }
  std::vector<uint32_t> cap_mont;
  // a hiding MMCS salts the preprocessed commitment too; it is made once per circuit: the nonce of `proof 0`
  const ZkKey prep_key = zk_key_of(ctx, 0);
  prep->tree = lde_and_commit<PP>(ctx, items, (int)ctx->cfg.log_blowup, prep->ldes, cap_mont, kSaltRound + ZK_ROUND_PREP, &prep_key);
  prep->cap_canonical.resize(cap_mont.size());
  for (size_t i = 0; i < cap_mont.size(); ++i) prep->cap_canonical[i] = F::raw(cap_mont[i]).to_canonical();
  return prep;
}

// One committed round of a proof.  `mats` in commit order: per matrix the committed evaluations (what is opened), their
// LDE (what FRI reduces and the queries open), the opening points and the opened values.
template <class PP, int DC>
struct ProofRound {
  using E = typename Chal<PP, DC>::type;
  struct Mat {
    int inst;                                     // the instance the matrix belongs to
    const p3r_dmat *ev, *lde;
    Fp<PP> shift;                                 // `ev` holds evaluations over shift * <w>
    std::vector<E> z;                             // the opening points
    size_t job = 0;                               // its Opener job
    std::vector<std::vector<E>> vals, codewords;  // per point: the AIR's columns, then (ZK) the R random codewords
  };
  std::unique_ptr<p3r_tree> own;
  const p3r_tree* tree = nullptr;                 // null: not a round of this proof (preprocessed: the preparation's)
  std::vector<uint32_t> cap;                      // Montgomery form
  std::vector<std::unique_ptr<p3r_dmat>> keep, lde;  // what this proof made for the round: evaluations, masks; LDEs
  std::vector<Mat> mats;
};

// One proof of prove_batch: a member function per protocol phase, in transcript order, over the state that one phase
// leaves for a later one.  Every device buffer held here lives until the proof is written.
// DC: the degree of the challenge field (p3r_config.challenge_degree): 4, or 5 = KoalaBear's quintic trinomial
// extension.  Extension vectors on the device are DC planes ([DC][n]); the proof writes DC words per element.
template <class PP, int DC>
struct BatchProver {
  using F = Fp<PP>;
  using E = typename Chal<PP, DC>::type;
  using Round = ProofRound<PP, DC>;
  using Mat = typename Round::Mat;
  static constexpr size_t kMaxPhases = 32;

  p3r_ctx* const ctx;
  const p3r_prep* const prep;
  const p3r_dmat* const* const mains;
  const size_t ni;
  const p3r_config& cfg;
  const int log_blowup;
  // ZK (HidingFriPcs): every committed matrix lives over the extended trace domain (log_e = log_n + 1) with R random
  // codeword columns; the nonce in `zk_key` keys this proof's random values (zk_rand.h)
  const int zk, R;
  const ZkKey zk_key;
  std::vector<LookupLayout> layouts;
  std::vector<int> log_n, log_e;
  const F gen = F::generator();
  std::vector<uint32_t> rc_mont;
  HostChallenger<PP, DC> ch;
  ProofWriter<PP, DC> W;
  Round main_round, perm_round, quot_round, rand_round, prep_round;
  LookupChT<DC> lc{};
  std::vector<E> terminals;
  E alpha, zeta;
  DevBuf d_apow, d_fapow;
  Opener<PP, DC> op;  // keeps the opened values on the device for the reduced openings
  std::map<std::array<uint64_t, 6>, uint32_t*> inv_cache;  // (log_height, z) -> 1/(z - x_r)
  std::vector<DevBuf> inv_keep;
  std::map<int, std::pair<E, DevBuf>> ros;  // log_height -> (alpha power, ro planes [DC][h])
  struct Phase { int la; size_t rows; DevBuf folded_in; std::unique_ptr<p3r_tree> tree; std::vector<uint32_t> cap; };
  std::vector<Phase> phases;
  int log_max = 0;
  DevBuf folded, d_tstate, d_phase;
  std::vector<F> commit_pow_witnesses;
  std::vector<E> final_poly;
  F query_pow_witness;
  // an opening proof inside a query's block, from `at` on: per level of the tree (mmcs4.h) the siblings at positions
  // pos ^ 1 .. pos ^ (step - 1), written out in ascending position
  struct QPath { uint32_t at = 0; const p3r_tree* t = nullptr; };
  struct QRound { std::vector<std::pair<uint32_t, uint32_t>> rows; QPath path; uint32_t tree_shift; };
  struct QPhase { uint32_t sib_at[16]; QPath path; int shift; uint32_t salt_at = 0; };
  std::vector<size_t> indices;
  std::vector<QRound> qrounds;
  std::vector<QPhase> qphases;
  uint32_t words_per_query = 0;
  const uint32_t* gathered = nullptr;  // in the ctx's pinned landing area, read in place when serialising

  // Checks the traces against the preparation; a proof that needs a nonce draws it here.
  BatchProver(p3r_ctx* c, const p3r_prep* p, const p3r_dmat* const* m, size_t n, bool canonical_encoding)
      : ctx(c), prep(p), mains(m), ni(n), cfg(c->cfg), log_blowup((int)cfg.log_blowup), zk(cfg.zk ? 1 : 0), R(zk_codewords(cfg)),
        zk_key(zk_key_of(c, (zk || cfg.mmcs_salt_elems) ? c->zk_nonce++ : 0)),  // (the salts of a hiding MMCS are per proof too)
        layouts(n), log_n(n), log_e(n), rc_mont(c->rc_canonical.size()), ch(rc_mont.data()), terminals(n, E::zero()),
        op(c) {
    const int p2w = p2_perm_cols<PP>() + 2;
    for (size_t i = 0; i < ni; ++i) {
      const AirParams& a = prep->airs[i];
      if (mains[i]->h != prep->heights[i])
        fail(P3R_EINVAL, "instance %zu: trace height %zu != preprocessed height %zu", i, mains[i]->h, prep->heights[i]);
      if ((int)mains[i]->w != air_width_of(a, p2w, p2w_perm_cols<PP>() + 4))
        fail(P3R_EINVAL, "instance %zu: trace width %zu, the AIR expects %d", i, mains[i]->w, air_width_of(a, p2w, p2w_perm_cols<PP>() + 4));
      log_n[i] = log2_exact(mains[i]->h, "trace height");
      log_e[i] = log_n[i] + zk;
      layouts[i] = lookup_layout(a, zk);
      if (layouts[i].log_chunks > log_blowup) fail(P3R_EUNSUPPORTED, "quotient domain larger than the LDE (zk %d, log_blowup %d)", zk, log_blowup);
      if ((1 << (layouts[i].log_chunks + zk)) > 8) fail(P3R_EUNSUPPORTED, "more than 8 quotient chunks");
    }
    for (size_t i = 0; i < rc_mont.size(); ++i) rc_mont[i] = F::from_canonical(ctx->rc_canonical[i]).v;
    W.canonical = canonical_encoding;
    prep_round.tree = prep->tree.get();
    for (size_t i = 0; i < ni; ++i) prep_round.mats.push_back({(int)i, prep->committed(i), prep->ldes[i].get(), F::one()});
  }

  // The verifier's round order (batch_stark.rs:645-852), followed by the openings, a query's rounds and the ZK codeword
  // values: [random,] main, quotient, preprocessed, permutation.  (The transcript observes main, perm., quotient, random.)
  std::vector<Round*> rounds() {
    std::vector<Round*> rs;
    for (Round* r : {&rand_round, &main_round, &quot_round, &prep_round, &perm_round})
      if (r->tree) rs.push_back(r);
    return rs;
  }

  // the permutation round's matrix of instance i; null: the instance has no lookups
  const Mat* perm_mat(size_t i) const {
    for (const Mat& m : perm_round.mats)
      if (m.inst == (int)i) return &m;
    return nullptr;
  }

  // Coset LDE + commitment of a round's matrices.  The LDE evaluates each polynomial on gen * <w>: a shift of
  // GENERATOR / domain shift.  The caller observes the commitment.
  void commit(Round& r, int zk_round) {
    std::vector<LdeItem> items;
    for (const Mat& m : r.mats) items.push_back({m.ev, (gen * m.shift.inv()).to_canonical()});
    r.own = lde_and_commit<PP>(ctx, items, log_blowup, r.lde, r.cap, kSaltRound + zk_round, &zk_key);
    r.tree = r.own.get();
    for (size_t k = 0; k < r.mats.size(); ++k) r.mats[k].lde = r.lde[k].get();
  }

  // ZK: what a round commits and opens are the randomised extensions of its matrices
  void randomise(Round& r, int zk_round) {
    std::vector<const p3r_dmat*> src;
    std::vector<size_t> hs, ws;
    std::vector<uint32_t> keys;
    for (size_t k = 0; k < r.mats.size(); ++k) {
      const p3r_dmat* a = r.mats[k].ev;
      src.push_back(a); hs.push_back(a->h); ws.push_back(a->w); keys.push_back(zk_stream_id(zk_round, k));
    }
    auto rs = zk_randomize<PP>(ctx, src, hs, ws, R, keys, zk_key, false);
    for (size_t k = 0; k < rs.size(); ++k) {
      r.mats[k].ev = rs[k].get();
      r.keep.push_back(std::move(rs[k]));
    }
  }

  // ---- 1. main LDEs + commitment
  void main_lde_commit() {
    prof_stage(ctx, "main_lde_commit");
    for (size_t i = 0; i < ni; ++i) main_round.mats.push_back({(int)i, mains[i], nullptr, F::one()});
    if (zk) randomise(main_round, ZK_ROUND_MAIN);
    commit(main_round, ZK_ROUND_MAIN);
  }

  // ---- 2. transcript head
  void transcript_head() {
    prof_stage(ctx, "transcript_head");
    ch.observe_base_as_ext(ni);
    for (size_t i = 0; i < ni; ++i) {
      ch.observe_base_as_ext(log_e[i]);   // extended degree bits, base degree bits, width, chunk count (:538-558)
      ch.observe_base_as_ext(log_n[i]);
      ch.observe_base_as_ext(mains[i]->w);
      ch.observe_base_as_ext(uint64_t(1) << (layouts[i].log_chunks + zk));
    }
    for (uint32_t v : main_round.cap) ch.observe(F::raw(v));
    for (size_t i = 0; i < ni; ++i) ch.observe_base_as_ext(air_prep_width_of(prep->airs[i]));
    for (uint32_t v : prep->cap_canonical) ch.observe(F::from_canonical(v));
  }

  // ---- 3. LogUp: challenges, aux traces, commitment, terminals
  void logup_aux_commit() {
    prof_stage(ctx, "logup_aux_commit");
    bool any_lookup = false;
    for (auto& L : layouts) any_lookup |= L.n_groups > 0;
    if (!any_lookup) return;
    E alpha_l = ch.sample_ext(), beta_l = ch.sample_ext();
    E bp = E::one();
    // the widest tuple on the bus is (idx, v_0..v_{D-1}): gamma = beta^(D+1)
    const int tuple_w = (int)ctx->cfg.ext_degree + 1;
    for (int j = 0; j < tuple_w; ++j) { lc.beta_pow[j] = to_e4<PP, DC>(bp); bp *= beta_l; }
    lc.prefix = to_e4<PP, DC>(alpha_l + bp);  // alpha + beta^(D+1), bus id 0
    DevBuf totals(DC * ni);
    P3R_HIP(fill_async(ctx->stream, totals.p, 0, 4 * DC * ni));
    // aux traces of all tables: fractions per row, then the running sum as a three-phase scan
    std::vector<LogupJob> jobs;
    std::vector<DevBuf> scratch;
    uint32_t row_blocks = 0, tiles = 0;
    for (size_t i = 0; i < ni; ++i) {
      const auto& L = layouts[i];
      if (!L.n_groups) continue;
      const size_t n = mains[i]->h;
      perm_round.keep.push_back(dmat_alloc(n, (size_t)L.aux_width() * DC));
      LogupJob j{};
      j.air = prep->airs[i];
      j.main = mains[i]->d;
      // the preprocessed TRACE (not the LDE): kept from preparation for this pass and the openings
      j.prep = prep->traces[i]->d;
      j.aux = perm_round.keep.back()->d;
      j.n = n;
      j.pair = L.pair;
      j.n_tiles = (uint32_t)((n + kScanTile - 1) / kScanTile);
      scratch.emplace_back(DC * n);
      j.rowsum = scratch.back().p;
      scratch.emplace_back(DC * (size_t)j.n_tiles);
      j.agg = scratch.back().p;
      j.total = totals.p + DC * i;
      j.block0 = row_blocks;
      j.tile0 = tiles;
      row_blocks += blocks_for(n);
      tiles += j.n_tiles;
      jobs.push_back(j);
      perm_round.mats.push_back({(int)i, perm_round.keep.back().get(), nullptr, F::one()});
    }
    {
      scratch.emplace_back((jobs.size() * sizeof(LogupJob) + 3) / 4);
      const auto* d_jobs = reinterpret_cast<const LogupJob*>(scratch.back().p);
      P3R_HIP(ctx->stage.upload(ctx->stream, scratch.back().p, jobs.data(), jobs.size() * sizeof(LogupJob)));
      const int nj = (int)jobs.size();
      ProfScope ps(ctx, "logup_aux");
      launch_logup_aux<PP, DC>(ctx, row_blocks, d_jobs, nj, lc);
      hipLaunchKernelGGL((k_ef_scan<PP, DC>), dim3(tiles), dim3(kBlock), 0, ctx->stream, 0, d_jobs, nj);
      hipLaunchKernelGGL((k_ef_scan<PP, DC>), dim3((unsigned)nj), dim3(kBlock), 0, ctx->stream, 1, d_jobs, nj);
      hipLaunchKernelGGL((k_ef_scan<PP, DC>), dim3(tiles), dim3(kBlock), 0, ctx->stream, 2, d_jobs, nj);
      P3R_HIP(hipGetLastError());
    }
    if (zk) randomise(perm_round, ZK_ROUND_PERM);
    commit(perm_round, ZK_ROUND_PERM);
    {
      // every table's global sum in one transfer
      auto all = download_ef<PP, DC>(ctx, totals.p, ni);
      for (const Mat& m : perm_round.mats) terminals[m.inst] = all[m.inst];
    }
    for (uint32_t v : perm_round.cap) ch.observe(F::raw(v));
    for (const Mat& m : perm_round.mats) ch.observe_ext(terminals[m.inst]);
  }

  // ---- 4. alpha, quotient chunks, commitment; ZK: the random round
  void quotient_commit() {
    prof_stage(ctx, "quotient_commit");
    alpha = ch.sample_ext();
    // one table of alpha powers for all AIRs: constraint k of N is weighted alpha^(N-1-k)
    auto n_constraints = [&](size_t i) {
      return air_num_base_constraints<PP>(prep->airs[i]) + (layouts[i].n_groups ? layouts[i].n_groups + 3 : 0);
    };
    int n_max = 1;
    for (size_t i = 0; i < ni; ++i) n_max = std::max(n_max, n_constraints(i));
    d_apow.alloc((size_t)n_max * DC);
    {
      std::vector<uint32_t> apow((size_t)n_max * DC);
      E p = E::one();
      for (int k = 0; k < n_max; ++k) {
        for (int c = 0; c < DC; ++c) apow[DC * k + c] = p.c[c].v;
        p *= alpha;
      }
      P3R_HIP(ctx->stage.upload(ctx->stream, d_apow.p, apow.data(), apow.size() * 4));
    }
    std::vector<QuotientArgs> quot_jobs;  // every table's quotient in one launch
    uint32_t quot_blocks = 0;
    for (size_t i = 0; i < ni; ++i) {
      const AirParams& a = prep->airs[i];
      const auto& L = layouts[i];
      // quotient domain of 2^(log_qd + is_zk) chunk cosets of the BASE trace size (batch_stark.rs:701-717)
      const int lq = L.log_chunks + zk, C = 1 << lq;
      const size_t n = mains[i]->h;
      const int n_base = air_num_base_constraints<PP>(a);
      QuotientArgs q{};
      q.n_constraints = n_constraints(i);
      q.air = a;
      q.main = main_round.mats[i].lde->d;
      q.prep = prep->ldes[i]->d;
      q.aux = L.n_groups ? perm_mat(i)->lde->d : nullptr;
      q.lde_h = main_round.mats[i].lde->h;
      q.log_n = log_n[i];
      q.log_chunks = lq;
      q.apow = d_apow.p;
      q.n_base = n_base; q.n_groups = L.n_groups; q.pair = L.pair;
      for (int k = 0; k < DC; ++k) q.terminal[k] = terminals[i].c[k].v;
      q.gen = gen.v;
      const F wq = F::two_adic_generator(log_n[i] + lq);
      q.w_q = wq.v;
      q.g_inv = F::two_adic_generator(log_n[i]).inv().v;
      const F gen_n = gen.pow(n), w_c = F::two_adic_generator(lq);
      for (int c = 0; c < C; ++c) {
        F zh = gen_n * w_c.pow(c) - F::one();
        q.zh[c] = zh.v;
        q.zh_inv[c] = zh.inv().v;
      }
      auto chunk_buf = dmat_alloc(n, (size_t)DC * C);  // [C][DC][n]
      q.out = chunk_buf->d;
      q.block0 = quot_blocks;
      quot_blocks += blocks_for(n << lq);
      quot_jobs.push_back(q);
      for (int c = 0; c < C; ++c) {   // chunk c: a view, n x DC column-major
        quot_round.keep.push_back(std::make_unique<p3r_dmat>(p3r_dmat{{}, chunk_buf->d + (size_t)c * DC * n, n, (size_t)DC}));
        quot_round.mats.push_back({(int)i, quot_round.keep.back().get(), nullptr, gen * wq.pow(c)});
      }
      quot_round.keep.push_back(std::move(chunk_buf));
    }
    {
      DevBuf d_quot((quot_jobs.size() * sizeof(QuotientArgs) + 3) / 4);
      P3R_HIP(ctx->stage.upload(ctx->stream, d_quot.p, quot_jobs.data(), quot_jobs.size() * sizeof(QuotientArgs)));
      ProfScope ps(ctx, "quotient");
      launch_quotient<PP, DC>(ctx, quot_blocks, reinterpret_cast<const QuotientArgs*>(d_quot.p), (int)quot_jobs.size(), lc);
      P3R_HIP(hipGetLastError());
    }
    if (zk) randomise_quotient();
    commit(quot_round, ZK_ROUND_QUOTIENT);
    for (uint32_t v : quot_round.cap) ch.observe(F::raw(v));
    if (zk) {
      // ZK: the random round - per instance a fully random matrix of Challenge::DIMENSION (+ R) columns over the
      // extended trace domain, opened at zeta; its commitment is observed after the quotient's (batch_stark.rs:623-625)
      std::vector<const p3r_dmat*> src(ni, nullptr);
      std::vector<size_t> hs, ws(ni, (size_t)DC);
      std::vector<uint32_t> keys;
      for (size_t i = 0; i < ni; ++i) { hs.push_back(mains[i]->h); keys.push_back(zk_stream_id(ZK_ROUND_RANDOM, i)); }
      rand_round.keep = zk_randomize<PP>(ctx, src, hs, ws, R, keys, zk_key, false);
      for (size_t i = 0; i < ni; ++i) rand_round.mats.push_back({(int)i, rand_round.keep[i].get(), nullptr, F::one()});
      commit(rand_round, ZK_ROUND_RANDOM);
      for (uint32_t v : rand_round.cap) ch.observe(F::raw(v));
    }
    zeta = ch.sample_ext();
  }

  // HidingFriPcs::commit_quotient from the acceptance side.  The verifier opens chunk c over
  // natural_domain_for_degree(2n) (batch_stark.rs:719-727) and recomposes quotient(zeta) = sum_c zp_c(zeta) q'_c(zeta),
  // zp_c(x) = prod_{j != c} Z_j(x) / Z_j(s_c), Z_j(x) = (x / s_j)^n - 1 (verifier/quotient.rs).  q'_c = q_c + Z_c t_c
  // leaves the sum unchanged iff sum_c k_c t_c = 0, k_c = prod_{j != c} 1 / Z_j(s_c): C - 1 independent random masks
  // t_c of degree < n and t_{C-1} = -(1 / k_{C-1}) sum_{c < C-1} k_c t_c.  Each mask is n random evaluations over the
  // common coset U = u <g_n>, u = s_{C-1} g_2n; the committed matrix of chunk c is q'_c over s_c <g_2n>: even rows
  // the chunk evaluations, odd rows q_c - 2 t_c on s_c g_2n <g_n> (Z_c = g_2n^n - 1 = -2 there), plus R random
  // codeword columns.  q_c and t_c reach the odd coset by a coset move (the LDE with no added bits).
  void randomise_quotient() {
    std::vector<LdeItem> q_moves, t_moves;
    size_t k0 = 0;
    for (size_t i = 0; i < ni; ++i) {
      const int lq = layouts[i].log_chunks + zk, C = 1 << lq;
      const size_t n = mains[i]->h;
      const F wq = F::two_adic_generator(log_n[i] + lq), g2 = F::two_adic_generator(log_n[i] + 1);
      std::vector<F> sh(C), kc(C);
      for (int c = 0; c < C; ++c) sh[c] = gen * wq.pow(c);
      for (int c = 0; c < C; ++c) {
        F d = F::one();
        for (int j = 0; j < C; ++j)
          if (j != c) d *= (sh[c] * sh[j].inv()).pow(n) - F::one();
        kc[c] = d.inv();
      }
      const F u = sh[C - 1] * g2, neg_inv_last = -(kc[C - 1].inv());
      ZkMaskArgs ma{};
      ma.n = n; ma.C = C; ma.DC = DC; ma.key = zk_key;
      for (int c = 0; c < C; ++c) {
        quot_round.keep.push_back(dmat_alloc(n, DC));
        ma.t[c] = quot_round.keep.back()->d;
        ma.stream[c] = zk_stream_id(ZK_ROUND_QMASK, k0 + c);
        ma.coef[c] = (kc[c] * neg_inv_last).v;
        t_moves.push_back({quot_round.keep.back().get(), (sh[c] * g2 * u.inv()).to_canonical()});
        q_moves.push_back({quot_round.mats[k0 + c].ev, g2.to_canonical()});
      }
      {
        ProfScope ps(ctx, "zk_masks");
        hipLaunchKernelGGL(k_zk_masks<PP>, dim3(blocks_for(n * DC)), dim3(kBlock), 0, ctx->stream, ma);
      }
      P3R_HIP(hipGetLastError());
      k0 += C;
    }
    auto q_odd = coset_lde_batch<PP>(ctx, q_moves, 0), t_odd = coset_lde_batch<PP>(ctx, t_moves, 0);
    std::vector<ZkChunkJob> jobs;
    uint64_t blocks = 0;
    for (size_t k = 0; k < quot_round.mats.size(); ++k) {
      const size_t n = quot_round.mats[k].ev->h;
      auto m = dmat_alloc(2 * n, (size_t)DC + R);
      ZkChunkJob j{};
      j.q = quot_round.mats[k].ev->d; j.q_odd = q_odd[k]->d; j.t_odd = t_odd[k]->d; j.dst = m->d;
      j.n = n; j.log_n = log_n[quot_round.mats[k].inst]; j.DC = DC; j.R = R;
      j.stream = zk_stream_id(ZK_ROUND_QUOTIENT, k);
      j.block0 = (uint32_t)blocks;
      blocks += (uint64_t)(DC + R) * ((2 * n + kBlock - 1) / kBlock);
      jobs.push_back(j);
      quot_round.mats[k].ev = m.get();   // the committed evaluations: 2n x (DC + R) over s_c <g_2n>
      quot_round.keep.push_back(std::move(m));
    }
    if (blocks >= (uint64_t(1) << 31)) fail(P3R_EUNSUPPORTED, "ZK chunk launch of %llu tiles", (unsigned long long)blocks);
    DevBuf d_jobs((jobs.size() * sizeof(ZkChunkJob) + 3) / 4);
    P3R_HIP(ctx->stage.upload(ctx->stream, d_jobs.p, jobs.data(), jobs.size() * sizeof(ZkChunkJob)));
    {
      ProfScope ps(ctx, "zk_chunks");
      hipLaunchKernelGGL(k_zk_chunk<PP>, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream,
                         reinterpret_cast<const ZkChunkJob*>(d_jobs.p), (int)jobs.size(), zk_key);
    }
    P3R_HIP(hipGetLastError());
    for (auto& m : q_odd) quot_round.keep.push_back(std::move(m));   // the stream still reads them
    for (auto& m : t_odd) quot_round.keep.push_back(std::move(m));
  }

  // ---- 5. openings, observed in round / matrix / point order.  Every committed matrix is opened in full; under ZK the
  // last R values of each opening are the random codewords' - HidingFriPcs splits them off into the opening proof's
  // first item and the verifier merges them back before observing (:855-864, :1116-1260).
  void openings() {
    prof_stage(ctx, "openings");
    for (Round* r : rounds())
      for (Mat& m : r->mats) {
        m.z = {zeta};
        // zeta * g of the BASE trace domain (:663-700): main (an AIR that reads the next row), preprocessed, permutation
        if (r == &prep_round || r == &perm_round || (r == &main_round && air_uses_next(prep->airs[m.inst])))
          m.z.push_back(zeta * F::two_adic_generator(log_n[m.inst]));
        m.job = op.open(m.ev->d, m.ev->h, (int)m.ev->w, m.shift, m.z);
      }
    auto all = op.finish();
    launch_inv_points();
    // the proof's own fields hold the values of the AIR's columns: the openings without their R codeword values
    for (Round* r : rounds())
      for (Mat& m : r->mats)
        for (auto& pv : all[m.job]) {
          for (auto& v : pv) ch.observe_ext(v);
          m.vals.emplace_back(pv.begin(), pv.end() - R);
          m.codewords.emplace_back(pv.end() - R, pv.end());
        }
    check_at_zeta();
  }

  static std::array<uint64_t, 6> inv_key(int lh, const E& z) {
    std::array<uint64_t, 6> key{(uint64_t)lh, 0, 0, 0, 0, 0};
    for (int k = 0; k < DC; ++k) key[1 + k] = z.c[k].v;
    return key;
  }

  // 1/(zeta - x) vectors of the reduced openings depend on the opening points only: the device
  // computes them while the host absorbs the opened values into the transcript
  void launch_inv_points() {
    std::vector<FriInvJobT<DC>> inv_jobs;
    uint32_t inv_blocks = 0;
    for (Round* r : rounds())
      for (const Mat& m : r->mats) {
        const int lh = log_e[m.inst] + log_blowup;
        for (const E& z : m.z) {
          const auto key = inv_key(lh, z);
          if (inv_cache.count(key)) continue;
          inv_keep.emplace_back((size_t)DC << lh);
          FriInvJobT<DC> j{};
          j.inv = inv_keep.back().p;
          j.h = uint64_t(1) << lh;
          j.log_h = lh;
          if (lh < 2) fail(P3R_EINVAL, "FRI: an LDE of fewer than four rows");
          j.w_h = F::two_adic_generator(lh).v;
          j.w_4 = F::two_adic_generator(2).v;
          j.z = to_e4<PP, DC>(z);
          j.block0 = inv_blocks;
          inv_blocks += blocks_for((size_t(1) << lh) / 4);
          inv_jobs.push_back(j);
          inv_cache.emplace(key, j.inv);
        }
      }
    inv_keep.emplace_back((inv_jobs.size() * sizeof(FriInvJobT<DC>) + 3) / 4);
    P3R_HIP(ctx->stage.upload(ctx->stream, inv_keep.back().p, inv_jobs.data(), inv_jobs.size() * sizeof(FriInvJobT<DC>)));
    ProfScope ps(ctx, "fri_inv_points");
    hipLaunchKernelGGL((k_fri_inv_points<PP, DC>), dim3(inv_blocks), dim3(kBlock), 0, ctx->stream,
                       reinterpret_cast<const FriInvJobT<DC>*>(inv_keep.back().p), (int)inv_jobs.size(), gen.v);
    P3R_HIP(hipGetLastError());
  }

  // Self-check before anything is serialised: the opened values must satisfy the verifier's
  // out-of-domain identity, folded constraints(zeta) / Z_H(zeta) == quotient(zeta), per instance
  // (the same routine the native verifier runs).  Traces that violate a constraint or unbalance a
  // lookup fail it with overwhelming probability: P3R_EINVAL instead of an unverifiable proof -
  // the counterpart of prove_batch's internal constraint check (include/p3r.h).  Host work of a few
  // extension-field evaluations per table, done while the device computes the 1/(z - x) vectors.
  void check_at_zeta() {
    E l_beta_pow[kMaxExtD + 1];
    for (int j = 0; j <= kMaxExtD; ++j) l_beta_pow[j] = e4_load<PP, DC>(lc.beta_pow[j]);
    const E l_prefix = e4_load<PP, DC>(lc.prefix);
    std::vector<std::vector<std::vector<E>>> inst_chunks(ni);
    for (const Mat& m : quot_round.mats) inst_chunks[m.inst].push_back(m.vals[0]);
    static const std::vector<E> empty;
    for (size_t i = 0; i < ni; ++i) {
      const auto& omain = main_round.mats[i].vals;
      const Mat* pm = perm_mat(i);
      ZetaInstance<PP, DC> zi{&omain[0], omain.size() > 1 ? &omain[1] : nullptr, &prep_round.mats[i].vals[0],
                          &prep_round.mats[i].vals[1], pm ? &pm->vals[0] : &empty, pm ? &pm->vals[1] : &empty,
                          &inst_chunks[i], pm ? &terminals[i] : nullptr};
      try {
        check_instance_at_zeta<PP, DC>(prep->airs[i], layouts[i], log_n[i], zi, alpha, zeta, l_prefix, l_beta_pow,
                                   ctx->rc_mont_host.data(), i, zk);
      } catch (const VerifyFailure& e) {
        fail(P3R_EINVAL, "the traces do not satisfy the constraints (%s)", e.what());
      }
    }
    E tsum = E::zero();
    for (const Mat& m : perm_round.mats) tsum += terminals[m.inst];
    if (!tsum.is_zero()) fail(P3R_EINVAL, "the traces do not satisfy the constraints (global lookup sum is not zero)");
  }

  // ---- 6. FRI batching challenge and per-height reduced openings
  void fri_reduce() {
    prof_stage(ctx, "fri_reduce");
    const E fri_alpha = ch.sample_ext();
    size_t max_w = 1, n_opened = 0;
    for (Round* r : rounds())
      for (const Mat& m : r->mats) { max_w = std::max(max_w, m.lde->w); ++n_opened; }
    std::vector<E> fa_pow(max_w + 1);
    fa_pow[0] = E::one();
    for (size_t c = 1; c <= max_w; ++c) fa_pow[c] = fa_pow[c - 1] * fri_alpha;
    d_fapow.alloc(max_w * DC);
    {
      std::vector<uint32_t> h(max_w * DC);
      for (size_t c = 0; c < max_w; ++c)
        for (int k = 0; k < DC; ++k) h[c * DC + k] = fa_pow[c].c[k].v;
      P3R_HIP(ctx->stage.upload(ctx->stream, d_fapow.p, h.data(), h.size() * 4));
    }
    // One pass per height over all its matrices (kernels_fri_reduce.hip.h); alpha powers restart per
    // height and run on across that height's matrices and points in round order.
    std::map<int, std::vector<FriReduceMatT<DC>>> by_height;
    std::vector<DevBuf> keep;
    std::vector<FriVsumJob> vsum_jobs;
    DevBuf vsums(2 * DC * n_opened);
    for (Round* r : rounds())
      for (const Mat& m : r->mats) {
        const int lh = log_e[m.inst] + log_blowup;
        auto f = ros.find(lh);
        if (f == ros.end()) f = ros.emplace(lh, std::make_pair(E::one(), DevBuf((size_t)DC << lh))).first;
        FriReduceMatT<DC> a{};
        a.mat = m.lde->d;
        a.w = (int)m.lde->w;
        a.n_points = (int)m.z.size();
        E ap = f->second.first;
        for (size_t p = 0; p < m.z.size(); ++p) {
          a.inv[p] = inv_cache.at(inv_key(lh, m.z[p]));
          // V = sum_c alpha^c * opened value c, formed on the device (k_fri_vsum)
          a.v[p] = vsums.p + DC * vsum_jobs.size();
          vsum_jobs.push_back({op.values_dev(m.job, (int)p), vsums.p + DC * vsum_jobs.size(), (int)m.ev->w});
          a.off[p] = to_e4<PP, DC>(ap);
          ap *= fa_pow[m.lde->w];
        }
        f->second.first = ap;
        by_height[lh].push_back(a);
      }
    std::vector<FriReduceMatT<DC>> mats;
    std::vector<FriReduceJob> jobs;
    uint32_t blocks = 0;
    for (auto& kv : by_height) {
      FriReduceJob j{};
      j.ro = ros[kv.first].second.p;
      j.h = uint64_t(1) << kv.first;
      j.mat0 = (uint32_t)mats.size();
      j.n_mats = (uint32_t)kv.second.size();
      j.block0 = blocks;
      blocks += blocks_for(size_t(1) << kv.first);
      jobs.push_back(j);
      mats.insert(mats.end(), kv.second.begin(), kv.second.end());
    }
    // the three job lists travel in one transfer
    const size_t b_mats = mats.size() * sizeof(FriReduceMatT<DC>), b_jobs = jobs.size() * sizeof(FriReduceJob),
                 b_vsum = vsum_jobs.size() * sizeof(FriVsumJob);
    const size_t o_jobs = (b_mats + 15) & ~size_t(15), o_vsum = (o_jobs + b_jobs + 15) & ~size_t(15);
    std::vector<unsigned char> blob(o_vsum + b_vsum);
    std::memcpy(blob.data(), mats.data(), b_mats);
    std::memcpy(blob.data() + o_jobs, jobs.data(), b_jobs);
    std::memcpy(blob.data() + o_vsum, vsum_jobs.data(), b_vsum);
    keep.emplace_back((blob.size() + 3) / 4);
    unsigned char* d_blob = reinterpret_cast<unsigned char*>(keep.back().p);
    P3R_HIP(ctx->stage.upload(ctx->stream, d_blob, blob.data(), blob.size()));
    const auto* d_mats = reinterpret_cast<const FriReduceMatT<DC>*>(d_blob);
    const auto* d_jobs = reinterpret_cast<const FriReduceJob*>(d_blob + o_jobs);
    const auto* d_vsum = reinterpret_cast<const FriVsumJob*>(d_blob + o_vsum);
    {
      ProfScope ps(ctx, "fri_reduce");
      hipLaunchKernelGGL((k_fri_vsum<PP, DC>), dim3((unsigned)vsum_jobs.size()), dim3(kBlock), 0, ctx->stream, d_vsum,
                         d_fapow.p);
      hipLaunchKernelGGL((k_fri_reduce_pre<PP, DC>), dim3(blocks), dim3(kBlock), 0, ctx->stream, d_jobs, (int)jobs.size(),
                         d_mats, d_fapow.p);
    }
    P3R_HIP(hipGetLastError());
  }

  // ---- 7. FRI commit phase, final polynomial, query proof of work
  void fri_commit_phase() {
    prof_stage(ctx, "fri_commit_phase");
    std::vector<int> heights;
    for (auto& kv : ros) heights.push_back(kv.first);
    std::sort(heights.rbegin(), heights.rend());
    log_max = heights[0];
    const int log_final = (int)cfg.log_final_poly_len + log_blowup;
    folded = std::move(ros[log_max].second);
    size_t next_h = 1;
    int log_cur = log_max;
    // The folding challenges stay on the device.  With a one-digest cap and no commit-phase proof of
    // work the transcript steps between the phases run there too (k_fri_transcript_step), so the whole
    // commit phase is enqueued without a host round trip; the host replays them afterwards.
    const bool device_transcript = cfg.cap_height == 0 && cfg.commit_pow_bits == 0 && ch.in_buf.empty();
    d_tstate.alloc(P2_WIDTH);
    d_phase.alloc((DC + P2_DIGEST) * kMaxPhases);  // challenges, then roots
    uint32_t* const d_betas = d_phase.p;
    uint32_t* const d_caps = d_phase.p + DC * kMaxPhases;
    if (device_transcript) {
      uint32_t st[P2_WIDTH];
      for (int k = 0; k < P2_WIDTH; ++k) st[k] = ch.state[k].v;
      P3R_HIP(ctx->stage.upload(ctx->stream, d_tstate.p, st, sizeof st));
    }
    while (log_cur > log_final) {
      int log_next = next_h < heights.size() ? heights[next_h] : -1;
      int la = fri_log_arity(ctx->fri_log_arities, phases.size(), (int)cfg.max_log_arity, log_cur, log_final, log_next);
      if (la < 0) fail(P3R_EINVAL, "fri_log_arities does not fit the proof: phase %zu at height 2^%d", phases.size(), log_cur);
      if (la > 4) fail(P3R_EUNSUPPORTED, "max_log_arity > 4 is not supported");
      const size_t arity = size_t(1) << la, rows = (size_t(1) << log_cur) >> la;
      Phase ph{la, rows};
      commit_phase_leaves(ph, log_cur);
      const size_t pi = phases.size();
      if (pi >= kMaxPhases) fail(P3R_EUNSUPPORTED, "more than %zu FRI commit phases", kMaxPhases);
      TranscriptStep step{d_tstate.p, d_betas + DC * pi, d_caps + P2_DIGEST * pi};
      step.dc = DC;
      mmcs_build_levels<PP>(ctx, ph.tree.get(), nullptr, device_transcript ? &step : nullptr);
      if (device_transcript) {
        if (!step.done)  // a tree whose root is not produced by a single-workgroup launch (one leaf)
          hipLaunchKernelGGL(k_fri_transcript_step<PP>, dim3(1), dim3(64), 0, ctx->stream, ph.tree->layers.back().p,
                             step.state, step.beta, step.cap, ctx->rc.p, ctx->p2_diag.p, DC);
      } else {
        ph.cap = mmcs_cap_mont(ctx, ph.tree.get());
        for (uint32_t v : ph.cap) ch.observe(F::raw(v));
        commit_pow_witnesses.push_back(grind_witness<PP>(ctx, ch, (int)cfg.commit_pow_bits));
        const E beta = ch.sample_ext();
        uint32_t bw[DC];
        for (int k = 0; k < DC; ++k) bw[k] = beta.c[k].v;
        P3R_HIP(ctx->stage.upload(ctx->stream, d_betas + DC * pi, bw, sizeof bw));
      }
      DevBuf out(DC * rows);
      FriFoldArgs fa{};
      fa.in = folded.p; fa.out = out.p; fa.rows = rows; fa.log_rows = log_cur - la;
      fa.beta = d_betas + DC * pi;
      const bool roll = next_h < heights.size() && heights[next_h] == log_cur - la;
      fa.roll = roll ? ros[heights[next_h]].second.p : nullptr;
      fa.w_inv = F::two_adic_generator(log_cur).inv().v;
      const F omega = F::two_adic_generator(la);
      for (int s = 0; s < la; ++s) {
        F om_s = omega.pow(uint64_t(1) << s);
        for (int j = 0; j < (int)(arity >> (s + 1)); ++j)
          fa.tw_inv[s][j] = om_s.pow(bit_reverse(2 * j, la - s)).inv().v;
      }
      fa.neg_half = (-(F::from_canonical(2).inv())).v;
      {
        ProfScope ps(ctx, "fri_fold");
        // one instance per arity (kernels_stark.hip.h)
        static constexpr void (*kFold[4])(FriFoldArgs) = {k_fri_fold<PP, DC, 1>, k_fri_fold<PP, DC, 2>, k_fri_fold<PP, DC, 3>,
                                                          k_fri_fold<PP, DC, 4>};
        hipLaunchKernelGGL(kFold[la - 1], dim3(blocks_for(rows)), dim3(kBlock), 0, ctx->stream, fa);
      }
      P3R_HIP(hipGetLastError());
      if (roll) ++next_h;
      ph.folded_in = std::move(folded);
      folded = std::move(out);
      log_cur -= la;
      phases.push_back(std::move(ph));
    }
    if (next_h != heights.size()) fail(P3R_EINVAL, "FRI: an input height was never rolled in");
    final_polynomial(log_cur, device_transcript);
    for (auto& c : final_poly) ch.observe_ext(c);
    for (auto& ph : phases) ch.observe(F::from_canonical((uint32_t)ph.la));
    // query proof of work: smallest witness (device search)
    query_pow_witness = grind_witness<PP>(ctx, ch, (int)cfg.query_pow_bits);
  }

  // The leaf digests of the commit phase that folds `folded` (2^log_cur rows) by 2^ph.la.
  void commit_phase_leaves(Phase& ph, int log_cur) {
    const size_t arity = size_t(1) << ph.la, rows = ph.rows, n_in = size_t(1) << log_cur;
    if ((int)cfg.cap_height > log_cur - ph.la)
      fail(P3R_EINVAL, "cap_height %d exceeds the height of FRI commit phase %zu (2^%d rows)", (int)cfg.cap_height,
           phases.size(), log_cur - ph.la);
    ph.tree = std::make_unique<p3r_tree>();
    mmcs_begin(ctx, ph.tree.get(), {rows});
    // leaves: row r = the 2^la sibling evaluations, EF flattened -> column (j*DC+k) = plane k, offset j, stride arity
    std::vector<const uint32_t*> cols;
    for (size_t j = 0; j < arity; ++j)
      for (int k = 0; k < DC; ++k) cols.push_back(folded.p + (size_t)k * n_in + j);
    if (cfg.mmcs_salt_elems) {
      // ExtensionMmcs over a hiding MMCS: the flattened row, then its salt (recursion/src/pcs/mmcs.rs:470-486).  The salt
      // columns take the leaf kernels' strided layout: column c of row r at [c * n_in + r * arity]
      const uint32_t S = cfg.mmcs_salt_elems;
      p3r_tree& T = *ph.tree;
      T.salt_elems = (int)S; T.phase_salt_stride = arity; T.phase_rows = rows;
      T.phase_salts.alloc((size_t)S * n_in);
      std::vector<ZkTileJob> tj(1);
      tj[0].dst = T.phase_salts.p; tj[0].rows = rows; tj[0].w2 = S; tj[0].mode = 1; tj[0].stride = (uint32_t)arity;
      tj[0].stream = zk_stream_id(kSaltRoundFri, phases.size());
      launch_zk_tiles<PP>(ctx, tj, zk_key, "mmcs_salts");
      for (uint32_t c = 0; c < S; ++c) cols.push_back(T.phase_salts.p + (size_t)c * n_in);
    }
    mmcs_hash_rows_strided<PP>(ctx, ph.tree.get(), cols, rows, arity);
  }

  // The final polynomial (host: <= 2^(log_final) extension elements); a device transcript is replayed on the host first
  void final_polynomial(int log_cur, bool device_transcript) {
    const size_t m = size_t(1) << log_cur;
    std::vector<uint32_t> raw(DC * m), phase_words(d_phase.n);
    if (device_transcript && !phases.empty()) P3R_HIP(fetch_small(ctx, d_phase.p, phase_words.size(), phase_words.data()));
    P3R_HIP(fetch_small(ctx, folded.p, raw.size(), raw.data()));
    const uint32_t* betas = phase_words.data();
    const uint32_t* caps = betas + DC * kMaxPhases;
    if (device_transcript) {
      // replay the commit phase on the host transcript; the challenges must be the device's
      for (size_t pi = 0; pi < phases.size(); ++pi) {
        phases[pi].cap.assign(caps + P2_DIGEST * pi, caps + P2_DIGEST * (pi + 1));
        for (uint32_t v : phases[pi].cap) ch.observe(F::raw(v));
        commit_pow_witnesses.push_back(grind_witness<PP>(ctx, ch, 0));
        const E beta = ch.sample_ext();
        for (int k = 0; k < DC; ++k)
          if (beta.c[k].v != betas[DC * pi + k]) fail(P3R_EHIP, "internal: device and host FRI transcripts disagree");
      }
    }
    final_poly = fri_final_poly<PP, DC>(raw.data(), log_cur, cfg.log_final_poly_len);
  }

  // ---- 8. queries: one gather launch for every opened row / sibling of every query
  void queries() {
    prof_stage(ctx, "queries");
    indices.resize(cfg.num_queries);
    for (auto& ix : indices) ix = ch.sample_bits(log_max);
    // the item list is the same for every query (kernels_stark.hip.h, k_gather); offsets are relative
    // to a query's block of `words_per_query` words in the output
    std::vector<QueryItem> q_items;
    uint32_t cursor = 0;
    auto push = [&](const uint32_t* base, uint64_t stride, uint32_t count, uint32_t shift, uint32_t flip, uint32_t mul) {
      q_items.push_back({base, stride, count, cursor, shift, flip, mul});
      const uint32_t at = cursor;
      cursor += count;
      return at;
    };
    // `base_shift`: the tree's index = query index >> base_shift
    auto push_path = [&](const p3r_tree* t, uint32_t base_shift) {
      const QPath qp{cursor, t};
      for (size_t l = 0; l < t->levels.size(); ++l)
        for (int f = 1; f < t->levels[l].step; ++f)
          push(t->layers[l].p, t->layer_n[l], P2_DIGEST, base_shift + (uint32_t)t->levels[l].bits, (uint32_t)f, 1);
      return qp;
    };
    for (Round* r : rounds()) {
      const p3r_tree* t = r->tree;
      const uint32_t tree_shift = (uint32_t)(log_max - t->log_max_h);  // tree index = query index >> tree_shift
      QRound qr;
      for (const p3r_dmat* m : t->mats) {
        const int lh = log2_exact(m->h, "height");
        qr.rows.emplace_back(push(m->d, m->h, (uint32_t)m->w, (uint32_t)(log_max - lh), 0, 1), (uint32_t)m->w);
      }
      qr.tree_shift = tree_shift;
      qr.path = push_path(t, tree_shift);
      qrounds.push_back(std::move(qr));
    }
    int shift = 0;  // the phase's index = query index >> shift
    for (auto& ph : phases) {
      const size_t arity = size_t(1) << ph.la, n_in = ph.rows << ph.la;
      QPhase qp;
      qp.shift = shift;
      // sibling j of the row: the DC planes of one extension element, at row * arity + j
      for (size_t j = 0; j < arity; ++j)
        qp.sib_at[j] = push(ph.folded_in.p + j, n_in, DC, (uint32_t)(shift + ph.la), 0, (uint32_t)arity);
      if (ph.tree->salt_elems)   // the salt of the opened row (strided layout: commit_phase_leaves)
        qp.salt_at = push(ph.tree->phase_salts.p, n_in, (uint32_t)ph.tree->salt_elems, (uint32_t)(shift + ph.la), 0, (uint32_t)arity);
      qp.path = push_path(ph.tree.get(), (uint32_t)(shift + ph.la));
      qphases.push_back(std::move(qp));
      shift += ph.la;
    }
    words_per_query = cursor;
    const auto* d_items = static_cast<const QueryItem*>(const_table(ctx, q_items.data(), q_items.size() * sizeof(QueryItem)));
    std::vector<uint32_t> idx32(indices.begin(), indices.end());
    DevBuf d_idx(idx32.size()), d_out((size_t)words_per_query * indices.size());
    hipError_t e = ctx->stage.upload(ctx->stream, d_idx.p, idx32.data(), idx32.size() * 4);
    if (e == hipSuccess) {
      ProfScope ps(ctx, "query_gather");
      hipLaunchKernelGGL(k_gather<PP>, dim3((unsigned)q_items.size(), (unsigned)indices.size()), dim3(64), 0, ctx->stream,
                         d_items, d_idx.p, words_per_query, d_out.p);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = ctx->landing.fetch(ctx->stream, d_out.p, d_out.n * 4, &gathered);
    P3R_HIP(e);
  }

  void write_path(const QPath& qp, const uint32_t* g, size_t tree_index) {
    W.varint(mmcs_proof_len(qp.t->levels));
    const uint32_t* sibs = g + qp.at;   // of this level: the gathered positions pos ^ 1 .. pos ^ (step - 1)
    const std::vector<MmcsLevel>& lv = qp.t->levels;
    for (size_t l = 0; l < lv.size();) {
      size_t run = 0;   // levels of step 2 have one sibling each, gathered in order: a run of them is written at once
      while (l + run < lv.size() && lv[l + run].step == 2) ++run;
      W.words(sibs, run * P2_DIGEST);
      sibs += run * P2_DIGEST;
      l += run;
      if (l == lv.size()) break;
      const size_t step = lv[l].step, pos = (tree_index >> lv[l].bits) & (step - 1);
      for (size_t j = 0; j < step; ++j)
        if (j != pos) W.words(sibs + ((j ^ pos) - 1) * P2_DIGEST, P2_DIGEST);
      sibs += (step - 1) * P2_DIGEST;
      ++l;
    }
  }

  void write_queries() {
    W.varint(indices.size());
    for (size_t qi = 0; qi < indices.size(); ++qi) {
      const uint32_t* g = gathered + (size_t)qi * words_per_query;  // this query's answers
      W.varint(qrounds.size());
      for (auto& qr : qrounds) {
        // a hiding MMCS's tree lists [M0, S0, M1, S1, ..]: opened values are the rows of the even entries, and the opening
        // proof is the tuple (salts = rows of the odd entries, siblings) (SaltedMmcsProof, mmcs.rs:763-768)
        const size_t step = qr.path.t->salt_elems ? 2 : 1;
        for (size_t first = 0; first < step; ++first) {
          W.varint(qr.rows.size() / step);
          for (size_t k = first; k < qr.rows.size(); k += step) {
            W.varint(qr.rows[k].second);
            W.words(g + qr.rows[k].first, qr.rows[k].second);
          }
        }
        write_path(qr.path, g, indices[qi] >> qr.tree_shift);
      }
      W.varint(qphases.size());
      for (size_t p = 0; p < phases.size(); ++p) {
        auto& qp = qphases[p];
        const size_t arity = size_t(1) << phases[p].la;
        const size_t pos = (indices[qi] >> qp.shift) & (arity - 1);  // the query's own position in the row
        W.byte((uint8_t)phases[p].la);
        W.varint(arity - 1);
        for (size_t j = 0; j < arity; ++j)
          if (j != pos) W.words(g + qp.sib_at[j], DC);
        if (qp.path.t->salt_elems) {   // (salts of the phase's one matrix, siblings)
          W.varint(1);
          W.varint((size_t)qp.path.t->salt_elems);
          W.words(g + qp.salt_at, (size_t)qp.path.t->salt_elems);
        }
        write_path(qp.path, g, indices[qi] >> (qp.shift + phases[p].la));
      }
    }
  }

  // ---- 9. serialise BatchProof; the order of the fields of each struct is ctx->proof_layout
  // (host_transcript.h::ProofLayout, identity by default)
  void serialize() {
    prof_stage(ctx, "serialize");
    const ProofLayout& PL = ctx->proof_layout;
    auto write_opened = [&] {
      W.varint(ni);
      size_t ck = 0;
      for (size_t i = 0; i < ni; ++i) {
        const auto& om = main_round.mats[i].vals;
        const Mat* pm = perm_mat(i);
        const size_t C = size_t(1) << (layouts[i].log_chunks + zk);
        for (int f = 0; f < 8; ++f) {
          switch (PL.opened[f]) {
            case 0: W.vec_ef(om[0]); break;
            case 1: if (om.size() == 2) { W.byte(1); W.vec_ef(om[1]); } else W.byte(0); break;
            case 2: W.byte(1); W.vec_ef(prep_round.mats[i].vals[0]); break;
            case 3: W.byte(1); W.vec_ef(prep_round.mats[i].vals[1]); break;
            case 4:
              W.varint(C);
              for (size_t c = 0; c < C; ++c) W.vec_ef(quot_round.mats[ck++].vals[0]);
              break;
            case 5: if (zk) { W.byte(1); W.vec_ef(rand_round.mats[i].vals[0]); } else W.byte(0); break;  // random: Option<Vec<Challenge>>
            case 6: if (pm) W.vec_ef(pm->vals[0]); else W.varint(0); break;
            default: if (pm) W.vec_ef(pm->vals[1]); else W.varint(0); break;
          }
        }
      }
    };
    auto write_fri = [&] {
      if (zk) {
        // HidingFriPcs::Proof = (OpenedValues<Challenge>, FriProof): rounds -> matrices -> points -> the R codeword values
        // (pcs/fri/targets.rs:956-1005); a tuple has no framing of its own
        W.varint(rounds().size());
        for (const Round* r : rounds()) {
          W.varint(r->mats.size());
          for (const Mat& m : r->mats) {
            W.varint(m.codewords.size());
            for (auto& pv : m.codewords) W.vec_ef(pv);
          }
        }
      }
      for (int f = 0; f < 5; ++f) {
        switch (PL.fri[f]) {
          case 0:
            W.varint(phases.size());
            for (auto& ph : phases) W.cap_mont(ph.cap);
            break;
          case 1:
            W.varint(commit_pow_witnesses.size());
            for (auto& w : commit_pow_witnesses) W.fe(w);
            break;
          case 2: write_queries(); break;
          case 3: W.vec_ef(final_poly); break;
          default: W.fe(query_pow_witness); break;
        }
      }
    };
    for (int f = 0; f < 5; ++f) {
      switch (PL.batch[f]) {
        case 0:   // optional commitments: Some iff the round is in the proof (random: iff Pcs::ZK, batch_stark.rs:424-428)
          W.cap_mont(main_round.cap);
          if (perm_round.tree) { W.byte(1); W.cap_mont(perm_round.cap); } else W.byte(0);
          W.cap_mont(quot_round.cap);
          if (rand_round.tree) { W.byte(1); W.cap_mont(rand_round.cap); } else W.byte(0);
          break;
        case 1: write_opened(); break;
        case 2: write_fri(); break;
        case 3:
          W.varint(ni);
          for (size_t i = 0; i < ni; ++i)
            if (layouts[i].n_groups) { W.byte(1); W.ef(terminals[i]); } else W.byte(0);
          break;
        default:
          W.varint(ni);
          for (size_t i = 0; i < ni; ++i) W.varint(log_e[i]);   // ZK: the extended degree bits
          break;
      }
    }
  }
};

template <class PP, int DC = 4>
std::vector<uint8_t> prove_batch(p3r_ctx* ctx, const p3r_prep* prep, const p3r_dmat* const* mains, size_t ni,
                                 bool canonical_encoding) {
  host_timeline_begin();
  {
    // the waits of this proof repeat those of the last proof of the same shape (HostPost::post)
    uint64_t shape = 0x9E3779B97F4A7C15ull ^ ni;
    for (size_t i = 0; i < ni; ++i) shape = (shape ^ (mains[i]->h * 31 + mains[i]->w)) * 0x100000001B3ull;
    // (not while profiling: the stage marks drain the stream, the results are there when they are asked for)
    if (ctx->prof_enabled) ctx->post.end_proof(); else ctx->post.begin_proof(shape);
  }
  struct EndProofWaits {
    HostPost& p;
    ~EndProofWaits() { p.end_proof(); }
  } end_proof_waits{ctx->post};
  if (ni != prep->airs.size()) fail(P3R_EINVAL, "%zu traces for %zu preprocessed instances", ni, prep->airs.size());
  if (prep->zk_codewords != zk_codewords(ctx->cfg)) fail(P3R_EINVAL, "the preprocessed data was committed under another ZK setting");
  BatchProver<PP, DC> pf(ctx, prep, mains, ni, canonical_encoding);
  pf.main_lde_commit();
  pf.transcript_head();
  pf.logup_aux_commit();
  pf.quotient_commit();
  pf.openings();
  pf.fri_reduce();
  pf.fri_commit_phase();
  pf.queries();
  pf.serialize();
  P3R_HIP(hipStreamSynchronize(ctx->stream));
  prof_stage(ctx, nullptr);
  host_timeline_dump();
  return pf.W.take();
}

// prove_batch over the context's challenge field (p3r_config.challenge_degree)
template <class PP>
std::vector<uint8_t> prove_batch_any(p3r_ctx* ctx, const p3r_prep* prep, const p3r_dmat* const* mains, size_t ni,
                                     bool canonical_encoding) {
  if (ctx->cfg.challenge_degree == 5) {
    if constexpr (kHasQuintic<PP>) return prove_batch<PP, 5>(ctx, prep, mains, ni, canonical_encoding);
    else fail(P3R_EUNSUPPORTED, "UnsupportedChallengeDegree: the quintic challenge field is KoalaBear's");
  }
  return prove_batch<PP, 4>(ctx, prep, mains, ni, canonical_encoding);
}

}  // namespace
