// K6 on the host side: the device Merkle tree (MMCS) of both arities.  Included into p3r_core.hip before prove_impl.hip.h.
//
// A p3r_tree (context.h) is its level schedule (mmcs4.h) and one digest buffer per layer, whatever the arity; the arity
// only chooses the kernels: the width-16 permutation (kernels.hip.h, kernels_stark.hip.h, kernels_coop.hip.h) or the
// width-32 one (tu_mmcs4.hip).  What is here:
//   mmcs_begin               schedule + leaf layer of a tree over given heights
//   mmcs_build_levels        the layers above the leaf layer (injections, the FRI transcript step)
//   mmcs_hash_rows_strided   the leaf digests of a FRI commit phase
//   mmcs_cap_mont            the cap, downloaded
//   mmcs_commit / mmcs_open  MerkleTreeMmcs::commit / open_batch over device matrices
//   mmcs_open_batch          open_batch for many indices (and the salts of a hiding tree): one launch, one copy back
// The salts of a hiding MMCS are drawn by the callers (prove_impl.hip.h, p3r_core.hip: they need a key stream).

namespace {

// Row digests of several height classes in one launch: classes[c] = the matrices of one height
// (their rows are concatenated in the given order), digs[c] = [8][h_c].
template <class PP>
void hash_rows(p3r_ctx* ctx, const std::vector<std::vector<const p3r_dmat*>>& classes,
               const std::vector<uint32_t*>& digs) {
  std::vector<HashRowsJob> jobs;
  for (size_t c = 0; c < classes.size(); ++c) {
    std::vector<const uint32_t*> cols;
    for (const p3r_dmat* m : classes[c])
      for (size_t k = 0; k < m->w; ++k) cols.push_back(m->d + k * m->h);
    HashRowsJob j{};
    j.cols = col_table(ctx, cols);
    j.dig = digs[c];
    j.h = classes[c][0]->h;
    j.wtot = (int)cols.size();
    jobs.push_back(j);
  }
  // widest rows first: their blocks run longest
  std::stable_sort(jobs.begin(), jobs.end(),
                   [](const HashRowsJob& a, const HashRowsJob& b) { return a.wtot > b.wtot; });
  uint32_t blocks = 0;
  double perms = 0;
  for (auto& j : jobs) {
    j.block0 = blocks;
    blocks += blocks_for(j.h);
    perms += (double)j.h * ((j.wtot + P2_RATE - 1) / P2_RATE);
  }
  prof_count(ctx, "hash_rows_perms", perms);
  const auto* d_jobs =
      static_cast<const HashRowsJob*>(const_table(ctx, jobs.data(), jobs.size() * sizeof(HashRowsJob)));
  ProfScope ps(ctx, "mmcs_hash_rows");
  hipLaunchKernelGGL(k_mmcs_hash_rows<PP>, dim3(blocks), dim3(kBlock), 0, ctx->stream, d_jobs, (int)jobs.size(),
                     ctx->rcd());
  P3R_HIP(hipGetLastError());
}

// One 2-to-1 layer, one permutation per lane: for layers large enough to fill the chip.  Smaller
// ones are latency-bound and go through mmcs_subtree below (16 lanes per node, several levels per launch).
// A lane-cooperative permutation costs 16 lanes x ~1.2 k instructions against ~3.9 k FP64 operations of one
// lane: it is the faster way through a level only while the level is latency-bound, i.e. up to about
// one 16-lane row per SIMD and pass (4096 nodes a pass on 256 CUs; a pass is ~2.7 us, a launch of the
// one-permutation-per-lane kernel ~11 us whatever its size).  P3R_COOP_MAX_NODES / _LEAF_ROWS: tuning.
// (tuning knobs are rounded down to a power of two: the kernels index by shifts and halvings)
inline size_t env_pow2(const char* name, size_t dflt, size_t lo, size_t hi) {
  const char* e = tuning_knob(name);
  size_t v = e ? (size_t)atol(e) : dflt;
  v = std::min(std::max(v, lo), hi);
  while (v & (v - 1)) v &= v - 1;
  return v;
}
inline size_t coop_max_nodes() {
  static const size_t v = env_pow2("P3R_COOP_MAX_NODES", 16384, 1, size_t(1) << 30);
  return v;
}
inline size_t coop_max_leaf_rows() {
  static const size_t v = env_pow2("P3R_COOP_MAX_LEAF_ROWS", 8192, 1, size_t(1) << 30);
  return v;
}
// Digests per workgroup of a k_mmcs_subtree launch: with 32, level 0 is one pass of 16 rows - one wave
// per SIMD - and the five levels of the launch are all latency-bound; with 256 (eight levels per launch)
// levels 0 and 1 queued 8 and 4 waves per SIMD on the few CUs that had a workgroup.
inline size_t subtree_nodes() {
  static const size_t v = env_pow2("P3R_SUBTREE_NODES", 32, 2, kSubtreeNodes);
  return v;
}
template <class PP>
void launch_compress(p3r_ctx* ctx, const uint32_t* prev, const uint32_t* inj, uint32_t* out, size_t n) {
  ProfScope ps(ctx, "mmcs_compress");
  hipLaunchKernelGGL(k_mmcs_compress<PP>, dim3(blocks_for(n)), dim3(kBlock), 0, ctx->stream, prev, inj, out, n,
                     ctx->rcd());
  P3R_HIP(hipGetLastError());
}

// `inject`: height -> row digests of the matrices of that height (null: none, the FRI commit-phase trees).
using InjectMap = std::map<size_t, DevBuf>;
inline const uint32_t* injected_at(const InjectMap* inject, const MmcsLevel& lv) {
  if (!lv.inject_h) return nullptr;
  // (mmcs4_schedule injects a height at the level of its next power of two: only a power of two lands on a layer)
  if (!inject || !inject->count(lv.inject_h) || lv.inject_h != lv.logical_next)
    fail(P3R_EINVAL, "MMCS: matrix heights must be powers of two");
  return inject->at(lv.inject_h).p;
}
inline void push_layer(p3r_tree* tree, size_t n) {
  tree->layers.emplace_back(P2_DIGEST * n);
  tree->layer_n.push_back(n);
}

// FRI commit phase only: when the launch that produces the root is a single workgroup of k_mmcs_subtree (cap of one
// digest) the transcript step runs inside it and `done` is set.
struct TranscriptStep {
  uint32_t *state, *beta, *cap;
  bool done = false;
  int dc = 4;   // words of the folding challenge (the challenge degree)
};
// Up to log2(subtree_nodes()) binary levels, from tree->levels[l] on, in one launch (k_mmcs_subtree): for layers small
// enough to be latency-bound.  Returns how many levels it built; 0: the layer is too large for this path.
template <class PP>
size_t mmcs_subtree(p3r_ctx* ctx, p3r_tree* tree, size_t l, const InjectMap* inject, TranscriptStep* step) {
  const size_t n = tree->layer_n.back();
  if (n / 2 > coop_max_nodes()) return 0;
  SubtreeArgs a{};
  a.in = tree->layers.back().p;
  a.n_in = (uint32_t)n;
  const size_t local = std::min<size_t>(n, subtree_nodes());
  a.local = (uint32_t)local;
  for (size_t shrink = local; shrink > 1 && l + a.n_levels < tree->levels.size() && a.n_levels < kSubtreeLevels; shrink /= 2) {
    const MmcsLevel& lv = tree->levels[l + a.n_levels];
    push_layer(tree, lv.padded_next);
    a.out[a.n_levels] = tree->layers.back().p;
    a.inj[a.n_levels] = injected_at(inject, lv);
    ++a.n_levels;
  }
  if (step && tree->layer_n.back() == 1 && n == local) {
    a.t_state = step->state;
    a.t_beta = step->beta;
    a.t_cap = step->cap;
    a.t_dc = step->dc;
    step->done = true;
  }
  ProfScope ps(ctx, "mmcs_compress");
  const unsigned lanes = (unsigned)std::min<size_t>(std::max<size_t>(local * 8, 64), kSubtreeBlock);
  hipLaunchKernelGGL(k_mmcs_subtree<PP>, dim3((unsigned)(n / local)), dim3(lanes), 0, ctx->stream, a,
                     ctx->rc.p, ctx->p2_diag.p);
  P3R_HIP(hipGetLastError());
  return (size_t)a.n_levels;
}

// Begins a tree over matrices of the given heights under the context's MMCS: its schedule, and the leaf layer at its
// padded length (the zero digests of the padding written).  The caller fills layers[0] with the leaf digests.
inline void mmcs_begin(p3r_ctx* ctx, p3r_tree* tree, const std::vector<size_t>& heights) {
  const size_t hmax = *std::max_element(heights.begin(), heights.end());
  tree->arity = ctx->cfg.mmcs_arity == 4 ? 4 : 2;
  tree->log_max_h = log2_exact(hmax, "matrix height");
  tree->cap_height = (int)ctx->cfg.cap_height;  // 0 under the arity-4 MMCS (p3r_create)
  tree->levels = tree->arity == 4 ? mmcs4_schedule(heights) : mmcs2_schedule(heights, tree->log_max_h, tree->cap_height);
  tree->layers.clear();
  tree->layer_n.clear();
  const size_t n0 = tree->arity == 4 ? mmcs4_padded_len(hmax) : hmax;
  push_layer(tree, n0);
  if (n0 != hmax) P3R_HIP(fill_async(ctx->stream, tree->layers[0].p, 0, P2_DIGEST * n0 * 4));
}

// The layers above the leaf layer: arity 4 - one launch per level; binary - one launch per level while a level fills the
// chip, then several levels per launch (mmcs_subtree).
template <class PP>
void mmcs_build_levels(p3r_ctx* ctx, p3r_tree* tree, const InjectMap* inject, TranscriptStep* step = nullptr) {
  for (size_t l = 0; l < tree->levels.size();) {
    if (tree->arity != 4) {
      const size_t built = mmcs_subtree<PP>(ctx, tree, l, inject, step);
      if (built) {
        l += built;
        continue;
      }
    }
    const MmcsLevel& lv = tree->levels[l++];
    DevBuf next(P2_DIGEST * lv.padded_next);
    const uint32_t* inj = injected_at(inject, lv);
    if (tree->arity == 4)
      mmcs4_compress<PP>(ctx, tree->layers.back().p, tree->layer_n.back(), lv.step, inj, next.p, lv.logical_next, lv.padded_next);
    else
      launch_compress<PP>(ctx, tree->layers.back().p, inj, next.p, lv.padded_next);
    tree->layers.push_back(std::move(next));
    tree->layer_n.push_back(lv.padded_next);
  }
}

// Leaf digests of a FRI commit-phase tree (begun over {rows}): row r of its one matrix is cols[c][r * stride] over c.
template <class PP>
void mmcs_hash_rows_strided(p3r_ctx* ctx, p3r_tree* tree, const std::vector<const uint32_t*>& cols, size_t rows, size_t stride) {
  const uint32_t* const* dcols = col_table(ctx, cols);
  uint32_t* dig = tree->layers[0].p;
  if (tree->arity == 4) {
    // ExtensionMmcs over the arity-4 MMCS: the same flattened rows under the width-32 sponge
    mmcs4_hash_rows_strided<PP>(ctx, dcols, (int)cols.size(), rows, stride, dig, tree->layer_n[0]);
  } else {
    ProfScope ps(ctx, "mmcs_hash_rows_strided");
    if (rows <= coop_max_leaf_rows())  // latency-bound: sixteen lanes per row
      hipLaunchKernelGGL(k_mmcs_hash_rows_strided_coop<PP>, dim3(blocks_for(rows * 16)), dim3(kBlock), 0,
                         ctx->stream, dcols, (int)cols.size(), rows, stride, dig, ctx->rc.p, ctx->p2_diag.p);
    else
      hipLaunchKernelGGL(k_mmcs_hash_rows_strided<PP>, dim3(blocks_for(rows)), dim3(kBlock), 0, ctx->stream,
                         dcols, (int)cols.size(), rows, stride, dig, ctx->rcd());
  }
  P3R_HIP(hipGetLastError());
}

// The cap (the last layer), digest-major, in Montgomery form.
inline std::vector<uint32_t> mmcs_cap_mont(p3r_ctx* ctx, const p3r_tree* tree) {
  const size_t cap_n = tree->layer_n.back();
  std::vector<uint32_t> soa(P2_DIGEST * cap_n), cap(P2_DIGEST * cap_n);
  P3R_HIP(fetch_small(ctx, tree->layers.back().p, soa.size(), soa.data()));
  for (size_t j = 0; j < cap_n; ++j)
    for (int k = 0; k < P2_DIGEST; ++k) cap[j * P2_DIGEST + k] = soa[(size_t)k * cap_n + j];
  return cap;
}

// Commits tree->mats (commit order); returns the cap as mmcs_cap_mont gives it.  Leaf digests of every height class in
// one launch, then the levels.
template <class PP>
std::vector<uint32_t> mmcs_commit(p3r_ctx* ctx, p3r_tree* tree) {
  const auto& mats = tree->mats;
  if (mats.empty()) fail(P3R_EINVAL, "MMCS commit needs at least one matrix");
  // tallest first, stable (recursion/src/pcs/mmcs.rs:355-425)
  std::vector<size_t> order(mats.size()), heights, class_h;
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(),
                   [&](size_t a, size_t b) { return mats[a]->h > mats[b]->h; });
  const size_t hmax = mats[order[0]]->h;
  const int log_max_h = log2_exact(hmax, "matrix height");
  if ((int)ctx->cfg.cap_height > log_max_h)
    fail(P3R_EINVAL, "cap_height %d exceeds log2 of the tallest matrix (%d)", (int)ctx->cfg.cap_height, log_max_h);
  tree->total_width = 0;
  for (auto* m : mats) {
    tree->total_width += m->w;
    heights.push_back(m->h);
  }
  mmcs_begin(ctx, tree, heights);
  for (size_t i : order)
    if (class_h.empty() || class_h.back() != mats[i]->h) class_h.push_back(mats[i]->h);
  InjectMap inject;
  {
    std::vector<std::vector<const p3r_dmat*>> classes;
    std::vector<uint32_t*> digs;
    std::vector<size_t> allocs;
    for (size_t h : class_h) {
      std::vector<const p3r_dmat*> v;
      for (size_t i : order)
        if (mats[i]->h == h) v.push_back(mats[i]);
      classes.push_back(std::move(v));
      digs.push_back(h == hmax ? tree->layers[0].p : inject.emplace(h, DevBuf(P2_DIGEST * h)).first->second.p);
      allocs.push_back(h == hmax ? tree->layer_n[0] : h);
    }
    if (tree->arity == 4) mmcs4_hash_rows<PP>(ctx, classes, digs, allocs);
    else hash_rows<PP>(ctx, classes, digs);
  }
  mmcs_build_levels<PP>(ctx, tree, &inject);
  return mmcs_cap_mont(ctx, tree);
}

// Opens row `index` (of the tallest matrices; shorter ones at their own scale): the rows, then per level the step - 1
// siblings in ascending position, the node's own left out (recursion/src/pcs/mmcs.rs:1413-1461).  Canonical.
template <class PP>
void mmcs_open(p3r_ctx* ctx, const p3r_tree* tree, size_t index, uint32_t* opened, uint32_t* proof) {
  using F = Fp<PP>;
  if (index >> tree->log_max_h) fail(P3R_EINVAL, "open index %zu out of range", index);
  size_t off = 0;
  for (const p3r_dmat* m : tree->mats) {
    int lh = log2_exact(m->h, "matrix height");
    size_t row = index >> (tree->log_max_h - lh);
    // strided gather of one row: w scattered 4-byte cells
    P3R_HIP(hipMemcpy2DAsync(opened + off, 4, m->d + row, m->h * 4, 4, m->w, hipMemcpyDeviceToHost,
                             ctx->stream));
    off += m->w;
  }
  size_t depth = 0;
  for (size_t l = 0; l < tree->levels.size(); ++l) {
    const size_t step = tree->levels[l].step, idx = index >> tree->levels[l].bits, pos = idx & (step - 1);
    for (size_t j = 0; j < step; ++j) {
      if (j == pos) continue;
      P3R_HIP(hipMemcpy2DAsync(proof + depth * P2_DIGEST, 4, tree->layers[l].p + (idx - pos + j), tree->layer_n[l] * 4, 4,
                               P2_DIGEST, hipMemcpyDeviceToHost, ctx->stream));
      ++depth;
    }
  }
  P3R_HIP(hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < off; ++i) opened[i] = F::raw(opened[i]).to_canonical();
  for (size_t i = 0; i < depth * P2_DIGEST; ++i) proof[i] = F::raw(proof[i]).to_canonical();
}

// Where the words of one opening come from: the same for every index of a call, only the position depends on the index.
// One item per committed matrix, per salt matrix and per sibling slot; an index's block of the output is
// [rows, total_width | salts, num_matrices x salt_elems | siblings, proof_len x 8] and the items are sorted by `dst`.
struct OpenItem {
  const uint32_t* base;  // a matrix (column-major) or a layer's digests ([8][layer_n])
  uint64_t n;            // its height / layer_n: the words between consecutive elements of the item
  uint32_t dst;          // first output word of the item inside an index's block
  uint32_t shift;        // position = index >> shift (log_max_h - log_h of a matrix, the level's `bits` of a sibling)
  uint32_t step, slot;   // siblings: children per node and which of its step - 1 siblings in ascending position, the
                         // node's own left out; rows: step = 0
};
// One workgroup per index, its lanes over the words of that index's block.  Canonical output.
template <class PP>
__global__ void __launch_bounds__(256)
k_mmcs_open_batch(const OpenItem* __restrict__ items, uint32_t n_items, const uint32_t* __restrict__ indices, uint32_t words,
                  uint32_t* __restrict__ out) {
  const uint32_t index = indices[blockIdx.x];
  uint32_t* dst = out + (size_t)blockIdx.x * words;
  for (uint32_t w = threadIdx.x; w < words; w += 256) {
    uint32_t lo = 0, hi = n_items;  // the item of word w: the last one that begins at or before it
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) / 2;
      if (items[mid].dst <= w) lo = mid; else hi = mid;
    }
    const OpenItem it = items[lo];
    size_t pos = index >> it.shift;
    if (it.step) {
      const size_t own = pos & (it.step - 1);
      pos = pos - own + it.slot + (it.slot >= own ? 1 : 0);
    }
    dst[w] = Fp<PP>::raw(as_global(it.base)[(size_t)(w - it.dst) * it.n + pos]).to_canonical();
  }
}

// Mmcs::open_batch for every index of `indices`: rows in commit order at each matrix's own scale, under a hiding tree the
// per-matrix salts in commit order, the siblings bottom-up as mmcs_open gives them.  One gather launch into one device
// buffer, one copy back, one wait.  opened: n x total_width, salts: n x num_matrices x salt_elems, proofs: n x proof_len x 8.
template <class PP>
void mmcs_open_batch(p3r_ctx* ctx, const p3r_tree* tree, const size_t* indices, size_t n, uint32_t* opened, uint32_t* salts,
                     uint32_t* proofs) {
  if (tree->log_max_h > 31) fail(P3R_EUNSUPPORTED, "open_batch of a tree of 2^%d rows", tree->log_max_h);
  std::vector<uint32_t> idx32(n);
  for (size_t i = 0; i < n; ++i) {
    if (indices[i] >> tree->log_max_h) fail(P3R_EINVAL, "open index %zu (entry %zu) out of range", indices[i], i);
    idx32[i] = (uint32_t)indices[i];
  }
  const size_t S = (size_t)tree->salt_elems, per = S ? 2 : 1, n_mats = tree->mats.size() / per;
  const size_t w_rows = tree->total_width, w_salts = n_mats * S, w_proof = mmcs_proof_len(tree->levels) * P2_DIGEST;
  const size_t words = w_rows + w_salts + w_proof;
  if (words >> 31 || n >> 31) fail(P3R_EUNSUPPORTED, "open_batch of %zu indices of %zu words each", n, words);
  std::vector<OpenItem> items;
  size_t off = 0;
  for (size_t i = 0; i < n_mats; ++i) {
    const p3r_dmat* m = tree->mats[i * per];
    const uint32_t shift = (uint32_t)(tree->log_max_h - log2_exact(m->h, "matrix height"));
    if (m->w) items.push_back(OpenItem{m->d, m->h, (uint32_t)off, shift, 0, 0});
    off += m->w;
    if (S) items.push_back(OpenItem{tree->mats[i * per + 1]->d, m->h, (uint32_t)(w_rows + i * S), shift, 0, 0});
  }
  off = w_rows + w_salts;
  const size_t last = (size_t(1) << tree->log_max_h) - 1;
  for (size_t l = 0; l < tree->levels.size(); ++l) {
    const MmcsLevel& lv = tree->levels[l];
    if (((last >> lv.bits) | (size_t)(lv.step - 1)) >= tree->layer_n[l]) fail(P3R_EHIP, "internal: Merkle layer %zu shorter than its level", l);
    for (int j = 0; j + 1 < lv.step; ++j, off += P2_DIGEST)
      items.push_back(OpenItem{tree->layers[l].p, tree->layer_n[l], (uint32_t)off, (uint32_t)lv.bits, (uint32_t)lv.step, (uint32_t)j});
  }
  if (!words) return;
  std::stable_sort(items.begin(), items.end(), [](const OpenItem& a, const OpenItem& b) { return a.dst < b.dst; });
  DevBuf d_items((items.size() * sizeof(OpenItem) + 3) / 4), d_idx(n), d_out(n * words);
  P3R_HIP(ctx->stage.upload(ctx->stream, d_items.p, items.data(), items.size() * sizeof(OpenItem)));
  P3R_HIP(ctx->stage.upload(ctx->stream, d_idx.p, idx32.data(), n * 4));
  {
    ProfScope ps(ctx, "mmcs_open_batch");
    hipLaunchKernelGGL(k_mmcs_open_batch<PP>, dim3((unsigned)n), dim3(256), 0, ctx->stream,
                       reinterpret_cast<const OpenItem*>(d_items.p), (uint32_t)items.size(), d_idx.p, (uint32_t)words, d_out.p);
    P3R_HIP(hipGetLastError());
  }
  const uint32_t* got = nullptr;
  P3R_HIP(ctx->landing.fetch(ctx->stream, d_out.p, n * words * 4, &got));
  for (size_t i = 0; i < n; ++i) {
    const uint32_t* g = got + i * words;
    std::memcpy(opened + i * w_rows, g, w_rows * 4);
    if (w_salts) std::memcpy(salts + i * w_salts, g + w_rows, w_salts * 4);
    std::memcpy(proofs + i * w_proof, g + w_rows + w_salts, w_proof * 4);
  }
}

}  // namespace
