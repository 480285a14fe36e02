// The level schedule of an MMCS tree, host only: how a p3r_tree (context.h) of either arity is described.  Shared by the
// prover's tree module (mmcs_impl.hip.h), its query phase (prove_impl.hip.h) and the native verifier (verify_impl.h).
//
// Binary MMCS (MerkleTreeMmcs<.., 2, 8> over the width-16 permutation): mmcs2_schedule - every level compresses 2.
//
// Arity-4 MMCS (MerkleTreeMmcs<.., 4, 8> over the width-32 permutation: `MyMmcsArity4`,
// recursion/examples/recursive_aggregation.rs:1024-1046): mmcs4_schedule.
// What such a tree is, as far as the reference states it, is its in-circuit verifier (recursion/src/pcs/mmcs.rs:
// 866-960 `padded_len`, `arity4_path_schedule` - "matching native arity_schedule"): a level compresses `step`
// children, 4, or 2 (a bridge, zero-padded to four chunks) when a matrix that is still to be injected is taller
// than the next quaternary layer; a logical layer of 2 or 3 nodes is padded to 4 with zero digests; the matrices
// whose height equals the new layer's are injected after the level as one more compression
// (node, their row digest, 0, 0).  The native tree builder (p3-merkle-tree) is not in the tree.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

namespace p3r {

struct MmcsLevel {
  int step;             // children per node: 2 or 4; an opening carries the step - 1 siblings
  size_t logical_next;  // nodes of the layer this level produces
  size_t padded_next;   // its allocated width (zero digests above logical_next)
  size_t inject_h;      // height of the matrices injected after the level, 0: none
  int bits;             // index bits consumed before this level
};

inline size_t mmcs4_npt(size_t n) { size_t p = 1; while (p < n) p <<= 1; return p; }
inline size_t mmcs4_padded_len(size_t raw, size_t n = 4) { return raw <= 1 ? raw : (raw >= n ? (raw + n - 1) / n * n : n); }

// `heights`: the heights of the committed matrices, any order.  One root (cap_height 0).
inline std::vector<MmcsLevel> mmcs4_schedule(std::vector<size_t> heights) {
  std::stable_sort(heights.begin(), heights.end(), [](size_t a, size_t b) { return a > b; });
  const size_t max_height = heights.at(0), leaf_npt = mmcs4_npt(max_height);
  size_t at = 0;
  while (at < heights.size() && mmcs4_npt(heights[at]) == leaf_npt) ++at;
  std::vector<MmcsLevel> levels;
  size_t curr = mmcs4_padded_len(max_height);
  int bits = 0;
  while (curr > 1) {
    int step = 2;
    if (curr >= 4) {
      const size_t target = mmcs4_npt(curr / 4);
      bool intermediate = false;
      for (size_t k = at; k < heights.size(); ++k) intermediate |= mmcs4_npt(heights[k]) > target;
      step = intermediate ? 2 : 4;
    }
    const size_t logical_next = curr / step;
    curr = mmcs4_padded_len(logical_next);
    size_t inject = 0;
    if (at < heights.size() && mmcs4_npt(heights[at]) == mmcs4_npt(logical_next)) {
      inject = heights[at];
      while (at < heights.size() && heights[at] == inject) ++at;
    }
    levels.push_back({step, logical_next, curr, inject, bits});
    bits += step == 4 ? 2 : 1;
  }
  return levels;
}
// The binary tree over the same heights, cut at a cap of 2^cap_height digests: level l halves a layer of
// 2^(H - l) nodes (2^H = the tallest height, H = log_max_h) and injects the matrices whose height is the new layer's.
// (Matrices shorter than the cap are hashed by the commit but belong to no level: the loop ends at the cap.)
inline std::vector<MmcsLevel> mmcs2_schedule(const std::vector<size_t>& heights, int log_max_h, int cap_height) {
  std::vector<MmcsLevel> levels;
  for (int l = 0; l < log_max_h - cap_height; ++l) {
    const size_t next = size_t(1) << (log_max_h - l - 1);
    const bool inject = std::find(heights.begin(), heights.end(), next) != heights.end();
    levels.push_back({2, next, next, inject ? next : 0, l});
  }
  return levels;
}
// siblings of an opening proof
inline size_t mmcs_proof_len(const std::vector<MmcsLevel>& levels) {
  size_t n = 0;
  for (auto& l : levels) n += l.step - 1;
  return n;
}

}  // namespace p3r
