// Mmcs::verify_batch as a verifier runs it, for both MMCS arities and the hiding MMCS: host code free of HIP, shared by
// the native batch verifier (verify_impl.h), p3r_mmcs_verify (host_abi.h) and the FRI verifier (fri_verify.h).
//   MMCS openings (mixed heights, injection, cap)   recursion/src/pcs/mmcs.rs:319-426, circuit/src/ops/mmcs.rs:81-209
#pragma once
#include <array>
#include <vector>

#include "host_challenger.h"
#include "mmcs4.h"

namespace p3r {

// ---- MMCS
// a digest is the first P2_DIGEST words of the permutation state, at either width
template <class F>
std::array<F, P2_DIGEST> state_digest(const F* s) {
  std::array<F, P2_DIGEST> d;
  std::copy(s, s + P2_DIGEST, d.begin());
  return d;
}
template <class PP>
std::array<Fp<PP>, P2_DIGEST> sponge_hash(const std::vector<Fp<PP>>& row, const uint32_t* rc) {
  using F = Fp<PP>;
  F s[P2_WIDTH];
  for (auto& x : s) x = F::zero();
  size_t g = 0;
  // overwrite-mode PaddingFreeSponge, rate 8 (recursion/src/pcs/mmcs.rs:38-179)
  for (; g < row.size(); g += P2_RATE) {
    for (size_t j = 0; j < (size_t)P2_RATE && g + j < row.size(); ++j) s[j] = row[g + j];
    host_permute<PP>(s, rc);
  }
  return state_digest(s);
}
template <class PP>
std::array<Fp<PP>, P2_DIGEST> compress2(const std::array<Fp<PP>, P2_DIGEST>& l, const std::array<Fp<PP>, P2_DIGEST>& r,
                                        const uint32_t* rc) {
  Fp<PP> s[P2_WIDTH];
  for (int k = 0; k < P2_DIGEST; ++k) { s[k] = l[k]; s[P2_DIGEST + k] = r[k]; }
  host_permute<PP>(s, rc);
  return state_digest(s);
}

// verify_batch of one commitment: `log_heights[m]` / rows[m] in COMMIT order; index addresses the
// tallest matrix.  (recursion/src/pcs/mmcs.rs:319-426)
template <class PP>
void mmcs_verify(const std::vector<std::array<Fp<PP>, P2_DIGEST>>& cap, int cap_height, const std::vector<int>& log_heights,
                 const std::vector<std::vector<Fp<PP>>>& rows, size_t index,
                 const std::vector<std::array<Fp<PP>, P2_DIGEST>>& path, const uint32_t* rc, const char* what) {
  using F = Fp<PP>;
  if (rows.size() != log_heights.size()) vfail("%s: %zu opened rows for %zu matrices", what, rows.size(), log_heights.size());
  int log_max = 0;
  for (int lh : log_heights) log_max = std::max(log_max, lh);
  if (cap_height > log_max || cap.size() != (size_t(1) << cap_height)) vfail("%s: bad cap", what);
  if ((int)path.size() != log_max - cap_height) vfail("%s: opening proof has %zu siblings, expected %d", what, path.size(), log_max - cap_height);
  if (index >> log_max) vfail("%s: index out of range", what);
  auto concat = [&](int lh) {
    std::vector<F> r;
    for (size_t m = 0; m < rows.size(); ++m)
      if (log_heights[m] == lh) r.insert(r.end(), rows[m].begin(), rows[m].end());
    return r;
  };
  auto any_at = [&](int lh) {
    for (int x : log_heights) if (x == lh) return true;
    return false;
  };
  auto node = sponge_hash<PP>(concat(log_max), rc);
  size_t idx = index;
  for (int lvl = 0; lvl < log_max - cap_height; ++lvl) {
    node = (idx & 1) ? compress2<PP>(path[lvl], node, rc) : compress2<PP>(node, path[lvl], rc);
    idx >>= 1;
    const int lh = log_max - lvl - 1;
    if (any_at(lh)) node = compress2<PP>(node, sponge_hash<PP>(concat(lh), rc), rc);  // injection
  }
  if (node != cap.at(idx)) vfail("%s: Merkle root mismatch", what);
}

// Arity-4 MMCS (mmcs4.h): leaf = width-32 sponge of rate 24 over the rows of the tallest matrices; per level step - 1
// siblings in ascending position around the running digest at `pos = index mod step`, chunks above `step` zero; an
// injected class as one more compression (node, digest of its rows, 0, 0).  recursion/src/pcs/mmcs.rs:1165-1316 is
// the same walk in circuit form.  `rcw`: the width-32 constant table (Montgomery), rc + p2_num_constants.
template <class PP>
std::array<Fp<PP>, P2_DIGEST> sponge_hash_w32(const std::vector<Fp<PP>>& row, const uint32_t* rcw) {
  using F = Fp<PP>;
  F s[P2W_WIDTH];
  for (auto& x : s) x = F::zero();
  struct { void put(F) {} } sink;
  for (size_t g = 0; g < row.size(); g += 24) {
    for (size_t j = 0; j < 24 && g + j < row.size(); ++j) s[j] = row[g + j];
    p2w_permute_traced<PP>(s, rcw, sink);
  }
  return state_digest(s);
}
template <class PP>
std::array<Fp<PP>, P2_DIGEST> compress4(const std::array<Fp<PP>, P2_DIGEST>* c, const uint32_t* rcw) {
  using F = Fp<PP>;
  F s[P2W_WIDTH];
  for (int j = 0; j < 4; ++j)
    for (int k = 0; k < P2_DIGEST; ++k) s[j * P2_DIGEST + k] = c[j][k];
  struct { void put(F) {} } sink;
  p2w_permute_traced<PP>(s, rcw, sink);
  return state_digest(s);
}
template <class PP>
void mmcs_verify4(const std::vector<std::array<Fp<PP>, P2_DIGEST>>& cap, int cap_height, const std::vector<int>& log_heights,
                  const std::vector<std::vector<Fp<PP>>>& rows, size_t index,
                  const std::vector<std::array<Fp<PP>, P2_DIGEST>>& path, const uint32_t* rcw, const char* what) {
  using F = Fp<PP>;
  using Digest = std::array<F, P2_DIGEST>;
  if (rows.size() != log_heights.size() || rows.empty()) vfail("%s: %zu opened rows for %zu matrices", what, rows.size(), log_heights.size());
  if (cap_height != 0 || cap.size() != 1) vfail("%s: bad cap (the arity-4 MMCS has a one-digest cap)", what);
  int log_max = 0;
  std::vector<size_t> heights;
  for (int lh : log_heights) {
    log_max = std::max(log_max, lh);
    heights.push_back(size_t(1) << lh);
  }
  if (index >> log_max) vfail("%s: index out of range", what);
  const std::vector<MmcsLevel> levels = mmcs4_schedule(heights);
  if (path.size() != mmcs_proof_len(levels))
    vfail("%s: opening proof has %zu siblings, expected %zu", what, path.size(), mmcs_proof_len(levels));
  auto concat = [&](size_t h) {
    std::vector<F> r;
    for (size_t m = 0; m < rows.size(); ++m)
      if (heights[m] == h) r.insert(r.end(), rows[m].begin(), rows[m].end());
    return r;
  };
  Digest zero;
  zero.fill(F::zero());
  Digest node = sponge_hash_w32<PP>(concat(size_t(1) << log_max), rcw);
  size_t at = 0;
  for (const MmcsLevel& lv : levels) {
    const size_t pos = (index >> lv.bits) & (size_t)(lv.step - 1);
    Digest c[4] = {zero, zero, zero, zero};
    for (size_t j = 0; j < (size_t)lv.step; ++j) c[j] = j == pos ? node : path[at++];
    node = compress4<PP>(c, rcw);
    if (lv.inject_h) {
      Digest in[4] = {node, sponge_hash_w32<PP>(concat(lv.inject_h), rcw), zero, zero};
      node = compress4<PP>(in, rcw);
    }
  }
  if (node != cap[0]) vfail("%s: Merkle root mismatch", what);
}

// MerkleTreeHidingMmcs::verify_batch through the plain walk: the leaf preimage of a height class is the concatenation of
// [row | salt] per matrix (recursion/src/pcs/mmcs.rs:375-389 for base rows, :470-486 for flattened extension rows), i.e.
// the plain preimage of the matrices widened by their salts.
template <class F>
std::vector<std::vector<F>> salted_rows(const std::vector<std::vector<F>>& rows, const std::vector<std::vector<F>>& salts, int salt_elems,
                                        const char* what) {
  if (!salt_elems) {
    if (!salts.empty()) vfail("%s: salts under a non-hiding MMCS", what);
    return rows;
  }
  if (salts.size() != rows.size()) vfail("%s: %zu salts for %zu matrices", what, salts.size(), rows.size());
  std::vector<std::vector<F>> out(rows);
  for (size_t m = 0; m < rows.size(); ++m) {
    if ((int)salts[m].size() != salt_elems) vfail("%s: a salt of %zu elements, expected %d", what, salts[m].size(), salt_elems);
    out[m].insert(out[m].end(), salts[m].begin(), salts[m].end());
  }
  return out;
}

// One MMCS as a verifier sees it.  `rc`: the permutation constants in Montgomery form, the width-16 round constants
// followed by the width-32 table (poseidon2.h; csrc/p3r_core.hip::constants_table).
template <class PP>
struct MmcsChecker {
  using F = Fp<PP>;
  using Digest = std::array<F, P2_DIGEST>;
  int arity, salt_elems;
  const uint32_t* rc;
  // Mmcs::verify_batch of one opening: salt the rows, then the walk of the configured arity over its own constants
  void check_opening(const std::vector<Digest>& cap, int cap_height, const std::vector<int>& log_heights,
                     const std::vector<std::vector<F>>& rows, const std::vector<std::vector<F>>& salts, size_t index,
                     const std::vector<Digest>& path, const char* what) const {
    const auto leaf_rows = salted_rows<F>(rows, salts, salt_elems, what);
    if (arity == 4) mmcs_verify4<PP>(cap, cap_height, log_heights, leaf_rows, index, path, rc + p2_num_constants<PP>(), what);
    else mmcs_verify<PP>(cap, cap_height, log_heights, leaf_rows, index, path, rc, what);
  }
};

template <class PP>
std::vector<uint32_t> montgomery_constants(const std::vector<uint32_t>& rc_canonical) {
  if (rc_canonical.size() != (size_t)p2_num_constants<PP>() + (size_t)p2w_num_constants<PP>()) vfail("wrong number of permutation constants");
  std::vector<uint32_t> rc(rc_canonical.size());
  for (size_t i = 0; i < rc.size(); ++i) rc[i] = Fp<PP>::from_canonical(rc_canonical[i]).v;
  return rc;
}

}  // namespace p3r
