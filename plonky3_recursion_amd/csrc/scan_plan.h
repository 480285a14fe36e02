// The host half of the recurrence seam (p3r_affine_scan_info, p3r_affine_scan_dmat; include/p3r.h): what is decided about
// a caller's p3r_recurrence descriptors before anything touches the device, and the geometry of the three passes.  Host
// only, no HIP and no context: tu_air.hip turns a plan into three launches of k_affine_scan (kernels_scan.hip.h),
// tests/scan_plan_host_main.cpp walks it with g++ alone.
//
//   scan_plan          validation of the descriptors against the matrix widths, the form of each recurrence (sum, product,
//                      affine; base or extension), the width W of the output and the counts of p3r_scan_info
//   scan_log_height    what the seam refuses about the height of its traces
//   kAff*              the tiling: a thread of passes 0 and 2 owns kAffItems consecutive rows (one 16-byte access per
//                      column word), a workgroup a tile of kAffTile rows; pass 1 is one workgroup of kAffBlock threads per
//                      recurrence, each carrying ceil(n_tiles / kAffBlock) tiles
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "error.h"

namespace p3r {

constexpr int kAffBlock = 256;                       // threads of a workgroup, every pass
constexpr int kAffItems = 4;                         // consecutive rows per thread: one 16-byte access
constexpr int kAffTile = kAffBlock * kAffItems;      // rows per workgroup of passes 0 and 2
constexpr int kAffMaxDC = 5;                         // words of the widest challenge field
constexpr size_t kAffMaxRecs = 65535;                // the recurrence index is blockIdx.y
constexpr uint32_t kAffKnownFlags = P3R_SCAN_EXT | P3R_SCAN_INCLUSIVE;

// the compile-time form a recurrence is run in (kernels_scan.hip.h): bits of ScanPlan::form
enum : uint32_t { AFF_EXT = 1, AFF_MUL = 2, AFF_ADD = 4 };

struct ScanPlan {
  p3r_scan_info info{};
  std::vector<uint32_t> form;   // per recurrence: AFF_EXT | AFF_MUL | AFF_ADD
};

inline size_t scan_tiles(size_t h) { return (h + kAffTile - 1) / kAffTile; }
// the tiles one thread of pass 1 carries
inline size_t scan_tiles_per_thread(size_t n_tiles) { return (n_tiles + kAffBlock - 1) / kAffBlock; }

inline int scan_log_height(size_t h, int two_adicity) {
  if (h == 0 || (h & (h - 1))) fail(P3R_EINVAL, "matrix height (%zu) must be a power of two: the traces of a table live on a two-adic domain", h);
  int l = 0;
  while ((size_t(1) << l) < h) ++l;
  if (l > two_adicity) fail(P3R_EINVAL, "2^%d rows exceed the field's two-adicity (%d)", l, two_adicity);
  return l;
}

// Everything that can be refused about the descriptors on their own.  p: the field's modulus; dc: the challenge degree.
// Every output column below W has exactly one writer when this returns.
inline ScanPlan scan_plan(const p3r_recurrence* recs, size_t n_recs, const size_t* widths, size_t n_mats, int dc, uint32_t p) {
  if (n_recs == 0) fail(P3R_EINVAL, "n_recs == 0: no recurrence to scan");
  if (!recs) fail(P3R_EINVAL, "recs is NULL");
  if (n_recs > kAffMaxRecs) fail(P3R_EINVAL, "%zu recurrences in one call: at most %zu", n_recs, kAffMaxRecs);
  if (n_mats == 0) fail(P3R_EINVAL, "n_mats == 0: no trace to read the recurrences' columns from");
  if (!widths) fail(P3R_EINVAL, "widths is NULL");
  ScanPlan pl;
  pl.form.resize(n_recs);
  struct Span { uint64_t lo, hi; size_t rec; };
  std::vector<Span> spans(n_recs);
  for (size_t i = 0; i < n_recs; ++i) {
    const p3r_recurrence& r = recs[i];
    if (r.flags & ~kAffKnownFlags) fail(P3R_EINVAL, "recurrence %zu: unknown flag bits 0x%x", i, r.flags & ~kAffKnownFlags);
    const bool ext = r.flags & P3R_SCAN_EXT, mul = r.mul_mat != P3R_SCAN_NONE, add = r.add_mat != P3R_SCAN_NONE;
    const uint32_t d = ext ? (uint32_t)dc : 1u;
    if (!mul && !add)
      fail(P3R_EINVAL, "recurrence %zu has neither mul nor add: a constant column belongs in a witness program (p3r_witness_program_dmat)", i);
    const struct { const char* what; bool used; uint32_t mat, col; } ins[2] = {{"mul", mul, r.mul_mat, r.mul_col}, {"add", add, r.add_mat, r.add_col}};
    for (const auto& in : ins) {
      if (!in.used) continue;
      if (in.mat >= n_mats) fail(P3R_EINVAL, "recurrence %zu: %s reads matrix %u of %zu", i, in.what, in.mat, n_mats);
      if ((uint64_t)in.col + d <= widths[in.mat]) continue;
      if (ext) fail(P3R_EINVAL, "recurrence %zu: %s reads columns %u .. %u + DC of matrix %u, which has %zu", i, in.what, in.col, in.col, in.mat, widths[in.mat]);
      fail(P3R_EINVAL, "recurrence %zu: %s reads column %u of matrix %u, which has %zu", i, in.what, in.col, in.mat, widths[in.mat]);
    }
    for (uint32_t k = 0; k < (uint32_t)kAffMaxDC; ++k) {
      if (k < d && r.init[k] >= p) fail(P3R_EINVAL, "recurrence %zu: non-canonical word %u of init", i, k);
      if (k >= d && r.init[k] != 0) fail(P3R_EINVAL, "recurrence %zu: word %u of init is not zero (init is zero-padded after its %u word%s)", i, k, d, d == 1 ? "" : "s");
    }
    if ((uint64_t)r.out_col + d > 0x7fffffffu) fail(P3R_EINVAL, "recurrence %zu: output column %u is out of range", i, r.out_col);
    spans[i] = Span{r.out_col, (uint64_t)r.out_col + d, i};
    pl.form[i] = (ext ? AFF_EXT : 0u) | (mul ? AFF_MUL : 0u) | (add ? AFF_ADD : 0u);
    ++(mul && add ? pl.info.n_affine : mul ? pl.info.n_products : pl.info.n_sums);
  }
  std::sort(spans.begin(), spans.end(), [](const Span& a, const Span& b) { return a.lo != b.lo ? a.lo < b.lo : a.rec < b.rec; });
  uint64_t next = 0;   // one past the highest column written so far
  for (size_t k = 0; k < n_recs; ++k) {
    if (spans[k].lo < next)
      fail(P3R_EINVAL, "the output columns of recurrences %zu and %zu overlap at column %llu", std::min(spans[k - 1].rec, spans[k].rec),
           std::max(spans[k - 1].rec, spans[k].rec), (unsigned long long)spans[k].lo);
    if (spans[k].lo > next)
      fail(P3R_EINVAL, "output column %llu, below W = %llu, is written by no recurrence", (unsigned long long)next,
           (unsigned long long)spans.back().hi);
    next = spans[k].hi;
  }
  pl.info.n_out_columns = (uint32_t)next;
  return pl;
}

}  // namespace p3r
