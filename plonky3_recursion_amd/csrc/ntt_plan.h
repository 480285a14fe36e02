// K5: the geometry of the NTT passes as pure integer functions - how a transform of 2^log_n rows splits into two
// passes, which kernel family takes them, the tile of a workgroup and the workgroups of a pass.  Host only, no device
// type and no context: tu_lde.hip turns these decisions into job lists and launches, tests/ntt_plan_host_main.cpp walks
// them for every height the fields admit.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "error.h"

namespace p3r {

constexpr int kNtt2LogTile = 13;  // the lean kernels' tile (kernels_ntt2.hip.h): 2^13 cells = 512 lanes x 16 cells
// The sub-transform sizes the lean kernels are instantiated for: the `switch` ranges of tu_lde.hip::launch_col /
// launch_fwd_line and of k_ntt_col_mixed / k_ntt_fwd_line_mixed.  A line of 2^13 cells is one 2^13-cell tile.
constexpr int kNtt2MinLogR = 5, kNtt2MaxLogR = 12, kNtt2MaxLineLogR = 13;
constexpr int kNttSingleMaxLogN = 11;         // up to here a whole polynomial is one LDS tile of k_ntt_tile: one pass
constexpr size_t kNttMaxLdsBytes = 160 * 1024;  // the LDS of a workgroup
constexpr int kBitrevMinTiled = 10;           // log_n from which k_bitrev_rows takes its tiled form

// Workgroups of a pass over `w` columns of 2^log_cells cells each, a workgroup per 2^log_tile-cell tile.
inline uint64_t ntt_pass_blocks(uint64_t w, int log_cells, int log_tile) {
  if (log_tile < 0 || log_tile > log_cells)
    fail(P3R_EUNSUPPORTED, "NTT pass: a 2^%d-cell tile does not divide a column of 2^%d cells", log_tile, log_cells);
  return w << (log_cells - log_tile);
}

// N = 2^log_n = N1 x N2 with N1 = 2^la the strided dimension (index n1 * N2 + n2), N2 = 2^lb.
struct NttSplit {
  bool single;   // one pass over whole columns, each one LDS tile of k_ntt_tile (la = 0, lb = log_n)
  bool lean;     // the kernels of kernels_ntt2.hip.h take both passes, on the tiles below; else k_ntt_tile
  int la, lb;
  int log_tile1, log_tile2;  // lean: cells of the tile of pass 1 (a column pass) and of pass 2 (inverse: column, forward: line)
};
inline NttSplit ntt_split(int log_n, int la) {
  NttSplit s{};
  s.single = log_n <= kNttSingleMaxLogN;
  s.la = s.single ? 0 : la;
  s.lb = log_n - s.la;
  return s;
}

// Column tile of a lean pass of 2^log_r-row sub-transforms: 2^14 cells (two items per lane) where the 2^13-cell tile
// would be narrower than 2^min_log_cols columns, i.e. its rows too short a run of contiguous bytes - if a column holds one.
inline int ntt_col_log_tile(int log_r, int log_n, int min_log_cols) {
  return (kNtt2LogTile - log_r < min_log_cols && log_n >= kNtt2LogTile + 1) ? kNtt2LogTile + 1 : kNtt2LogTile;
}

// Inverse transform: the balanced split.  Lean from one tile per column (2^13 rows) up to 2^12 x 2^12 (lb >= la, so
// la <= kNtt2MaxLogR and lb >= kNtt2MinLogR follow from the two bounds tested).
// 2^14-cell tiles when the 2^13 tile would be narrower than 16 columns (from 2^10-row sub-transforms on).
inline NttSplit ntt_inverse_split(int log_n) {
  NttSplit s = ntt_split(log_n, log_n / 2);
  s.lean = s.la >= kNtt2MinLogR && s.lb <= kNtt2MaxLogR && log_n >= kNtt2LogTile;
  s.log_tile1 = ntt_col_log_tile(s.la, log_n, 4);
  s.log_tile2 = ntt_col_log_tile(s.lb, log_n, 4);
  return s;
}
// The two-level split of the coefficient index of a coset inverse transform (tu_lde.hip::get_inv_pow): its low part
// is the contiguous dimension of the last inverse pass.
inline int ntt_inv_pow_log_lo(int log_n) { return ntt_inverse_split(log_n).single ? log_n : log_n / 2; }

// Forward transform (all cosets of an LDE).  It has its own split: its strided pass wants few rows per tile (long
// contiguous segments per row), its second pass is contiguous whatever N2 is.
// (measured: 2^8 x 2^12 beats 2^10 x 2^10 at n = 2^20)
// The lean kernels' contiguous pass takes lines of up to 2^13 cells (one tile), so the strided pass keeps
// 2^la_cap = 2^8 rows (128-byte segments) up to 2^21 rows and grows only beyond that (2^22: 2^9 rows, 64-byte
// segments; the balanced 2^11 x 2^11 split moved 16-byte segments).
// Column tile: 2^14 cells when the 2^13 tile would be narrower than 32 columns (measured: slower at 2^8 rows x 32
// columns, faster from 2^9 rows on).
// Line tile: lines of up to 2^12 cells on 2^12-cell tiles (256 lanes, six workgroups per CU): measured 10 % faster
// than 2^13-cell tiles at the same waves per CU - the pass is VALU-bound (it does not slow down with a third fewer
// waves) and smaller workgroups wait less at their barriers.  line_log_tile = 13 (P3R_NTT_LINE_LOG_TILE): tuning.
// la_cap: P3R_NTT_FWD_LOG_N1, default 8.
inline NttSplit ntt_forward_split(int log_n, int la_cap, int line_log_tile) {
  NttSplit s = ntt_split(log_n, std::max(std::min(log_n / 2, la_cap), log_n - kNtt2MaxLineLogR));
  s.lean = s.la >= kNtt2MinLogR && s.la <= kNtt2MaxLogR && s.lb >= kNtt2MinLogR && s.lb <= kNtt2MaxLineLogR &&
           log_n >= kNtt2LogTile;
  s.log_tile1 = ntt_col_log_tile(s.la, log_n, 5);
  s.log_tile2 = (line_log_tile == 12 && s.lb <= 12) ? 12 : kNtt2LogTile;
  return s;
}

// k_ntt_tile (the generic kernel): log2 of the lines per tile of a pass of 2^log_r-cell sub-transforms over 2^log_lines
// lines.  log_tile: P3R_NTT_LOG_TILE, default 13 (2^13 cells, 512 lanes: 4 tiles per CU overlap their phases).
inline int ntt_generic_log_t(int log_r, int log_lines, bool strided, int log_tile) {
  int log_t = std::max(0, std::min(log_tile, 13) - log_r);
  if (strided && log_t > 5) log_t = 5;  // 128-byte segments are enough when strided
  return std::min(log_t, log_lines);
}
// ... and the LDS of its workgroup: the padded tile and the twiddle table (kernels_ntt.hip.h::lds_addr).
inline size_t ntt_generic_lds_bytes(int log_r, int log_t) {
  const size_t R = size_t(1) << log_r, T = size_t(1) << log_t;
  const size_t lds = (R * (T + 1) + (R >> 5) + 2 + R + 2) * sizeof(uint32_t);
  if (lds > kNttMaxLdsBytes) fail(P3R_EUNSUPPORTED, "NTT tile of 2^%d rows does not fit LDS", log_r);
  return lds;
}

// k_bitrev_rows: a workgroup takes 2^log_t x 2^log_t cells (log_t = 6, or 5 for 2^10 and 2^11 rows); log_t = 0: a
// whole column, cell by cell.
inline int ntt_bitrev_log_t(int log_n) { return log_n >= 12 ? 6 : log_n >= kBitrevMinTiled ? 5 : 0; }
inline int ntt_bitrev_log_tile(int log_n) { return ntt_bitrev_log_t(log_n) ? 2 * ntt_bitrev_log_t(log_n) : log_n; }

}  // namespace p3r
