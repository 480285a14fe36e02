// The geometry of the NTT passes (csrc/ntt_plan.h) compiled by g++ alone and walked for both fields: every log_n up to the
// field's two-adicity, every added_bits in 0..3 that stays inside it, widths 1 and 33, the default tuning values and
// P3R_NTT_LINE_LOG_TILE = 13.  Every case is checked for the properties the launches rely on (CHECK below); a violated one
// is exit status 1 with a line on stderr.  stdout: one line per field, direction, line-tile value and log_n -
//   <field> inv|fwd <line_log_tile> <log_n> single|generic|lean|refused <la> <lb> <log_tile1> <log_tile2>
// (tiles 0 unless lean; `refused`: the generic kernel's LDS rule refuses the height) - which tests/test_ntt_plan_host.py
// pins at the points read off the rules.
#include <cstdio>
#include <cstdlib>

#include "field.h"
#include "ntt_plan.h"

using namespace p3r;

#define CHECK(cond, ...)                                             \
  do {                                                               \
    if (!(cond)) {                                                   \
      fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond);     \
      fprintf(stderr, __VA_ARGS__);                                  \
      fprintf(stderr, "\n");                                         \
      exit(1);                                                       \
    }                                                                \
  } while (0)

static const uint64_t kWidths[2] = {1, 33};
static const int kFwdLaCap = 8, kGenericLogTile = 13;  // the defaults of P3R_NTT_FWD_LOG_N1 and P3R_NTT_LOG_TILE

// A pass of `w` columns of 2^log_cells cells on 2^log_tile-cell tiles covers exactly those cells.
static void check_blocks(uint64_t w, int log_cells, int log_tile, const char* what, int log_n) {
  CHECK(log_tile >= 0 && log_cells - log_tile >= 0, "%s of 2^%d rows: shift by %d", what, log_n, log_cells - log_tile);
  const uint64_t blocks = ntt_pass_blocks(w, log_cells, log_tile);
  CHECK((blocks << log_tile) == (w << log_cells), "%s of 2^%d rows: %llu tiles of 2^%d cells", what, log_n,
        (unsigned long long)blocks, log_tile);
}
// A pass of the generic kernel as tu_lde.hip::launch_ntt lays it out; false: the LDS rule refuses it.
static bool check_generic(uint64_t w, int log_r, int log_lines, bool strided, int log_cosets, int log_n) {
  const int log_t = ntt_generic_log_t(log_r, log_lines, strided, kGenericLogTile);
  CHECK(log_t >= 0 && log_t <= log_lines, "generic pass of 2^%d rows: 2^%d lines a tile of 2^%d", log_n, log_t, log_lines);
  try {
    CHECK(ntt_generic_lds_bytes(log_r, log_t) <= kNttMaxLdsBytes, "generic pass of 2^%d rows: LDS", log_n);
  } catch (const Error& e) {
    CHECK(e.code == P3R_EUNSUPPORTED, "generic pass of 2^%d rows refused with code %d", log_n, e.code);
    return false;
  }
  check_blocks(w, log_r + log_lines + log_cosets, log_r + log_t, "generic pass", log_n);
  return true;
}
static void print_plan(const char* field, const char* dir, int line_log_tile, int log_n, const NttSplit& s, bool refused) {
  printf("%s %s %d %d %s %d %d %d %d\n", field, dir, line_log_tile, log_n,
         refused ? "refused" : s.single ? "single" : s.lean ? "lean" : "generic", s.la, s.lb, s.lean ? s.log_tile1 : 0,
         s.lean ? s.log_tile2 : 0);
}

template <class PP>
static void walk(const char* field) {
  for (int log_n = 0; log_n <= PP::TWO_ADICITY; ++log_n) {
    // ---- inverse
    const NttSplit s = ntt_inverse_split(log_n);
    CHECK(s.la + s.lb == log_n, "inverse 2^%d: %d + %d", log_n, s.la, s.lb);
    CHECK(s.single == (s.la == 0) && !(s.single && s.lean), "inverse 2^%d", log_n);
    CHECK(ntt_inv_pow_log_lo(log_n) == (s.single ? log_n : s.la), "inverse 2^%d: power table split", log_n);
    bool refused = false;
    for (uint64_t w : kWidths) {
      if (s.lean) {
        CHECK(s.la >= kNtt2MinLogR && s.la <= kNtt2MaxLogR && s.lb >= kNtt2MinLogR && s.lb <= kNtt2MaxLogR,
              "inverse 2^%d: column passes of 2^%d and 2^%d rows", log_n, s.la, s.lb);
        for (int t : {s.log_tile1, s.log_tile2}) CHECK(t == 13 || t == 14, "inverse 2^%d: column tile 2^%d", log_n, t);
        check_blocks(w, log_n, s.log_tile1, "inverse pass 1", log_n);
        check_blocks(w, log_n, s.log_tile2, "inverse pass 2", log_n);
      } else if (s.single) {
        refused |= !check_generic(w, log_n, 0, false, 0, log_n);
      } else {
        refused |= !check_generic(w, s.la, s.lb, true, 0, log_n) || !check_generic(w, s.lb, s.la, true, 0, log_n);
      }
    }
    print_plan(field, "inv", 12, log_n, s, refused);
    // ---- forward
    for (int line_log_tile : {12, 13}) {
      const NttSplit f = ntt_forward_split(log_n, kFwdLaCap, line_log_tile);
      CHECK(f.la + f.lb == log_n, "forward 2^%d: %d + %d", log_n, f.la, f.lb);
      CHECK(f.single == (f.la == 0) && !(f.single && f.lean), "forward 2^%d", log_n);
      refused = false;
      for (int added_bits = 0; added_bits <= 3 && log_n + added_bits <= PP::TWO_ADICITY; ++added_bits)
        for (uint64_t w : kWidths) {
          if (f.lean) {
            CHECK(f.la >= kNtt2MinLogR && f.la <= kNtt2MaxLogR, "forward 2^%d: column pass of 2^%d rows", log_n, f.la);
            CHECK(f.lb >= kNtt2MinLogR && f.lb <= kNtt2MaxLineLogR, "forward 2^%d: lines of 2^%d cells", log_n, f.lb);
            CHECK(f.log_tile1 == 13 || f.log_tile1 == 14, "forward 2^%d: column tile 2^%d", log_n, f.log_tile1);
            CHECK(f.log_tile2 == 12 || f.log_tile2 == 13, "forward 2^%d: line tile 2^%d", log_n, f.log_tile2);
            CHECK(f.lb <= f.log_tile2, "forward 2^%d: lines of 2^%d cells on 2^%d-cell tiles", log_n, f.lb, f.log_tile2);
            CHECK(f.log_tile2 == 13 || (line_log_tile == 12 && f.lb <= 12), "forward 2^%d: 2^12-cell line tile", log_n);
            check_blocks(w, log_n, f.log_tile1, "forward pass 1, one coset", log_n);  // the tile count xcd_map looks at
            check_blocks(w, log_n + added_bits, f.log_tile1, "forward pass 1", log_n);
            check_blocks(w, log_n + added_bits, f.log_tile2, "forward pass 2", log_n);
          } else if (f.single) {
            refused |= !check_generic(w, log_n, 0, false, added_bits, log_n);
          } else {
            refused |= !check_generic(w, f.la, f.lb, true, added_bits, log_n) ||
                       !check_generic(w, f.lb, f.la + added_bits, false, 0, log_n);
          }
        }
      print_plan(field, "fwd", line_log_tile, log_n, f, refused);
    }
    // ---- row bit-reversal
    const int log_t = ntt_bitrev_log_t(log_n);
    CHECK(log_t == 0 || log_t == 5 || log_t == 6, "bit-reversal of 2^%d rows: log_t = %d", log_n, log_t);
    CHECK(2 * log_t <= log_n, "bit-reversal of 2^%d rows: tiles of 2^%d x 2^%d cells", log_n, log_t, log_t);
    for (uint64_t w : kWidths) check_blocks(w, log_n, ntt_bitrev_log_tile(log_n), "bit-reversal", log_n);
  }
}

int main() {
  // a tile larger than the column is refused, not shifted by a negative amount
  try {
    ntt_pass_blocks(1, 12, 13);
    CHECK(false, "a 2^13-cell tile of a 2^12-cell column was accepted");
  } catch (const Error& e) {
    CHECK(e.code == P3R_EUNSUPPORTED, "refusal code %d", e.code);
  }
  walk<KoalaBearParams>("koala-bear");
  walk<BabyBearParams>("baby-bear");
  return 0;
}
