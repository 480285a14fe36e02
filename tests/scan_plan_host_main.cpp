// The host half of the recurrence seam (csrc/scan_plan.h) compiled by g++ alone: every refusal a set of p3r_recurrence
// descriptors or the height of their traces can earn on the host, each with its message; the edges a valid set may stand
// on; the forms, the width and the counts of a mixed set; the geometry of the three passes.  A violated check is exit
// status 1 with a line on stderr.
// stdout, pinned by tests/test_affine_scan_host.py:
//   refused <name> <code>                                       one line per refusal
//   accepted <name> <n_out_columns>                             one line per accepted edge case
//   info <n_out_columns> <n_products> <n_sums> <n_affine>
//   forms <form of each recurrence of the mixed set>
//   geometry <kAffItems> <kAffBlock> <kAffTile> <smallest height with two tiles per thread of pass 1>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#include "scan_plan.h"

using namespace p3r;
using Recs = std::vector<p3r_recurrence>;

#define CHECK(cond, ...)                                             \
  do {                                                               \
    if (!(cond)) {                                                   \
      fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond);     \
      fprintf(stderr, __VA_ARGS__);                                  \
      fprintf(stderr, "\n");                                         \
      exit(1);                                                       \
    }                                                                \
  } while (0)

static const uint32_t P = 0x7f000001u;   // KoalaBear
static const int DC = 4;
static const size_t kWidths[2] = {3, 8};   // three base columns; two flattened extension columns
static const uint32_t NONE = P3R_SCAN_NONE, EXT = P3R_SCAN_EXT, INCL = P3R_SCAN_INCLUSIVE;

static p3r_recurrence rec(uint32_t flags, uint32_t mm, uint32_t mc, uint32_t am, uint32_t ac, uint32_t out, std::vector<uint32_t> init = {}) {
  p3r_recurrence r{};
  r.flags = flags, r.mul_mat = mm, r.mul_col = mc, r.add_mat = am, r.add_col = ac, r.out_col = out;
  for (size_t k = 0; k < init.size() && k < 5; ++k) r.init[k] = init[k];
  return r;
}
static ScanPlan plan_of(const Recs& r, size_t n_mats = 2, int dc = DC) { return scan_plan(r.data(), r.size(), kWidths, n_mats, dc, P); }
// the code of a refusal whose message holds `text`; 0 when nothing is refused
static int code_of(const std::function<void()>& fn, const char* text = "") {
  try {
    fn();
  } catch (const Error& e) {
    CHECK(e.what()[0] != 0, "a refusal without a message");
    CHECK(strstr(e.what(), text), "the message \"%s\" does not say \"%s\"", e.what(), text);
    return e.code;
  }
  return 0;
}
static void refused(const char* name, const char* text, const std::function<void()>& fn) {
  const int got = code_of(fn, text);
  CHECK(got == P3R_EINVAL, "%s: code %d, expected %d", name, got, P3R_EINVAL);
  printf("refused %s %d\n", name, got);
}
static void refused(const char* name, const char* text, const Recs& r) {
  refused(name, text, [&] { plan_of(r); });
}
static void accepted(const char* name, const Recs& r, int dc = DC) {
  uint32_t w = 0;
  CHECK(code_of([&] { w = plan_of(r, 2, dc).info.n_out_columns; }) == 0, "%s is refused", name);
  printf("accepted %s %u\n", name, w);
}

int main() {
  // ---- a set of every form, outputs interleaved: ext affine at 0, base sum at 4, base product at 5, ext product at 6,
  // base affine at 10, ext sum at 11
  const Recs mixed = {rec(0, NONE, 0, 0, 0, 4),           rec(EXT, 1, 0, 1, 4, 0, {1, 2, 3, 4}), rec(INCL, 0, 1, NONE, 0, 5, {1}),
                      rec(EXT, 1, 4, NONE, 0, 6, {1}),    rec(0, 0, 2, 0, 0, 10, {P - 1}),       rec(EXT | INCL, NONE, 0, 1, 0, 11)};
  {
    const ScanPlan pl = plan_of(mixed);
    printf("info %u %u %u %u\n", pl.info.n_out_columns, pl.info.n_products, pl.info.n_sums, pl.info.n_affine);
    printf("forms");
    for (uint32_t f : pl.form) printf(" %u", f);
    printf("\n");
    CHECK(pl.form.size() == mixed.size(), "one form per recurrence");
  }
  auto but = [&](size_t i, const p3r_recurrence& r) {
    Recs out = mixed;
    out[i] = r;
    return out;
  };

  // ---- refusals
  refused("no_recurrences", "n_recs == 0", [&] { scan_plan(mixed.data(), 0, kWidths, 2, DC, P); });
  refused("null_recs", "recs is NULL", [&] { scan_plan(nullptr, 1, kWidths, 2, DC, P); });
  refused("too_many_recurrences", "at most 65535", [&] { scan_plan(mixed.data(), 65536, kWidths, 2, DC, P); });
  refused("no_matrices", "n_mats == 0", [&] { scan_plan(mixed.data(), mixed.size(), kWidths, 0, DC, P); });
  refused("null_widths", "widths is NULL", [&] { scan_plan(mixed.data(), mixed.size(), nullptr, 2, DC, P); });
  refused("unknown_flag", "unknown flag bits 0x4", Recs{rec(4, NONE, 0, 0, 0, 0)});
  refused("unknown_flag_high", "unknown flag bits 0x80000000", Recs{rec(0x80000001u, NONE, 0, 1, 0, 0)});
  refused("neither_mul_nor_add", "neither mul nor add", but(2, rec(0, NONE, 0, NONE, 0, 5)));
  refused("mul_matrix_out_of_range", "mul reads matrix 2 of 2", but(2, rec(0, 2, 0, NONE, 0, 5)));
  refused("add_matrix_out_of_range", "add reads matrix 7 of 2", but(0, rec(0, NONE, 0, 7, 0, 4)));
  refused("matrix_just_below_none", "mul reads matrix 4294967294 of 2", but(2, rec(0, 0xfffffffeu, 0, NONE, 0, 5)));
  refused("column_out_of_range", "add reads column 3 of matrix 0", but(0, rec(0, NONE, 0, 0, 3, 4)));
  refused("column_wraps", "mul reads column 4294967295 of matrix 0", but(2, rec(0, 0, 0xffffffffu, NONE, 0, 5)));
  refused("ext_columns_out_of_range", "mul reads columns 5 .. 5 + DC of matrix 1", but(3, rec(EXT, 1, 5, NONE, 0, 6, {1})));
  refused("ext_columns_of_a_narrow_matrix", "add reads columns 0 .. 0 + DC of matrix 0", but(5, rec(EXT, NONE, 0, 0, 0, 11)));
  refused("ext_columns_wrap", "+ DC of matrix 1", but(3, rec(EXT, 1, 0xfffffffeu, NONE, 0, 6, {1})));
  refused("init_not_canonical", "non-canonical word 0 of init", but(4, rec(0, 0, 2, 0, 0, 10, {P})));
  refused("ext_init_not_canonical", "non-canonical word 3 of init", but(1, rec(EXT, 1, 0, 1, 4, 0, {0, 0, 0, 0xffffffffu})));
  refused("base_init_not_padded", "word 1 of init is not zero", but(4, rec(0, 0, 2, 0, 0, 10, {1, 1})));
  refused("ext_init_not_padded", "word 4 of init is not zero", but(1, rec(EXT, 1, 0, 1, 4, 0, {1, 2, 3, 4, 5})));
  refused("same_output_column", "recurrences 0 and 2 overlap at column 4", but(2, rec(INCL, 0, 1, NONE, 0, 4, {1})));
  refused("base_inside_ext_output", "recurrences 0 and 1 overlap at column 3", but(0, rec(0, NONE, 0, 0, 0, 3)));
  refused("ext_outputs_overlap", "recurrences 3 and 5 overlap at column 9", but(5, rec(EXT | INCL, NONE, 0, 1, 0, 9)));
  refused("gap_below_w", "output column 15, below W = 17, is written by no recurrence", [&] {
    Recs r = mixed;
    r.push_back(rec(0, NONE, 0, 0, 0, 16));
    plan_of(r);
  });
  refused("column_0_not_written", "output column 0, below W = 2", Recs{rec(0, NONE, 0, 0, 0, 1)});
  refused("gap_before_ext_output", "output column 1, below W = 6", Recs{rec(0, NONE, 0, 0, 0, 0), rec(EXT, 1, 0, NONE, 0, 2)});
  refused("output_column_out_of_range", "output column 4294967295 is out of range", Recs{rec(0, NONE, 0, 0, 0, 0xffffffffu)});
  refused("ext_output_column_out_of_range", "is out of range", Recs{rec(EXT, 1, 0, NONE, 0, 0x7ffffffcu)});
  refused("height_0", "power of two", [&] { scan_log_height(0, 24); });
  refused("height_3", "power of two", [&] { scan_log_height(3, 24); });
  refused("height_above_two_adicity", "two-adicity", [&] { scan_log_height(size_t(1) << 25, 24); });

  // ---- the edges a valid set may stand on
  accepted("one_base_sum", Recs{rec(0, NONE, 0, 0, 2, 0, {P - 1})});
  accepted("last_columns_read", Recs{rec(0, 0, 2, 0, 2, 0), rec(EXT, 1, 4, 1, 4, 1, {P - 1, P - 1, P - 1, P - 1})});
  accepted("outputs_in_any_order", Recs{rec(EXT, 1, 0, NONE, 0, 1), rec(0, NONE, 0, 0, 0, 0), rec(0, 0, 0, NONE, 0, 5)});
  accepted("same_input_for_a_and_b", Recs{rec(0, 0, 1, 0, 1, 0), rec(0, 0, 1, NONE, 0, 1), rec(0, NONE, 0, 0, 1, 2)});
  accepted("quintic_init_of_five_words", Recs{rec(EXT, 1, 0, 1, 3, 0, {1, 2, 3, 4, 5})}, 5);
  CHECK(scan_log_height(1, 24) == 0 && scan_log_height(size_t(1) << 24, 24) == 24, "heights 1 and 2^24 stand");

  // ---- the geometry: a thread owns kAffItems rows, a workgroup kAffTile; a thread of pass 1 carries a second tile from
  // kAffBlock + 1 tiles on
  CHECK(kAffTile == kAffBlock * kAffItems && kAffItems == 4, "a thread's rows are one 16-byte access");
  CHECK(scan_tiles(1) == 1 && scan_tiles(kAffTile) == 1 && scan_tiles(kAffTile + 1) == 2 && scan_tiles(2 * (size_t)kAffTile) == 2, "tiles");
  size_t h = 1;
  while (scan_tiles_per_thread(scan_tiles(h)) < 2) h <<= 1;
  CHECK(scan_tiles_per_thread(scan_tiles(h / 2)) == 1 && scan_tiles(h / 2) == (size_t)kAffBlock, "one tile per thread up to kAffBlock tiles");
  printf("geometry %d %d %d %zu\n", kAffItems, kAffBlock, kAffTile, h);
  return 0;
}
