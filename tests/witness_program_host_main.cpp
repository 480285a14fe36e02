// The host half of the witness seam (csrc/air_program.h in AIR_MODE_WITNESS) compiled by g++ alone: every refusal a
// witness program or the height of its output can earn on the host, each with its message; typing, slots and peak_live
// with STORE as a sink that takes no slot; the counts of p3r_witness_info; the compiled stream's new ops; the live limit
// from both sides; and that the two other modes still take the four witness ops for unknown ops.  A violated check is
// exit status 1 with a line on stderr.
// stdout, pinned by tests/test_witness_program_host.py:
//   refused <name> <code>                                       one line per refusal
//   accepted <name>                                             one line per accepted edge case
//   info <n_stores> <n_out_columns> <n_inversions> <peak_live>
//   live <peak> accepted|refused
//   stream <inv> <bits> <row> <stores>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#include "air_program.h"

using namespace p3r;
using Prog = std::vector<p3r_air_insn>;

#define CHECK(cond, ...)                                             \
  do {                                                               \
    if (!(cond)) {                                                   \
      fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond);     \
      fprintf(stderr, __VA_ARGS__);                                  \
      fprintf(stderr, "\n");                                         \
      exit(1);                                                       \
    }                                                                \
  } while (0)

static const uint32_t P = KoalaBearParams::P;
static const int DC = 4;
static const size_t kWidths[2] = {3, 8};
enum : uint32_t { LOCAL = P3R_AIR_LOCAL, NEXT = P3R_AIR_NEXT, LOCAL_EXT = P3R_AIR_LOCAL_EXT, CHAL = P3R_AIR_CHALLENGE, CONST = P3R_AIR_CONST,
                  PUB = P3R_AIR_PUBLIC, ADD = P3R_AIR_ADD, MUL = P3R_AIR_MUL, INV = P3R_AIR_INV, BITS = P3R_AIR_BITS, ROW = P3R_AIR_ROW,
                  STORE = P3R_AIR_STORE };
static uint32_t field_of(uint32_t lo, uint32_t n) { return lo | n << 8; }

static AirPlan plan_of(const Prog& p, AirMode mode = AIR_MODE_WITNESS, size_t n_public = 2, size_t n_chal = 2, uint32_t max_live = P3R_AIR_MAX_LIVE) {
  return air_plan(p.data(), p.size(), kWidths, 2, DC, P, n_public, n_chal, max_live, mode);
}
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
static void refused(const char* name, int want, const char* text, const std::function<void()>& fn) {
  const int got = code_of(fn, text);
  CHECK(got == want, "%s: code %d, expected %d", name, got, want);
  printf("refused %s %d\n", name, got);
}
static void accepted(const char* name, const Prog& p) {
  CHECK(code_of([&] { plan_of(p); }) == 0, "%s is refused", name);
  printf("accepted %s\n", name);
}

// n cells loaded, then summed in load order (every cell is alive when the last is loaded); the sum is stored
static Prog live_program(uint32_t n) {
  Prog p;
  for (uint32_t k = 0; k < n; ++k) p.push_back({LOCAL, 1, k % 8});
  uint32_t acc = 0;
  for (uint32_t k = 1; k < n; ++k) {
    p.push_back({ADD, acc, k});
    acc = (uint32_t)p.size() - 1;
  }
  p.push_back({STORE, acc, 0});
  return p;
}

int main() {
  // ---- refusals, one per rule
  const Prog good{{LOCAL, 0, 0}, {STORE, 0, 0}};
  CHECK(code_of([&] { plan_of(good); }) == 0, "a good witness program");
  // ... the sinks of the other seams
  refused("assert_zero", P3R_EINVAL, "ASSERT_ZERO in a witness program", [] { plan_of({{LOCAL, 0, 0}, {STORE, 0, 0}, {P3R_AIR_ASSERT_ZERO, 0, 0}}); });
  refused("lookup", P3R_EINVAL, "LOOKUP in a witness program", [] { plan_of({{LOCAL, 0, 0}, {STORE, 0, 0}, {P3R_AIR_LOOKUP, 0, 0}}); });
  refused("lookup_end", P3R_EINVAL, "LOOKUP_END in a witness program", [] { plan_of({{LOCAL, 0, 0}, {STORE, 0, 0}, {P3R_AIR_LOOKUP_END, 0, 0}}); });
  // ... BITS
  refused("bits_of_extension", P3R_EINVAL, "BITS of an extension value", [] { plan_of({{CHAL, 0, 0}, {BITS, 0, field_of(0, 8)}, {STORE, 1, 0}}); });
  refused("bits_none", P3R_EINVAL, "at least one bit", [] { plan_of({{LOCAL, 0, 0}, {BITS, 0, field_of(3, 0)}, {STORE, 1, 0}}); });
  refused("bits_1_31", P3R_EINVAL, "none above bit 30", [] { plan_of({{LOCAL, 0, 0}, {BITS, 0, field_of(1, 31)}, {STORE, 1, 0}}); });
  refused("bits_31_1", P3R_EINVAL, "none above bit 30", [] { plan_of({{LOCAL, 0, 0}, {BITS, 0, field_of(31, 1)}, {STORE, 1, 0}}); });
  refused("bits_huge_count", P3R_EINVAL, "none above bit 30", [] { plan_of({{LOCAL, 0, 0}, {BITS, 0, 0xffffff00u}, {STORE, 1, 0}}); });
  accepted("bits_0_31", {{LOCAL, 0, 0}, {BITS, 0, field_of(0, 31)}, {STORE, 1, 0}});
  accepted("bits_30_1", {{LOCAL, 0, 0}, {BITS, 0, field_of(30, 1)}, {STORE, 1, 0}});
  // ... operands of the four ops
  refused("inv_operand_not_earlier", P3R_EINVAL, "not an earlier value", [] { plan_of({{INV, 0, 0}, {STORE, 0, 0}}); });
  refused("bits_operand_not_earlier", P3R_EINVAL, "not an earlier value", [] { plan_of({{LOCAL, 0, 0}, {BITS, 5, field_of(0, 8)}, {STORE, 0, 0}}); });
  refused("store_operand_not_earlier", P3R_EINVAL, "not an earlier value", [] { plan_of({{LOCAL, 0, 0}, {STORE, 1, 0}}); });
  refused("store_of_store", P3R_EINVAL, "a STORE, which has no value", [] { plan_of({{LOCAL, 0, 0}, {STORE, 0, 0}, {STORE, 1, 1}}); });
  refused("inv_of_store", P3R_EINVAL, "a STORE, which has no value", [] { plan_of({{LOCAL, 0, 0}, {STORE, 0, 0}, {INV, 1, 0}, {STORE, 2, 1}}); });
  refused("add_of_store", P3R_EINVAL, "a STORE, which has no value", [] { plan_of({{LOCAL, 0, 0}, {STORE, 0, 0}, {ADD, 0, 1}, {STORE, 2, 1}}); });
  // ... the output columns
  refused("no_store", P3R_EINVAL, "no STORE", [] { plan_of({{LOCAL, 0, 0}, {INV, 0, 0}}); });
  refused("empty", P3R_EINVAL, "no STORE", [] { air_plan(nullptr, 0, kWidths, 2, DC, P, 0, 0, P3R_AIR_MAX_LIVE, AIR_MODE_WITNESS); });
  refused("stored_twice", P3R_EINVAL, "column 1 is stored twice", [] { plan_of({{LOCAL, 0, 0}, {STORE, 0, 0}, {STORE, 0, 1}, {STORE, 0, 1}}); });
  refused("ext_store_overlaps_later", P3R_EINVAL, "column 3 is stored twice", [] { plan_of({{LOCAL, 0, 0}, {CHAL, 0, 0}, {STORE, 1, 0}, {STORE, 0, 3}}); });
  refused("ext_store_overlaps_earlier", P3R_EINVAL, "stored twice", [] { plan_of({{LOCAL, 0, 0}, {CHAL, 0, 0}, {STORE, 0, 0}, {STORE, 0, 1}, {STORE, 1, 1}}); });
  refused("column_not_stored", P3R_EINVAL, "column 1 is stored by no instruction", [] { plan_of({{LOCAL, 0, 0}, {STORE, 0, 0}, {STORE, 0, 2}}); });
  refused("column_0_not_stored", P3R_EINVAL, "column 0 is stored by no instruction", [] { plan_of({{LOCAL, 0, 0}, {STORE, 0, 1}}); });
  refused("gap_before_ext_store", P3R_EINVAL, "column 1 is stored by no instruction", [] { plan_of({{LOCAL, 0, 0}, {CHAL, 0, 0}, {STORE, 0, 0}, {STORE, 1, 2}}); });
  refused("too_many_columns", P3R_EINVAL, "too many output columns", [] { plan_of({{LOCAL, 0, 0}, {STORE, 0, 0x7fffffffu}}); });
  refused("ext_store_wraps", P3R_EINVAL, "too many output columns", [] { plan_of({{CHAL, 0, 0}, {STORE, 0, 0xfffffffeu}}); });
  // an extension store at W - DC, between two base stores and as the last columns
  accepted("ext_store_at_w_minus_dc", {{LOCAL, 0, 0}, {CHAL, 0, 0}, {STORE, 0, 0}, {STORE, 1, 1}});
  accepted("ext_store_between_base_stores", {{LOCAL, 0, 0}, {CHAL, 0, 0}, {STORE, 0, 5}, {STORE, 1, 1}, {STORE, 0, 0}});
  {
    const Prog p{{LOCAL, 0, 0}, {CHAL, 0, 0}, {STORE, 0, 0}, {STORE, 1, 1}};
    CHECK(plan_of(p).witness.n_out_columns == 1 + DC, "W of a base and an extension store");
  }
  // ... and what a witness program shares with the other programs
  refused("unknown_op", P3R_EINVAL, "unknown op 27", [] { plan_of({{27, 0, 0}, {LOCAL, 0, 0}, {STORE, 1, 0}}); });
  refused("unknown_op_low", P3R_EINVAL, "unknown op 5", [] { plan_of({{5, 0, 0}, {LOCAL, 0, 0}, {STORE, 1, 0}}); });
  refused("matrix_out_of_range", P3R_EINVAL, "matrix 2 of 2", [] { plan_of({{LOCAL, 2, 0}, {STORE, 0, 0}}); });
  refused("column_out_of_range", P3R_EINVAL, "column 3 of matrix 0", [] { plan_of({{NEXT, 0, 3}, {STORE, 0, 0}}); });
  refused("ext_columns_out_of_range", P3R_EINVAL, "columns 5 .. + DC", [] { plan_of({{LOCAL_EXT, 1, 5}, {STORE, 0, 0}}); });
  refused("public_out_of_range", P3R_EINVAL, "public value 2 of 2", [] { plan_of({{PUB, 2, 0}, {STORE, 0, 0}}); });
  refused("challenge_out_of_range", P3R_EINVAL, "challenge 2 of 2", [] { plan_of({{CHAL, 2, 0}, {STORE, 0, 0}}); });
  refused("non_canonical_constant", P3R_EINVAL, "non-canonical constant", [] { plan_of({{CONST, P, 0}, {STORE, 0, 0}}); });
  refused("input_with_no_matrix", P3R_EINVAL, "matrix 0 of 0", [] {
    const Prog p{{LOCAL, 0, 0}, {STORE, 0, 0}};
    air_plan(p.data(), p.size(), nullptr, 0, DC, P, 0, 0, P3R_AIR_MAX_LIVE, AIR_MODE_WITNESS);
  });
  // ... the height of a program with no input matrix: the seam's own check of it, walked here
  for (size_t h : {size_t(0), size_t(3), size_t(100)})
    refused("height_not_a_power_of_two", P3R_EINVAL, "must be a power of two", [h] { air_trace_log_height(h, KoalaBearParams::TWO_ADICITY); });
  refused("height_above_two_adicity", P3R_EINVAL, "two-adicity", [] { air_trace_log_height(size_t(1) << 25, KoalaBearParams::TWO_ADICITY); });
  // a program of ROW alone needs no matrix
  {
    const Prog p{{ROW, 0, 0}, {STORE, 0, 0}};
    const AirPlan pl = air_plan(p.data(), p.size(), nullptr, 0, DC, P, 0, 0, P3R_AIR_MAX_LIVE, AIR_MODE_WITNESS);
    CHECK(pl.witness.n_out_columns == 1 && pl.witness.n_stores == 1 && pl.witness.peak_live == 1, "the row table");
    printf("accepted row_with_no_matrix\n");
  }
  // the selectors have a value on the trace domain here
  accepted("selectors", {{P3R_AIR_IS_FIRST_ROW, 0, 0}, {P3R_AIR_IS_LAST_ROW, 0, 0}, {P3R_AIR_IS_TRANSITION, 0, 0}, {STORE, 0, 0}, {STORE, 1, 1}, {STORE, 2, 2}});
  // the other modes know none of the four ops
  for (uint32_t op : {INV, BITS, ROW, STORE}) {
    char text[32];
    snprintf(text, sizeof text, "unknown op %u", op);
    const uint32_t b = op == BITS ? field_of(0, 8) : 0;
    refused("constraint_mode_unknown_op", P3R_EINVAL, text,
            [op, b] { plan_of({{LOCAL, 0, 0}, {op, 0, b}, {P3R_AIR_ASSERT_ZERO, 0, 0}}, AIR_MODE_CONSTRAINTS); });
    refused("lookup_mode_unknown_op", P3R_EINVAL, text,
            [op, b] { plan_of({{LOCAL, 0, 0}, {op, 0, b}, {P3R_AIR_LOOKUP, 0, 0}, {P3R_AIR_LOOKUP_END, 0, 0}}, AIR_MODE_LOOKUP); });
    refused("default_mode_unknown_op", P3R_EINVAL, text, [op, b] {
      const Prog p{{LOCAL, 0, 0}, {op, 0, b}, {P3R_AIR_ASSERT_ZERO, 0, 0}};
      air_plan(p.data(), p.size(), kWidths, 2, DC, P, 2, 2, P3R_AIR_MAX_LIVE);
    });
  }

  // ---- typing, slots, liveness and the compiled stream
  {
    // ids: 0 cell, 1 chal (ext), 2 = inv 0 (base), 3 = inv 1 (ext), 4 = bits 0, 5 = row, 6 STORE(2 -> 0), 7 = 3 * 0 (ext), 8 STORE(7 -> 1),
    // 9 = 4 + 5, 10 STORE(9 -> 1 + DC), 11 STORE(3 -> 2 + DC)
    const Prog p{{LOCAL, 0, 0}, {CHAL, 1, 0}, {INV, 0, 0}, {INV, 1, 0}, {BITS, 0, field_of(8, 8)}, {ROW, 0, 0}, {STORE, 2, 0}, {MUL, 3, 0},
                 {STORE, 7, 1}, {ADD, 4, 5}, {STORE, 9, 1 + DC}, {STORE, 3, 2 + DC}};
    const AirPlan pl = plan_of(p);
    const uint8_t ext[12] = {0, 1, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0};
    for (int i = 0; i < 12; ++i) CHECK(pl.is_ext[i] == ext[i], "type of value %d", i);
    for (int i : {6, 8, 10, 11}) CHECK(pl.slot[i] == kAirNoSlot, "STORE %d has a slot", i);
    for (int i : {0, 1, 2, 3, 4, 5, 7, 9}) CHECK(pl.slot[i] != kAirNoSlot, "value %d has no slot", i);
    CHECK(pl.last_use[2] == 6 && pl.last_use[3] == 11 && pl.last_use[7] == 8 && pl.last_use[9] == 10, "the operand of a STORE is a use");
    // alive after instruction 5: 0, 2, 3, 4, 5 (1 died at 3) = 5; before it 0, 2, 3, 4 and at 3 the operand 1 is released first: the peak is 5
    CHECK(pl.witness.peak_live == 5 && pl.info.peak_live == 5, "peak_live %u", pl.witness.peak_live);
    CHECK(pl.witness.n_stores == 4 && pl.witness.n_out_columns == 2 + 2 * DC && pl.witness.n_inversions == 2, "counts");
    printf("info %u %u %u %u\n", pl.witness.n_stores, pl.witness.n_out_columns, pl.witness.n_inversions, pl.witness.peak_live);

    const uint32_t publics[2] = {5, P - 1}, challenges[2 * DC] = {1, 2, 3, 4, P - 1, 0, 1, P - 2};
    const AirCompiled code = air_compile<KoalaBearParams>(pl, p.data(), p.size(), kWidths, 2, DC, publics, challenges);
    CHECK(code.insns.size() == p.size(), "one device instruction per instruction");
    CHECK(code.insns[2].op == AIR_D_INV_B && code.insns[2].a == pl.word_of(0, DC) && code.insns[2].dst == pl.word_of(2, DC), "base inverse");
    CHECK(code.insns[3].op == AIR_D_INV_E && code.insns[3].a == pl.word_of(1, DC) && code.insns[3].dst == pl.word_of(3, DC), "extension inverse");
    CHECK(code.insns[4].op == AIR_D_BITS && code.insns[4].a == pl.word_of(0, DC) && code.insns[4].b == field_of(8, 8), "bit field");
    CHECK(code.insns[5].op == AIR_D_ROW && code.insns[5].dst == pl.word_of(5, DC), "row");
    CHECK(code.insns[6].op == AIR_D_STORE_B && code.insns[6].a == pl.word_of(2, DC) && code.insns[6].b == 0, "base store");
    CHECK(code.insns[8].op == AIR_D_STORE_E && code.insns[8].a == pl.word_of(7, DC) && code.insns[8].b == 1, "extension store");
    CHECK(code.insns[10].op == AIR_D_STORE_B && code.insns[10].b == 1 + DC && code.insns[11].op == AIR_D_STORE_E && code.insns[11].b == 2 + DC, "stores");
    size_t inv = 0, bits = 0, row = 0, stores = 0;
    for (const AirDevInsn& d : code.insns) {
      inv += d.op == AIR_D_INV_B || d.op == AIR_D_INV_E;
      bits += d.op == AIR_D_BITS;
      row += d.op == AIR_D_ROW;
      const bool st = d.op == AIR_D_STORE_B || d.op == AIR_D_STORE_E;
      stores += st;
      // every slot word an instruction names lies inside the lane's slot file, every output column inside the output
      if (st || d.op == AIR_D_INV_B || d.op == AIR_D_INV_E || d.op == AIR_D_BITS) CHECK(d.a < pl.words(DC), "operand word");
      if (st) CHECK(d.b + (d.op == AIR_D_STORE_E ? DC : 1) <= pl.witness.n_out_columns, "output column");
      CHECK(d.dst < pl.words(DC), "destination word");
    }
    printf("stream %zu %zu %zu %zu\n", inv, bits, row, stores);
  }

  // ---- the limit, from both sides: STORE takes no slot
  {
    const AirPlan pl = plan_of(live_program(P3R_AIR_MAX_LIVE));
    CHECK(pl.witness.peak_live == P3R_AIR_MAX_LIVE, "peak %u", pl.witness.peak_live);
    printf("live %u accepted\n", pl.witness.peak_live);
    CHECK(code_of([] { plan_of(live_program(P3R_AIR_MAX_LIVE + 1)); }, "P3R_AIR_MAX_LIVE") == P3R_EUNSUPPORTED, "one more live value");
    CHECK(plan_of(live_program(P3R_AIR_MAX_LIVE + 1), AIR_MODE_WITNESS, 2, 2, P3R_AIR_MAX_LIVE + 1).witness.peak_live == P3R_AIR_MAX_LIVE + 1, "peak of one more");
    printf("live %u refused\n", P3R_AIR_MAX_LIVE + 1);
  }
  return 0;
}
