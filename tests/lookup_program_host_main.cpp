// The host half of the lookup-program seam (csrc/air_program.h in AIR_MODE_LOOKUP) compiled by g++ alone: typing, slots
// and peak_live of lookup programs, the degree rule of a column's constraint on hand-computed cases, every refusal a
// lookup program or the height of its traces can earn on the host, the compiled stream's term and end-of-column ops, and
// that the constraint mode still takes P3R_AIR_LOOKUP / P3R_AIR_LOOKUP_END for unknown ops.  A violated check is exit
// status 1 with a line on stderr.
// stdout, pinned by tests/test_lookup_program_host.py:
//   refused <name> <code>                                  one line per refusal
//   degree <name> <max_constraint_degree>                  one line per hand-computed case
//   info <n_terms> <n_columns> <max_terms_per_column> <max_constraint_degree> <peak_live>
//   live <peak> accepted|refused
//   stream <terms> <columns>
#include <cstdio>
#include <cstdlib>
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
                  PUB = P3R_AIR_PUBLIC, ADD = P3R_AIR_ADD, SUB = P3R_AIR_SUB, MUL = P3R_AIR_MUL, LOOKUP = P3R_AIR_LOOKUP, END = P3R_AIR_LOOKUP_END };

static AirPlan plan_of(const Prog& p, AirMode mode = AIR_MODE_LOOKUP, size_t n_public = 2, size_t n_chal = 2, uint32_t max_live = P3R_AIR_MAX_LIVE) {
  return air_plan(p.data(), p.size(), kWidths, 2, DC, P, n_public, n_chal, max_live, mode);
}
static int code_of(const std::function<void()>& fn) {
  try {
    fn();
  } catch (const Error& e) {
    CHECK(e.what()[0] != 0, "a refusal without a message");
    return e.code;
  }
  return 0;
}
static void refused(const char* name, int want, const std::function<void()>& fn) {
  const int got = code_of(fn);
  CHECK(got == want, "%s: code %d, expected %d", name, got, want);
  printf("refused %s %d\n", name, got);
}
static void degree(const char* name, const Prog& p, uint32_t want, std::vector<uint32_t> per_column) {
  const AirPlan pl = plan_of(p);
  CHECK(pl.lookup.max_constraint_degree == want, "%s: degree %u, expected %u", name, pl.lookup.max_constraint_degree, want);
  CHECK(pl.column_degree == per_column, "%s: per-column degrees", name);
  printf("degree %s %u\n", name, pl.lookup.max_constraint_degree);
}

// n cells loaded, then summed in load order (every cell is alive when the last is loaded); the sum is the denominator
static Prog live_program(uint32_t n) {
  Prog p;
  for (uint32_t k = 0; k < n; ++k) p.push_back({LOCAL, 1, k % 8});
  uint32_t acc = 0;
  for (uint32_t k = 1; k < n; ++k) {
    p.push_back({ADD, acc, k});
    acc = (uint32_t)p.size() - 1;
  }
  p.push_back({CONST, 1, 0});
  p.push_back({LOOKUP, (uint32_t)p.size() - 1, acc});
  p.push_back({END, 0, 0});
  return p;
}

int main() {
  // ---- refusals
  const Prog good{{CONST, 1, 0}, {LOCAL, 0, 0}, {LOOKUP, 0, 1}, {END, 0, 0}};
  CHECK(code_of([&] { plan_of(good); }) == 0, "a good lookup program");
  refused("assert_zero", P3R_EINVAL, [] { plan_of({{CONST, 1, 0}, {LOCAL, 0, 0}, {LOOKUP, 0, 1}, {END, 0, 0}, {P3R_AIR_ASSERT_ZERO, 1, 0}}); });
  for (uint32_t op : {(uint32_t)P3R_AIR_IS_FIRST_ROW, (uint32_t)P3R_AIR_IS_LAST_ROW, (uint32_t)P3R_AIR_IS_TRANSITION})
    refused("selector", P3R_EINVAL, [op] { plan_of({{op, 0, 0}, {LOCAL, 0, 0}, {LOOKUP, 0, 1}, {END, 0, 0}}); });
  refused("operand_not_earlier", P3R_EINVAL, [] { plan_of({{CONST, 1, 0}, {LOOKUP, 0, 1}, {END, 0, 0}}); });
  refused("operand_later", P3R_EINVAL, [] { plan_of({{CONST, 1, 0}, {LOOKUP, 7, 0}, {END, 0, 0}}); });
  refused("operand_is_lookup", P3R_EINVAL, [] { plan_of({{CONST, 1, 0}, {LOCAL, 0, 0}, {LOOKUP, 0, 1}, {LOOKUP, 0, 2}, {END, 0, 0}}); });
  refused("operand_is_lookup_end", P3R_EINVAL, [] { plan_of({{CONST, 1, 0}, {LOCAL, 0, 0}, {LOOKUP, 0, 1}, {END, 0, 0}, {LOOKUP, 3, 1}, {END, 0, 0}}); });
  refused("value_of_a_sink", P3R_EINVAL, [] { plan_of({{CONST, 1, 0}, {LOCAL, 0, 0}, {LOOKUP, 0, 1}, {ADD, 2, 1}, {END, 0, 0}}); });
  refused("end_with_no_open_column", P3R_EINVAL, [] { plan_of({{CONST, 1, 0}, {END, 0, 0}, {LOCAL, 0, 0}, {LOOKUP, 0, 2}, {END, 0, 0}}); });
  refused("end_twice", P3R_EINVAL, [] { plan_of({{CONST, 1, 0}, {LOCAL, 0, 0}, {LOOKUP, 0, 1}, {END, 0, 0}, {END, 0, 0}}); });
  refused("column_still_open", P3R_EINVAL, [] { plan_of({{CONST, 1, 0}, {LOCAL, 0, 0}, {LOOKUP, 0, 1}}); });
  refused("no_lookup", P3R_EINVAL, [] { plan_of({{CONST, 1, 0}, {LOCAL, 0, 0}, {ADD, 0, 1}}); });
  refused("empty", P3R_EINVAL, [] { air_plan(nullptr, 0, kWidths, 2, DC, P, 0, 0, P3R_AIR_MAX_LIVE, AIR_MODE_LOOKUP); });
  // ... and what a lookup program shares with a constraint program
  refused("unknown_op", P3R_EINVAL, [] { plan_of({{23, 0, 0}, {LOCAL, 0, 0}, {LOOKUP, 0, 1}, {END, 0, 0}}); });
  refused("matrix_out_of_range", P3R_EINVAL, [] { plan_of({{CONST, 1, 0}, {LOCAL, 2, 0}, {LOOKUP, 0, 1}, {END, 0, 0}}); });
  refused("column_out_of_range", P3R_EINVAL, [] { plan_of({{CONST, 1, 0}, {NEXT, 0, 3}, {LOOKUP, 0, 1}, {END, 0, 0}}); });
  refused("ext_columns_out_of_range", P3R_EINVAL, [] { plan_of({{CONST, 1, 0}, {LOCAL_EXT, 1, 5}, {LOOKUP, 0, 1}, {END, 0, 0}}); });
  refused("public_out_of_range", P3R_EINVAL, [] { plan_of({{PUB, 2, 0}, {LOCAL, 0, 0}, {LOOKUP, 0, 1}, {END, 0, 0}}); });
  refused("challenge_out_of_range", P3R_EINVAL, [] { plan_of({{CONST, 1, 0}, {CHAL, 2, 0}, {LOOKUP, 0, 1}, {END, 0, 0}}); });
  refused("non_canonical_constant", P3R_EINVAL, [] { plan_of({{CONST, P, 0}, {LOCAL, 0, 0}, {LOOKUP, 0, 1}, {END, 0, 0}}); });
  // ... and of the traces' height: no device matrix of such a height can be made (every allocation of one asks for a power
  // of two), so the seam's own check of it is walked here
  for (size_t h : {size_t(0), size_t(3), size_t(6), size_t(12), size_t(1000), (size_t(1) << 20) + 1})
    refused("height_not_a_power_of_two", P3R_EINVAL, [h] { air_trace_log_height(h, KoalaBearParams::TWO_ADICITY); });
  refused("height_above_two_adicity", P3R_EINVAL, [] { air_trace_log_height(size_t(1) << 25, KoalaBearParams::TWO_ADICITY); });
  refused("height_above_two_adicity", P3R_EINVAL, [] { air_trace_log_height(size_t(1) << 28, BabyBearParams::TWO_ADICITY); });
  CHECK(air_trace_log_height(1, KoalaBearParams::TWO_ADICITY) == 0 && air_trace_log_height(64, KoalaBearParams::TWO_ADICITY) == 6 &&
            air_trace_log_height(size_t(1) << 24, KoalaBearParams::TWO_ADICITY) == 24 && air_trace_log_height(size_t(1) << 27, BabyBearParams::TWO_ADICITY) == 27,
        "heights the seam takes");
  // the constraint mode knows neither op
  for (uint32_t op : {(uint32_t)P3R_AIR_LOOKUP, (uint32_t)P3R_AIR_LOOKUP_END}) {
    refused("constraint_mode_unknown_op", P3R_EINVAL,
            [op] { plan_of({{CONST, 1, 0}, {LOCAL, 0, 0}, {op, 0, 1}, {P3R_AIR_ASSERT_ZERO, 1, 0}}, AIR_MODE_CONSTRAINTS); });
    refused("default_mode_unknown_op", P3R_EINVAL, [op] {
      const Prog p{{CONST, 1, 0}, {LOCAL, 0, 0}, {op, 0, 1}, {P3R_AIR_ASSERT_ZERO, 1, 0}};
      air_plan(p.data(), p.size(), kWidths, 2, DC, P, 2, 2, P3R_AIR_MAX_LIVE);
    });
  }

  // ---- the degree of a column's constraint: max(1 + sum_k deg d_k, max_k(deg m_k + sum_{l != k} deg d_l)), by hand
  // one term, m constant, d a cell: max(1 + 1, 0 + 0) = 2
  degree("one_term", good, 2, {2});
  // one term, m a cell (base), d of degree 1: max(1 + 1, 1 + 0) = 2
  degree("one_term_base_multiplicity", {{LOCAL, 0, 1}, {LOCAL, 0, 0}, {LOOKUP, 0, 1}, {END, 0, 0}}, 2, {2});
  // one term, m an extension cell times a cell (degree 2), d of degree 1: max(2, 2 + 0) = 2
  degree("one_term_ext_multiplicity", {{LOCAL_EXT, 1, 0}, {LOCAL, 0, 1}, {MUL, 0, 1}, {LOCAL, 0, 0}, {LOOKUP, 2, 3}, {END, 0, 0}}, 2, {2});
  // one term, m of degree 3, d of degree 1: max(2, 3) = 3 - the numerator decides
  degree("one_term_cubic_multiplicity", {{LOCAL, 0, 1}, {MUL, 0, 0}, {MUL, 1, 0}, {LOCAL, 0, 0}, {LOOKUP, 2, 3}, {END, 0, 0}}, 3, {3});
  // one term, d = (challenge + cell) * cell of degree 2, m constant: max(1 + 2, 0) = 3
  degree("one_term_quadratic_denominator",
         {{CONST, 1, 0}, {CHAL, 0, 0}, {LOCAL, 0, 0}, {ADD, 1, 2}, {NEXT, 0, 1}, {MUL, 3, 4}, {LOOKUP, 0, 5}, {END, 0, 0}}, 3, {3});
  // two terms, d's of degree 1, m's constant and a cell: max(1 + 2, max(0 + 1, 1 + 1)) = 3
  degree("two_terms", {{CONST, 1, 0}, {LOCAL, 0, 0}, {LOCAL, 0, 1}, {LOCAL, 0, 2}, {LOOKUP, 0, 1}, {LOOKUP, 2, 3}, {END, 0, 0}}, 3, {3});
  // two terms, d_0 of degree 2, d_1 of degree 1, m_0 constant, m_1 of degree 2: max(1 + 3, max(0 + 1, 2 + 2)) = 4
  degree("two_terms_mixed", {{CONST, 1, 0}, {LOCAL, 0, 0}, {MUL, 1, 1}, {LOCAL, 0, 2}, {LOOKUP, 0, 2}, {LOOKUP, 2, 3}, {END, 0, 0}}, 4, {4});
  // ... the same with m_1 of degree 3 (d_0 * cell): max(4, max(1, 3 + 2)) = 5 - a numerator above the denominator product
  degree("two_terms_numerator_decides",
         {{CONST, 1, 0}, {LOCAL, 0, 0}, {MUL, 1, 1}, {LOCAL, 0, 2}, {MUL, 2, 3}, {LOOKUP, 0, 2}, {LOOKUP, 4, 3}, {END, 0, 0}}, 5, {5});
  // three terms, d's of degree 1, m's constant: max(1 + 3, 0 + 2) = 4
  degree("three_terms", {{CONST, 1, 0}, {LOCAL, 0, 0}, {LOCAL, 0, 1}, {LOCAL, 0, 2}, {LOOKUP, 0, 1}, {LOOKUP, 0, 2}, {LOOKUP, 0, 3}, {END, 0, 0}}, 4, {4});
  // three terms, d's of degree 1, 2, 1, m's of degree 0, 0, 2: max(1 + 4, max(0 + 3, 0 + 2, 2 + 3)) = 5
  degree("three_terms_mixed", {{CONST, 1, 0}, {LOCAL, 0, 0}, {MUL, 1, 1}, {LOCAL, 0, 2}, {LOOKUP, 0, 1}, {LOOKUP, 0, 2}, {LOOKUP, 2, 3}, {END, 0, 0}},
         5, {5});
  // columns of degrees 2, 4 and 3: every column on its own, the largest reported
  degree("three_columns", {{CONST, 1, 0}, {LOCAL, 0, 0}, {LOCAL, 0, 1}, {LOCAL, 0, 2}, {LOOKUP, 0, 1}, {END, 0, 0}, {LOOKUP, 0, 1}, {LOOKUP, 0, 2},
                           {LOOKUP, 0, 3}, {END, 0, 0}, {LOOKUP, 0, 2}, {LOOKUP, 0, 3}, {END, 0, 0}},
         4, {2, 4, 3});
  // a constant denominator: degree max(1 + 0, 0) = 1
  degree("constant_denominator", {{CONST, 1, 0}, {CHAL, 1, 0}, {LOOKUP, 0, 1}, {END, 0, 0}}, 1, {1});

  // ---- typing, slots and liveness: the operands of a LOOKUP are uses, the sinks take no slot
  {
    // ids: 0 chal (ext), 1 chal (ext), 2 cell, 3 cell, 4 = 1 * 3 (ext), 5 = 0 + 4 + ... (ext), 6 = ext cell, 7 LOOKUP(2, 5), 8 LOOKUP(6, 5), 9 END,
    // 10 const, 11 LOOKUP(10, 2), 12 END
    const Prog p{{CHAL, 0, 0}, {CHAL, 1, 0}, {LOCAL, 0, 0}, {NEXT, 0, 1}, {MUL, 1, 3}, {ADD, 0, 4}, {LOCAL_EXT, 1, 4}, {LOOKUP, 2, 5}, {LOOKUP, 6, 5},
                 {END, 0, 0}, {CONST, 5, 0}, {LOOKUP, 10, 2}, {END, 0, 0}};
    const AirPlan pl = plan_of(p);
    const uint8_t ext[13] = {1, 1, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 13; ++i) CHECK(pl.is_ext[i] == ext[i], "type of value %d", i);
    for (int i : {7, 8, 9, 11, 12}) CHECK(pl.slot[i] == kAirNoSlot, "sink %d has a slot", i);
    for (int i : {0, 1, 2, 3, 4, 5, 6, 10}) CHECK(pl.slot[i] != kAirNoSlot, "value %d has no slot", i);
    CHECK(pl.last_use[5] == 8 && pl.last_use[6] == 8 && pl.last_use[2] == 11 && pl.last_use[10] == 11, "the operands of a LOOKUP are uses");
    // alive at instruction 4: 0, 1 (dies there), 2, 3 (dies there) -> 4 before, result placed after the release: 3; at 6: 2, 5, 6 = 3.
    // The peak is at instruction 3, when 0, 1, 2, 3 are alive: 4
    CHECK(pl.lookup.peak_live == 4 && pl.info.peak_live == 4, "peak_live %u", pl.lookup.peak_live);
    CHECK(pl.n_ext_slots == 2 && pl.n_base_slots == 2, "slot regions %u ext, %u base", pl.n_ext_slots, pl.n_base_slots);
    CHECK(pl.lookup.n_terms == 3 && pl.lookup.n_columns == 2 && pl.lookup.max_terms_per_column == 2, "counts");
    // column 0: d = chal + chal * cell of degree 1 twice, m a cell and an ext cell: max(1 + 2, 1 + 1) = 3; column 1: d a cell, m constant: 2
    CHECK(pl.column_degree == (std::vector<uint32_t>{3, 2}) && pl.lookup.max_constraint_degree == 3, "degrees");
    printf("info %u %u %u %u %u\n", pl.lookup.n_terms, pl.lookup.n_columns, pl.lookup.max_terms_per_column, pl.lookup.max_constraint_degree,
           pl.lookup.peak_live);

    // the compiled stream: terms specialised by the operand types, the end of a column carries its output column
    const uint32_t publics[2] = {5, P - 1}, challenges[2 * DC] = {1, 2, 3, 4, P - 1, 0, 1, P - 2};
    const AirCompiled code = air_compile<KoalaBearParams>(pl, p.data(), p.size(), kWidths, 2, DC, publics, challenges);
    CHECK(code.insns.size() == p.size(), "one device instruction per instruction");
    CHECK(code.insns[7].op == AIR_D_TERM_BE && code.insns[7].a == pl.word_of(2, DC) && code.insns[7].b == pl.word_of(5, DC), "term 0");
    CHECK(code.insns[8].op == AIR_D_TERM_EE && code.insns[8].a == pl.word_of(6, DC) && code.insns[8].b == pl.word_of(5, DC), "term 1");
    CHECK(code.insns[11].op == AIR_D_TERM_BB && code.insns[11].a == pl.word_of(10, DC) && code.insns[11].b == pl.word_of(2, DC), "term 2");
    CHECK(code.insns[9].op == AIR_D_COL_END && code.insns[9].a == 1 && code.insns[12].op == AIR_D_COL_END && code.insns[12].a == 2, "column ends");
    const Prog eb{{LOCAL_EXT, 1, 0}, {LOCAL, 0, 0}, {LOOKUP, 0, 1}, {END, 0, 0}};
    const AirPlan pe = plan_of(eb);
    CHECK(air_compile<KoalaBearParams>(pe, eb.data(), eb.size(), kWidths, 2, DC, publics, challenges).insns[2].op == AIR_D_TERM_EB, "ext / base term");
    size_t terms = 0, columns = 0;
    for (const AirDevInsn& d : code.insns) {
      terms += d.op >= AIR_D_TERM_BB && d.op <= AIR_D_TERM_EE;
      columns += d.op == AIR_D_COL_END;
      // every slot word an instruction names lies inside the lane's slot file
      if (d.op != AIR_D_COL_END && d.op != AIR_D_CONST && d.op != AIR_D_CONST_EXT && d.op != AIR_D_LOAD && d.op != AIR_D_LOAD_EXT)
        CHECK(d.a < pl.words(DC) && d.b < pl.words(DC), "operand words");
      CHECK(d.dst < pl.words(DC), "destination word");
    }
    printf("stream %zu %zu\n", terms, columns);
  }

  // ---- the limit, from both sides
  {
    const AirPlan pl = plan_of(live_program(P3R_AIR_MAX_LIVE));
    CHECK(pl.lookup.peak_live == P3R_AIR_MAX_LIVE, "peak %u", pl.lookup.peak_live);
    printf("live %u accepted\n", pl.lookup.peak_live);
    CHECK(code_of([] { plan_of(live_program(P3R_AIR_MAX_LIVE + 1)); }) == P3R_EUNSUPPORTED, "one more live value");
    CHECK(plan_of(live_program(P3R_AIR_MAX_LIVE + 1), AIR_MODE_LOOKUP, 2, 2, P3R_AIR_MAX_LIVE + 1).lookup.peak_live == P3R_AIR_MAX_LIVE + 1, "peak of one more");
    printf("live %u refused\n", P3R_AIR_MAX_LIVE + 1);
  }
  return 0;
}
