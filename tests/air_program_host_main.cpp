// The host half of the constraint-program seam (csrc/air_program.h) compiled by g++ alone: every refusal a program or a
// domain can earn on the host, the degree walk on hand-built programs of degree 1, 2, 3, 5 and 9, the limit
// P3R_AIR_MAX_LIVE from both sides, and the slot assignment - random programs of mixed base / extension values are
// replayed on integers twice, once value by value and once through the compiled instruction stream and its LDS words, and
// every asserted value must agree (two live values in one slot would clobber each other).  A violated check is exit status
// 1 with a line on stderr.  stdout, pinned by tests/test_air_program_host.py:
//   refused <name> <code>              one line per refusal
//   degree <d> <log_quotient_degree>   one line per hand-built program
//   live <peak> accepted|refused
//   replay <programs> <constraints>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <random>
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

static AirPlan plan_of(const Prog& p, size_t n_public = 2, size_t n_chal = 2, uint32_t max_live = P3R_AIR_MAX_LIVE) {
  return air_plan(p.data(), p.size(), kWidths, 2, DC, P, n_public, n_chal, max_live);
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

// x^d of one trace cell, asserted: degree d
static Prog power_program(int d) {
  Prog p{{P3R_AIR_LOCAL, 0, 0}};
  for (int k = 1; k < d; ++k) p.push_back({P3R_AIR_MUL, (uint32_t)p.size() - 1, 0});
  p.push_back({P3R_AIR_ASSERT_ZERO, (uint32_t)p.size() - 1, 0});
  return p;
}
// n cells loaded, then summed in load order: every cell is alive when the last is loaded
static Prog live_program(uint32_t n) {
  Prog p;
  for (uint32_t k = 0; k < n; ++k) p.push_back({P3R_AIR_LOCAL, 1, k % 8});
  uint32_t acc = 0;
  for (uint32_t k = 1; k < n; ++k) {
    p.push_back({P3R_AIR_ADD, acc, k});
    acc = (uint32_t)p.size() - 1;
  }
  p.push_back({P3R_AIR_ASSERT_ZERO, acc, 0});
  return p;
}

// ---- replay on integers.  An "extension" value is DC residues with the rules of the interpreter's mixed ops (a base
// operand adds to word 0, scales every word) and a word-by-word product: not a field, but the same on both sides.
struct Val { bool ext; uint64_t w[DC]; };
static uint64_t leaf_word(const p3r_air_insn& in, int k) { return (in.op * 2654435761ull + in.a * 40503ull + in.b * 97ull + k * 7919ull + 1) % P; }
static Val leaf(const p3r_air_insn& in, bool ext) {
  Val v{ext, {}};
  for (int k = 0; k < (ext ? DC : 1); ++k) v.w[k] = leaf_word(in, k);
  return v;
}
static Val arith(uint32_t op, const Val& x, const Val& y) {
  Val r{x.ext || y.ext, {}};
  const int n = r.ext ? DC : 1;
  for (int k = 0; k < n; ++k) {
    const uint64_t a = (x.ext || k == 0) ? x.w[k] : 0, b = (y.ext || k == 0) ? y.w[k] : 0;
    if (op == P3R_AIR_ADD) r.w[k] = (a + b) % P;
    else if (op == P3R_AIR_SUB) r.w[k] = (a + P - b) % P;
    else if (x.ext && y.ext) r.w[k] = a * b % P;
    else r.w[k] = (x.ext ? x.w[k] * y.w[0] : y.ext ? y.w[k] * x.w[0] : a * b) % P;
  }
  return r;
}
static std::vector<Val> replay_values(const Prog& p, const AirPlan& pl) {
  std::vector<Val> vals(p.size()), asserted;
  for (size_t i = 0; i < p.size(); ++i) {
    const p3r_air_insn& in = p[i];
    if (air_op_is_binary(in.op)) vals[i] = arith(in.op, vals[in.a], vals[in.b]);
    else if (in.op == P3R_AIR_NEG) vals[i] = arith(P3R_AIR_SUB, Val{vals[in.a].ext, {}}, vals[in.a]);
    else if (in.op == P3R_AIR_ASSERT_ZERO) asserted.push_back(vals[in.a]);
    else vals[i] = leaf(in, pl.is_ext[i]);
  }
  return asserted;
}
// the same through the compiled stream: operands are read from the lane's words, the result is written to its words
static std::vector<Val> replay_stream(const Prog& p, const AirPlan& pl, const AirCompiled& code) {
  std::vector<uint64_t> mem(pl.words(DC), 0xdeadbeef);
  std::vector<Val> asserted;
  auto rd = [&](uint32_t w, bool ext) {
    Val v{ext, {}};
    for (int k = 0; k < (ext ? DC : 1); ++k) {
      CHECK(w + k < mem.size(), "read of word %u of %zu", w + k, mem.size());
      v.w[k] = mem[w + k];
    }
    return v;
  };
  auto wr = [&](uint32_t w, const Val& v) {
    for (int k = 0; k < (v.ext ? DC : 1); ++k) {
      CHECK(w + k < mem.size(), "write of word %u of %zu", w + k, mem.size());
      mem[w + k] = v.w[k];
    }
  };
  CHECK(code.insns.size() == p.size(), "one device instruction per instruction");
  for (size_t i = 0; i < p.size(); ++i) {
    const AirDevInsn& d = code.insns[i];
    switch (d.op) {
      case AIR_D_ADD_BB: wr(d.dst, arith(P3R_AIR_ADD, rd(d.a, false), rd(d.b, false))); break;
      case AIR_D_ADD_EE: wr(d.dst, arith(P3R_AIR_ADD, rd(d.a, true), rd(d.b, true))); break;
      case AIR_D_ADD_EB: wr(d.dst, arith(P3R_AIR_ADD, rd(d.a, true), rd(d.b, false))); break;
      case AIR_D_SUB_BB: wr(d.dst, arith(P3R_AIR_SUB, rd(d.a, false), rd(d.b, false))); break;
      case AIR_D_SUB_EE: wr(d.dst, arith(P3R_AIR_SUB, rd(d.a, true), rd(d.b, true))); break;
      case AIR_D_SUB_EB: wr(d.dst, arith(P3R_AIR_SUB, rd(d.a, true), rd(d.b, false))); break;
      case AIR_D_SUB_BE: wr(d.dst, arith(P3R_AIR_SUB, rd(d.a, false), rd(d.b, true))); break;
      case AIR_D_MUL_BB: wr(d.dst, arith(P3R_AIR_MUL, rd(d.a, false), rd(d.b, false))); break;
      case AIR_D_MUL_EE: wr(d.dst, arith(P3R_AIR_MUL, rd(d.a, true), rd(d.b, true))); break;
      case AIR_D_MUL_EB: wr(d.dst, arith(P3R_AIR_MUL, rd(d.a, true), rd(d.b, false))); break;
      case AIR_D_NEG_B: wr(d.dst, arith(P3R_AIR_SUB, Val{false, {}}, rd(d.a, false))); break;
      case AIR_D_NEG_E: wr(d.dst, arith(P3R_AIR_SUB, Val{true, {}}, rd(d.a, true))); break;
      case AIR_D_ASSERT_B: asserted.push_back(rd(d.a, false)); break;
      case AIR_D_ASSERT_E: asserted.push_back(rd(d.a, true)); break;
      default: wr(d.dst, leaf(p[i], pl.is_ext[i])); break;
    }
  }
  return asserted;
}

static Prog random_program(std::mt19937& rng, int n_insns, int window) {
  Prog p;
  std::vector<uint32_t> values;   // ids that have a value
  auto pick = [&] {
    const size_t lo = values.size() > (size_t)window ? values.size() - window : 0;
    return values[lo + rng() % (values.size() - lo)];
  };
  while ((int)p.size() < n_insns) {
    const uint32_t r = rng() % 16, id = (uint32_t)p.size();
    if (values.size() < 2 || r < 3) {
      static const uint32_t leaves[] = {P3R_AIR_LOCAL, P3R_AIR_NEXT, P3R_AIR_LOCAL_EXT, P3R_AIR_NEXT_EXT, P3R_AIR_CHALLENGE,
                                        P3R_AIR_CONST, P3R_AIR_PUBLIC, P3R_AIR_IS_FIRST_ROW, P3R_AIR_IS_LAST_ROW, P3R_AIR_IS_TRANSITION};
      const uint32_t op = leaves[rng() % 10];
      const bool e = op == P3R_AIR_LOCAL_EXT || op == P3R_AIR_NEXT_EXT;
      if (op == P3R_AIR_CONST) p.push_back({op, (uint32_t)(rng() % P), 0});
      else if (op == P3R_AIR_PUBLIC || op == P3R_AIR_CHALLENGE) p.push_back({op, (uint32_t)(rng() % 2), 0});
      else p.push_back({op, 1, (uint32_t)(rng() % (e ? 5 : 8))});
      values.push_back(id);
    } else if (r < 12) {
      static const uint32_t ops[] = {P3R_AIR_ADD, P3R_AIR_SUB, P3R_AIR_MUL};
      p.push_back({ops[rng() % 3], pick(), pick()});
      values.push_back(id);
    } else if (r < 13) {
      p.push_back({P3R_AIR_NEG, pick(), 0});
      values.push_back(id);
    } else {
      p.push_back({P3R_AIR_ASSERT_ZERO, pick(), 0});
    }
  }
  p.push_back({P3R_AIR_ASSERT_ZERO, values.back(), 0});
  return p;
}

int main() {
  const Prog good = power_program(2);
  // ---- refusals of a program
  refused("operand_not_earlier", P3R_EINVAL, [] { plan_of({{P3R_AIR_LOCAL, 0, 0}, {P3R_AIR_ADD, 0, 1}, {P3R_AIR_ASSERT_ZERO, 1, 0}}); });
  refused("operand_later", P3R_EINVAL, [] { plan_of({{P3R_AIR_NEG, 5, 0}, {P3R_AIR_ASSERT_ZERO, 0, 0}}); });
  refused("operand_is_assert", P3R_EINVAL, [] { plan_of({{P3R_AIR_LOCAL, 0, 0}, {P3R_AIR_ASSERT_ZERO, 0, 0}, {P3R_AIR_ADD, 0, 1}, {P3R_AIR_ASSERT_ZERO, 2, 0}}); });
  refused("assert_of_assert", P3R_EINVAL, [] { plan_of({{P3R_AIR_LOCAL, 0, 0}, {P3R_AIR_ASSERT_ZERO, 0, 0}, {P3R_AIR_ASSERT_ZERO, 1, 0}}); });
  for (uint32_t op : {2u, 7u, 21u, 0xffffffffu})
    refused("unknown_op", P3R_EINVAL, [op] { plan_of({{op, 0, 0}, {P3R_AIR_ASSERT_ZERO, 0, 0}}); });
  refused("matrix_out_of_range", P3R_EINVAL, [] { plan_of({{P3R_AIR_LOCAL, 2, 0}, {P3R_AIR_ASSERT_ZERO, 0, 0}}); });
  refused("column_out_of_range", P3R_EINVAL, [] { plan_of({{P3R_AIR_NEXT, 0, 3}, {P3R_AIR_ASSERT_ZERO, 0, 0}}); });
  refused("ext_columns_out_of_range", P3R_EINVAL, [] { plan_of({{P3R_AIR_LOCAL_EXT, 1, 5}, {P3R_AIR_ASSERT_ZERO, 0, 0}}); });
  refused("ext_columns_narrow_matrix", P3R_EINVAL, [] { plan_of({{P3R_AIR_NEXT_EXT, 0, 0}, {P3R_AIR_ASSERT_ZERO, 0, 0}}); });
  refused("column_wraps", P3R_EINVAL, [] { plan_of({{P3R_AIR_LOCAL_EXT, 1, 0xffffffffu}, {P3R_AIR_ASSERT_ZERO, 0, 0}}); });
  refused("public_out_of_range", P3R_EINVAL, [] { plan_of({{P3R_AIR_PUBLIC, 2, 0}, {P3R_AIR_ASSERT_ZERO, 0, 0}}); });
  refused("challenge_out_of_range", P3R_EINVAL, [] { plan_of({{P3R_AIR_CHALLENGE, 2, 0}, {P3R_AIR_ASSERT_ZERO, 0, 0}}); });
  refused("non_canonical_constant", P3R_EINVAL, [] { plan_of({{P3R_AIR_CONST, P, 0}, {P3R_AIR_ASSERT_ZERO, 0, 0}}); });
  refused("no_assert", P3R_EINVAL, [] { plan_of({{P3R_AIR_LOCAL, 0, 0}, {P3R_AIR_NEG, 0, 0}}); });
  refused("empty", P3R_EINVAL, [] { air_plan(nullptr, 0, kWidths, 2, DC, P, 0, 0, P3R_AIR_MAX_LIVE); });
  // ... and of a domain
  refused("shift_h_is_one", P3R_EINVAL, [] { air_domain<KoalaBearParams>(1, 3, 0); });
  refused("shift_in_trace_domain", P3R_EINVAL, [] { air_domain<KoalaBearParams>(Fp<KoalaBearParams>::two_adic_generator(3).to_canonical(), 3, 0); });
  // shift^h = w_4: a root of x^h - 1 lies on chunk 3 of 4
  refused("shift_h_is_chunk_root", P3R_EINVAL, [] { air_domain<KoalaBearParams>(Fp<KoalaBearParams>::two_adic_generator(5).to_canonical(), 3, 2); });
  refused("non_canonical_shift", P3R_EINVAL, [] { air_domain<KoalaBearParams>(P, 3, 1); });
  refused("domain_above_two_adicity", P3R_EINVAL, [] { air_domain<KoalaBearParams>(0, 23, 2); });
  refused("log_quotient_degree_5", P3R_EUNSUPPORTED, [] { air_domain<KoalaBearParams>(0, 3, 5); });
  CHECK(code_of([&] { plan_of(good); air_domain<KoalaBearParams>(0, 3, 2); air_domain<BabyBearParams>(0, 0, 0); }) == 0, "a good program and domain");
  // the indices of an unknown count are left alone
  CHECK(code_of([] { plan_of({{P3R_AIR_PUBLIC, 99, 0}, {P3R_AIR_CHALLENGE, 99, 0}, {P3R_AIR_MUL, 0, 1}, {P3R_AIR_ASSERT_ZERO, 2, 0}}, kAirUnknownCount, kAirUnknownCount); }) == 0,
        "unknown counts");

  // ---- degrees
  for (int d : {1, 2, 3, 5, 9}) {
    const AirPlan pl = plan_of(power_program(d));
    CHECK((int)pl.info.max_degree == d && pl.info.n_constraints == 1, "x^%d: degree %u", d, pl.info.max_degree);
    printf("degree %d %u\n", d, pl.info.log_quotient_degree);
  }
  {
    // selectors and what counts nothing: is_first * (cell - public) is 2, is_transition * challenge * const * cell is 1,
    // the sum of a degree-3 and a degree-1 term is 3, and the largest constraint decides
    Prog p{{P3R_AIR_IS_FIRST_ROW, 0, 0}, {P3R_AIR_LOCAL, 0, 1}, {P3R_AIR_PUBLIC, 0, 0}, {P3R_AIR_SUB, 1, 2}, {P3R_AIR_MUL, 0, 3},
           {P3R_AIR_ASSERT_ZERO, 4, 0}};
    CHECK(plan_of(p).info.max_degree == 2 && plan_of(p).info.log_quotient_degree == 0, "boundary constraint");
    Prog t{{P3R_AIR_IS_TRANSITION, 0, 0}, {P3R_AIR_CHALLENGE, 1, 0}, {P3R_AIR_CONST, 7, 0}, {P3R_AIR_NEXT, 1, 2}, {P3R_AIR_MUL, 0, 1},
           {P3R_AIR_MUL, 4, 2}, {P3R_AIR_MUL, 5, 3}, {P3R_AIR_NEG, 6, 0}, {P3R_AIR_ASSERT_ZERO, 7, 0}};
    const AirPlan pt = plan_of(t);
    CHECK(pt.info.max_degree == 1 && pt.is_ext[7] && !pt.is_ext[3] && pt.uses_x && !pt.uses_inv, "transition constraint");
    Prog s = power_program(3);   // ids 0..2 values, 3 the assert
    s.push_back({P3R_AIR_LOCAL, 1, 0});
    s.push_back({P3R_AIR_ADD, 2, 4});
    s.push_back({P3R_AIR_ASSERT_ZERO, 5, 0});
    s.push_back({P3R_AIR_IS_LAST_ROW, 0, 0});
    s.push_back({P3R_AIR_ASSERT_ZERO, 7, 0});
    const AirPlan ps = plan_of(s);
    CHECK(ps.info.max_degree == 3 && ps.info.n_constraints == 3 && ps.info.log_quotient_degree == 1 && ps.uses_inv, "sum of degrees 3 and 1");
  }

  // ---- the limit, from both sides; the count is of values, whatever their kind
  {
    const AirPlan pl = plan_of(live_program(P3R_AIR_MAX_LIVE));
    CHECK(pl.info.peak_live == P3R_AIR_MAX_LIVE && pl.n_base_slots == P3R_AIR_MAX_LIVE && pl.n_ext_slots == 0, "peak %u", pl.info.peak_live);
    printf("live %u accepted\n", pl.info.peak_live);
    CHECK(code_of([] { plan_of(live_program(P3R_AIR_MAX_LIVE + 1)); }) == P3R_EUNSUPPORTED, "one more live value");
    CHECK(plan_of(live_program(P3R_AIR_MAX_LIVE + 1), 2, 2, P3R_AIR_MAX_LIVE + 1).info.peak_live == P3R_AIR_MAX_LIVE + 1, "peak of one more");
    printf("live %u refused\n", P3R_AIR_MAX_LIVE + 1);
    CHECK(kAirMaxLdsBytes <= 160 * 1024 && pl.lds_bytes(DC) == (size_t)P3R_AIR_MAX_LIVE * 256, "LDS of the slot file");
  }

  // ---- the slot assignment and the compiled stream against a replay value by value
  std::mt19937 rng(2024);
  const uint32_t publics[2] = {5, P - 1}, challenges[2 * DC] = {1, 2, 3, 4, P - 1, 0, 1, P - 2};
  size_t n_programs = 0, n_constraints = 0;
  for (int round = 0; round < 400; ++round) {
    const int window = 2 + (int)(rng() % 30);
    const Prog p = random_program(rng, 20 + (int)(rng() % 400), window);
    AirPlan pl;
    if (code_of([&] { pl = plan_of(p); }) != 0) continue;   // more than P3R_AIR_MAX_LIVE values alive
    const AirCompiled code = air_compile<KoalaBearParams>(pl, p.data(), p.size(), kWidths, 2, DC, publics, challenges);
    // no two values alive at once share a slot of their kind
    std::vector<int> owner[2];
    owner[0].assign(pl.n_base_slots, -1);
    owner[1].assign(pl.n_ext_slots, -1);
    for (size_t i = 0; i < p.size(); ++i) {
      for (auto& o : owner)
        for (int& v : o)
          if (v >= 0 && pl.last_use[v] <= i) v = -1;   // dies at i: released before the result is placed
      if (p[i].op == P3R_AIR_ASSERT_ZERO) continue;
      std::vector<int>& o = owner[pl.is_ext[i]];
      CHECK(pl.slot[i] < o.size(), "value %zu: slot %u of %zu", i, pl.slot[i], o.size());
      CHECK(o[pl.slot[i]] < 0, "value %zu placed on live value %d", i, o[pl.slot[i]]);
      if (pl.last_use[i] > i) o[pl.slot[i]] = (int)i;
    }
    const std::vector<Val> want = replay_values(p, pl), got = replay_stream(p, pl, code);
    CHECK(want.size() == got.size() && want.size() == pl.info.n_constraints, "constraint count");
    for (size_t k = 0; k < want.size(); ++k)
      for (int c = 0; c < DC; ++c)
        CHECK(want[k].ext == got[k].ext && want[k].w[c] == got[k].w[c], "round %d: constraint %zu word %d differs through the slots", round, k, c);
    ++n_programs;
    n_constraints += want.size();
  }
  CHECK(n_programs >= 100, "only %zu random programs fit the limit", n_programs);
  printf("replay %zu %zu\n", n_programs, n_constraints);
  return 0;
}
