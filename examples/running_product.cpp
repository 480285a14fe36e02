// C++ caller of p3r::affine_scan through include/p3r.hpp: a grand-product check that two columns are permutations of each
// other, with every derived column built on the device.
//
// Two columns of 64 rows are uploaded: x[r] = 1021 r + 7 mod 2^16 and y[r] = x[(5 r + 3) mod 64], a permutation of x.
// Under a fixed challenge gamma of the challenge field a witness program derives the factor f = (gamma - x) / (gamma - y),
// p3r::affine_scan the running product z[0] = 1, z[r + 1] = z[r] f[r], and hands back z[h] - which is one exactly when the
// multisets agree (up to the choice of gamma).  p3r::check_constraints confirms on the trace domain
//
//   f (gamma - y) = gamma - x,   is_first_row (z - 1),   is_transition (z' - f z),   is_last_row (f z - T)
//
// with T = z[h].  Then one cell of y is changed: z[h] is no longer one.  Nothing but x and y is computed on the host.
//
//   running_product <koala-bear|baby-bear> <challenge degree>
//
// Output: "columns <f and z width> rows <h>", "total one", "spoiled total not one", then "ok".
// Exits non-zero if a step does not find what it should.
#include <cstdio>
#include <cstring>
#include <iostream>

#include "p3r.hpp"

static bool is_one(const std::vector<uint32_t>& last) {
  bool one = last[0] == 1;
  for (size_t k = 1; k < 5; ++k) one = one && last[k] == 0;
  return one;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s <koala-bear|baby-bear> <challenge degree>\n", argv[0]);
    return 2;
  }
  try {
    const p3r::Field field = std::strcmp(argv[1], "koala-bear") == 0 ? p3r::Field::KoalaBear : p3r::Field::BabyBear;
    const uint32_t dc = (uint32_t)std::stoul(argv[2]);
    p3r::Context ctx(field, p3r::FriParams{}, 0, {}, 4, 0, dc);

    const size_t h = 64;
    std::vector<uint32_t> x(h), xy(h * 2), gamma(dc);
    for (size_t r = 0; r < h; ++r) x[r] = (uint32_t)((1021 * r + 7) % 65536);
    for (size_t r = 0; r < h; ++r) xy[2 * r] = x[r], xy[2 * r + 1] = x[(5 * r + 3) % h];
    for (uint32_t k = 0; k < dc; ++k) gamma[k] = 1000003u * (k + 1);

    // f = (gamma - x) / (gamma - y), an extension value in columns 0 .. DC
    p3r::AirProgram factor;
    {
      const auto g = factor.challenge(0);
      factor.store((g - factor.local(0, 0)) * factor.inv(g - factor.local(0, 1)), 0);
    }
    // the four constraints; matrix 0 = (x, y), matrix 1 = f, matrix 2 = z; challenge 0 = gamma, challenge 1 = T
    p3r::AirProgram air;
    {
      const auto g = air.challenge(0), total = air.challenge(1);
      const auto f = air.local_ext(1, 0), z = air.local_ext(2, 0), z_next = air.next_ext(2, 0);
      air.assert_zero(f * (g - air.local(0, 1)) - (g - air.local(0, 0)));
      air.assert_zero(air.is_first_row() * (z - air.constant(1)));
      air.assert_zero(air.is_transition() * (z_next - f * z));
      air.assert_zero(air.is_last_row() * (f * z - total));
    }

    bool reported = false;
    for (int spoiled = 0; spoiled < 2; ++spoiled) {
      if (spoiled) xy[2 * 21 + 1] += 1;   // one cell of y: no longer a permutation of x
      p3r_dmat* d_xy = ctx.ptr(p3r_dmat_upload(ctx.raw(), xy.data(), h, 2));
      p3r_dmat* d_f = p3r::witness_columns(ctx, factor, {d_xy}, 0, {}, gamma);
      const p3r::AffineScan scan = p3r::affine_scan(ctx, {p3r::Recurrence::product(0, 0, 0).ext()}, {d_f}, true);
      if (!reported) std::cout << "columns " << p3r_dmat_width(d_f) + p3r_dmat_width(scan.columns) << " rows " << p3r_dmat_height(scan.columns) << '\n';
      reported = true;
      std::vector<uint32_t> challenges = gamma;
      challenges.insert(challenges.end(), scan.last.begin(), scan.last.begin() + dc);
      const p3r::ConstraintCheck cc = p3r::check_constraints(ctx, air, {d_xy, d_f, scan.columns}, {}, challenges);
      p3r_dmat_free(ctx.raw(), scan.columns);
      p3r_dmat_free(ctx.raw(), d_f);
      p3r_dmat_free(ctx.raw(), d_xy);
      // the recurrence holds for any x and y: it is the total that tells
      if (!cc.satisfied()) throw std::runtime_error("the running product does not satisfy its constraints");
      if (is_one(scan.last) == (spoiled != 0)) throw std::runtime_error(spoiled ? "the total is one for columns that are no permutations" : "the total of two permuted columns is not one");
      std::cout << (spoiled ? "spoiled total not one" : "total one") << '\n';
    }
    std::cout << "ok" << std::endl;
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
