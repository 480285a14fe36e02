// C++ caller of the constraint-program seam through include/p3r.hpp: a three-column "Fibonacci with a cube" AIR written
// against p3r::AirProgram as an Air::eval is written against an AirBuilder, evaluated over the quotient domain of the
// trace's committed LDE by p3r::quotient_values (quotient_values + split_evals of p3_uni_stark::prove).  No trace leaves
// the device between the upload and the chunks.
//
//   row (a, b, c):  c = a^3 + b;  next.a = b, next.b = c on transitions;  first.a = public 0;  last.c = public 1
//
// The transition constraint c - (a^3 + b) has degree 3: log_quotient_degree 1, two chunks.
//
//   quotient_program <koala-bear|baby-bear> <challenge degree> <case file>
//
// case file (whitespace separated unsigned integers): log_blowup shift height, height * 3 row-major trace words
// (evaluations over the subgroup, natural order), 2 public values, DC words of alpha.  Output: "info" with the
// program's constraint count, largest degree, log_quotient_degree and peak of live values, then per chunk one line per
// row (DC words each), then "ok".
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

#include "p3r.hpp"

static p3r::AirProgram fibonacci_with_cube() {
  p3r::AirProgram air;
  const auto a = air.local(0, 0), b = air.local(0, 1), c = air.local(0, 2);
  air.assert_zero(c - (a * a * a + b));
  const auto t = air.is_transition();
  air.assert_zero(t * (air.next(0, 0) - b));
  air.assert_zero(t * (air.next(0, 1) - c));
  air.assert_zero(air.is_first_row() * (a - air.public_value(0)));
  air.assert_zero(air.is_last_row() * (c - air.public_value(1)));
  return air;
}

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: %s <koala-bear|baby-bear> <challenge degree> <case file>\n", argv[0]);
    return 2;
  }
  try {
    const p3r::Field field = std::strcmp(argv[1], "koala-bear") == 0 ? p3r::Field::KoalaBear : p3r::Field::BabyBear;
    const uint32_t dc = (uint32_t)std::stoul(argv[2]);
    p3r::Context ctx(field, p3r::FriParams{}, 0, {}, 4, 0, dc);
    std::ifstream in(argv[3]);
    uint32_t log_blowup, shift;
    size_t h;
    if (!(in >> log_blowup >> shift >> h)) throw std::runtime_error("bad case file");
    std::vector<uint32_t> trace(h * 3), publics(2), alpha(dc);
    for (auto& v : trace) in >> v;
    for (auto& v : publics) in >> v;
    for (auto& v : alpha) in >> v;
    if (!in) throw std::runtime_error("short case file");

    const p3r::AirProgram air = fibonacci_with_cube();
    const p3r_air_info info = air.info(ctx, {3});
    std::cout << "info " << info.n_constraints << ' ' << info.max_degree << ' ' << info.log_quotient_degree << ' ' << info.peak_live << '\n';
    p3r_dmat* t = ctx.ptr(p3r_dmat_upload(ctx.raw(), trace.data(), h, 3));
    const std::vector<p3r_dmat*> ldes = p3r::Dft(ctx).coset_lde_batch({t}, log_blowup, shift);   // Pcs::commit's LDE
    const std::vector<p3r_dmat*> chunks =
        p3r::quotient_values(ctx, air, {ldes[0]}, log_blowup, info.log_quotient_degree, alpha, publics, {}, shift);
    std::vector<uint32_t> rows(h * dc);
    for (p3r_dmat* chunk : chunks) {
      ctx.check(p3r_dmat_download(ctx.raw(), chunk, rows.data()));
      for (size_t r = 0; r < h; ++r) {
        for (uint32_t k = 0; k < dc; ++k) std::cout << rows[r * dc + k] << ' ';
        std::cout << '\n';
      }
      p3r_dmat_free(ctx.raw(), chunk);
    }
    p3r_dmat_free(ctx.raw(), ldes[0]);
    p3r_dmat_free(ctx.raw(), t);
    std::cout << "ok" << std::endl;
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
