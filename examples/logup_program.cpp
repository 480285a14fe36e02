// C++ caller of the lookup-program seam through include/p3r.hpp: two small tables on one bus.  The sender holds one tuple
// (t0, t1) per row and sends it with multiplicity 1; the receiver holds a permutation of the same tuples and receives each
// with multiplicity -1.  Both interactions are lookup programs written against p3r::AirProgram with the reference's bus
// form as the denominator, bus_prefix + t0 + beta * t1 (challenges [bus_prefix, beta]); p3r::logup_trace builds each
// table's permutation trace on the device and returns its sum.  The two sums cancel exactly when the receiver holds the
// sender's multiset: the program exits non-zero unless they do.
//
//   logup_program <koala-bear|baby-bear> <challenge degree> <case file>
//
// case file (whitespace separated unsigned integers): height, height * 2 row-major words of the sender's trace, height * 2
// of the receiver's, 2 * DC words of the challenges [bus_prefix, beta].  Output: "info" with the sender program's term
// count, column count, largest column-constraint degree and peak of live values; "sum" lines with the DC words of the
// sender's and the receiver's table sums; per table one line per row of its permutation trace (2 * DC words); then "ok".
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

#include "p3r.hpp"

// multiplicity: +1 for the sender; the receiver's -1 is the field's P - 1, which the program builds as 0 - 1
static p3r::AirProgram bus_interaction(bool receive) {
  p3r::AirProgram air;
  const auto denominator = air.challenge(0) + air.local(0, 0) + air.challenge(1) * air.local(0, 1);
  const auto one = air.constant(1);
  air.lookup(receive ? air.constant(0) - one : one, denominator);
  air.end_lookup_column();
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
    size_t h;
    if (!(in >> h)) throw std::runtime_error("bad case file");
    std::vector<uint32_t> traces[2] = {std::vector<uint32_t>(h * 2), std::vector<uint32_t>(h * 2)}, challenges(2 * dc);
    for (auto& t : traces)
      for (auto& v : t) in >> v;
    for (auto& v : challenges) in >> v;
    if (!in) throw std::runtime_error("short case file");

    const p3r_lookup_info info = bus_interaction(false).lookup_info(ctx, {2});
    std::cout << "info " << info.n_terms << ' ' << info.n_columns << ' ' << info.max_constraint_degree << ' ' << info.peak_live << '\n';
    p3r::LogupTrace aux[2];
    for (int t = 0; t < 2; ++t) {
      p3r_dmat* trace = ctx.ptr(p3r_dmat_upload(ctx.raw(), traces[t].data(), h, 2));
      aux[t] = p3r::logup_trace(ctx, bus_interaction(t == 1), {trace}, {}, challenges);
      p3r_dmat_free(ctx.raw(), trace);
      std::cout << "sum";
      for (uint32_t v : aux[t].sum) std::cout << ' ' << v;
      std::cout << '\n';
    }
    std::vector<uint32_t> rows(h * 2 * dc);
    for (int t = 0; t < 2; ++t) {
      ctx.check(p3r_dmat_download(ctx.raw(), aux[t].trace, rows.data()));
      for (size_t r = 0; r < h; ++r) {
        for (uint32_t k = 0; k < 2 * dc; ++k) std::cout << rows[r * 2 * dc + k] << ' ';
        std::cout << '\n';
      }
      p3r_dmat_free(ctx.raw(), aux[t].trace);
    }
    // the sums are canonical words: they cancel when each pair of coefficients adds to 0 or to the modulus
    const uint32_t p = field == p3r::Field::KoalaBear ? 0x7f000001u : 0x78000001u;
    for (uint32_t k = 0; k < dc; ++k)
      if ((aux[0].sum[k] + (uint64_t)aux[1].sum[k]) % p != 0) {
        std::fprintf(stderr, "the bus does not balance: coefficient %u of the two table sums does not cancel\n", k);
        return 1;
      }
    std::cout << "ok" << std::endl;
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
