// C++ caller of the value half of Pcs::open through include/p3r.hpp: reads matrices and points from a text file,
// uploads the matrices, opens them all in one p3r::CosetInterpolation::open_points call and prints the values.
//
//   open_points <koala-bear|baby-bear> <challenge degree> <case file>
//
// case file (whitespace separated unsigned integers): added_bits shift bit_reversed n_mats, then per matrix
// height width n_points, height*width row-major words, n_points*DC point words.  Output: one line per matrix with
// its [point][column][DC] words, then "ok".
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

#include "p3r.hpp"

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
    uint32_t added_bits, shift, bit_reversed;
    size_t n_mats;
    if (!(in >> added_bits >> shift >> bit_reversed >> n_mats)) throw std::runtime_error("bad case file");
    std::vector<p3r_dmat*> owned;
    p3r::CosetInterpolation::Mats mats;
    p3r::CosetInterpolation::Points points;
    for (size_t i = 0; i < n_mats; ++i) {
      size_t h, w, k;
      if (!(in >> h >> w >> k)) throw std::runtime_error("bad matrix header");
      std::vector<uint32_t> m(h * w), pts(k * dc);
      for (auto& v : m) in >> v;
      for (auto& v : pts) in >> v;
      if (!in) throw std::runtime_error("short case file");
      owned.push_back(ctx.ptr(p3r_dmat_upload(ctx.raw(), m.data(), h, w)));
      mats.push_back(owned.back());
      points.push_back(std::move(pts));
    }
    const auto values = p3r::CosetInterpolation(ctx).open_points(mats, points, added_bits, shift, bit_reversed != 0);
    for (const auto& v : values) {
      for (uint32_t x : v) std::cout << x << ' ';
      std::cout << '\n';
    }
    for (p3r_dmat* m : owned) p3r_dmat_free(ctx.raw(), m);
    std::cout << "ok" << std::endl;
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
