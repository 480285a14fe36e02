// C++ caller of the public PCS seams through include/p3r.hpp, from a trace to the final polynomial of FRI: uploads the
// traces of a case file, extends and commits them (Dft::coset_lde_batch + p3r_mmcs_commit_dmat = Pcs::commit), opens
// them at the file's points (CosetInterpolation::open_points), forms the reduced openings with the file's alpha
// (CosetInterpolation::reduced_openings), folds the tallest vector down with the file's schedule and challenges
// (TwoAdicFriFolding::fold_matrix, rolling each lower height in where the schedule lands on it), and turns the last
// vector into coefficients on the host (p3r_dft).  The challenges come from the file because the challenger is the
// caller's; with opened values that belong to the traces every coefficient from 2^log_final on is zero.
//
//   fri_seam <koala-bear|baby-bear> <challenge degree> <case file>
//
// case file (whitespace separated unsigned integers): log_blowup shift n_mats, then per matrix height width n_points,
// height*width row-major words (evaluations over the subgroup, natural order), n_points*DC point words; then DC words
// of alpha; then n_phases and per phase log_arity and DC words of beta.  Output: the commitment cap, then one line per
// coefficient of the final polynomial (DC words each), then "ok".
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
    uint32_t log_blowup, shift;
    size_t n_mats;
    if (!(in >> log_blowup >> shift >> n_mats)) throw std::runtime_error("bad case file");
    std::vector<p3r_dmat*> traces;
    p3r::CosetInterpolation::Points points;
    for (size_t i = 0; i < n_mats; ++i) {
      size_t h, w, k;
      if (!(in >> h >> w >> k)) throw std::runtime_error("bad matrix header");
      std::vector<uint32_t> m(h * w), pts(k * dc);
      for (auto& v : m) in >> v;
      for (auto& v : pts) in >> v;
      if (!in) throw std::runtime_error("short case file");
      traces.push_back(ctx.ptr(p3r_dmat_upload(ctx.raw(), m.data(), h, w)));
      points.push_back(std::move(pts));
    }
    std::vector<uint32_t> alpha(dc);
    for (auto& v : alpha) in >> v;
    size_t n_phases;
    if (!(in >> n_phases)) throw std::runtime_error("no folding schedule");
    std::vector<uint32_t> log_arities(n_phases);
    std::vector<std::vector<uint32_t>> betas(n_phases, std::vector<uint32_t>(dc));
    for (size_t i = 0; i < n_phases; ++i) {
      in >> log_arities[i];
      for (auto& v : betas[i]) in >> v;
    }
    if (!in) throw std::runtime_error("short folding schedule");

    // Pcs::commit
    const p3r::CosetInterpolation::Mats trace_mats(traces.begin(), traces.end());
    const std::vector<p3r_dmat*> ldes = p3r::Dft(ctx).coset_lde_batch(trace_mats, log_blowup, shift);
    const p3r::CosetInterpolation::Mats lde_mats(ldes.begin(), ldes.end());
    std::vector<uint32_t> cap(8u << ctx.fri().cap_height);
    p3r_tree* tree = nullptr;
    ctx.check(p3r_mmcs_commit_dmat(ctx.raw(), lde_mats.data(), lde_mats.size(), cap.data(), &tree));
    for (uint32_t x : cap) std::cout << x << ' ';
    std::cout << '\n';
    // Pcs::open, without the challenger: values, reduced openings, folds
    const p3r::CosetInterpolation pcs(ctx);
    const auto values = pcs.open_points(lde_mats, points, log_blowup, shift);
    std::vector<p3r_dmat*> ros = pcs.reduced_openings(lde_mats, points, values, alpha, shift);
    if (ros.empty()) throw std::runtime_error("no matrix has an opening point");
    const p3r::TwoAdicFriFolding folding(ctx);
    p3r_dmat* cur = ros[0];
    size_t next = 1;
    for (size_t i = 0; i < n_phases; ++i) {
      const size_t rows = p3r_dmat_height(cur) >> log_arities[i];
      const p3r_dmat* roll = next < ros.size() && p3r_dmat_height(ros[next]) == rows ? ros[next] : nullptr;
      p3r_dmat* folded = folding.fold_matrix(cur, log_arities[i], betas[i], roll);
      p3r_dmat_free(ctx.raw(), cur);
      if (roll) p3r_dmat_free(ctx.raw(), ros[next++]);
      cur = folded;
    }
    if (next != ros.size()) throw std::runtime_error("the schedule never lands on an input height");
    // the final polynomial: a host-sized inverse DFT over the subgroup, evaluations in bit-reversed order
    const size_t m = p3r_dmat_height(cur);
    std::vector<uint32_t> evals(m * dc), coeffs(m * dc);
    ctx.check(p3r_dmat_download(ctx.raw(), cur, evals.data()));
    ctx.check(p3r_dft(ctx.raw(), evals.data(), m, dc, P3R_DFT_INVERSE, 1, P3R_DFT_BITREV, coeffs.data()));
    for (size_t r = 0; r < m; ++r) {
      for (uint32_t k = 0; k < dc; ++k) std::cout << coeffs[r * dc + k] << ' ';
      std::cout << '\n';
    }
    p3r_dmat_free(ctx.raw(), cur);
    p3r_tree_free(ctx.raw(), tree);
    for (p3r_dmat* d : ldes) p3r_dmat_free(ctx.raw(), d);
    for (p3r_dmat* d : traces) p3r_dmat_free(ctx.raw(), d);
    std::cout << "ok" << std::endl;
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
