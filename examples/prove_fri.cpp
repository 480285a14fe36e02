// C++ caller of the whole PCS opening through include/p3r.hpp, with nothing of the PCS on the caller's side: uploads the
// traces of a case file, extends and commits them (Dft::coset_lde_batch + p3r_mmcs_commit_dmat = Pcs::commit), observes
// the commitment, opens the traces at the file's points (CosetInterpolation::open_points), observes the opened values,
// samples alpha, forms the reduced openings (CosetInterpolation::reduced_openings) and runs p3r::prove_fri on them with
// the same p3r::DuplexChallenger: commit phases, proofs of work, final polynomial, query indices and openings.
//
//   prove_fri <koala-bear|baby-bear> <challenge degree> <case file>
//
// case file (whitespace separated unsigned integers): log_blowup max_log_arity log_final_poly_len commit_pow_bits
// query_pow_bits num_queries shift n_mats, then per matrix height width n_points, height*width row-major words
// (evaluations over the subgroup, natural order) and n_points*DC point words.  Matrices of different heights give FRI
// inputs of different heights, which are rolled in.  Output, one line each, as canonical words: the commitment cap,
// alpha, "caps" and one line per commit phase, "pow" and the commit-phase witnesses, "arities", "final" and one line per
// coefficient, "query_pow", "indices", per query and phase the opened leaf row, then "ok".
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

#include "p3r.hpp"

static void line(const char* tag, const std::vector<uint32_t>& v) {
  std::cout << tag;
  for (uint32_t x : v) std::cout << ' ' << x;
  std::cout << '\n';
}

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: %s <koala-bear|baby-bear> <challenge degree> <case file>\n", argv[0]);
    return 2;
  }
  try {
    const p3r::Field field = std::strcmp(argv[1], "koala-bear") == 0 ? p3r::Field::KoalaBear : p3r::Field::BabyBear;
    const uint32_t dc = (uint32_t)std::stoul(argv[2]);
    std::ifstream in(argv[3]);
    p3r::FriParams fri;
    uint32_t shift;
    size_t n_mats;
    if (!(in >> fri.log_blowup >> fri.max_log_arity >> fri.log_final_poly_len >> fri.commit_pow_bits >> fri.query_pow_bits >>
          fri.num_queries >> shift >> n_mats))
      throw std::runtime_error("bad case file");
    p3r::Context ctx(field, fri, 0, {}, 4, 0, dc);
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

    // Pcs::commit
    const p3r::CosetInterpolation::Mats trace_mats(traces.begin(), traces.end());
    const std::vector<p3r_dmat*> ldes = p3r::Dft(ctx).coset_lde_batch(trace_mats, fri.log_blowup, shift);
    const p3r::CosetInterpolation::Mats lde_mats(ldes.begin(), ldes.end());
    std::vector<uint32_t> cap(8u << fri.cap_height);
    p3r_tree* tree = nullptr;
    ctx.check(p3r_mmcs_commit_dmat(ctx.raw(), lde_mats.data(), lde_mats.size(), cap.data(), &tree));
    line("commit", cap);
    // Pcs::open: the transcript is the library's challenger from here on
    p3r::DuplexChallenger challenger(ctx);
    challenger.observe(cap);
    const p3r::CosetInterpolation pcs(ctx);
    const auto values = pcs.open_points(lde_mats, points, fri.log_blowup, shift);
    for (const auto& v : values) challenger.observe(v);
    const std::vector<uint32_t> alpha = challenger.sample_ext();
    line("alpha", alpha);
    const std::vector<p3r_dmat*> ros = pcs.reduced_openings(lde_mats, points, values, alpha, shift);
    if (ros.empty()) throw std::runtime_error("no matrix has an opening point");
    const p3r::FriProof proof = p3r::prove_fri(ctx, challenger, std::vector<const p3r_dmat*>(ros.begin(), ros.end()));

    std::cout << "caps " << proof.commit_phase_caps.size() << '\n';
    for (const auto& c : proof.commit_phase_caps) line("cap", c);
    line("pow", proof.commit_pow_witnesses);
    line("arities", proof.log_arities);
    std::cout << "final " << proof.final_poly.size() / dc << '\n';
    for (size_t i = 0; i < proof.final_poly.size(); i += dc)
      line("coeff", std::vector<uint32_t>(proof.final_poly.begin() + i, proof.final_poly.begin() + i + dc));
    line("query_pow", {proof.query_pow_witness});
    line("indices", std::vector<uint32_t>(proof.query_indices.begin(), proof.query_indices.end()));
    for (const auto& q : proof.query_openings)
      for (const auto& o : q) line("row", o.row);
    for (p3r_dmat* d : ros) p3r_dmat_free(ctx.raw(), d);
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
