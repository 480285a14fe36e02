// C++ caller of both sides of the FRI seam through include/p3r.hpp: proves as examples/prove_fri.cpp does (LDE, commit,
// open_points, reduced openings, p3r::prove_fri with the library's challenger on the device), then verifies on the host
// with p3r::HostChallenger - made from the configuration alone - and p3r::verify_fri: the transcript replayed for the
// query indices, the reduced openings read at those indices, every query checked.  Then one word of the proof is flipped
// and the refusal is shown.
//
//   verify_fri <koala-bear|baby-bear> <challenge degree> <case file>
//
// The case file is examples/prove_fri.cpp's.  Output: "indices" and the verifier's query indices, "accepted", then
// "refused <code>: <message>" for the flipped proof, then "ok".
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

    // ---- the prover, on the device
    const p3r::CosetInterpolation::Mats trace_mats(traces.begin(), traces.end());
    const std::vector<p3r_dmat*> ldes = p3r::Dft(ctx).coset_lde_batch(trace_mats, fri.log_blowup, shift);
    const p3r::CosetInterpolation::Mats lde_mats(ldes.begin(), ldes.end());
    std::vector<uint32_t> cap(8u << fri.cap_height);
    p3r_tree* tree = nullptr;
    ctx.check(p3r_mmcs_commit_dmat(ctx.raw(), lde_mats.data(), lde_mats.size(), cap.data(), &tree));
    p3r::DuplexChallenger challenger(ctx);
    challenger.observe(cap);
    const p3r::CosetInterpolation pcs(ctx);
    const auto values = pcs.open_points(lde_mats, points, fri.log_blowup, shift);
    for (const auto& v : values) challenger.observe(v);
    const std::vector<uint32_t> alpha = challenger.sample_ext();
    const std::vector<p3r_dmat*> ros = pcs.reduced_openings(lde_mats, points, values, alpha, shift);
    if (ros.empty()) throw std::runtime_error("no matrix has an opening point");
    const p3r::FriProof proof = p3r::prove_fri(ctx, challenger, std::vector<const p3r_dmat*>(ros.begin(), ros.end()));
    // the reduced openings as the verifier will want them: here read back whole, a verifier forms them at its indices
    std::vector<std::vector<uint32_t>> ro_host;
    std::vector<uint32_t> ro_log;
    for (p3r_dmat* d : ros) {
      const size_t h = p3r_dmat_height(d);
      ro_host.emplace_back(h * dc);
      ctx.check(p3r_dmat_download(ctx.raw(), d, ro_host.back().data()));
      uint32_t l = 0;
      while ((size_t(1) << l) < h) ++l;
      ro_log.push_back(l);
    }

    // ---- the verifier, on the host: nothing below touches the context
    const p3r_config cfg = ctx.config();
    auto verify = [&](const p3r::FriProof& pf) {
      p3r::HostChallenger v(cfg);
      v.observe(cap);
      for (const auto& x : values) v.observe(x);
      if (v.sample_ext() != alpha) throw std::runtime_error("the verifier's alpha is not the prover's");
      p3r::HostChallenger probe(v);
      const p3r::FriTranscript t = p3r::verify_fri_transcript(cfg, probe, pf);
      std::vector<p3r::FriInput> inputs;
      for (size_t i = 0; i < ro_host.size(); ++i) {
        p3r::FriInput fi{ro_log[i], {}};
        for (uint32_t index : t.indices) {
          const size_t row = index >> (pf.log_max_height - ro_log[i]);
          fi.values.insert(fi.values.end(), ro_host[i].begin() + row * dc, ro_host[i].begin() + (row + 1) * dc);
        }
        inputs.push_back(std::move(fi));
      }
      p3r::verify_fri(cfg, v, pf, inputs);
      if (v.sample() != probe.sample()) throw std::runtime_error("the two entries leave the challenger in different places");
      return t.indices;
    };
    const std::vector<uint32_t> indices = verify(proof);
    std::cout << "indices";
    for (uint32_t i : indices) std::cout << ' ' << i;
    std::cout << "\naccepted\n";
    p3r::FriProof flipped = proof;
    flipped.query_openings.at(0).at(0).siblings.at(0) ^= 1u;
    try {
      verify(flipped);
      throw std::runtime_error("the flipped proof was accepted");
    } catch (const p3r::Error& e) {
      std::cout << "refused " << e.code << ": " << e.what() << '\n';
    }
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
