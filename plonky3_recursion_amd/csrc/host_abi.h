// The host-only entry points of the C ABI (include/p3r.h): `verify_batch` behind verify_all_tables, the proof parsers
// and `Mmcs::verify_batch` - no device, no p3r_ctx.  A parent node of an aggregation tree runs them on bytes that
// arrived from another rank (plonky3_recursion_amd/aggregation.py), so they are also compiled, without the device
// code, under AddressSanitizer + UBSan and driven by a structure-aware mutator (tests/san/).  Included once per
// library: by p3r_core.hip in the product, by tests/san/san_host.hip in the sanitizer build.
#pragma once
#include <algorithm>
#include <chrono>

#include "verify_impl.h"
#include "fri_verify_abi.h"

using namespace p3r;

namespace {

struct ProofFlags {
  bool canonical, zk, salted, quintic;
  p3r::ProofLayout PL;
  ProofFlags(uint32_t flags, const uint8_t* proof_layout)
      : canonical((flags & P3R_PROVE_CANONICAL_FIELD_ENCODING) != 0), zk((flags & P3R_PROOF_ZK) != 0), salted((flags & P3R_PROOF_SALTED) != 0),
        quintic((flags & P3R_PROOF_QUINTIC_CHALLENGE) != 0) {
    if (!PL.set(proof_layout, 18)) refuse(P3R_EINVAL, "proof_layout must be three permutations batch[5] | fri[5] | opened[8]");
  }
};

}  // namespace

extern "C" {

int p3r_mmcs_verify(const p3r_config* cfg, const uint32_t* cap, size_t n_mats, const size_t* heights, const size_t* widths,
                    size_t index, const uint32_t* opened_values, const uint32_t* proof, size_t proof_len, char* err_buf,
                    size_t err_cap) {
  return guarded(err_buf, err_cap, [&] {
    if (!cfg || !cap || !heights || !widths || !opened_values || (!proof && proof_len) || !n_mats) refuse(P3R_EINVAL, "NULL argument");
    if (cfg->abi_version != P3R_ABI_VERSION) refuse(P3R_EINVAL, "ABI version mismatch");
    check_mmcs_config(*cfg, false);
    // the cap is read before the tree is walked: bound it by the tallest matrix first (a shift by >= 64 is undefined, a
    // large one an allocation of that many digests and a read past `cap`)
    size_t hmax = 0;
    for (size_t m = 0; m < n_mats; ++m) {
      if (!heights[m] || (heights[m] & (heights[m] - 1))) refuse(P3R_EINVAL, "matrix heights must be powers of two");
      check_width(widths[m]);
      hmax = std::max(hmax, heights[m]);
    }
    if (cfg->cap_height >= 48 || (size_t(1) << cfg->cap_height) > hmax) refuse(P3R_EINVAL, "cap_height exceeds the height of the tallest matrix");
    if (proof_len > 64 * 3) refuse(P3R_EINVAL, "opening proof longer than any tree's");
    for_field(cfg->field, [&](auto tag) {
      using PP = decltype(tag);
      using F = p3r::Fp<PP>;
      using Digest = std::array<F, P2_DIGEST>;
      const std::vector<uint32_t> rc = p3r::montgomery_constants<PP>(host_constants_table<PP>(*cfg));
      auto fe = [](uint32_t v) {
        if (v >= PP::P) p3r::vfail("non-canonical field element");
        return F::from_canonical(v);
      };
      std::vector<Digest> capd(size_t(1) << cfg->cap_height), path(proof_len);
      const uint32_t* cp = cap;
      for (auto& d : capd) for (auto& x : d) x = fe(*cp++);
      const uint32_t* pf = proof;
      for (auto& d : path) for (auto& x : d) x = fe(*pf++);
      std::vector<int> lhs;
      std::vector<std::vector<F>> rows;
      const uint32_t* ov = opened_values;
      for (size_t m = 0; m < n_mats; ++m) {
        lhs.push_back(p3r::log2_exact(heights[m], "matrix height"));
        std::vector<F> r(widths[m]);
        for (auto& x : r) x = fe(*ov++);
        rows.push_back(std::move(r));
      }
      // the rows arrive with their salts appended (p3r_mmcs_verify_salted)
      p3r::MmcsChecker<PP>{cfg->mmcs_arity == 4 ? 4 : 2, 0, rc.data()}.check_opening(capd, (int)cfg->cap_height, lhs, rows, {}, index, path, "opening");
    });
    return P3R_OK;
  });
}

// ---- native verifier (verify_impl.h): host code, no device needed ----
// MerkleTreeHidingMmcs::verify_batch: the leaf preimage of a height class is the concatenation of [row | salt] per matrix
// (recursion/src/pcs/mmcs.rs:375-389), i.e. the plain walk over the matrices widened by cfg->mmcs_salt_elems columns.
int p3r_mmcs_verify_salted(const p3r_config* cfg, const uint32_t* cap, size_t n_mats, const size_t* heights, const size_t* widths,
                           size_t index, const uint32_t* opened_values, const uint32_t* salts, const uint32_t* proof,
                           size_t proof_len, char* err_buf, size_t err_cap) {
  std::vector<size_t> wide;
  std::vector<uint32_t> rows;
  const int rc = guarded(err_buf, err_cap, [&] {
    if (!cfg || !widths || !opened_values || !n_mats || (cfg->mmcs_salt_elems && !salts)) refuse(P3R_EINVAL, "NULL argument");
    check_salt_elems(*cfg);
    const size_t S = cfg->mmcs_salt_elems;
    wide.assign(widths, widths + n_mats);
    const uint32_t* ov = opened_values;
    for (size_t m = 0; m < n_mats; ++m) {
      check_width(widths[m]);
      rows.insert(rows.end(), ov, ov + widths[m]);
      ov += widths[m];
      if (S) rows.insert(rows.end(), salts + m * S, salts + (m + 1) * S);
      wide[m] += S;
    }
    return P3R_OK;
  });
  if (rc != P3R_OK) return rc;
  return p3r_mmcs_verify(cfg, cap, n_mats, heights, wide.data(), index, rows.data(), proof, proof_len, err_buf, err_cap);
}

int p3r_verify_batch(const p3r_config* cfg, const p3r_air_desc* airs, size_t n_airs,
                     const uint32_t* preprocessed_commitment, const uint32_t* degree_bits, const uint8_t* proof,
                     size_t proof_len, uint32_t flags, char* err_buf, size_t err_cap) {
  return guarded(err_buf, err_cap, [&] {
    if (!cfg || !airs || !preprocessed_commitment || !degree_bits || (!proof && proof_len)) refuse(P3R_EINVAL, "NULL argument");
    if (cfg->abi_version != P3R_ABI_VERSION) refuse(P3R_EINVAL, "ABI version mismatch");
    if (cfg->challenge_degree != 0 && cfg->challenge_degree != 4 && cfg->challenge_degree != 5) refuse(P3R_EUNSUPPORTED, "UnsupportedChallengeDegree");
    const bool generic_d = p3r::ext_degree_is_binomial_generic(cfg->ext_degree);
    if (generic_d && cfg->ext_w == 0) refuse(P3R_EINVAL, "MissingWForExtension");
    if (!generic_d && cfg->ext_degree != 1 && cfg->ext_degree != 4 && !(cfg->ext_degree == 5 && cfg->field == P3R_FIELD_KOALA_BEAR)) refuse(P3R_EUNSUPPORTED, "UnsupportedDegree");
    p3r::VerifyParams prm{(int)cfg->log_blowup, (int)cfg->max_log_arity, (int)cfg->cap_height, (int)cfg->log_final_poly_len,
                          (int)cfg->commit_pow_bits, (int)cfg->query_pow_bits, (int)cfg->num_queries, {}};
    if (cfg->fri_log_arities) prm.fri_log_arities.assign(cfg->fri_log_arities, cfg->fri_log_arities + cfg->fri_log_arities_len);
    bool w32_airs = false;
    for (size_t i = 0; i < n_airs; ++i) w32_airs = w32_airs || airs[i].kind == P3R_AIR_POSEIDON2_W32;
    check_mmcs_config(*cfg, w32_airs);
    prm.mmcs_arity = cfg->mmcs_arity == 4 ? 4 : 2;
    if (cfg->zk > 1 || cfg->num_random_codewords > 8) refuse(P3R_EINVAL, "zk must be 0 or 1, num_random_codewords at most 8");
    check_salt_elems(*cfg);
    prm.mmcs_salt_elems = (int)cfg->mmcs_salt_elems;
    prm.zk = (int)cfg->zk;
    prm.num_random_codewords = cfg->zk ? (cfg->num_random_codewords ? (int)cfg->num_random_codewords : 2) : 0;
    if (!prm.layout.set(cfg->proof_layout, cfg->proof_layout_len)) refuse(P3R_EINVAL, "proof_layout must be 18 bytes: three permutations");
    std::vector<p3r::AirParams> a(n_airs);
    for (size_t i = 0; i < n_airs; ++i) {
      if (airs[i].kind > P3R_AIR_POSEIDON2_W32 || !airs[i].lanes) refuse(P3R_EINVAL, "bad AIR descriptor");
      a[i] = {(int)airs[i].kind, (int)airs[i].lanes, (int)airs[i].horner_packed_steps, (int)airs[i].coeff_lookups,
              (cfg->ext_choices & P3R_EXT_LOOKUP_UNPACKED) ? 1 : 0, (int)cfg->ext_degree, 0u};
    }
    const bool canonical = (flags & P3R_PROVE_CANONICAL_FIELD_ENCODING) != 0;
    std::vector<uint32_t> cap(preprocessed_commitment, preprocessed_commitment + ((size_t)P2_DIGEST << cfg->cap_height));
    const std::vector<uint32_t> want_db(degree_bits, degree_bits + n_airs);
    for_field(cfg->field, [&](auto tag) {
      using PP = decltype(tag);
      const std::vector<uint32_t> table = host_constants_table<PP>(*cfg);
      for (auto& x : a) x.ext_w_mont = generic_d ? p3r::Fp<PP>::from_canonical(cfg->ext_w).v : 0u;
      if (cfg->challenge_degree == 5) {
        if constexpr (p3r::kHasQuintic<PP>)
          p3r::verify_batch<PP, 5>(prm, table, a, cap, want_db, proof, proof_len, canonical);
        else
          p3r::vfail("UnsupportedChallengeDegree: the quintic challenge field is KoalaBear's");
      } else {
        p3r::verify_batch<PP>(prm, table, a, cap, want_db, proof, proof_len, canonical);
      }
    });
    return P3R_OK;
  });
}

int p3r_batch_proof_len(uint32_t field, const uint8_t* bytes, size_t len, uint32_t flags, size_t* proof_len,
                        char* err_buf, size_t err_cap) {
  return p3r_batch_proof_len_layout(field, bytes, len, flags, nullptr, proof_len, err_buf, err_cap);
}
int p3r_batch_proof_len_layout(uint32_t field, const uint8_t* bytes, size_t len, uint32_t flags,
                               const uint8_t* proof_layout, size_t* proof_len, char* err_buf, size_t err_cap) {
  return guarded(err_buf, err_cap, [&] {
    if (!bytes || !proof_len) refuse(P3R_EINVAL, "NULL argument");
    const ProofFlags f(flags, proof_layout);
    for_field(field, [&](auto tag) {
      using PP = decltype(tag);
      p3r::ProofChecker<PP> R(bytes, len, f.quintic && p3r::kHasQuintic<PP> ? 5 : 4);   // the quintic challenge field is KoalaBear's
      *proof_len = p3r::walk_batch_proof(R, f.PL, f.zk, f.salted, true);
    });
    return P3R_OK;
  });
}

int p3r_batch_stark_proof_parse(uint32_t field, const uint8_t* bytes, size_t len, uint32_t flags,
                                const uint8_t* proof_layout, p3r_batch_stark_meta* out, char* err_buf,
                                size_t err_cap) {
  return guarded(err_buf, err_cap, [&] {
    if (!bytes || !out) refuse(P3R_EINVAL, "NULL argument");
    const auto t0 = std::chrono::steady_clock::now();
    const ProofFlags f(flags, proof_layout);
    for_field(field, [&](auto tag) {
      p3r::parse_batch_stark_meta<decltype(tag)>(bytes, len, f.canonical, f.PL, f.quintic ? 5 : 4, out, f.zk, f.salted);
    });
    out->parse_ns = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
    return P3R_OK;
  });
}

}  // extern "C"
