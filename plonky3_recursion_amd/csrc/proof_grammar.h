// The postcard grammar of a serialised BatchProof, stated once: the reader's side of proof_layout.h (the writer is
// prove_impl.hip.h's ProofWriter).  One cursor, one walk, two sinks:
//   PostcardCursor    bytes, option tags, varints and bounded lengths, with the refusals' texts
//   walk_batch_proof  everything that is grammar: the field order of a ProofLayout, every length bound, the option tags,
//                     the ZK prefix of the FRI proof, the (salts, siblings) tuples of a hiding MMCS, the trailing-bytes rule
//   ProofBuilder      sink that fills a ParsedProof (verify_batch)
//   ProofChecker      sink that builds nothing and allocates nothing: the framing is sound and every field element is in
//                     range - what a parent node of the aggregation tree needs before it hands a child to its verifier
//                     circuit (p3r_batch_proof_len[_layout], p3r_batch_stark_proof_parse)
// The walk names a place in the proof by an accessor (P3R_AT) that only the building sink ever calls.
#pragma once
#include <array>
#include <cstdarg>
#include <optional>
#include <stdexcept>
#include <vector>

#include "host_transcript.h"

namespace p3r {

// ---- postcard reader (mirror of ProofWriter)
struct PostcardCursor {
  const uint8_t* p;
  const uint8_t* end;
  uint8_t byte() {
    if (p >= end) vfail("proof truncated");
    return *p++;
  }
  bool flag() {  // Option / bool tag: postcard admits 0 and 1 only
    const uint8_t b = byte();
    if (b > 1) vfail("invalid option tag %u", b);
    return b != 0;
  }
  uint64_t varint() {
    uint64_t v = 0;
    for (int shift = 0; shift < 64; shift += 7) {
      uint8_t b = byte();
      if (shift == 63 && b > 1) vfail("varint overflows 64 bits");  // postcard: the tenth byte carries one bit
      v |= (uint64_t)(b & 0x7F) << shift;
      if (!(b & 0x80)) {
        if (b == 0 && shift > 0) vfail("non-canonical varint");
        return v;
      }
    }
    vfail("malformed varint");
  }
  size_t len(size_t max) {
    uint64_t v = varint();
    if (v > max) vfail("length %llu exceeds the bound %zu", (unsigned long long)v, max);
    return (size_t)v;
  }
};

template <class PP, int DC = 4>
struct ParsedProof {
  using F = Fp<PP>;
  using E = typename Chal<PP, DC>::type;
  using Digest = std::array<F, P2_DIGEST>;
  using Cap = std::vector<Digest>;
  Cap main_cap, quot_cap;
  std::optional<Cap> perm_cap, rand_cap;
  struct Inst {
    std::vector<E> main_local, prep_local, prep_next, perm_local, perm_next;
    std::optional<std::vector<E>> main_next, random;
    std::vector<std::vector<E>> chunks;
  };
  // HidingFriPcs::Proof = (OpenedValues<Challenge>, FriProof): rounds -> matrices -> points -> random codeword values
  std::vector<std::vector<std::vector<std::vector<E>>>> fri_random;
  std::vector<Inst> insts;
  std::vector<Cap> commit_caps;
  std::vector<F> commit_pow;
  // `salts`: MerkleTreeHidingMmcs - the opening proof is the tuple (per-matrix salts, sibling digests)
  // (SaltedMmcsProof, recursion/src/pcs/mmcs.rs:763-768); empty under the plain MMCS
  struct QRound { std::vector<std::vector<F>> rows; std::vector<Digest> path; std::vector<std::vector<F>> salts; };
  struct QPhase { int la; std::vector<E> sibs; std::vector<Digest> path; std::vector<std::vector<F>> salts; };
  struct Query { std::vector<QRound> rounds; std::vector<QPhase> phases; };
  std::vector<Query> queries;
  std::vector<E> final_poly;
  F query_pow;
  std::vector<std::optional<E>> terminals;
  std::vector<int> degree_bits;
};

// ---- the building sink.  A sink is a cursor plus what becomes of a count (`resize`), a plain value (`set`) and runs of
// field elements (`fe`, `ef`, `fes`, `efs`, `digests`) at the place `at` names.
template <class PP, int DC = 4>
struct ProofBuilder : PostcardCursor {
  using F = Fp<PP>;
  using E = typename Chal<PP, DC>::type;
  bool canonical;
  ParsedProof<PP, DC> P;
  ProofBuilder(const uint8_t* bytes, size_t n, bool canonical_) : PostcardCursor{bytes, bytes + n}, canonical(canonical_) {}
  F read_fe() {
    uint64_t v = varint();
    if (v >= PP::P) vfail("field element out of range");
    return canonical ? F::from_canonical((uint32_t)v) : F::raw((uint32_t)v);
  }
  E read_ef() { E e; for (int i = 0; i < DC; ++i) e.c[i] = read_fe(); return e; }
  template <class At> void resize(size_t n, At at) { at(P).resize(n); }
  template <class V, class At> void set(V v, At at) { at(P) = v; }
  template <class At> void fe(At at) { at(P) = read_fe(); }
  template <class At> void ef(At at) { at(P) = read_ef(); }
  template <class At> void fes(size_t k, At at) { auto& v = at(P); v.resize(k); for (auto& x : v) x = read_fe(); }
  template <class At> void efs(size_t k, At at) { auto& v = at(P); v.resize(k); for (auto& e : v) e = read_ef(); }
  template <class At> void digests(size_t k, At at) { auto& v = at(P); v.resize(k); for (auto& d : v) for (auto& x : d) x = read_fe(); }
};

// ---- the checking sink: no containers are built.  Runs of field elements take the five-byte fast path (a Montgomery
// word is >= 2^28 fifteen times out of sixteen): one 8-byte load, one bit-extract, one compare.
template <class PP>
struct ProofChecker : PostcardCursor {
  int dc = 4;   // words per extension element (the challenge degree)
  ProofChecker(const uint8_t* bytes, size_t n, int dc_) : PostcardCursor{bytes, bytes + n}, dc(dc_) {}
  void fes_scalar(size_t k) {
    for (size_t i = 0; i < k; ++i)
      if (varint() >= PP::P) vfail("field element out of range");
  }
#if defined(P3R_HOST_AVX512)
  __attribute__((target("bmi2"))) void fes_bmi2(size_t k) {
    const uint8_t* q = p;
    size_t i = 0;
    constexpr uint64_t M = 0x8080808080ull, T = 0x0080808080ull, X = 0x7F7F7F7F7Full;
    while (i < k) {
      // four at a time while all four are five-byte words (their positions are then known up front)
      while (i + 4 <= k && q + 23 <= end) {
        uint64_t x0, x1, x2, x3;
        std::memcpy(&x0, q, 8); std::memcpy(&x1, q + 5, 8); std::memcpy(&x2, q + 10, 8); std::memcpy(&x3, q + 15, 8);
        const bool five = ((x0 & M) == T) & ((x1 & M) == T) & ((x2 & M) == T) & ((x3 & M) == T) &
                          (((x0 >> 32) & 0x7F) != 0) & (((x1 >> 32) & 0x7F) != 0) & (((x2 >> 32) & 0x7F) != 0) &
                          (((x3 >> 32) & 0x7F) != 0);
        if (!five) break;
        if ((_pext_u64(x0, X) >= PP::P) | (_pext_u64(x1, X) >= PP::P) | (_pext_u64(x2, X) >= PP::P) |
            (_pext_u64(x3, X) >= PP::P))
          vfail("field element out of range");
        q += 20;
        i += 4;
      }
      // a shorter word among the next four (one word in sixteen is below 2^28): one at a time, then retry
      for (int j = 0; j < 4 && i < k; ++j, ++i) {
        uint64_t x = 0;
        if (q + 8 <= end) std::memcpy(&x, q, 8);
        if ((x & M) == T && ((x >> 32) & 0x7F)) {  // five bytes, canonical
          if (_pext_u64(x, X) >= PP::P) vfail("field element out of range");
          q += 5;
        } else {
          p = q;
          if (varint() >= PP::P) vfail("field element out of range");
          q = p;
        }
      }
    }
    p = q;
  }
#endif
  void run(size_t k) {
#if defined(P3R_HOST_AVX512)
    static const bool bmi2 = __builtin_cpu_supports("bmi2") && !(getenv("P3R_HOST_SIMD") && getenv("P3R_HOST_SIMD")[0] == '0');
    if (bmi2) return fes_bmi2(k);
#endif
    fes_scalar(k);
  }
  template <class At> void resize(size_t, At) {}
  template <class V, class At> void set(V, At) {}
  template <class At> void fe(At) { run(1); }
  template <class At> void ef(At) { run((size_t)dc); }
  template <class At> void fes(size_t k, At) { run(k); }
  template <class At> void efs(size_t k, At) { run((size_t)dc * k); }
  template <class At> void digests(size_t k, At) { run(P2_DIGEST * k); }
};

// ---- the walk.  `PL`: field order (p3r_config.proof_layout).  `zk`: the proof type is the hiding PCS's - a property of
// the configuration (SC::Pcs in the reference), not of the bytes.  `salted`: the MMCSs are hiding ones
// (p3r_config.mmcs_salt_elems > 0): every opening proof carries its salts first.  `trailing_ok`: bytes may follow (the
// outer BatchStarkProof appends its metadata, batch_stark_prover.rs:610-636).  Returns the length of the BatchProof.
#define P3R_AT(place) [&](auto& proof) -> auto& { return proof.place; }
template <class Sink>
size_t walk_batch_proof(Sink& s, const ProofLayout& PL, bool zk, bool salted, bool trailing_ok) {
  const uint8_t* const begin = s.p;
  auto cap = [&](auto at) { s.digests(s.len(1u << 16), at); };
  auto efs = [&](auto at, size_t max = 1u << 16) { s.efs(s.len(max), at); };
  auto count = [&](size_t max, auto at) { const size_t n = s.len(max); s.resize(n, at); return n; };
  auto mmcs_proof = [&](size_t max_mats, auto salts, auto path) {
    if (salted) {
      const size_t ns = count(max_mats, salts);
      for (size_t k = 0; k < ns; ++k) s.fes(s.len(64), [&](auto& proof) -> auto& { return salts(proof)[k]; });
    }
    s.digests(s.len(64), path);
  };
  auto commitments = [&] {
    cap(P3R_AT(main_cap));
    if (s.flag()) cap(P3R_AT(perm_cap.emplace()));
    cap(P3R_AT(quot_cap));
    if (s.flag()) cap(P3R_AT(rand_cap.emplace()));
  };
  auto opened_values = [&] {
    const size_t ni = count(64, P3R_AT(insts));
    for (size_t i = 0; i < ni; ++i)
      for (int f = 0; f < 8; ++f) {
        switch (PL.opened[f]) {
          case 0: efs(P3R_AT(insts[i].main_local)); break;
          case 1: if (s.flag()) efs(P3R_AT(insts[i].main_next.emplace())); break;
          case 2: if (!s.flag()) vfail("preprocessed_local missing"); efs(P3R_AT(insts[i].prep_local)); break;
          case 3: if (!s.flag()) vfail("preprocessed_next missing"); efs(P3R_AT(insts[i].prep_next)); break;
          case 4: {
            const size_t nc = count(8, P3R_AT(insts[i].chunks));
            for (size_t c = 0; c < nc; ++c) efs(P3R_AT(insts[i].chunks[c]));
            break;
          }
          case 5: if (s.flag()) efs(P3R_AT(insts[i].random.emplace())); break;
          case 6: efs(P3R_AT(insts[i].perm_local)); break;
          default: efs(P3R_AT(insts[i].perm_next)); break;
        }
      }
  };
  auto query_proofs = [&] {
    const size_t nq = count(1024, P3R_AT(queries));
    for (size_t q = 0; q < nq; ++q) {
      const size_t nr = count(8, P3R_AT(queries[q].rounds));
      for (size_t r = 0; r < nr; ++r) {
        const size_t rows = count(256, P3R_AT(queries[q].rounds[r].rows));
        for (size_t k = 0; k < rows; ++k) s.fes(s.len(1u << 16), P3R_AT(queries[q].rounds[r].rows[k]));
        mmcs_proof(256, P3R_AT(queries[q].rounds[r].salts), P3R_AT(queries[q].rounds[r].path));
      }
      const size_t nph = count(64, P3R_AT(queries[q].phases));
      for (size_t k = 0; k < nph; ++k) {
        s.set((int)s.byte(), P3R_AT(queries[q].phases[k].la));
        efs(P3R_AT(queries[q].phases[k].sibs), 16);
        mmcs_proof(4, P3R_AT(queries[q].phases[k].salts), P3R_AT(queries[q].phases[k].path));
      }
    }
  };
  auto fri_proof = [&] {
    if (zk) {
      const size_t nr = count(8, P3R_AT(fri_random));
      for (size_t r = 0; r < nr; ++r) {
        const size_t nm = count(256, P3R_AT(fri_random[r]));
        for (size_t m = 0; m < nm; ++m) {
          const size_t np = count(2, P3R_AT(fri_random[r][m]));
          for (size_t k = 0; k < np; ++k) efs(P3R_AT(fri_random[r][m][k]), 16);
        }
      }
    }
    for (int f = 0; f < 5; ++f) {
      switch (PL.fri[f]) {
        case 0: {
          const size_t nc = count(64, P3R_AT(commit_caps));
          for (size_t c = 0; c < nc; ++c) cap(P3R_AT(commit_caps[c]));
          break;
        }
        case 1: s.fes(s.len(64), P3R_AT(commit_pow)); break;
        case 2: query_proofs(); break;
        case 3: efs(P3R_AT(final_poly)); break;
        default: s.fe(P3R_AT(query_pow)); break;
      }
    }
  };
  for (int f = 0; f < 5; ++f) {
    switch (PL.batch[f]) {
      case 0: commitments(); break;
      case 1: opened_values(); break;
      case 2: fri_proof(); break;
      case 3: {
        const size_t nt = count(64, P3R_AT(terminals));
        for (size_t t = 0; t < nt; ++t)
          if (s.flag()) s.ef(P3R_AT(terminals[t]));
        break;
      }
      default: {
        const size_t nd = count(64, P3R_AT(degree_bits));
        for (size_t d = 0; d < nd; ++d) s.set((int)s.len(40), P3R_AT(degree_bits[d]));
        break;
      }
    }
  }
  if (!trailing_ok && s.p != s.end) vfail("%zu trailing bytes after the proof", (size_t)(s.end - s.p));
  return (size_t)(s.p - begin);
}
#undef P3R_AT

}  // namespace p3r
