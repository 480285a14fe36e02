// Functions that cross the translation units of libp3r_hip.so.  The library is several units so that they build
// side by side (one unit took ten minutes): p3r_core.hip (C ABI, the Merkle tree module mmcs_impl.hip.h, prover
// sequencing, circuit boundary),
// tu_lde.hip (K5: NTT tables, passes and the coset LDE), tu_quotient.hip / tu_logup.hip (the two kernels with the
// AIR constraint systems inlined, one instance per circuit degree and challenge degree), tu_open.hip (K9 at the public
// opening seam: it includes open_impl.hip.h, as p3r_core.hip does, for the planner OpenPlan and instantiates the K9
// kernels of kernels_open.hip.h with the seam's entry point), tu_fri.hip (the reduced openings and the fold at the public
// FRI seam and the commit-phase leaf view: kernels_fri_points.hip.h, and its own instances of k_fri_inv_points, k_fri_vsum
// and k_fri_fold), tu_air.hip (the constraint-program and lookup-program seams: the interpreters k_quotient_program and
// k_trace_program of kernels_air.hip.h over the plan and instruction stream of air_program.h),
// prep_device.hip.
// Kernels never call across units; only these host entry points do.
#pragma once
#include <memory>
#include <vector>

#include "context.h"
#include "kernels_stark.hip.h"

namespace p3r {

inline std::unique_ptr<p3r_dmat> dmat_alloc(size_t h, size_t w) {
  log2_exact(h, "matrix height");
  auto m = std::make_unique<p3r_dmat>();
  m->buf.alloc(h * w);
  m->d = m->buf.p;
  m->h = h;
  m->w = w;
  return m;
}

// Device copy of a small read-only table (see p3r_ctx::const_tables).
inline const void* const_table(p3r_ctx* ctx, const void* data, size_t bytes) {
  std::string key(static_cast<const char*>(data), bytes);
  auto it = ctx->const_tables.find(key);
  if (it == ctx->const_tables.end()) {
    DevBuf b((bytes + 3) / 4);
    P3R_HIP(ctx->stage.upload(ctx->stream, b.p, data, bytes));
    it = ctx->const_tables.emplace(std::move(key), std::move(b)).first;
  }
  return it->second.p;
}
inline const uint32_t* const* col_table(p3r_ctx* ctx, const std::vector<const uint32_t*>& cols) {
  return static_cast<const uint32_t* const*>(const_table(ctx, cols.data(), cols.size() * sizeof(void*)));
}

// The context's challenge degree as a compile-time constant: fn(std::integral_constant<int, 4>) or <int, 5>, the quintic
// degree refused over BabyBear.  What the entries of the public seams open with.
template <class PP, class Fn>
inline decltype(auto) with_challenge_degree(const p3r_ctx* ctx, Fn&& fn) {
  if (ctx->cfg.challenge_degree == 5) {
    if constexpr (kHasQuintic<PP>) return fn(std::integral_constant<int, 5>{});
    else fail(P3R_EUNSUPPORTED, "UnsupportedChallengeDegree: the quintic challenge field is KoalaBear's");
  }
  return fn(std::integral_constant<int, 4>{});
}

// K5 for a batch of matrices (tu_lde.hip).  in: h x w evaluations over the subgroup (natural order, column-major
// Montgomery).  Returns (h << added_bits) x w, rows in bit-reversed order over shift * <w_{h << added_bits}>.
struct LdeItem {
  const p3r_dmat* in;
  uint32_t shift;  // canonical coset shift
};
template <class PP>
std::vector<std::unique_ptr<p3r_dmat>> coset_lde_batch(p3r_ctx* ctx, const std::vector<LdeItem>& items, int added_bits);
// The halves of the LDE on their own (tu_lde.hip): TwoAdicSubgroupDft::dft_batch / idft_batch (shift 1) and
// coset_dft_batch / coset_idft_batch.  Every column of an h x w matrix is a polynomial of degree < h; the coefficient
// side is in natural order, `bit_reversed` says whether evaluation row i is the point shift * w_h^bitrev(i) or
// shift * w_h^i - the output of a forward call, the input of an inverse one.  Inputs are read only.
// dft_check: what both refuse, before anything is allocated or launched.
template <class PP>
inline void dft_check(size_t h, size_t w, uint32_t shift) {
  const int log_n = log2_exact(h, "DFT height");
  if (log_n > PP::TWO_ADICITY) fail(P3R_EINVAL, "DFT of 2^%d rows exceeds the field's two-adicity (%d)", log_n, PP::TWO_ADICITY);
  if (w == 0) fail(P3R_EINVAL, "matrix width must be positive");
  if (shift == 0 || shift >= PP::P) fail(P3R_EINVAL, "coset shift must be a non-zero canonical element");
}
template <class PP>
std::vector<std::unique_ptr<p3r_dmat>> dft_batch(p3r_ctx* ctx, const std::vector<LdeItem>& items, bool inverse, bool bit_reversed);
// once per context: kernel attributes of the unit's kernels
template <class PP>
void lde_init(p3r_ctx* ctx);

// The value half of TwoAdicFriPcs::open (tu_open.hip): every column of each matrix at its points, over the context's
// challenge field.  `d`: h x w, column-major Montgomery (null when w == 0).  The evaluations of the interpolant are rows
// 0 .. h >> added_bits (bit_reversed: the low coset of a bit-reversed LDE) or rows k << added_bits (natural order), over
// shift * <w_{h >> added_bits}> in that order; shift 0 = the field's generator.  Points p0 .. p1 of `points` (canonical,
// DC words each) belong to the matrix, and p0 of a matrix is p1 of the one before.  values_out (host): [matrix][point]
// [column][DC], canonical.  Everything that is refused is refused before anything is allocated or launched.
struct OpenPointsItem {
  const uint32_t* d;
  size_t h, w;
  size_t p0, p1;
};
template <class PP>
void open_points(p3r_ctx* ctx, const std::vector<OpenPointsItem>& items, int added_bits, uint32_t shift, bool bit_reversed,
                 const uint32_t* points, uint32_t* values_out);

// The reduced openings of Pcs::open and FriFoldingStrategy::fold_matrix with the roll-in (tu_fri.hip), over the context's
// challenge field (DC words).  fri_reduce: `d` is a whole committed LDE, h x w, bit-reversed rows over shift * <w_h>
// (null when w == 0; shift 0 = the field's generator); points p0 .. p1 of `points` belong to the matrix; `values` (host,
// canonical) is [matrix][point][column][DC], what open_points wrote.  Returns one h x DC matrix per distinct height that
// has a point, tallest first.  fri_fold: `in` n x DC over <w_n> in bit-reversed order -> (n >> log_arity) x DC.
// Everything that is refused is refused before anything is allocated or launched; both only enqueue.
struct FriReduceItem {
  const uint32_t* d;
  size_t h, w;
  size_t p0, p1;
};
template <class PP>
std::vector<std::unique_ptr<p3r_dmat>> fri_reduce(p3r_ctx* ctx, const std::vector<FriReduceItem>& items, uint32_t shift,
                                                  const uint32_t* points, const uint32_t* values, const uint32_t* alpha);
template <class PP>
std::unique_ptr<p3r_dmat> fri_fold(p3r_ctx* ctx, const p3r_dmat* in, uint32_t log_arity, const uint32_t* beta, const p3r_dmat* roll_in);
// The commit-phase leaf matrix of a folded vector (tu_fri.hip): `vec` n x DC -> (n >> log_arity) x (DC << log_arity), row r
// = the flattened elements r << log_arity .. (r + 1) << log_arity.  Refuses what fri_fold refuses; only enqueues.
template <class PP>
std::unique_ptr<p3r_dmat> fri_leaf_view(p3r_ctx* ctx, const p3r_dmat* vec, uint32_t log_arity);

// quotient_values + split_evals for a caller's AIR (tu_air.hip): the p3r_air_insn program `prog` evaluated on the quotient
// domain of 2^log_quotient_degree cosets of the trace domain, read from the first rows of the bit-reversed LDEs `mats` (one
// height, blow-up 2^added_bits, over shift * <w>; shift 0 = the field's generator).  publics / challenges / alpha: canonical
// host words.  Returns the 2^log_quotient_degree chunks, each h x DC in natural order.  Everything that is refused is
// refused before anything is allocated or launched (include/p3r.h lists it); only enqueues.
template <class PP>
std::vector<std::unique_ptr<p3r_dmat>> quotient_program(p3r_ctx* ctx, const p3r_air_insn* prog, size_t n_insns,
                                                        const std::vector<const p3r_dmat*>& mats, uint32_t added_bits, uint32_t shift,
                                                        uint32_t log_quotient_degree, const uint32_t* publics, size_t n_public,
                                                        const uint32_t* challenges, size_t n_challenges, const uint32_t* alpha);

// The LogUp gadget for a caller's lookups (tu_air.hip): the lookup program `prog` (p3r_air_insn with P3R_AIR_LOOKUP /
// P3R_AIR_LOOKUP_END as sinks) evaluated on every row of the traces `mats` (one height h, natural order).  Returns the
// h x DC * (1 + G) auxiliary trace - the running sum, then one fraction column per closed column - and writes the table's
// sum to sum_out (host, canonical).  Everything that is refused is refused before anything is allocated or launched, but
// a zero denominator, which is found on the device: P3R_EINVAL, nothing returned.  Waits for the stream.
template <class PP>
std::unique_ptr<p3r_dmat> logup_program(p3r_ctx* ctx, const p3r_air_insn* prog, size_t n_insns, const std::vector<const p3r_dmat*>& mats,
                                        const uint32_t* publics, size_t n_public, const uint32_t* challenges, size_t n_challenges,
                                        uint32_t* sum_out);

// check_air_satisfies for a caller's AIR (tu_air.hip): the constraint program `prog` on every row of the TRACES `mats`
// (one height h, natural order) with 0 / 1 selectors.  first_row_out / n_failed_out (host, n_constraints each, may be
// null): the smallest row in which constraint k does not vanish (0xffffffff: none) and the number of such rows; the
// report is derived from them.  A failing trace is a result.  Refuses before anything is allocated or launched; waits
// for the stream.
template <class PP>
void check_program(p3r_ctx* ctx, const p3r_air_insn* prog, size_t n_insns, const std::vector<const p3r_dmat*>& mats, const uint32_t* publics,
                   size_t n_public, const uint32_t* challenges, size_t n_challenges, p3r_check_report* report, uint32_t* first_row_out,
                   uint64_t* n_failed_out);

// check_lookups for a caller's lookup programs (tu_air.hip): the terms of every instance with a non-zero multiplicity are
// records keyed by their denominator; a key whose multiplicities do not sum to zero is unbalanced.  Writes their number
// and the min(cap, number) of them whose first records come earliest.  Refuses before anything is allocated or launched;
// waits for the stream.
struct LookupCheckInstance {
  const p3r_air_insn* prog;
  size_t n_insns;
  std::vector<const p3r_dmat*> mats;
  const uint32_t* publics;
  size_t n_public;
};
template <class PP>
void lookup_check(p3r_ctx* ctx, const std::vector<LookupCheckInstance>& insts, const uint32_t* challenges, size_t n_challenges,
                  p3r_lookup_imbalance* out, size_t cap, uint64_t* n_unbalanced_out);
// The multiplicity column of a table (tu_air.hip): insts[0] is the table, the others its queries.  Returns the fresh
// h_T x n_terms_T matrix in which the first table slot that offers a key holds the sum of the query multiplicities of that
// key, every other cell 0; writes the number of keys that are asked for (net non-zero) and offered by no table slot, and
// the min(cap, number) of them whose first records come earliest.  Refuses before anything is allocated or launched;
// waits for the stream.
template <class PP>
std::unique_ptr<p3r_dmat> lookup_multiplicities(p3r_ctx* ctx, const std::vector<LookupCheckInstance>& insts, const uint32_t* challenges,
                                                size_t n_challenges, p3r_lookup_imbalance* missing, size_t cap, uint64_t* n_missing_out);

// Derived columns of a caller's trace (tu_air.hip): the witness program `prog` (p3r_air_insn with P3R_AIR_STORE as its sink
// and INV / BITS / ROW among its value ops) evaluated on every row of the traces `mats` (one height h, natural order; none:
// `height` rows).  Returns the fresh h x W matrix of the stored columns.  Everything that is refused is refused before
// anything is allocated or launched (include/p3r.h lists it); only enqueues.
template <class PP>
std::unique_ptr<p3r_dmat> witness_program(p3r_ctx* ctx, const p3r_air_insn* prog, size_t n_insns, const std::vector<const p3r_dmat*>& mats,
                                          size_t height, const uint32_t* publics, size_t n_public, const uint32_t* challenges,
                                          size_t n_challenges);

// Accumulator columns of a caller's trace (tu_air.hip): the recurrences `recs` (s[r + 1] = a[r] s[r] + b[r], a and b columns
// of the traces `mats`: one height h, natural order) as the columns of a fresh h x W matrix.  `last_out` (host, n_recs x 5,
// may be NULL): s[h] of each, canonical; with it the call waits for the stream, without it it only enqueues.  Everything
// that is refused is refused before anything is allocated or launched (include/p3r.h lists it; scan_plan.h decides it).
template <class PP>
std::unique_ptr<p3r_dmat> affine_scan(p3r_ctx* ctx, const p3r_recurrence* recs, size_t n_recs, const std::vector<const p3r_dmat*>& mats,
                                      uint32_t* last_out);

// K7 / K8 launches (tu_logup.hip, tu_quotient.hip): the instance of the context's circuit degree
template <class PP, int DC>
void launch_logup_aux(p3r_ctx* ctx, unsigned blocks, const LogupJob* d_jobs, int n_jobs, const LookupChT<DC>& lc);
template <class PP, int DC>
void launch_quotient(p3r_ctx* ctx, unsigned blocks, const QuotientArgs* d_jobs, int n_jobs, const LookupChT<DC>& lc);

// K6 of the arity-4 MMCS (tu_mmcs4.hip; kernels_mmcs4.hip.h), launched by the tree module (mmcs_impl.hip.h).
// classes[c] = the matrices of one height, digs[c] =
// [8][allocs[c]] with allocs[c] >= that height.
template <class PP>
void mmcs4_hash_rows(p3r_ctx* ctx, const std::vector<std::vector<const p3r_dmat*>>& classes, const std::vector<uint32_t*>& digs,
                     const std::vector<size_t>& allocs);
template <class PP>
void mmcs4_hash_rows_strided(p3r_ctx* ctx, const uint32_t* const* dcols, int wtot, size_t rows, size_t stride, uint32_t* dig,
                             size_t alloc);
template <class PP>
void mmcs4_compress(p3r_ctx* ctx, const uint32_t* prev, size_t n_prev, int step, const uint32_t* inj, uint32_t* out,
                    size_t n_logical, size_t n_out);

}  // namespace p3r
