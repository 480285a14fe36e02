/* p3r.h - C ABI of the MI355X-native batch-STARK prover for the p3-recursion
 * `prove_next_layer` hot path.
 *
 * The reference (Plonky3/Plonky3-recursion) is pure Rust and exposes NO FFI for a device
 * backend; the seam this library replaces is
 *
 *   BatchStarkProver::prove_all_tables      circuit-prover/src/batch_stark_prover.rs:1203-1222
 *     -> prove::<EF,D>                       circuit-prover/src/batch_stark_prover.rs:1275-1642
 *       -> p3_batch_stark::prove_batch       call site batch_stark_prover.rs:1595
 *   ProverData::from_airs_and_degrees        call sites recursion/src/recursion.rs:376,487,737,859
 *
 * plus the finer unit seams a Rust integrator can bind one at a time:
 *
 *   TableProver::batch_instance_d4 (Poseidon2 table)   batch_stark_prover/dynamic_air.rs:324-419
 *     -> Poseidon2CircuitAir::generate_trace_rows       poseidon2-circuit-air/src/air.rs:280-520
 *   Mmcs::commit / open_batch (MerkleTreeMmcs)          circuit-prover/src/config.rs:56-63,129
 *   TwoAdicSubgroupDft::coset_lde_batch                 circuit-prover/src/config.rs:55,131
 *   TwoAdicSubgroupDft::dft_batch / idft_batch / coset_dft_batch / coset_idft_batch   (the same Dft; p3r_dft*)
 *   CryptographicPermutation<[F;16]>::permute           circuit-prover/src/config.rs:126-136
 *
 * Conventions (mirroring the reference's Result<_, String> stringification at
 * recursion/src/recursion.rs:34-36):
 *   - every int-returning call returns 0 on success and a negative P3R_E* code on failure;
 *     p3r_last_error(ctx) then returns a human-readable message (ctx may be NULL for
 *     failures of p3r_create itself);
 *   - one p3r_ctx per GPU, NOT thread-safe, one call in flight per ctx (RecursionOutput is
 *     !Send in the reference: recursion/src/recursion.rs:117-139);
 *   - every field element crossing this ABI is a CANONICAL u32 (< p); matrices are
 *     ROW-MAJOR exactly like p3_matrix::dense::RowMajorMatrix; extension-field elements are
 *     4 consecutive base coefficients (basis 1,x,x^2,x^3);
 *   - the caller owns all host buffers; the ctx owns all device memory;
 *   - there is NO CPU fallback: without a usable gfx950 device p3r_create fails.
 */
#ifndef P3R_H
#define P3R_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define P3R_ABI_VERSION 8

enum {
  P3R_OK = 0,
  P3R_EINVAL = -1,   /* bad argument / shape (reference: InvalidProofShape-style errors) */
  P3R_ENODEV = -2,   /* no usable HIP device */
  P3R_EHIP = -3,     /* HIP runtime error */
  P3R_ENOMEM = -4,
  P3R_EUNSUPPORTED = -5, /* reference: BatchStarkProverError::UnsupportedDegree */
  P3R_EBUFFER = -6,  /* caller buffer too small */
  P3R_EVERIFY = -7   /* a well-formed proof that a verifier rejects (the FRI verifier seam; p3r_verify_batch, the older
                      * entry, keeps reporting a rejection as P3R_EINVAL with the reason in its error buffer) */
};

enum { P3R_FIELD_KOALA_BEAR = 0, P3R_FIELD_BABY_BEAR = 1 };

/* Mirrors the FRI/PCS parameters the examples build
 * (recursion/examples/common/mod.rs:464-486, recursive_fibonacci.rs:71-147) plus the
 * field selection of circuit-prover/src/config.rs:180-183. */
typedef struct p3r_config {
  uint32_t abi_version;        /* P3R_ABI_VERSION */
  uint32_t field;              /* P3R_FIELD_* */
  uint32_t ext_degree;         /* circuit extension degree D of the traces: 1 (base-field circuits, CircuitBuilder<F>: the
                                * base proof of recursive_fibonacci.rs:315-331; bus tuples (idx, v)), 4 (binomial
                                * x^4 = W), 2 / 6 / 8 (binomial x^D = ext_w, below), or 5 over KoalaBear
                                * (quintic trinomial x^5 + x^2 - 1: QuinticTrinomialExtensionField, proved under the
                                * same D = 4 STARK configuration as in circuit-prover/src/batch_stark_prover/
                                * tests.rs:844-1029).  Under D = 1 / D = 5 values are n x D / n x 4D, witness indices in
                                * the preprocessed columns are scaled by D and the Poseidon2 table is the compact-D1
                                * one (p3r_layer_desc).  The circuit boundary (p3r_circuit_create ...) runs such
                                * circuits too: constants carry D coefficients, inputs are n x D, Poseidon2 ops are
                                * base-mode permutations (p3r_op_kind). */
  uint32_t log_blowup;
  uint32_t max_log_arity;      /* 1..4 on the device prover: a commit phase folds by at most 16 (the reference's usual
                                * setting is 4); a phase the rule or the schedule makes wider is P3R_EUNSUPPORTED */
  uint32_t cap_height;
  uint32_t log_final_poly_len;
  uint32_t commit_pow_bits;
  uint32_t query_pow_bits;
  uint32_t num_queries;
  int32_t device;              /* HIP device ordinal */
  /* Poseidon2 width-16 round constants, canonical, flat:
   *   [4][16] external-initial | [partial_rounds] internal | [4][16] external-final
   * (the p3_{koala,baby}_bear::*_POSEIDON2_RC_16_* statics a Rust caller passes through,
   * poseidon2-circuit-air/src/public_types.rs:48-54,220-226).  NULL selects the library's
   * built-in table, which is self-generated and NOT pinned to upstream. */
  const uint32_t* poseidon2_rc;
  uint32_t poseidon2_rc_len;
  /* Protocol details the in-tree reference does not pin (they live in un-vendored p3-* crates, DESIGN.md
   * section 4) are selectable, so that a run of tools/rust_pin against upstream is a configuration
   * change and not a code change:
   *   ext_choices      P3R_EXT_* bits below
   *   fri_log_arities  optional explicit FRI folding schedule (one log2 arity per commit phase, tallest
   *                    first); NULL selects the rule min(max_log_arity, distance to the final height,
   *                    distance to the next roll-in height).  Must reach every input height and the
   *                    final height exactly, and no entry may exceed max_log_arity (the verifier's
   *                    bound on a step's arity).  Prover and verifier must be given the same schedule. */
  uint32_t ext_choices;
  const uint8_t* fri_log_arities;
  uint32_t fri_log_arities_len;
  /*   proof_layout     optional order of the fields of the postcard-serialised structs: 18 bytes, three
   *                    permutations batch[5] | fri[5] | opened[8] (csrc/host_transcript.h::ProofLayout
   *                    lists the fields); NULL = the order read off the in-tree destructuring patterns. */
  const uint8_t* proof_layout;
  uint32_t proof_layout_len;
  /* ABI version 4.  W of the binomial extension x^D = W for ext_degree 2, 6, 8 (canonical; BinomiallyExtendable<D>::W
   * of the caller's field crate - the value the proof carries as w_binomial).  Such layers hold the primitive tables
   * and Recompose (batch_stark_prover/tests.rs:486: test_koalabear_batch_stark_extension_field_d8) and enter at the
   * prove_all_tables boundary.  0 for the other degrees: 4 uses the field's W (3 / 11), 1 and 5 have none. */
  uint32_t ext_w;
  /* ABI version 4.  Degree of the STARK's CHALLENGE field (SC::Challenge): 0 / 4 = the quartic binomial extension
   * (every BASELINE configuration); 5 = KoalaBear's quintic trinomial extension, the configuration of
   * koala_bear_quintic_params (test-utils/src/lib.rs:414-460; recursive_fibonacci --quintic;
   * recursion/tests/fibonacci_batch_stark_prover_quintic.rs).  Extension elements of the proof then hold five words. */
  uint32_t challenge_degree;
  /* ABI version 6.  Constants of the WIDTH-32 Poseidon2 permutation (Poseidon2{Koala,Baby}Bear<32>, the permutation of
   * the arity-4 MMCS: Poseidon2Config::{KOALA,BABY}_BEAR_D4_W32, circuit/src/ops/poseidon2_perm/config.rs:88-100,
   * :164-172; 31 / 30 partial rounds).  poseidon2_w32_rc: [4][32] external-initial | [partial] internal | [4][32]
   * external-final, canonical (p3_{koala,baby}_bear::*_POSEIDON2_RC_32_*, poseidon2-circuit-air/src/public_types.rs:
   * 179-187,396-404); poseidon2_w32_diag: the 32 entries of the internal layer's diagonal
   * (GenericPoseidon2LinearLayers<32> of the field crate).  Both live in un-vendored crates, so - like the width-16
   * round constants - they are the caller's DATA; NULL selects self-generated defaults (tools/
   * gen_poseidon2_constants.py: Grain LFSR constants, a diagonal of small integers and inverse powers of two), which
   * are NOT pinned to upstream.  Used by the width-32 Poseidon2 table (P3R_AIR_POSEIDON2_W32). */
  const uint32_t* poseidon2_w32_rc;
  uint32_t poseidon2_w32_rc_len;
  const uint32_t* poseidon2_w32_diag;   /* 32 canonical values, or NULL */
  /* ABI version 6.  Arity of the prover's own MMCS: 0 / 2 = binary trees over the width-16 permutation
   * (PaddingFreeSponge<Perm16, 16, 8, 8>, TruncatedPermutation<Perm16, 2, 8, 16>: every BASELINE configuration);
   * 4 = the arity-4 MMCS of `recursive_aggregation --arity4` (recursion/examples/recursive_aggregation.rs:1024-1046:
   * MerkleTreeMmcs<.., 4, 8> with PaddingFreeSponge<Perm32, 32, 24, 8> leaves and TruncatedPermutation<Perm32, 4, 8, 32>
   * levels over the width-32 permutation above; the challenger keeps the width-16 permutation).  Trace, quotient and
   * FRI commit-phase trees, their opening proofs (step - 1 sibling digests per level, recursion/src/pcs/mmcs.rs:
   * 866-1316) and both verifiers follow.  cap_height must be 0 with arity 4. */
  uint32_t mmcs_arity;
  /* ABI version 7.  ZK: the PCS is HidingFriPcs (create_config_zk, recursion/examples/common/mod.rs:511-553:
   * `MyPcsZk::new(dft, val_mmcs, fri_params, 2, SmallRng::seed_from_u64(rng_seed))` over the SAME non-hiding MMCS;
   * `recursive_fibonacci --zk`, `recursive_aggregation --zk`, recursion/tests/fibonacci_batch_stark_prover_zk.rs).
   *   zk = 1: every committed matrix (preprocessed, main, permutation, quotient chunks) is committed over the EXTENDED
   *     trace domain of twice the height - original rows interleaved with random rows - with `num_random_codewords`
   *     random columns appended; a random round (Challenge::DIMENSION + num_random_codewords columns per instance) is
   *     committed and opened at zeta; the quotient has 2^(log_chunks + 1) chunks, each masked by a random multiple of
   *     its vanishing polynomial; degree_bits in the proof and in the preprocessed metadata are the extended ones
   *     (recursion.rs:374); the opening proof is HidingFriPcs's tuple (random opened values, FriProof).  What the
   *     verifiers enforce is recursion/src/verifier/batch_stark.rs:424-428,487-490,536,623-661,701-735,855-864,1116-1260;
   *     the prover side of HidingFriPcs lives in the un-vendored p3-fri crate and its proofs are randomised, so byte
   *     parity with upstream is undefined by construction - the construction is written from those acceptance
   *     conditions.  The preprocessed round is padded with zeros, not random values: its commitment
   *     depends on the circuit shape only.
   *   num_random_codewords: 0 selects 2 (the examples' value); 1..8.
   *   zk_key (ABI version 8; versions up to 7 had a 64-bit `zk_seed` here): 256-bit key of the random values - the
   *     counterpart of HidingFriPcs's `rng: R`, which is the caller's to choose (common/mod.rs:536-542).  The values come
   *     from a keyed counter-based generator, ChaCha with 8 rounds over (key, proofs made so far by the ctx, round,
   *     matrix, cell), field elements by rejection sampling (csrc/zk_rand.h).  By default p3r_create mixes 128 bits of
   *     operating-system entropy (getrandom) into the key: two contexts, or two runs, never mask different witnesses with
   *     the same values, whatever the caller passes - an all-zero key is fine.  P3R_EXT_ZK_DETERMINISTIC in ext_choices
   *     takes the key as it is and lets p3r_zk_set_nonce move the proof counter: reproducible proofs for tests and
   *     replay, and NO hiding if a (key, nonce) pair is ever used for two witnesses. */
  uint32_t zk;
  uint32_t num_random_codewords;
  uint32_t zk_key[8];
  /* ABI version 8.  MerkleTreeHidingMmcs for the input MMCS and (through ExtensionMmcs) the FRI commit-phase MMCS -
   * "the upstream-recommended ZK setup" of recursion/tests/zk_hiding_mmcs.rs (SALT_ELEMS = 4 there): every committed
   * matrix gets mmcs_salt_elems random elements per row, a leaf preimage is the concatenation of [row | salt] over the
   * matrices of its height class (recursion/src/pcs/mmcs.rs:315-413, :430-510), and an MMCS opening proof is the tuple
   * (per-matrix salts, sibling digests) (:763-790).  0: the plain MerkleTreeMmcs; 1..16.  The salts come from the
   * generator of zk_key (which is therefore keyed also when zk = 0); both arities; independent of zk, as the MMCS type is
   * independent of the PCS type upstream.  The preprocessed commitment is salted too (it is made once per circuit). */
  uint32_t mmcs_salt_elems;
} p3r_config;
/* LogUp: one auxiliary column per interaction instead of packing same-bus interactions greedily up to
 * the degree budget 2^log_chunks + 1 (batch_stark_prover.rs:925-941 `pack_same_bus`). */
#define P3R_EXT_LOOKUP_UNPACKED 1u
/* ABI version 7.  The width-32 permutation - the one of the arity-4 MMCS (mmcs_arity = 4) and of the width-32 Poseidon2
 * table - has its constants in un-vendored crates, and the library's built-in defaults for them are SELF-GENERATED: a
 * proof made with them verifies nowhere else.  Using that permutation with poseidon2_w32_rc or poseidon2_w32_diag NULL
 * therefore needs this acknowledgement in ext_choices; without it p3r_create (mmcs_arity = 4), the width-32 entry points,
 * p3r_prep_create / p3r_layer_create of a batch holding P3R_AIR_POSEIDON2_W32, p3r_verify_batch and p3r_mmcs_verify
 * refuse with P3R_EINVAL.  (The width-16 defaults are believed to be upstream's; the width-32 ones are known not to be.) */
#define P3R_EXT_UNPINNED_W32_DEFAULTS 2u
/* ABI version 8.  ZK: use p3r_config.zk_key as it is (no operating-system entropy mixed in) and allow p3r_zk_set_nonce:
 * the proofs of a context are then a function of (key, nonce, inputs) - what the parity tests against the CPU oracle
 * need, and what a deployment must NOT set (see zk_key). */
#define P3R_EXT_ZK_DETERMINISTIC 4u

typedef struct p3r_ctx p3r_ctx;
typedef struct p3r_dmat p3r_dmat; /* device-resident matrix (power-of-two height) */
typedef struct p3r_tree p3r_tree; /* device-resident MMCS prover data */
typedef struct p3r_challenger p3r_challenger; /* host-side Fiat-Shamir transcript (DuplexChallenger) */

/* ---- context ---- */
p3r_ctx* p3r_create(const p3r_config* cfg);
void p3r_destroy(p3r_ctx* ctx);
const char* p3r_last_error(const p3r_ctx* ctx);
/* Width of the Poseidon2 circuit-table main trace (166 KoalaBear / 300 BabyBear), i.e.
 * BaseAir::width of Poseidon2CircuitAir (poseidon2-circuit-air/src/air.rs:561-585). */
uint32_t p3r_poseidon2_trace_width(const p3r_ctx* ctx);
/* Number of round constants the configured field expects (148 / 141). */
uint32_t p3r_poseidon2_num_constants(const p3r_ctx* ctx);
/* The round constants in use (canonical, the flat layout of p3r_config.poseidon2_rc); `out` holds
 * p3r_poseidon2_num_constants values. */
int p3r_poseidon2_round_constants(const p3r_ctx* ctx, uint32_t* out);
/* ABI version 7.  Proofs made so far under a ZK configuration (the state of the hiding PCS's RNG): read it, or - under
 * P3R_EXT_ZK_DETERMINISTIC only (ABI version 8; P3R_EINVAL otherwise: replaying a nonce repeats the masks) - set it to
 * replay / skip ahead (parity tests set it so that the CPU oracle can be given the same value). */
uint64_t p3r_zk_nonce(const p3r_ctx* ctx);
int p3r_zk_set_nonce(p3r_ctx* ctx, uint64_t nonce);
/* Blocks until all work queued on the ctx's stream has completed. */
int p3r_sync(p3r_ctx* ctx);
/* Device memory a ctx has released stays in its pool for reuse (a 2^20-row prove keeps several GB
 * cached between proofs; context.h::DevPool).  p3r_trim returns the cached blocks of this ctx to the
 * driver and reports how many bytes that was; an allocation that fails with out-of-memory trims the
 * pools of EVERY ctx of the process before it is reported as P3R_ENOMEM. */
int p3r_trim(p3r_ctx* ctx, uint64_t* freed_bytes);

/* ---- device matrices (inputs stay resident in HBM between calls) ---- */
p3r_dmat* p3r_dmat_upload(p3r_ctx* ctx, const uint32_t* rowmajor, size_t height, size_t width);
p3r_dmat* p3r_dmat_alloc(p3r_ctx* ctx, size_t height, size_t width);
int p3r_dmat_download(p3r_ctx* ctx, const p3r_dmat* m, uint32_t* rowmajor_out);
size_t p3r_dmat_height(const p3r_dmat* m);
size_t p3r_dmat_width(const p3r_dmat* m);
void p3r_dmat_free(p3r_ctx* ctx, p3r_dmat* m);

/* ---- K3: Poseidon2 (CryptographicPermutation + circuit-table trace fill) ---- */

/* n independent width-16 permutations; in/out are n x 16 row-major. */
int p3r_poseidon2_permute_batch(p3r_ctx* ctx, const uint32_t* in, uint32_t* out, size_t n);
/* Device-resident form: states is an n x 16 matrix permuted in place. */
int p3r_poseidon2_permute_dmat(p3r_ctx* ctx, p3r_dmat* states);

/* Flattened Vec<Poseidon2CircuitRow<F>> (circuit/src/ops/poseidon2_perm/trace.rs:94-125),
 * already padded to a power of two by the caller exactly as Poseidon2Prover does
 * (circuit-prover/src/batch_stark_prover/poseidon2.rs:1125-1140). Only the fields the
 * main trace depends on are carried; the CTL fields feed the preprocessed trace. */
typedef struct p3r_p2_rows {
  size_t n;                       /* power of two */
  const uint32_t* input_values;   /* n x 16 row-major */
  const uint8_t* new_start;       /* n */
  const uint8_t* merkle_path;     /* n */
  const uint8_t* mmcs_bit;        /* n */
  const uint32_t* mmcs_index_sum; /* n */
} p3r_p2_rows;
/* ABI version 6.  Rows of the WIDTH-32 table (arity-4 compression shape, 4 * CAPACITY_EXT == WIDTH_EXT:
 * Poseidon2CircuitRow with mmcs_bit2; poseidon2-circuit-air/src/air.rs:370-432).  The main trace is
 * [Poseidon2Cols<32> | mmcs_bit | mmcs_bit2 | mmcs_bit * mmcs_bit2 | mmcs_index_sum]; the index accumulator of a
 * Merkle continuation row is 4 * previous + mmcs_bit + 2 * mmcs_bit2. */
typedef struct p3r_p2w_rows {
  size_t n;                       /* un-padded row count (0: the layer has no width-32 table) */
  const uint32_t* input_values;   /* n x 32 row-major */
  const uint8_t* new_start;       /* n */
  const uint8_t* merkle_path;     /* n */
  const uint8_t* mmcs_bit;        /* n: low bit of the position pos = mmcs_bit + 2 * mmcs_bit2 */
  const uint8_t* mmcs_bit2;       /* n: high bit */
  const uint32_t* mmcs_index_sum; /* n */
} p3r_p2w_rows;

/* Unit seams of the width-32 permutation and its table (ABI 6): Poseidon2{Koala,Baby}Bear<32> on n row-major
 * canonical states; generate_trace_rows of the arity-4 layout (trace_out is n x p3r_poseidon2_w32_trace_width(),
 * n a power of two). */
int p3r_poseidon2_w32_permute_batch(p3r_ctx* ctx, const uint32_t* in, uint32_t* out, size_t n);
int p3r_poseidon2_w32_trace_fill(p3r_ctx* ctx, const p3r_p2w_rows* rows, uint32_t* trace_out);
uint32_t p3r_poseidon2_w32_trace_width(const p3r_ctx* ctx);

/* Poseidon2CircuitAir::generate_trace_rows: trace_out is n x p3r_poseidon2_trace_width(). */
int p3r_poseidon2_trace_fill(p3r_ctx* ctx, const p3r_p2_rows* rows, uint32_t* trace_out);
/* Same, leaving the trace in HBM. */
p3r_dmat* p3r_poseidon2_trace_fill_dmat(p3r_ctx* ctx, const p3r_p2_rows* rows);
/* Rows kept resident in HBM (so a prove can start from device-resident inputs). */
typedef struct p3r_p2_dev p3r_p2_dev;
p3r_p2_dev* p3r_p2_rows_upload(p3r_ctx* ctx, const p3r_p2_rows* rows);
void p3r_p2_rows_free(p3r_ctx* ctx, p3r_p2_dev* rows);
p3r_dmat* p3r_poseidon2_trace_fill_dev(p3r_ctx* ctx, const p3r_p2_dev* rows);

/* ---- K5: coset low-degree extension (TwoAdicSubgroupDft::coset_lde_batch followed by
 * bit_reverse_rows, as TwoAdicFriPcs::commit applies it) ----
 * evals: h x w evaluations over the size-h subgroup (natural order).
 * out  : (h << added_bits) x w, row i = evaluation at shift * w_{h<<added_bits}^{bitrev(i)}. */
int p3r_coset_lde(p3r_ctx* ctx, const uint32_t* evals, size_t h, size_t w, uint32_t added_bits,
                  uint32_t shift, uint32_t* out);
p3r_dmat* p3r_coset_lde_dmat(p3r_ctx* ctx, const p3r_dmat* evals, uint32_t added_bits,
                             uint32_t shift);

/* The two halves of the LDE on their own: the `Dft` of a configuration (the Radix2DitParallel<F> of
 * circuit-prover/src/config.rs:55,131), i.e. p3_dft::TwoAdicSubgroupDft.  Every column of an h x w matrix is one
 * polynomial of degree < h.  The COEFFICIENT side is always in natural order (row k = coefficient of x^k);
 * eval_order describes the EVALUATION side in both directions - the output of a P3R_DFT_FORWARD call, the input of
 * a P3R_DFT_INVERSE call.
 *   TwoAdicSubgroupDft::dft_batch          P3R_DFT_FORWARD, shift 1, P3R_DFT_NATURAL   (the one required method)
 *   TwoAdicSubgroupDft::idft_batch         P3R_DFT_INVERSE, shift 1, P3R_DFT_NATURAL
 *   TwoAdicSubgroupDft::coset_dft_batch    P3R_DFT_FORWARD, any other non-zero canonical shift
 *   TwoAdicSubgroupDft::coset_idft_batch   P3R_DFT_INVERSE, any other non-zero canonical shift
 *   P3R_DFT_BITREV                         the same followed (forward) / preceded (inverse) by
 *                                          BitReversibleMatrix::bit_reverse_rows, without a pass of its own over a
 *                                          forward result (the passes produce that order)
 *   TwoAdicSubgroupDft::dft_algebra_batch  needs no entry: an h x w matrix of D-word extension elements IS the
 *                                          h x (w * D) base matrix (the transform is linear over the base field)
 * Inputs are never modified; outs[i] is a fresh matrix the caller frees.  Heights are powers of two from 1 to
 * 2^TWO_ADICITY (24 KoalaBear, 27 BabyBear), widths >= 1 (2^27 rows, BabyBear only, is P3R_EUNSUPPORTED here as in
 * p3r_coset_lde: its 2^14-row NTT tile does not fit the LDS).  P3R_EINVAL, before anything is allocated or launched: a
 * height that is not a power of two or is above the two-adicity, shift 0 or >= p, an unknown direction or order,
 * n_mats == 0, a non-canonical host word.  All matrices of a batch go through the device together (one launch per
 * pass), whatever their heights. */
#define P3R_DFT_FORWARD 0   /* coefficients -> evaluations */
#define P3R_DFT_INVERSE 1   /* evaluations -> coefficients */
#define P3R_DFT_NATURAL 0   /* evaluation row i is the point shift * w_h^i */
#define P3R_DFT_BITREV  1   /* evaluation row i is the point shift * w_h^bitrev(i) */
int p3r_dft(p3r_ctx* ctx, const uint32_t* rowmajor_in, size_t h, size_t w, uint32_t direction, uint32_t shift,
            uint32_t eval_order, uint32_t* rowmajor_out);
int p3r_dft_batch_dmat(p3r_ctx* ctx, const p3r_dmat* const* mats, size_t n_mats, uint32_t direction,
                       const uint32_t* shifts /* n_mats, canonical */, uint32_t eval_order,
                       p3r_dmat** outs /* n_mats, caller frees */);

/* ---- K6: MMCS (MerkleTreeMmcs<PaddingFreeSponge<Perm,16,8,8>, TruncatedPermutation<Perm,2,8,16>>) ---- */

typedef struct p3r_matrix {
  const uint32_t* values; /* height x width row-major */
  size_t height;          /* power of two */
  size_t width;
} p3r_matrix;

/* Mmcs::commit over host matrices of mixed heights; cap_out receives (8 << cap_height)
 * elements; *tree_out (optional, may be NULL) receives the prover data for p3r_mmcs_open. */
int p3r_mmcs_commit(p3r_ctx* ctx, const p3r_matrix* mats, size_t n_mats, uint32_t* cap_out,
                    p3r_tree** tree_out);
/* Same over device-resident matrices; the tree borrows (does not own) the matrices. */
int p3r_mmcs_commit_dmat(p3r_ctx* ctx, const p3r_dmat* const* mats, size_t n_mats,
                         uint32_t* cap_out, p3r_tree** tree_out);
/* Mmcs::open_batch(index): writes, for each committed matrix in commit order, its row
 * (index >> (log_max_height - log_height)) into opened_values (concatenated, sum of widths
 * elements), and the sibling digests bottom-up into proof_out
 * (p3r_tree_proof_len(tree) x 8 elements: log_max_height - cap_height digests for a binary tree; for an arity-4 tree
 * step - 1 digests per level in ascending position, the opened node's own left out). */
int p3r_mmcs_open(p3r_ctx* ctx, const p3r_tree* tree, size_t index, uint32_t* opened_values,
                  uint32_t* proof_out);
/* Digests of one opening proof of this tree (`Mmcs::Proof = Vec<[F; 8]>`). */
size_t p3r_tree_proof_len(const p3r_tree* tree);
/* The hiding MMCS at this seam (cfg.mmcs_salt_elems = S > 0; MerkleTreeHidingMmcs, recursion/src/pcs/mmcs.rs:315-413,
 * :763-790).  p3r_mmcs_commit / p3r_mmcs_commit_dmat then draw one salt matrix (height_i x S, owned by the tree; with
 * _dmat the caller's matrices stay borrowed) per committed matrix and commit [M0 | S0], [M1 | S1], ..  The salts come from
 * the generator of zk_key at the context's proof counter, on a stream of their own: EVERY PUBLIC COMMIT ON A HIDING
 * CONTEXT ADVANCES THE PROOF COUNTER (p3r_zk_nonce) BY ONE, as a proof does, so two commits of the same matrices give
 * different caps and no commit shares a value with a proof; under P3R_EXT_ZK_DETERMINISTIC, p3r_zk_set_nonce makes a
 * commit reproducible.  zk = 1 with mmcs_salt_elems = 0 stays a plain commit (HidingFriPcs runs over the non-hiding MMCS).
 * p3r_tree_total_width stays the words of opened_values per index - the caller's widths, without the salts;
 * p3r_tree_salt_elems is S (0: a plain tree) and p3r_tree_num_matrices the number of matrices the caller committed.
 * p3r_mmcs_open has no salt output: on a hiding tree it returns P3R_EINVAL; open with p3r_mmcs_open_batch. */
size_t p3r_tree_salt_elems(const p3r_tree* tree);
size_t p3r_tree_num_matrices(const p3r_tree* tree);
/* Mmcs::open_batch for each of `n` indices (any order, repeats allowed) in one gather launch, one copy back and one
 * wait - what a PCS opens for its query indices.  For entry i: opened_values[i] = the rows in commit order, each matrix
 * at its own scale (indices[i] >> (log_max_height - log_height)); salts[i] = the per-matrix salts in commit order - the
 * first half of the hiding MMCS's opening proof `(salts, siblings)` (mmcs.rs:763-790), what p3r_mmcs_verify_salted takes;
 * proofs[i] = the sibling digests as p3r_mmcs_open gives them.  Everything canonical.  n == 0: P3R_OK, nothing touched.
 * An index >= 2^log_max_height, or salts == NULL on a hiding tree: P3R_EINVAL before anything is launched. */
int p3r_mmcs_open_batch(p3r_ctx* ctx, const p3r_tree* tree, const size_t* indices, size_t n,
                        uint32_t* opened_values, /* n x p3r_tree_total_width */
                        uint32_t* salts,         /* n x num_matrices x salt_elems; may be NULL iff salt_elems == 0 */
                        uint32_t* proofs);       /* n x p3r_tree_proof_len x 8 */
/* Mmcs::verify_batch on the host, no context: heights / widths of the committed matrices in commit order, the opened
 * rows concatenated in that order, `proof` = proof_len digests.  Honours cfg->mmcs_arity (and, for arity 4, the
 * width-32 constants of cfg).  Returns P3R_OK when the opening is accepted, P3R_EINVAL with the reason in err_buf
 * otherwise. */
int p3r_mmcs_verify(const p3r_config* cfg, const uint32_t* cap, size_t n_mats, const size_t* heights, const size_t* widths,
                    size_t index, const uint32_t* opened_values, const uint32_t* proof, size_t proof_len, char* err_buf,
                    size_t err_cap);
/* ABI version 8.  The same for a hiding MMCS (cfg->mmcs_salt_elems > 0: MerkleTreeHidingMmcs::verify_batch,
 * recursion/src/pcs/mmcs.rs:315-413): `salts` = n_mats x mmcs_salt_elems, the first half of the opening proof
 * `(salts, siblings)`; every leaf preimage is the concatenation of [row | salt] per matrix of its height class. */
int p3r_mmcs_verify_salted(const p3r_config* cfg, const uint32_t* cap, size_t n_mats, const size_t* heights, const size_t* widths,
                           size_t index, const uint32_t* opened_values, const uint32_t* salts, const uint32_t* proof,
                           size_t proof_len, char* err_buf, size_t err_cap);
size_t p3r_tree_log_max_height(const p3r_tree* tree);
size_t p3r_tree_total_width(const p3r_tree* tree);
void p3r_tree_free(p3r_ctx* ctx, p3r_tree* tree);

/* ---- the value half of Pcs::open ----
 *
 * TwoAdicFriPcs::open (p3_fri::TwoAdicFriPcs as the `Pcs` of circuit-prover/src/config.rs) has two halves: it evaluates
 * every committed matrix at its opening points (p3_interpolation::interpolate_coset on the low coset of the
 * bit-reversed LDE), then runs FRI over the reduced openings.  These entries are the first half alone: no transcript,
 * no randomness, no proof bytes.  With p3r_coset_lde_dmat + p3r_mmcs_commit_dmat (= Pcs::commit) a caller holds the
 * committed LDEs on the device and gets the `OpenedValues` of Pcs::open from them without downloading a trace.
 *
 * p3r_open_points_dmat  == the `mats_and_points` loop of Pcs::open: for matrix i of height H_i let h_i = H_i >>
 *                          added_bits.  The evaluations of the interpolant are rows 0 .. h_i (eval_order P3R_DFT_BITREV:
 *                          the first h_i rows of a bit-reversed LDE of blow-up 2^added_bits, which is how upstream's
 *                          open reads them) or rows k << added_bits (P3R_DFT_NATURAL).  They are taken as the values over
 *                          shift * <w_{h_i}>, in that order, of the unique polynomials of degree < h_i, one per column;
 *                          shift 0 = the field's generator (the shift of Pcs::commit), added_bits 0 = the whole matrix.
 *                          `points`: canonical words, DC per point (DC = the context's challenge degree, 4 or 5); points
 *                          point_offsets[i] .. point_offsets[i + 1] belong to matrix i.  values_out (HOST memory):
 *                          [matrix][point][column][DC] canonical words, i.e. OpenedValues with the rounds flattened.
 *                          Any number of points per matrix; a matrix element is read once for every
 *                          P3R_OPEN_POINTS_PER_PASS of them, and all matrices of a call share one weights launch, one
 *                          dot launch, one reduce launch and one wait.  A matrix of width 0 or without points is legal
 *                          and contributes nothing.
 * p3r_open_points       == the same over host matrices (row-major canonical), as p3r_dft stands next to
 *                          p3r_dft_batch_dmat.
 * P3R_EINVAL, with a message, before anything is launched: a height that is not a power of two, is smaller than
 * 2^added_bits or leaves more than 2^TWO_ADICITY evaluations; point_offsets that decrease; a non-canonical point word or
 * shift; an unknown order; a point that lies IN the evaluation coset (z^h == shift^h) - interpolate_coset divides by
 * zero there, so the call is refused and no wrong value is returned. */
#define P3R_OPEN_POINTS_PER_PASS 4 /* points that share one read of a matrix (the accumulators' registers) */
int p3r_open_points_dmat(p3r_ctx* ctx, const p3r_dmat* const* mats, size_t n_mats, uint32_t added_bits, uint32_t shift,
                         uint32_t eval_order, const size_t* point_offsets /* n_mats + 1 */, const uint32_t* points,
                         uint32_t* values_out);
int p3r_open_points(p3r_ctx* ctx, const p3r_matrix* mats, size_t n_mats, uint32_t added_bits, uint32_t shift,
                    uint32_t eval_order, const size_t* point_offsets /* n_mats + 1 */, const uint32_t* points,
                    uint32_t* values_out);

/* ---- the reduced openings of Pcs::open, and FriFoldingStrategy::fold_matrix with the roll-in ----
 *
 * The two deterministic steps of the second half of TwoAdicFriPcs::open: no transcript, no randomness, no proof bytes -
 * alpha and beta are the caller's challenger's.  With p3r_coset_lde_dmat, p3r_mmcs_commit_dmat, p3r_open_points_dmat,
 * p3r_mmcs_open_batch and the entries of the next section (the challenger, the commit-phase leaf view, the final
 * polynomial and the folding schedule), a caller owns nothing of the PCS any more: what it brings is its AIR.
 *
 * p3r_fri_reduce_dmat == the reduced openings of Pcs::open.  Matrix i is a whole committed LDE: H_i x w_i, rows in
 *                        bit-reversed order, row r at x_r = shift * w_{H_i}^bitrev(r); shift 0 = the field's generator.
 *                        `points`: canonical words, DC per point; points point_offsets[i] .. point_offsets[i + 1] belong
 *                        to matrix i.  `values` (HOST memory): [matrix][point][column][DC] canonical words, exactly what
 *                        p3r_open_points_dmat wrote for the same matrices and points; `alpha`: DC canonical words.  The
 *                        matrices are walked in call order and a matrix's points in order, with one running factor a_H
 *                        per distinct height H, 1 at first; for each (matrix, point)
 *                            ro_H[r] += a_H * sum_c alpha^c * (V_{i,p,c} - M_i[r][c]) / (z_{i,p} - x_r),
 *                        then a_H *= alpha^{w_i} - the order of TwoAdicFriPcs::open.  outs (room for n_mats handles)
 *                        receives one fresh H x DC matrix per distinct height that has a point, tallest first: column k
 *                        is coefficient k and rows stay in the committed order (the flattening of dft_algebra_batch
 *                        above); *n_outs says how many.  The caller frees them; inputs are never modified.  A matrix of
 *                        width 0 or without points is legal and adds nothing; a matrix element is read once per call
 *                        however many points its matrix has, and all heights share one launch.  The values need not be
 *                        the matrices' own openings: every output word is the formula's.
 *                        P3R_EINVAL, with a message, before anything is allocated or launched: n_mats == 0; a height
 *                        that is not a power of two or is above 2^TWO_ADICITY; point_offsets that decrease; a
 *                        non-canonical word in points, values, alpha or shift; values == NULL while a matrix has both
 *                        points and columns; a point IN a matrix's evaluation coset (z^H == shift^H), where the quotient
 *                        divides by zero - as p3r_open_points refuses it, so no wrong vector is returned.
 * p3r_fri_fold_dmat   == FriFoldingStrategy::fold_matrix of TwoAdicFriFolding for log_arity = 1 .. 4, then the roll-in.
 *                        `in`: n x DC, n = 2^L, row i the value at s_i = w_n^bitrev(i) (FRI folds over the subgroup: no
 *                        shift).  Row r of the result is log_arity sequential arity-2 folds of rows r << log_arity ..
 *                        (r + 1) << log_arity with beta, beta^2, beta^4, ..; one step is
 *                            fold2(e0, e1, beta, x0) = (e0 + e1) / 2 + beta * (e0 - e1) / (2 * x0),  x0 the point of e0;
 *                        with roll_in ((n >> log_arity) x DC; may be NULL), beta^(2^log_arity) * roll_in[r] is added.
 *                        *out: a fresh (n >> log_arity) x DC matrix the caller frees; inputs are never modified.
 *                        P3R_EINVAL: log_arity == 0, n < 2^log_arity, n not a power of two (or above 2^TWO_ADICITY), a
 *                        width of `in` or roll_in other than DC, a roll_in of another height, a non-canonical beta word.
 *                        P3R_EUNSUPPORTED: log_arity > 4, as in the prover.
 * Both calls only enqueue on the context's stream; a refused call leaves the context usable. */
int p3r_fri_reduce_dmat(p3r_ctx* ctx, const p3r_dmat* const* mats, size_t n_mats, uint32_t shift,
                        const size_t* point_offsets /* n_mats + 1 */, const uint32_t* points,
                        const uint32_t* values /* [matrix][point][column][DC]: what p3r_open_points_dmat wrote */,
                        const uint32_t* alpha /* DC canonical words */,
                        p3r_dmat** outs /* room for n_mats */, size_t* n_outs);
int p3r_fri_fold_dmat(p3r_ctx* ctx, const p3r_dmat* in, uint32_t log_arity, const uint32_t* beta /* DC */,
                      const p3r_dmat* roll_in /* may be NULL */, p3r_dmat** out);

/* ---- the rest of p3_fri::prover::prove_fri: challenger, commit-phase leaf view, final polynomial, folding schedule ----
 *
 * Functions are only added: P3R_ABI_VERSION stays as it is (no struct and no existing entry changes meaning).
 *
 * p3r_challenger == DuplexChallenger<F, Perm16, 16, 8> of circuit-prover/src/config.rs over the context's width-16
 *                   Poseidon2 constants (recursion/src/challenger/circuit.rs:97-156, :337-430) - the transcript the
 *                   prover itself runs.  Host state; only p3r_challenger_grind touches the device.  A handle belongs to
 *                   the context that made it and must be freed before that context is destroyed.
 *   _create / _clone / _free   a fresh transcript (all-zero sponge), an independent copy, the end of one.  NULL on
 *                              failure (p3r_last_error of the context; of NULL for a NULL argument).
 *   _observe(words, n)         n canonical base elements, in order.
 *   _sample(out, n)            n base elements.
 *   _sample_ext(out)           one challenge-field element: DC words, which are DC consecutive samples.
 *   _sample_bits(bits, out)    the low `bits` bits of one sample.
 *   _check_witness(bits, w, ok_out)  observes w and samples `bits` bits, as check_witness does: *ok_out = 1 when they are
 *                              zero.  bits == 0: accepted, transcript untouched.
 *   _grind(ctx, bits, w_out)   the prover's proof-of-work search on the device: the SMALLEST canonical witness the check
 *                              accepts; the challenger is left in the post-check state.  bits == 0: witness 0, transcript
 *                              untouched.
 *   P3R_EINVAL with a message and the challenger's state unchanged: a non-canonical word (nothing of the call is
 *   observed), bits > 30, a NULL handle or buffer, a challenger of another context.  On a NULL handle the message is
 *   p3r_last_error(NULL)'s.
 *
 * p3r_fri_leaf_view_dmat  == the matrix ExtensionMmcs::commit_matrix commits in commit_phase.  `vec`: n x DC, n = 2^L, in
 *                            the layout p3r_fri_fold_dmat takes.  *out: a fresh (n >> log_arity) x (DC << log_arity) matrix
 *                            the caller frees; row r is the flattened extension elements r << log_arity ..
 *                            (r + 1) << log_arity: column j * DC + k of row r is coefficient k of element
 *                            (r << log_arity) + j.  A plain p3r_dmat: p3r_mmcs_commit_dmat commits it and
 *                            p3r_mmcs_open_batch opens it, so both MMCS arities, the hiding MMCS and cap_height serve a
 *                            commit phase as they are.  The proof's sibling_values of a query are the opened row without
 *                            the element index & (2^log_arity - 1).  Refusals as p3r_fri_fold_dmat's, before anything is
 *                            allocated: log_arity == 0, a width other than DC, n not a power of two (or above
 *                            2^TWO_ADICITY) or n < 2^log_arity P3R_EINVAL; log_arity > 4 P3R_EUNSUPPORTED.  Only enqueues.
 * p3r_fri_final_poly_dmat == the final polynomial: `vec` is m x DC, the last folded vector over <w_m> in bit-reversed
 *                            order; coeffs_out (HOST) receives 2^log_final_poly_len x DC canonical words, the
 *                            coefficients in natural order (the prover's own inverse DFT).  P3R_EINVAL: a non-zero
 *                            coefficient at or above 2^log_final_poly_len (the prover's message: the input is not of low
 *                            degree), m < 2^log_final_poly_len, m > 2^16 (the vector is fetched to the host; the cap keeps
 *                            a misuse from downloading an LDE), a width other than DC.
 * p3r_fri_log_arity       == the folding schedule the prover follows: log2 of the arity of commit phase `phase` at height
 *                            2^log_cur, with the context's max_log_arity and fri_log_arities.  Without an explicit
 *                            schedule: min(max_log_arity, log_cur - log_final, log_cur - log_next_input), at least 1 -
 *                            fold as far as allowed without passing the next roll-in height (log_next_input; -1: none)
 *                            or the final height.  With one: its entry when it is legal.  -1 where the schedule does
 *                            not fit (or ctx is NULL). */
p3r_challenger* p3r_challenger_create(p3r_ctx* ctx);
p3r_challenger* p3r_challenger_clone(const p3r_challenger* ch);
void p3r_challenger_free(p3r_challenger* ch);
int p3r_challenger_observe(p3r_challenger* ch, const uint32_t* words, size_t n);
int p3r_challenger_sample(p3r_challenger* ch, uint32_t* out, size_t n);
int p3r_challenger_sample_ext(p3r_challenger* ch, uint32_t* out /* DC */);
int p3r_challenger_sample_bits(p3r_challenger* ch, uint32_t bits, uint32_t* out);
int p3r_challenger_check_witness(p3r_challenger* ch, uint32_t bits, uint32_t witness, int* ok_out);
int p3r_challenger_grind(p3r_ctx* ctx, p3r_challenger* ch, uint32_t bits, uint32_t* witness_out);
int p3r_fri_leaf_view_dmat(p3r_ctx* ctx, const p3r_dmat* vec, uint32_t log_arity, p3r_dmat** out);
int p3r_fri_final_poly_dmat(p3r_ctx* ctx, const p3r_dmat* vec, uint32_t log_final_poly_len,
                            uint32_t* coeffs_out /* 2^log_final_poly_len x DC */);
int p3r_fri_log_arity(const p3r_ctx* ctx, size_t phase, int log_cur, int log_final, int log_next_input /* -1: none */);

/* ---- the verifier's side of the FRI seam: p3_fri::verifier::verify_fri on the host ----
 *
 * Functions are only added: P3R_ABI_VERSION stays as it is (no struct and no existing entry changes meaning).
 *
 * Host code, no context and no device: a proof made by the calls of the two sections above (Context.prove_fri,
 * p3r::prove_fri) is checked on a machine without a GPU.  The in-tree statement is recursion/src/pcs/fri/verifier.rs:
 * 1371-1838; the code is the FRI part of p3r_verify_batch (csrc/fri_verify.h), which both entries run.
 *
 * p3r_challenger_create_host == p3r_challenger_create from a configuration alone, as p3r_mmcs_verify takes its
 *                            parameters: the same handle, the same sponge over cfg->poseidon2_rc (NULL: the defaults), the
 *                            same behaviour in every p3r_challenger_* entry, _clone and _free included.  Only
 *                            p3r_challenger_grind refuses it (P3R_EINVAL, state unchanged): the search runs on a device.
 *                            The message of that refusal is where p3r_challenger_grind's always is: p3r_last_error of the
 *                            ctx it was given (of NULL for a NULL ctx); every other refusal on a host handle is
 *                            p3r_last_error(NULL)'s.
 *                            NULL on failure, with the message in p3r_last_error(NULL): a NULL cfg, an ABI mismatch, an
 *                            unknown field or challenge degree, constants of the wrong length or not canonical.
 * p3r_fri_log_arity_cfg      == p3r_fri_log_arity with the max_log_arity and fri_log_arities of a configuration.
 *
 * p3r_fri_proof_view: what prove_fri returns, every array a pointer and a length in WORDS (canonical), n_phases =
 * log_arities_len:
 *   log_max_height              log2 of the tallest input's height: the bits of a query index
 *   commit_caps                 n_phases x 2^cap_height x 8: the caps of the commit phases, in order
 *   commit_pow                  n_phases: the commit proof-of-work witnesses (0 where commit_pow_bits == 0)
 *   log_arities                 n_phases bytes: log2 of every phase's arity
 *   final_poly                  2^log_final_poly_len x DC: the coefficients in natural order
 *   query_pow                   the query proof-of-work witness
 *   n_queries, openings         n_queries x n_phases p3r_fri_phase_opening_view, query-major.  For query index i and
 *                               phase p over a tree of 2^L rows (L = log_max_height - the arities up to and including p):
 *     row       (2^log_arity - 1) x DC: the opened leaf row WITHOUT the element at (i >> earlier arities) & (2^log_arity - 1)
 *               - the proof's sibling_values; the verifier puts its own folded value there
 *     salts     mmcs_salt_elems words under a hiding MMCS, else length 0
 *     siblings  proof_len x 8, as p3r_mmcs_open_batch wrote them for the phase's tree (binary: L - cap_height digests;
 *               arity 4: step - 1 per level)
 * p3r_fri_input_view: one per input height, tallest first, strictly decreasing, the first at log_max_height (as
 * prove_fri takes its inputs): `values` = n_queries x DC, entry q the reduced opening of that height at
 * index_q >> (log_max_height - log_height).
 *
 * p3r_fri_verify_transcript == the transcript of verify_fri up to the query indices, which exist only after it: per phase
 *                            the cap is observed, the commit proof of work checked and beta sampled; the final polynomial
 *                            and the log arities are observed (as prove_fri observes them); the query proof of work is
 *                            checked; n_queries indices of log_max_height bits are sampled.  betas_out: n_phases x DC,
 *                            indices_out: n_queries.  On P3R_OK `ch` is where prove_fri left the prover's challenger; on
 *                            any other result it has not moved.  Without the input heights the schedule is checked as far
 *                            as it can be: every arity in 1 .. max_log_arity (the explicit schedule's entry where there is
 *                            one) and their sum log_max_height - log_final_poly_len - log_blowup.
 * p3r_fri_verify         == verify_fri.  `ch` is the challenger BEFORE the proof (a clone of the one the transcript entry
 *                            is given): the replay is done again, then every query is checked:
 *                              - the log arities are exactly what p3r_fri_log_arity gives for the input heights;
 *                              - the fold chain starts from the tallest input's value and uses the arithmetic of
 *                                p3r_fri_fold_dmat: fold2 with beta, beta^2, beta^4, .., and beta^(2^log_arity) * input
 *                                added at the height where an input joins;
 *                              - every phase's row, with the folded value put back, opens the phase's cap under the
 *                                configuration's MMCS (arity 2 or 4, cap_height, salts);
 *                              - the end of the chain is the final polynomial at the query's point.
 *                            On P3R_OK `ch` is left as the transcript entry leaves it; otherwise it has not moved.
 * Results.  P3R_OK: accepted.  P3R_EVERIFY: rejected, the message (p3r_last_error(NULL)) names the rule and the place -
 * "commit proof-of-work of phase 1", "query 2: final polynomial mismatch", "FRI commit phase 0 of query 1: Merkle root
 * mismatch", a log arity the schedule does not give, a number of phases or queries other than the configuration's.
 * P3R_EINVAL: malformed - a NULL pointer with a non-zero length, a non-canonical word, a length that does not fit the
 * configuration and the schedule, an input height above log_max_height, repeated or out of order, no input at
 * log_max_height, a challenger of another field or challenge degree.  P3R_EUNSUPPORTED: zk = 1 (the hiding PCS's opening
 * proof is out of scope, as in the program seams); the hiding MMCS (mmcs_salt_elems > 0) is served.  No call reads
 * outside the lengths it was given. */
typedef struct p3r_fri_phase_opening_view {
  const uint32_t* row;      size_t row_len;
  const uint32_t* salts;    size_t salts_len;
  const uint32_t* siblings; size_t siblings_len;
} p3r_fri_phase_opening_view;
typedef struct p3r_fri_proof_view {
  uint32_t log_max_height;
  uint32_t query_pow;
  const uint32_t* commit_caps; size_t commit_caps_len;
  const uint32_t* commit_pow;  size_t commit_pow_len;
  const uint8_t* log_arities;  size_t log_arities_len;
  const uint32_t* final_poly;  size_t final_poly_len;
  const p3r_fri_phase_opening_view* openings; size_t openings_len;   /* n_queries x n_phases */
  size_t n_queries;
} p3r_fri_proof_view;
typedef struct p3r_fri_input_view {
  uint32_t log_height;
  const uint32_t* values; size_t values_len;   /* n_queries x DC */
} p3r_fri_input_view;
p3r_challenger* p3r_challenger_create_host(const p3r_config* cfg);
int p3r_fri_log_arity_cfg(const p3r_config* cfg, size_t phase, int log_cur, int log_final, int log_next_input /* -1: none */);
int p3r_fri_verify_transcript(const p3r_config* cfg, p3r_challenger* ch, const p3r_fri_proof_view* proof,
                              uint32_t* betas_out /* n_phases x DC */, uint32_t* indices_out /* n_queries */);
int p3r_fri_verify(const p3r_config* cfg, p3r_challenger* ch, const p3r_fri_proof_view* proof,
                   const p3r_fri_input_view* inputs, size_t n_inputs);

/* ---- the caller's AIR: constraint programs evaluated over the quotient domain of resident LDEs ----
 *
 * Functions are only added: P3R_ABI_VERSION stays as it is.
 *
 * The prover half of p3_uni_stark::prove between the trace commitment and the quotient commitment - quotient_values
 * (Air::eval through ProverConstraintFolder on every row of the quotient domain, divided by the vanishing polynomial)
 * followed by split_evals - for an AIR the CALLER brings.  Upstream's constraints are Rust trait code; here they are
 * data, the straight-line program a SymbolicAirBuilder run of the same Air::eval would record.
 *
 * A program is an array of p3r_air_insn in SSA form: instruction i defines value i, and operands name EARLIER
 * instructions only.  A value is a base-field element or a challenge-field element of DC words (DC = the context's
 * challenge degree, 4 or 5); the type follows from the operands: base (op) base is base, anything with an extension
 * operand is an extension value.
 *
 *   op                         operands                                   value
 *   P3R_AIR_CONST              a = canonical base word                    base   (the enumerator of the table kinds
 *   P3R_AIR_PUBLIC             a = index into public_values               base    below: 0 and 1 in both roles)
 *   P3R_AIR_CHALLENGE          a = index into challenges (DC words each)  ext
 *   P3R_AIR_LOCAL / _NEXT      a = matrix, b = column                     base: that cell of the current / next row
 *   P3R_AIR_LOCAL_EXT / P3R_AIR_NEXT_EXT
 *                              a = matrix, b = first of DC consecutive    ext: sum_k col[b + k] * X^k - how a
 *                                  columns                                permutation / LogUp trace is stored flattened
 *   P3R_AIR_IS_FIRST_ROW, P3R_AIR_IS_LAST_ROW, P3R_AIR_IS_TRANSITION
 *                              none                                       base, defined below
 *   P3R_AIR_ADD / _SUB / _MUL  a, b = value ids
 *   P3R_AIR_NEG                a = value id
 *   P3R_AIR_ASSERT_ZERO        a = value id                               none (it may not be referenced); constraint
 *                                                                         number k is the k-th ASSERT_ZERO in program order
 *
 * Semantics.  h = trace height, q = log_quotient_degree, N = h * 2^q, shift 0 = the field's generator, w_m = the
 * two-adic generator of order m.  All input matrices are committed LDEs of ONE height H = h << added_bits, rows in
 * bit-reversed order as p3r_coset_lde_dmat writes them over shift * <w_H>, added_bits >= q; only their first N rows are
 * read (they are the coset shift * <w_N> in bit-reversed order).  For the natural index i in [0, N):
 *   x_i = shift * w_N^i; the current row is storage row bitrev_{log N}(i), the next row the storage row of
 *   (i + 2^q) mod N (h = 1: the row itself);
 *   is_transition = x - w_h^-1,  is_first_row = (x^h - 1) / (x - 1),  is_last_row = (x^h - 1) / (x - w_h^-1);
 *   with n constraints C_0 .. C_{n-1}:  Q_i = (x_i^h - 1)^-1 * sum_k alpha^(n-1-k) * C_k(i)  - Horner in program order,
 *   as ProverConstraintFolder accumulates.
 * outs[c], c in [0, 2^q), is a fresh h x DC matrix the caller frees: row r is Q at i = r * 2^q + c, the point
 * (shift * w_N^c) * w_h^r, in natural row order, column k coefficient k - what split_evals returns and what the
 * prover's own quotient kernel writes.  Chunk c is therefore a matrix of evaluations over the coset (shift * w_N^c) * <w_h>;
 * to extend it onto the commit coset G * <w_{h << added_bits}> (G the field's generator, as TwoAdicFriPcs::commit does with
 * `GENERATOR / domain.shift()`), pass p3r_coset_lde_dmat(outs[c], added_bits, G / (shift * w_N^c)) - with the default
 * shift that is w_N^-c - and commit the results with p3r_mmcs_commit_dmat.  The DFT seam takes a chunk as it is
 * (P3R_DFT_INVERSE with shift * w_N^c, P3R_DFT_NATURAL, gives the chunk's coefficients).
 *
 * Degree rule of p3r_air_program_info: trace cells, is_first_row and is_last_row count 1; constants, publics, challenges
 * and is_transition count 0; ADD / SUB take the maximum, MUL the sum, NEG its operand's.  The needed
 * log_quotient_degree is log2_ceil(max(d, 2) - 1) for the largest constraint degree d.
 *
 * p3r_air_program_info (host only, no context: `cfg` gives the field and the challenge degree, as p3r_mmcs_verify takes
 * it) validates a program against the matrix widths and reports n_constraints, max_degree, log_quotient_degree and
 * peak_live, the most values alive at one instruction.  n_public / n_challenges are not known to it: indices are
 * checked by p3r_quotient_program_dmat.  P3R_OK, or the refusal p3r_quotient_program_dmat would give for the program
 * (message: p3r_last_error(NULL), as for a failed p3r_create).
 *
 * Refusals of p3r_quotient_program_dmat, with a message, before anything is allocated or launched.  P3R_EINVAL: an
 * operand that is not an earlier value or is an ASSERT_ZERO; an unknown op; a matrix or column out of range (for _EXT:
 * column + DC > width); a public or challenge index out of range; a non-canonical word anywhere (constants, publics,
 * challenges, alpha, shift); no ASSERT_ZERO; matrices of different heights; added_bits < log_quotient_degree;
 * log_quotient_degree below what the program needs; a height that is not a power of two, is below 2^added_bits or is
 * above 2^TWO_ADICITY; a shift for which x^h - 1 has a zero in the quotient domain (shift^h a 2^q-th root of unity;
 * shift^h == 1 is the case q = 0).  P3R_EUNSUPPORTED: more simultaneously live values than P3R_AIR_MAX_LIVE;
 * log_quotient_degree > 4; zk contexts (their doubled domains are out of scope here).  A refused call leaves the
 * context usable; the call only enqueues on the context's stream.
 *
 * P3R_AIR_MAX_LIVE: a lane of the interpreter keeps the live values of its row in LDS, [slot][word][lane] over the 64
 * lanes of a one-wave workgroup: 256 bytes per base value, DC * 256 per extension value.  The two kinds have a slot
 * region each, sized by the program's own peak, so the worst program (48 base values alive at one point, 48 quintic
 * ones at another) takes 48 * (5 + 1) * 256 = 73,728 of the CU's 163,840 bytes - two workgroups per CU - while 48 live
 * base values, one width-16 Poseidon2 round with its inputs, outputs and 16 temporaries, take 12 KiB (13 per CU). */
enum {
  P3R_AIR_CHALLENGE = 8, P3R_AIR_LOCAL = 9, P3R_AIR_NEXT = 10, P3R_AIR_LOCAL_EXT = 11, P3R_AIR_NEXT_EXT = 12,
  P3R_AIR_IS_FIRST_ROW = 13, P3R_AIR_IS_LAST_ROW = 14, P3R_AIR_IS_TRANSITION = 15,
  P3R_AIR_ADD = 16, P3R_AIR_SUB = 17, P3R_AIR_MUL = 18, P3R_AIR_NEG = 19, P3R_AIR_ASSERT_ZERO = 20,
  P3R_AIR_LOOKUP = 21, P3R_AIR_LOOKUP_END = 22   /* lookup programs only (below); unknown ops to the two entries above */
};
#define P3R_AIR_MAX_LIVE 48
typedef struct p3r_air_insn {
  uint32_t op, a, b;
} p3r_air_insn;
typedef struct p3r_air_info {
  uint32_t n_constraints;
  uint32_t max_degree;            /* the largest constraint degree under the rule above */
  uint32_t log_quotient_degree;   /* the smallest the program may be evaluated with */
  uint32_t peak_live;             /* <= P3R_AIR_MAX_LIVE for a program the device entry takes */
} p3r_air_info;
int p3r_air_program_info(const p3r_config* cfg, const p3r_air_insn* prog, size_t n_insns, const size_t* widths, size_t n_mats,
                         p3r_air_info* out);
int p3r_quotient_program_dmat(p3r_ctx* ctx, const p3r_air_insn* prog, size_t n_insns, const p3r_dmat* const* mats, size_t n_mats,
                              uint32_t added_bits, uint32_t shift, uint32_t log_quotient_degree,
                              const uint32_t* public_values, size_t n_public,
                              const uint32_t* challenges /* n_challenges x DC */, size_t n_challenges,
                              const uint32_t* alpha /* DC */, p3r_dmat** outs /* 2^log_quotient_degree */);

/* p3r_air_program_eval == the verifier's side of a constraint program: VerifierConstraintFolder for the programs
 * p3r_quotient_program_dmat takes, at one out-of-domain point.  Host only, no context (cfg gives the field and the
 * challenge degree, as for p3r_air_program_info); functions are only added.
 *   local / next     sum(widths) x DC canonical words: the opened values, one challenge-field element per trace cell, at
 *                    zeta and at zeta * w_h (h = 2^log_height), matrices in order.  LOCAL / NEXT read the element of that
 *                    column; LOCAL_EXT / NEXT_EXT read sum_k X^k * opened[col + k], a product in the challenge field - how a
 *                    verifier recombines the flattened columns of a permutation trace.
 *   selectors        the formulas above at x = zeta: is_transition = zeta - w_h^-1, is_first_row = (zeta^h - 1) / (zeta - 1),
 *                    is_last_row = (zeta^h - 1) / (zeta - w_h^-1).
 *   folded_out       DC words: sum_k alpha^(n-1-k) * C_k(zeta), Horner in program order.
 *   inv_zh_out       DC words: 1 / (zeta^h - 1).  folded * inv_zh is what the quotient recombined from its chunks' openings
 *                    must equal.
 * Refusals (message: p3r_last_error(NULL)).  P3R_EINVAL: everything p3r_air_program_info refuses about the program; a
 * public or challenge index out of range; a non-canonical word anywhere; a NULL pointer; log_height above the field's
 * two-adicity; zeta == 1, zeta == w_h^-1 or zeta^h == 1 - a division by zero, so the call is refused and no wrong value
 * is returned.  P3R_EUNSUPPORTED: zk configurations.  There is no P3R_AIR_MAX_LIVE here: the host keeps all values. */
int p3r_air_program_eval(const p3r_config* cfg, const p3r_air_insn* prog, size_t n_insns, const size_t* widths, size_t n_mats,
                         const uint32_t* local /* sum(widths) x DC */, const uint32_t* next /* same */, uint32_t log_height,
                         const uint32_t* zeta /* DC */, const uint32_t* public_values, size_t n_public,
                         const uint32_t* challenges /* n_challenges x DC */, size_t n_challenges, const uint32_t* alpha /* DC */,
                         uint32_t* folded_out /* DC */, uint32_t* inv_zh_out /* DC */);

/* ---- the caller's lookups: lookup programs build the permutation (LogUp) trace of resident traces ----
 *
 * Functions are only added: P3R_ABI_VERSION stays as it is.
 *
 * The step of a prover between the trace commitment and the quotient for an AIR on a bus: p3_lookup's LogUp gadget
 * (LogUpGadget: one auxiliary column per packed group of interactions, the fractions sum_k m_k / d_k, and the running sum
 * over the rows) for interactions the CALLER brings.  The auxiliary trace it returns is the matrix P3R_AIR_LOCAL_EXT /
 * P3R_AIR_NEXT_EXT read: it goes to p3r_coset_lde_dmat, p3r_mmcs_commit_dmat and p3r_quotient_program_dmat as it is.
 *
 * A lookup program is a p3r_air_insn array in the SSA form above, with other sinks:
 *
 *   P3R_AIR_LOOKUP             a = multiplicity value id,                 none (it may not be referenced): adds the term
 *                              b = denominator value id                   m / d to the open auxiliary column, and opens
 *                                                                         one if none is open
 *   P3R_AIR_LOOKUP_END         none                                       none: closes the open column
 *
 * Multiplicity and denominator are base or extension values; a base value is lifted.  The denominator is program data:
 * the seam fixes no bus convention.  The reference's form, bus_prefix + sum_j beta^j * field_j with the challenges laid out
 * [bus_prefix, beta] per lookup (recursion/src/verifier/batch_stark.rs:1086-1110), is a few CHALLENGE / MUL / ADD
 * instructions.  Nor does it fix a packing: the caller groups terms into columns with LOOKUP_END, as pack_same_bus does
 * under its degree budget.  ASSERT_ZERO and the three selectors are refused in a lookup program (upstream's trace-domain
 * values of the selectors are un-vendored and not guessed); LOOKUP and LOOKUP_END stay unknown ops to
 * p3r_air_program_info and p3r_quotient_program_dmat.
 *
 * Semantics.  All input matrices are TRACES on the trace domain: h rows (a power of two), natural order, not LDEs.  Row
 * r is the current row, (r + 1) mod h the next (h = 1: the row itself).  With G closed columns:
 *   f_g[r] = sum over the terms k of column g of m_k(r) / d_k(r);
 *   s[0] = 0,  s[r + 1] = s[r] + sum_g f_g[r]  - the exclusive prefix, as the prover's own auxiliary trace has it in column 0;
 *   T = s[h - 1] + sum_g f_g[h - 1], the table's sum.
 * *out is one fresh h x DC * (1 + G) matrix the caller frees: columns [0, DC) hold the coefficients of s, columns
 * [DC * (1 + g), DC * (2 + g)) those of f_g.  T goes to sum_out (HOST, DC canonical words): the caller's challenger
 * observes it, so p3r_logup_program_dmat WAITS for the stream, unlike p3r_quotient_program_dmat.
 *
 * The constraints the caller then writes in its constraint program ("LogUp per-row constraints"), with
 * f_g = LOCAL_EXT(aux, DC * (1 + g)), s = LOCAL_EXT(aux, 0), s' = NEXT_EXT(aux, 0) and T a challenge:
 *   f_g * prod_k d_k - sum_k m_k * prod_{l != k} d_l    for each column g
 *   is_first_row * s
 *   is_transition * (s' - s - sum_g f_g)
 *   is_last_row * (s + sum_g f_g - T)
 * The first has the degree max(1 + sum_k deg d_k, max_k(deg m_k + sum_{l != k} deg d_l)) under the degree rule above;
 * p3r_lookup_program_info reports the largest over the columns, which the quotient's log_quotient_degree must admit.
 *
 * A zero denominator: upstream divides by zero there.  Here no wrong trace is returned: the call frees the output and
 * returns P3R_EINVAL with "zero denominator in row R", R the smallest row in which the denominator product of a column
 * vanishes.  The context stays usable.
 *
 * p3r_lookup_program_info (host only, no context, as p3r_air_program_info) validates a program against the matrix widths
 * and reports n_terms, n_columns, max_terms_per_column, max_constraint_degree and peak_live.  P3R_OK, or the refusal
 * p3r_logup_program_dmat would give for the program (message: p3r_last_error(NULL)).
 *
 * Refusals of p3r_logup_program_dmat, with a message, before anything is allocated or launched.  P3R_EINVAL: what
 * p3r_quotient_program_dmat refuses about operands, ops, matrices, columns, indices and non-canonical words; an ASSERT_ZERO
 * or a selector; a LOOKUP operand that is not an earlier value or is a LOOKUP / LOOKUP_END; a LOOKUP_END with no open
 * column; a program that ends with a column open; no LOOKUP; n_mats == 0; matrices of different heights; a height that
 * is not a power of two or is above 2^TWO_ADICITY; a NULL out or sum_out.  P3R_EUNSUPPORTED: more live values than
 * P3R_AIR_MAX_LIVE (the interpreter keeps them in LDS exactly as above; LOOKUP and LOOKUP_END take no slot); zk contexts. */
typedef struct p3r_lookup_info {
  uint32_t n_terms, n_columns;
  uint32_t max_terms_per_column;
  uint32_t max_constraint_degree;   /* largest column-constraint degree: what the caller's quotient budget must admit */
  uint32_t peak_live;
} p3r_lookup_info;
int p3r_lookup_program_info(const p3r_config* cfg, const p3r_air_insn* prog, size_t n_insns, const size_t* widths, size_t n_mats,
                            p3r_lookup_info* out);
int p3r_logup_program_dmat(p3r_ctx* ctx, const p3r_air_insn* prog, size_t n_insns, const p3r_dmat* const* mats, size_t n_mats,
                           const uint32_t* public_values, size_t n_public,
                           const uint32_t* challenges /* n_challenges x DC */, size_t n_challenges,
                           p3r_dmat** out, uint32_t* sum_out /* DC, HOST */);

/* ---- is the trace right?  Unsatisfied constraints and unbalanced lookups of resident traces, located ----
 *
 * Functions are only added: P3R_ABI_VERSION stays as it is, no op is added, and no entry above changes.
 *
 * A broken constraint otherwise shows up at the far end, as p3r_fri_final_poly_dmat refusing with "the input is not of
 * low degree"; an unbalanced bus as table sums that do not cancel.  Neither names a row, a constraint or a tuple.  The
 * reference has both tools and uses them on this path: DebugConstraintBuilder runs Air::eval on every (row, next row)
 * pair with 0/1 selectors and reports the first failing row (test-utils/src/lib.rs:165-260, check_air_satisfies; every
 * table wrapper of the batch prover implements it: batch_stark_prover.rs:883-890, poseidon2.rs:808-822,
 * dynamic_air.rs:138-248), and p3_lookup::debug_util::check_lookups runs over all instances before prove_batch when
 * debug_lookups is set (batch_stark_prover.rs:1546-1593).  Both entries refuse zk contexts (P3R_EUNSUPPORTED), as the
 * two program seams do, and both WAIT for the stream.
 *
 * p3r_check_program_dmat: a constraint program (the p3r_air_insn form of p3r_quotient_program_dmat) on the TRACE domain.
 * The inputs are traces, not LDEs: h rows, h a power of two, in natural order, all matrices of one height - the lookup
 * seam's convention.  Row r is the current row and (r + 1) mod h the next one (h = 1: the row itself).  The selectors
 * take the values of DebugConstraintBuilder: is_first_row = [r == 0], is_last_row = [r == h - 1], is_transition =
 * [r != h - 1].  Constraint k is the k-th ASSERT_ZERO; it fails in row r when its value is non-zero - for an extension
 * value, when any coefficient is.  first_row_out[k] (HOST, n_constraints words, may be NULL) is the smallest failing row of
 * constraint k, or 0xffffffff if there is none; n_failed_out[k] (HOST, may be NULL) its number of failing rows.  The report
 * is derived from those two arrays on the host.  A trace that does not satisfy the program is a RESULT, not an error:
 * the call returns P3R_OK.
 * Refusals, with a message, before anything is allocated or launched: what p3r_quotient_program_dmat refuses about
 * programs, operands, matrices, indices and non-canonical words (LOOKUP and LOOKUP_END stay unknown ops here), what
 * p3r_logup_program_dmat refuses about heights, a NULL report (P3R_EINVAL); more live values than P3R_AIR_MAX_LIVE, zk
 * contexts (P3R_EUNSUPPORTED).  The interpreter is the one of the two seams above with a third sink: one wave-wide vote
 * per constraint, and at most two atomic operations per wave and constraint - none at all on a satisfying trace.
 *
 * p3r_lookup_check_dmat: the multiset balance of lookup programs across tables.  An instance is a lookup program as
 * p3r_logup_program_dmat takes it, with its traces (one height per instance) and public values; the challenges are
 * shared.  Every LOOKUP term t of instance p in row r with a non-zero multiplicity is a record (d, m), both lifted to
 * the challenge field; a term with zero multiplicity is no record.  Record order is lexicographic in (instance, row,
 * term).  The key of a record is its denominator value: with the caller's challenges, equal tuples on one bus are equal
 * denominators; the grouping into columns (LOOKUP_END) does not matter here.  Nothing is inverted - a zero denominator is
 * an ordinary key.  A key is unbalanced when the sum of its multiplicities is non-zero.  *n_unbalanced_out counts the
 * unbalanced keys; `out` receives the min(cap, count) of them whose first records come earliest in record order,
 * ascending: the place of the key's first record, the number of records that share the key, the key (canonical, DC words
 * used, the rest zero) and the sum of its multiplicities (canonical, non-zero).  The call returns P3R_OK whatever the
 * count.
 * Refusals, before anything is allocated or launched: each instance for what p3r_logup_program_dmat would refuse it for
 * (the message names the instance); n_inst == 0, a NULL n_unbalanced_out, a NULL out with cap > 0 (P3R_EINVAL); more
 * than P3R_LOOKUP_CHECK_MAX_RECORDS term slots sum_p h_p * n_terms_p, zk contexts (P3R_EUNSUPPORTED).
 * The records are written by the interpreter with a fourth sink, compacted, ordered by key with a stable radix sort
 * (least significant coefficient word first), and summed per run of equal keys with exclusive sums of 64-bit words; the
 * device memory it takes, about (2 DC + 1) words per slot and 4 DC + 10 per record, is freed before it returns. */
typedef struct p3r_check_report {
  uint64_t n_failures;        /* (row, constraint) pairs whose asserted value is not zero */
  uint32_t first_row;         /* smallest failing row; 0xffffffff: the trace satisfies the program */
  uint32_t first_constraint;  /* smallest failing constraint in that row */
} p3r_check_report;
int p3r_check_program_dmat(p3r_ctx* ctx, const p3r_air_insn* prog, size_t n_insns, const p3r_dmat* const* mats, size_t n_mats,
                           const uint32_t* public_values, size_t n_public,
                           const uint32_t* challenges /* n_challenges x DC */, size_t n_challenges,
                           p3r_check_report* report, uint32_t* first_row_out /* n_constraints, may be NULL */,
                           uint64_t* n_failed_out /* n_constraints, may be NULL */);
#define P3R_LOOKUP_CHECK_MAX_RECORDS (1u << 28)
typedef const p3r_dmat* p3r_dmat_cptr;           /* so that a member below reads as one pointer to one word: the type is the same */
typedef struct p3r_lookup_instance {
  const p3r_air_insn* prog; size_t n_insns;      /* a lookup program, as p3r_logup_program_dmat takes it */
  const p3r_dmat_cptr* mats; size_t n_mats;      /* = const p3r_dmat* const* mats: its traces, one height per instance */
  const uint32_t* public_values; size_t n_public;
} p3r_lookup_instance;
typedef struct p3r_lookup_imbalance {
  uint32_t instance, row, term;   /* the first record of the key, in record order */
  uint32_t n_records;             /* records that share the key */
  uint32_t denominator[5];        /* the key, canonical, DC words used */
  uint32_t net[5];                /* the sum of its multiplicities, canonical, non-zero */
} p3r_lookup_imbalance;
int p3r_lookup_check_dmat(p3r_ctx* ctx, const p3r_lookup_instance* inst, size_t n_inst,
                          const uint32_t* challenges /* n_challenges x DC */, size_t n_challenges,
                          p3r_lookup_imbalance* out, size_t cap, uint64_t* n_unbalanced_out);

/* ---- a table's multiplicity column, built on the device from resident traces ----
 *
 * Functions are only added: P3R_ABI_VERSION stays as it is, no op is added, and no entry above changes.
 *
 * Range checks, byte tables and opcode tables need a column that says how often each table row is asked for.  It belongs
 * to the MAIN trace, so it must exist before the trace commitment; p3r_lookup_multiplicities_dmat joins a table against
 * its queries where the traces already lie.  `table` and the `queries` are lookup programs with their traces, exactly as
 * p3r_lookup_check_dmat takes instances: the same validation, the same slots (term t of row r) and the same record order,
 * with the table's slots before those of query 0, query 1, ...
 *
 * Keys.  The key of a slot is the value of its LOOKUP denominator, lifted to the challenge field, as in the check; nothing
 * is inverted.
 * Table slots.  Slot (r, t) of the table OFFERS its key when the multiplicity value of that term is non-zero.  The value
 * is otherwise unused: it is an enable flag, with which a caller switches off padding rows.
 * Query records.  Every LOOKUP term of a query with a non-zero multiplicity is a record (key, m).  Query multiplicities
 * must be statically typed base values - the output is a base column.
 * Output.  *out is a fresh h_T x n_terms_T matrix the caller frees, of the form every p3r_dmat has.  out[r][t] = the sum
 * modulo p of m over all query records whose key is the key of table slot (r, t), if (r, t) is the first offering table
 * slot with that key in (row, term) order; every other cell is 0: later duplicates, disabled slots, keys nobody asks
 * for.  It is a trace column like any other: it goes to p3r_logup_program_dmat, the LDE, the commit and
 * p3r_check_program_dmat as it is, and the table's own lookup program then uses its negation as the multiplicity.
 * Misses.  A key carried by query records is missing when no table slot offers it and its multiplicities do not sum to
 * zero.  *n_missing_out counts them; `missing` receives the first min(cap, count), ordered by their first query record:
 * instance is the index into `queries`, row and term the place of the first record, n_records, denominator and net as
 * in the check.  A non-zero count is a RESULT: the call returns P3R_OK and *out is produced all the same.
 * The call WAITS for the stream.  n_queries == 0 is legal and gives a zero column.
 *
 * WHICH CHALLENGES.  The column is built before the transcript has produced any LogUp challenge, so the `challenges`
 * passed here are the CALLER'S OWN, not the transcript's; they only have to make equal tuples equal keys and different
 * tuples different keys.
 *   - With the basis elements 1, X, .., X^(DC-1) as challenges, a tuple (a_0, .., a_(k-1)) of k <= DC base values under the
 *     denominator sum_j X^j * a_j is its own key: the join is exact.
 *   - A single-field key c - v is exact for any constant c.
 *   - A longer tuple is joined under a challenge beta the caller draws privately, key = sum_j beta^j * a_j.  Two different
 *     tuples of length k share a key only if beta is a root of a non-zero polynomial of degree below k: with N = T + Q table
 *     slots and query records, Pr[two different tuples share a key] <= N * (N - 1) / 2 * (k - 1) / p^DC over the choice of
 *     beta, as long as the traces do not depend on beta.
 *
 * Refusals, with a message, before anything is allocated or launched; the context stays usable.  Each instance for what
 * p3r_logup_program_dmat would refuse it for (the message names "table" or "query i"); a NULL table, out or
 * n_missing_out, a NULL missing with cap > 0 (P3R_EINVAL); more than P3R_LOOKUP_CHECK_MAX_RECORDS term slots summed over
 * the table and the queries, a query LOOKUP whose multiplicity is of extension type, zk contexts (P3R_EUNSUPPORTED).
 * The pass is the check's - records, compaction, the stable sort by key, head marks, exclusive sums of 64-bit words, here of
 * coefficient word 0 with the table's slots counted as zero - and ends in one kernel in which the head of every run
 * either stores the run's sum to its cell of the zeroed output (a table slot: one writer per cell, no atomics) or is
 * flagged as a miss (a query slot). */
int p3r_lookup_multiplicities_dmat(p3r_ctx* ctx,
                                   const p3r_lookup_instance* table,                    /* the table that offers keys */
                                   const p3r_lookup_instance* queries, size_t n_queries,
                                   const uint32_t* challenges /* n_challenges x DC */, size_t n_challenges,
                                   p3r_dmat** out,                                      /* fresh h_T x n_terms_T, the caller frees */
                                   p3r_lookup_imbalance* missing, size_t cap, uint64_t* n_missing_out);

/* ---- derived trace columns: witness programs store values of resident traces as columns ----
 *
 * Functions and enumerators are only added: P3R_ABI_VERSION stays as it is, and no entry above changes what it accepts,
 * refuses or says.
 *
 * The limbs a range check looks up, the column 0 .. h-1 that IS the range table, the inverse witness of an is-zero gadget,
 * products, selector columns, the flattened key of a bus: row-local functions of columns that already lie in device
 * memory, and part of the MAIN trace, so they must exist before the trace commitment.  p3r_witness_program_dmat derives
 * them where the traces lie, as p3r_lookup_multiplicities_dmat derives the multiplicity column.
 *
 * A witness program is a p3r_air_insn array in the SSA form above - the same typing, operand rules and canonical words,
 * the same liveness against P3R_AIR_MAX_LIVE.  It takes every value op of a constraint program, and the three selectors
 * with the values p3r_check_program_dmat gives them on the trace domain (is_first_row = [r == 0], is_last_row =
 * [r == h - 1], is_transition = [r != h - 1]).  Four ops are its own; they stay unknown ops to every entry above:
 *
 *   P3R_AIR_INV                a = value id                               the operand's type: its inverse, and 0 for 0 -
 *                                                                         try_inverse().unwrap_or_default(), the witness of
 *                                                                         an is-zero gadget; defined behaviour, not an error
 *   P3R_AIR_BITS               a = value id (base only), b = lo | n << 8  base: bits [lo, lo + n) of the CANONICAL word of
 *                                                                         the operand; n >= 1 and lo + n <= 31
 *   P3R_AIR_ROW                none                                       base: the row index r
 *   P3R_AIR_STORE              a = value id, b = output column            none (it may not be referenced): a base value
 *                                                                         fills column b, an extension value the columns
 *                                                                         b .. b + DC, coefficient k in column b + k - the
 *                                                                         flattening P3R_AIR_LOCAL_EXT reads
 *
 * ASSERT_ZERO, LOOKUP and LOOKUP_END are refused in a witness program.
 *
 * Semantics.  The inputs are TRACES, exactly as p3r_logup_program_dmat takes them: h rows (a power of two), natural
 * order, one common height, not LDEs.  Row r is the current row; NEXT reads row (r + 1) mod h of an INPUT (h = 1: the row
 * itself).  n_mats == 0 is legal - a table built from ROW alone has no input - and then `height` gives h; otherwise
 * `height` must be 0 or the matrices' height.  *out is one fresh h x W matrix the caller frees, W one past the highest
 * stored column, rows in natural order: it goes to p3r_coset_lde_dmat, p3r_check_program_dmat and the lookup entries as it
 * is.  The call only enqueues on the context's stream, like p3r_quotient_program_dmat; nothing is read back.
 *
 * Out of scope: recurrences - a column that reads its own previous row - and prefix sums.  A program reads inputs only,
 * never what it stores.  Such columns stay with the caller, or with the running sum of p3r_logup_program_dmat.
 *
 * p3r_witness_program_info (host only, no context, as p3r_air_program_info) validates a program against the matrix widths
 * and reports n_stores, n_out_columns (W), n_inversions and peak_live.  P3R_OK, or the refusal p3r_witness_program_dmat
 * would give for the program (message: p3r_last_error(NULL)).
 *
 * Refusals of p3r_witness_program_dmat, with a message, before anything is allocated or launched; the context stays
 * usable.  P3R_EINVAL: everything p3r_logup_program_dmat refuses about operands, ops, matrices, columns, indices, heights
 * and non-canonical words; a sink op of another seam; BITS on an extension value, or with n == 0 or lo + n > 31; INV, BITS
 * or STORE with an operand that is not an earlier value or is a STORE; no STORE; an output column stored twice, or an
 * extension store that overlaps another store; an output column below W that nothing stores; n_mats == 0 with a height
 * that is 0, not a power of two or above 2^TWO_ADICITY; a height that is not the matrices'; a NULL out.  P3R_EUNSUPPORTED:
 * more live values than P3R_AIR_MAX_LIVE (STORE takes no slot); zk contexts.  The interpreter is the one of the seams
 * above with a fifth sink: a lane stores its row's word of a column, consecutive lanes consecutive words, no atomics. */
enum { P3R_AIR_INV = 23, P3R_AIR_BITS = 24, P3R_AIR_ROW = 25, P3R_AIR_STORE = 26 };   /* witness programs only */
typedef struct p3r_witness_info {
  uint32_t n_stores;
  uint32_t n_out_columns;   /* W: the width of the matrix p3r_witness_program_dmat returns */
  uint32_t n_inversions;    /* INV instructions: one field inversion per row each */
  uint32_t peak_live;
} p3r_witness_info;
int p3r_witness_program_info(const p3r_config* cfg, const p3r_air_insn* prog, size_t n_insns, const size_t* widths, size_t n_mats,
                             p3r_witness_info* out);
int p3r_witness_program_dmat(p3r_ctx* ctx, const p3r_air_insn* prog, size_t n_insns, const p3r_dmat* const* mats, size_t n_mats,
                             size_t height, const uint32_t* public_values, size_t n_public,
                             const uint32_t* challenges /* n_challenges x DC */, size_t n_challenges,
                             p3r_dmat** out);

/* ---- accumulator columns: first-order affine recurrences down the rows of resident traces ----
 *
 * Functions and types are only added: P3R_ABI_VERSION stays as it is, no P3R_AIR_* op is added, and no entry above
 * changes what it accepts, refuses or says.
 *
 * The columns the witness section leaves with the caller - a column that reads its own previous row - now go to
 * p3r_affine_scan_dmat: running sums and cumulative counters, running products (grand-product and memory-permutation
 * arguments), Horner evaluation down the rows, segmented accumulators that reset on a flag, index accumulators such as
 * the base-four one of the width-32 Poseidon2 table.  All of them are s[r + 1] = a[r] * s[r] + b[r] with a and b
 * row-local, and a and b already lie in device memory or come from a witness program: z[r + 1] = z[r] * (gamma - x[r]) /
 * (gamma - y[r]) takes its factor column from p3r_witness_program_dmat and z from here, with no trip to the host.
 *
 * Inputs.  TRACES, exactly as the witness and lookup entries take them: h rows, a power of two up to 2^TWO_ADICITY,
 * natural order, one common height, not LDEs.
 *
 * A recurrence (p3r_recurrence) reads one column for a (mul_mat, mul_col), one for b (add_mat, add_col) and writes one
 * column of *out (out_col).  With P3R_SCAN_EXT all three are DC consecutive columns, coefficient k in column + k - the
 * flattening P3R_AIR_LOCAL_EXT reads - and the arithmetic is the challenge field's.  Mixed types are not offered: a
 * caller lifts a base factor with a witness program.  mul_mat == P3R_SCAN_NONE: a = 1 everywhere (a running sum, and no
 * multiplication is done); add_mat == P3R_SCAN_NONE: b = 0 everywhere (a running product).  init is s[0]: canonical, DC
 * words for EXT and word 0 otherwise, the rest zero.
 *
 *   s[0] = init,   s[r + 1] = a[r] * s[r] + b[r]   for r in [0, h)
 *
 * *out is one fresh h x W matrix the caller frees, W one past the highest written column, rows in natural order: a trace
 * like any other.  Row r holds s[r], the state ENTERING the row, as column 0 of p3r_logup_program_dmat does; with
 * P3R_SCAN_INCLUSIVE row r holds s[r + 1].  last_out[5 i .. 5 i + 5) receives s[h] of recurrence i - DC canonical words
 * (one for a base recurrence), the rest zero: the total a challenger observes, or a last-row constraint compares against.
 * With last_out == NULL the call only enqueues on the context's stream; otherwise it waits, as p3r_logup_program_dmat
 * does.
 *
 * The constraints the caller then writes for an exclusive column s, with T = last_out:
 *
 *   is_first_row  * (s - init)
 *   is_transition * (s' - a * s - b)
 *   is_last_row   * (a * s + b - T)
 *
 * a = 0 in a row resets the accumulator to b: segmented sums, and the index accumulator above.  Nothing is inverted, and
 * no error depends on the data.
 *
 * Out of scope: coupled or vector-state recurrences (Fibonacci's 2 x 2 step), non-linear recurrences, heights that are
 * not powers of two.
 *
 * p3r_affine_scan_info (host only, no context, as p3r_witness_program_info) validates the descriptors against the matrix
 * widths and reports W and how many recurrences run as products (no add), sums (no mul) and affine maps.  P3R_OK, or
 * the refusal p3r_affine_scan_dmat would give for them (message: p3r_last_error(NULL)).
 *
 * Refusals of p3r_affine_scan_dmat, with a message, before anything is allocated or launched; the context stays usable.
 * P3R_EINVAL: n_recs == 0 or above 65535; a NULL recs, out or mats entry; n_mats == 0; matrices of different heights, a
 * height that is not a power of two or is above 2^TWO_ADICITY; a matrix or column out of range (EXT: column + DC >
 * width); unknown flag bits; a non-canonical or non-zero-padded init word; two recurrences whose output columns overlap;
 * an output column below W that nothing writes; a recurrence with neither mul nor add - a constant column, which belongs
 * in a witness program.  P3R_EUNSUPPORTED: zk contexts.
 *
 * Three launches whatever n_recs is (reduce, then scan: per-tile composites of the maps x -> a x + b, one workgroup per
 * recurrence that carries them across the tiles, then the column); the combine is not commutative and is applied in row
 * order.  No workgroup waits for another.  Field arithmetic is exact: the result does not depend on the tiling. */
enum { P3R_SCAN_EXT = 1, P3R_SCAN_INCLUSIVE = 2 };          /* p3r_recurrence.flags */
#define P3R_SCAN_NONE 0xffffffffu
typedef struct p3r_recurrence {
  uint32_t flags;
  uint32_t mul_mat, mul_col;   /* a: matrix, (first) column; mul_mat == P3R_SCAN_NONE: a = 1 everywhere */
  uint32_t add_mat, add_col;   /* b: likewise; add_mat == P3R_SCAN_NONE: b = 0 everywhere */
  uint32_t out_col;            /* (first) column of *out */
  uint32_t init[5];            /* s[0], canonical, DC words used for EXT, word 0 otherwise, the rest zero */
} p3r_recurrence;
typedef struct p3r_scan_info { uint32_t n_out_columns, n_products, n_sums, n_affine; } p3r_scan_info;
int p3r_affine_scan_info(const p3r_config* cfg, const p3r_recurrence* recs, size_t n_recs,
                         const size_t* widths, size_t n_mats, p3r_scan_info* out);
int p3r_affine_scan_dmat(p3r_ctx* ctx, const p3r_recurrence* recs, size_t n_recs,
                         const p3r_dmat* const* mats, size_t n_mats,
                         p3r_dmat** out, uint32_t* last_out /* n_recs x 5, HOST, may be NULL */);

/* ---- batch-STARK proving (the chosen drop-in seam) ----
 *
 * p3r_prep_create  == ProverData::from_airs_and_degrees + CircuitProverData::new as called by
 *                     build_next_layer_prep (recursion/src/recursion.rs:342-394): LDE and one
 *                     global MMCS commitment of every AIR's preprocessed trace, kept in HBM.
 * p3r_prove_batch  == p3_batch_stark::prove_batch(&config, &instances, &prover_data)
 *                     (circuit-prover/src/batch_stark_prover.rs:1543-1595): takes the per-table
 *                     main traces in instance order [Const, Public, Alu, dynamic...]
 *                     (batch_stark_prover.rs:1493-1519) and writes the postcard bytes of
 *                     BatchProof (recursion/src/types/proof.rs:403-409).
 */
/* P3R_AIR_POSEIDON2_W32 (ABI 6): Poseidon2CircuitAir{Koala,Baby}BearD4Width32, the table of the arity-4 MMCS rows -
 * eval_arity4 (poseidon2-circuit-air/src/air.rs:1178-1342), 48 preprocessed columns, 16 bus interactions. */
enum { P3R_AIR_CONST = 0, P3R_AIR_PUBLIC = 1, P3R_AIR_ALU = 2, P3R_AIR_POSEIDON2 = 3, P3R_AIR_RECOMPOSE = 4, P3R_AIR_POSEIDON2_W32 = 5 };

/* One CircuitTableAir (circuit-prover/src/common.rs:90-100) of extension degree D = 4. */
typedef struct p3r_air_desc {
  uint32_t kind;                /* P3R_AIR_* */
  uint32_t lanes;               /* TablePacking lanes of this table (packing.rs:10-27) */
  uint32_t horner_packed_steps; /* ALU only: TablePacking::horner_packed_steps, 2..8 */
  uint32_t coeff_lookups;       /* Recompose only: challenger.d() != D (backend/fri.rs:693-721) */
} p3r_air_desc;

typedef struct p3r_prep p3r_prep;

/* prep_mats[i] = BaseAir::preprocessed_trace() of instance i (row-major, padded height).
 * commit_out receives the global preprocessed commitment (8 << cap_height elements). */
p3r_prep* p3r_prep_create(p3r_ctx* ctx, const p3r_air_desc* airs, const p3r_matrix* prep_mats,
                          size_t n_instances, uint32_t* commit_out);
void p3r_prep_free(p3r_ctx* ctx, p3r_prep* prep);

#define P3R_PROOF_QUINTIC_CHALLENGE 2u /* flags of the proof PARSERS (p3r_batch_proof_len*, p3r_batch_stark_proof_parse):
                                        * extension elements are five words (p3r_config.challenge_degree = 5) */
#define P3R_PROOF_ZK 4u /* flags of the proof PARSERS: the proof is a hiding PCS's (p3r_config.zk = 1): its opening proof
                        * is the tuple (random opened values, FriProof) - the proof TYPE, which the bytes do not announce */
#define P3R_PROOF_SALTED 8u /* flags of the proof PARSERS (ABI 8): the MMCSs are hiding ones (p3r_config.mmcs_salt_elems > 0):
                            * every MMCS opening proof is the tuple (per-matrix salts, sibling digests) */
#define P3R_PROVE_CANONICAL_FIELD_ENCODING 1u /* flags: write canonical u32 instead of the
                                               * Montgomery word p3-monty-31's serde emits */

/* Main traces resident in HBM (n_instances device matrices, instance order). On success
 * *proof_len bytes of proof_buf hold the serialized BatchProof; P3R_EBUFFER reports the
 * needed size through *proof_len. P3R_EINVAL with "do not satisfy the constraints" is the
 * counterpart of prove_batch's internal-inconsistency panic. */
int p3r_prove_batch(p3r_ctx* ctx, const p3r_prep* prep, const p3r_dmat* const* main_traces,
                    size_t n_instances, uint32_t flags, uint8_t* proof_buf, size_t proof_cap,
                    size_t* proof_len);
/* The proof of the last prove call on this context that returned P3R_EBUFFER (any of p3r_prove_batch[_host],
 * p3r_prove_all_tables[_resident], p3r_prove_next_layer[_resident]): the bytes are KEPT, not recomputed - a second prove
 * call costs a second proof, and under zk = 1 or a hiding MMCS it IS another proof, of another length, so retrying with
 * the reported size can fail again.  The binding of a growable byte vector (Vec<u8>): call, on P3R_EBUFFER resize to
 * *proof_len and take.  The bytes are dropped by the next prove call and by a successful take; P3R_EINVAL when none is
 * waiting, P3R_EBUFFER (size in *proof_len) when proof_cap is still too small. */
int p3r_take_proof(p3r_ctx* ctx, uint8_t* proof_buf, size_t proof_cap, size_t* proof_len);
/* Same from host matrices (row-major canonical). */
int p3r_prove_batch_host(p3r_ctx* ctx, const p3r_prep* prep, const p3r_matrix* main_traces,
                         size_t n_instances, uint32_t flags, uint8_t* proof_buf, size_t proof_cap,
                         size_t* proof_len);

/* ---- prove_all_tables: the recursion layer as the reference sees it ----
 *
 * p3r_layer_create == build_next_layer_prep (recursion/src/recursion.rs:342-394): everything
 *   that depends only on the verifier-circuit shape - get_airs_and_degrees_with_prep's
 *   preprocessed op lists (circuit-prover/src/common.rs:127-390), the ALU lane schedule
 *   (circuit-prover/src/air/alu_air.rs:349-463), the preprocessed traces and their commitment.
 *   It is the object NextLayerPrepCache caches (recursion.rs:295-298).
 * p3r_prove_all_tables == BatchStarkProver::prove_all_tables(&traces, &circuit_prover_data)
 *   (circuit-prover/src/batch_stark_prover.rs:1203-1222): builds the five main traces in
 *   instance order [Const, Public, Alu, Poseidon2, Recompose] (K1-K3) and proves them.
 *   It returns the inner BatchProof bytes; the Rust shim wraps them with the metadata fields
 *   of BatchStarkProof (batch_stark_prover.rs:1631-1641), which it already owns.
 */
typedef struct p3r_layer_desc_counts {
  size_t n_const, n_public, n_alu, n_p2, n_recompose; /* ops / rows before padding */
  /* ABI version 5.  Rows of the SECOND Recompose table, `recompose/coeff`, of a layer that holds both kinds: a
   * backend created with coefficient lookups registers the two table provers side by side
   * (recompose_table_provers(lanes, true), batch_stark_prover.rs:1914-1932: [`recompose`, `recompose/coeff`]) and a
   * verifier circuit uses both - plain recomposition in the challenger and the MMCS gadgets
   * (recursion/src/challenger/circuit.rs:206-384, pcs/mmcs.rs:106-140), the coefficient kind for decomposition links
   * (circuit_builder.rs:1438-1477).  0: one Recompose table, of the kind recompose_coeff_lookups names. */
  size_t n_recompose_coeff;
  /* ABI version 6.  Rows of the width-32 Poseidon2 table (`poseidon2_perm/<field>_d4_w32`), proved right after the
   * width-16 one - the order a mixed-config verifier circuit enables them in (W16 challenger, W32 MMCS:
   * recursion/examples/recursive_aggregation.rs:902-1000).  D = 4 circuits; 0: no such table. */
  size_t n_p2w;
} p3r_layer_desc_counts;

typedef struct p3r_layer_desc {
  p3r_layer_desc_counts counts;
  /* TablePacking (circuit-prover/src/batch_stark_prover/packing.rs:10-27) */
  uint32_t public_lanes, alu_lanes, horner_packed_steps, recompose_lanes, min_trace_height;
  /* per-op preprocessed data exactly as get_airs_and_degrees_with_prep leaves it */
  const uint32_t* const_prep;     /* n_const x 2: [ext_mult, D*witness_idx]   (common.rs:353-368) */
  const uint32_t* public_prep;    /* n_public x 2                              (common.rs:324-351) */
  const uint32_t* alu_prep13;     /* n_alu x 13: AluPrepLaneCols               (common.rs:198-323) */
  const uint32_t* recompose_prep; /* n_recompose x 2: [D*output_idx, out_mult]; with recompose_coeff_lookups (below)
                                   * n_recompose x (2 + 2D): ... then (D*coeff_idx_i, coeff_mult_i) for i < D */
  /* Poseidon2CircuitRow CTL fields after poseidon_preprocess_for_prover
   * (circuit-prover/src/batch_stark_prover.rs:97-246); witness ids are NOT yet D-scaled */
  const uint8_t* p2_new_start;        /* n_p2 */
  const uint8_t* p2_merkle_path;      /* n_p2 */
  const uint8_t* p2_mmcs_ctl_enabled; /* n_p2 */
  const uint8_t* p2_in_ctl;           /* n_p2 x IL */
  const uint32_t* p2_input_indices;   /* n_p2 x IL */
  const uint32_t* p2_out_ctl;         /* n_p2 x OL, multiplicity as a canonical field element */
  const uint32_t* p2_output_indices;  /* n_p2 x OL */
  const uint32_t* p2_mmcs_index_sum_idx; /* n_p2 */
  /* IL x OL = 4 x 2 limbs of four base elements for ext_degree 4 (the D4 width-16 table).  Under ext_degree 5 the
   * table is the compact-D1 one, KOALA_BEAR_D1_W16 on the 5-slot witness bus (poseidon2-circuit-air/src/air.rs:730-763,
   * circuit-prover/src/batch_stark_prover/poseidon2.rs:1244-1285): IL x OL = 16 x 8, one witness per state element,
   * and p2_absorb_len (n_p2, NULL = zeros) is the prefix-free sponge length tag the executor writes into the header
   * (circuit/src/ops/poseidon_perm/executor.rs:720-741).  Since ABI version 4. */
  const uint8_t* p2_absorb_len;
  /* 1: the Recompose table is the "recompose/coeff" variant (NpoTypeId::recompose_with_coeff_lookups, circuit/src/ops/
   * npo.rs:53-60; circuit-prover/src/air/recompose_air.rs:196-226): each coefficient is also a bus tuple
   * (D*coeff_idx, c, 0, ..) with the multiplicity batch_stark_prover/recompose.rs:341-352 computes.  It is what a backend
   * registers when the permutation's degree differs from the circuit's (backend/fri.rs:693-721, :741-852: always under
   * ext_degree 5, where the permutation is the D1 one).  Since ABI version 4. */
  uint32_t recompose_coeff_lookups;
  /* ABI version 5.  n_recompose_coeff x (2 + 2D): the rows of the second Recompose table (then recompose_prep holds
   * the plain kind and recompose_coeff_lookups must be 0).  The batch lists `recompose` before `recompose/coeff`. */
  const uint32_t* recompose_coeff_prep;
  /* ABI version 6.  n_p2w x 48: the ASSEMBLED preprocessed rows of the width-32 table, Poseidon2PreprocessedRow<8, 6>
   * as extract_preprocessed_from_operations + the prover's multiplicity pass leave them (poseidon-circuit-cols/src/
   * preprocessed.rs; witness indices already D-scaled, canonical): 8 x {idx, in_ctl, normal_chain_sel,
   * merkle_chain_sel} | 6 x {idx, out_ctl} | witness idx of mmcs_bit | witness idx of mmcs_bit2 | new_start |
   * merkle_path.  Padding rows are added here (air.rs:613-649). */
  const uint32_t* p2w_prep;
} p3r_layer_desc;

/* Flattened Traces<EF> (circuit/src/tables/mod.rs:49-62), canonical; D = p3r_config.ext_degree. */
typedef struct p3r_traces {
  size_t n_const;     const uint32_t* const_values;     /* n x D (D = p3r_config.ext_degree) */
  size_t n_public;    const uint32_t* public_values;    /* n x D */
  size_t n_alu;       const uint32_t* alu_values;       /* n x 4D: AluTrace.values [a,b,c,out] */
  p3r_p2_rows p2;     /* n = un-padded Poseidon2 row count (any n, padding is done here) */
  size_t n_recompose; const uint32_t* recompose_values; /* n x D */
  size_t n_recompose_coeff; const uint32_t* recompose_coeff_values; /* n x D: rows of the second Recompose table (ABI 5) */
  p3r_p2w_rows p2w;   /* rows of the width-32 Poseidon2 table (ABI 6; n = 0 without one) */
} p3r_traces;

typedef struct p3r_layer p3r_layer;
typedef struct p3r_dtraces p3r_dtraces;

p3r_layer* p3r_layer_create(p3r_ctx* ctx, const p3r_layer_desc* desc, uint32_t* commit_out);
void p3r_layer_free(p3r_ctx* ctx, p3r_layer* layer);
/* Padded heights of [Const, Public, ALU, Poseidon2, Recompose]; 0 = the table is not part of the
 * batch: a non-primitive table with no rows is left out, as `batch_instance_*` returning None does
 * (batch_stark_prover/poseidon2.rs:1089-1092, recompose.rs:77-80). */
int p3r_layer_table_heights(const p3r_layer* layer, size_t heights_out[5]);
/* Padded height of the width-32 Poseidon2 table (ABI version 6); 0 = absent. */
int p3r_layer_p2w_height(const p3r_layer* layer, size_t* height_out);
/* Padded height of the second Recompose table (`recompose/coeff` next to `recompose`, ABI version 5); 0 = absent. */
int p3r_layer_recompose_coeff_height(const p3r_layer* layer, size_t* height_out);
/* 1: the table at position 4 is the `recompose/coeff` kind (p3r_layer_desc.recompose_coeff_lookups, or a circuit whose
 * Recompose ops all carry aux = 1) - the name the proof's metadata gives it. */
int p3r_layer_recompose_kind(const p3r_layer* layer, uint32_t* coeff_lookups_out);
/* The packing the proof was made with: Public / ALU lanes fall back to 1 when the table holds at
 * most the dummy op (reduce_lanes_if_dummy, batch_stark_prover.rs:1305-1318); BatchStarkProof
 * stores this effective packing (:1617-1622). */
int p3r_layer_effective_lanes(const p3r_layer* layer, uint32_t* public_lanes, uint32_t* alu_lanes);

/* Per-proof inputs made resident in HBM once; a prove can then be repeated without PCIe. */
p3r_dtraces* p3r_traces_upload(p3r_ctx* ctx, const p3r_layer* layer, const p3r_traces* traces);
void p3r_traces_free(p3r_ctx* ctx, p3r_dtraces* traces);

int p3r_prove_all_tables(p3r_ctx* ctx, const p3r_layer* layer, const p3r_traces* traces, uint32_t flags,
                         uint8_t* proof_buf, size_t proof_cap, size_t* proof_len);
int p3r_prove_all_tables_resident(p3r_ctx* ctx, const p3r_layer* layer, const p3r_dtraces* traces,
                                  uint32_t flags, uint8_t* proof_buf, size_t proof_cap, size_t* proof_len);
/* K1-K3 only: the main trace of table `table` (0..4; 5 = the second Recompose table) as a device matrix (parity tests). */
p3r_dmat* p3r_layer_build_main_trace(p3r_ctx* ctx, const p3r_layer* layer, const p3r_dtraces* traces,
                                     uint32_t table);

/* ---- verification -------------------------------------------------------------------------------
 * `p3_batch_stark::verify_batch(&config, &airs, &proof, &public_values, &common)` as
 * `BatchStarkProver::verify_all_tables` calls it (circuit-prover/src/batch_stark_prover.rs:1230-1268,
 * 1649-1727), for proofs made with the same p3r_config.  `airs` are the proved tables in instance
 * order, `preprocessed_commitment` the (1 << cap_height) x 8 canonical digests of the
 * CircuitProverData, `degree_bits[i]` the log2 trace height the verifier's preprocessed metadata
 * holds for instance i (CommonData.preprocessed.instances[i].degree_bits): a proof declaring any
 * other degree is rejected as recursion/src/verifier/batch_stark.rs:793 does (InvalidProofShape) -
 * the prover must not choose the domains.  Host code, no device and no p3r_ctx needed.  Returns P3R_OK when the proof
 * is accepted; otherwise an error code and the reason in err_buf (the analogue of
 * BatchStarkProverError::Verify(String)). */
int p3r_verify_batch(const p3r_config* cfg, const p3r_air_desc* airs, size_t n_airs,
                     const uint32_t* preprocessed_commitment, const uint32_t* degree_bits, const uint8_t* proof,
                     size_t proof_len, uint32_t flags, char* err_buf, size_t err_cap);

/* Length of the postcard-encoded `BatchProof` at the head of `bytes` (what p3r_prove_* return; the
 * serialised `BatchStarkProof` continues with its metadata, batch_stark_prover.rs:610-636). */
int p3r_batch_proof_len(uint32_t field, const uint8_t* bytes, size_t len, uint32_t flags, size_t* proof_len,
                        char* err_buf, size_t err_cap);
/* Same for proofs written with a non-default p3r_config.proof_layout (18 bytes, or NULL). */
int p3r_batch_proof_len_layout(uint32_t field, const uint8_t* bytes, size_t len, uint32_t flags,
                               const uint8_t* proof_layout, size_t* proof_len, char* err_buf, size_t err_cap);

/* The whole serialised `BatchStarkProof` (what `to_postcard` / the Rust `postcard::to_allocvec(&proof)` emits):
 * the inner `BatchProof` followed by the metadata fields of batch_stark_prover.rs:610-636 (TablePacking
 * packing.rs:9-27, RowCounts :459-460, NonPrimitiveTableEntry :272-290, SerializedStarkCommon :505-511).
 * p3r_batch_stark_proof_parse walks the bytes once without building containers (framing, every field
 * element in range), decodes the metadata into `out` (field elements canonical) and applies the structural
 * rules a `#[derive(Deserialize)]` bypasses (batch_stark_prover.rs:666-681, packing.rs:140-161).  It is what
 * a parent node of the aggregation tree runs on each child before proving (recursion.rs:656-762 receives the
 * children already deserialised): host code, no device, no p3r_ctx. */
#define P3R_META_MAX_NPO 8
#define P3R_META_MAX_INSTANCES 16
#define P3R_META_MAX_CAP 64
typedef struct p3r_npo_table_entry {
  char op_type[64];        /* NpoTypeId(String), NUL-terminated */
  uint64_t rows;
  uint32_t lanes;
  uint32_t air_variant;    /* 0 Baseline, 1 Optimized */
  uint32_t n_public_values;
  uint32_t public_values[8];
} p3r_npo_table_entry;
typedef struct p3r_batch_stark_meta {
  uint64_t proof_len;      /* length of the inner BatchProof at the head of the bytes */
  uint64_t parse_ns;       /* time this call spent (steady clock): what a parent node pays per child */
  uint32_t public_lanes, alu_lanes, min_trace_height, horner_packed_steps;
  uint32_t n_npo_lanes;    /* TablePacking.npo_lanes: Vec<(NpoTypeId, usize)> */
  struct { char op_type[64]; uint32_t lanes; } npo_lanes[P3R_META_MAX_NPO];
  uint64_t rows[3];        /* RowCounts([const, public, alu]) */
  uint32_t alu_variant, ext_degree;
  uint32_t has_w_binomial, w_binomial, alu_quintic_trinomial;
  uint32_t n_non_primitives;
  p3r_npo_table_entry non_primitives[P3R_META_MAX_NPO];
  uint32_t has_stark_common;
  uint32_t cap_len;        /* digests of the preprocessed commitment */
  uint32_t commitment[8 * P3R_META_MAX_CAP];
  uint32_t n_instances;    /* SerializedStarkCommon.instances (Some entries, in order) */
  uint32_t preprocessed_widths[P3R_META_MAX_INSTANCES];
  uint32_t degree_bits[P3R_META_MAX_INSTANCES];
} p3r_batch_stark_meta;
int p3r_batch_stark_proof_parse(uint32_t field, const uint8_t* bytes, size_t len, uint32_t flags,
                                const uint8_t* proof_layout, p3r_batch_stark_meta* out, char* err_buf,
                                size_t err_cap);

/* ---- the caller side of prove_next_layer: the circuit itself ------------------------------------
 * `prove_next_layer` (recursion/src/recursion.rs:401-502) receives a `Circuit<EF>`, sets its public
 * inputs and the Merkle-sibling private data, RUNS it (`CircuitRunner::run`,
 * circuit/src/tables/runner.rs:195-253) and proves the resulting `Traces`.  The entry points below
 * take the flattened `Circuit<EF>` (circuit/src/circuit.rs:152-181) instead of pre-computed
 * `Traces` + preprocessed columns:
 *   p3r_circuit_create  == Circuit::generate_preprocessed_columns::<4> (circuit.rs:237-510)
 *                          + get_airs_and_degrees_with_prep (circuit-prover/src/common.rs:127-390)
 *                          + poseidon_preprocess_for_prover (batch_stark_prover.rs:97-246)
 *                          + recompose_preprocess_for_op (batch_stark_prover/recompose.rs:294-358)
 *                          + ProverData::from_airs_and_degrees            (build_next_layer_prep)
 *   p3r_circuit_run     == set_public_inputs / set_private_inputs / set_private_data + run()
 *                          (runner.rs:83-253) with the witness table and the Traces kept in HBM
 *   p3r_prove_next_layer== run + prove_all_tables
 * D = 4 (extension-field witnesses), Poseidon2 D4 width 16, Recompose without coefficient lookups:
 * the tables FriRecursionBackend registers (recursion/src/backend/fri.rs:693-721) - and, since ABI version 8, the
 * width-32 Poseidon2 table of a mixed-config verifier circuit (P3R_OP_POSEIDON2_W32_PERM). */
#define P3R_NO_WITNESS 0xFFFFFFFFu

enum p3r_op_kind {               /* circuit/src/ops/op.rs `Op`, AluOpKind */
  P3R_OP_CONST = 0,              /* out; ext[ext_off..+4] = value coefficients (canonical) */
  P3R_OP_PUBLIC = 1,             /* out; aux = public_pos */
  P3R_OP_ALU_ADD = 2,            /* a, b, out                    (c = aux = P3R_NO_WITNESS) */
  P3R_OP_ALU_MUL = 3,
  P3R_OP_ALU_BOOL_CHECK = 4,     /* a, b, out */
  P3R_OP_ALU_MUL_ADD = 5,        /* a, b, c or NO_WITNESS, out; aux = intermediate_out or NO_WITNESS */
  P3R_OP_ALU_HORNER_ACC = 6,     /* a, b, c, out; aux = acc (intermediate_out) */
  P3R_OP_HINT_EXT_DECOMPOSITION = 7,    /* a = input; ext = 4 output witnesses
                                           (circuit/src/builder/circuit_builder.rs:1659-1728) */
  P3R_OP_HINT_BINARY_DECOMPOSITION = 8, /* a = input; ext = ext_len output witnesses (:1750-1810) */
  P3R_OP_POSEIDON2_PERM = 9,     /* a = NonPrimitiveOpId; aux = flags (bit 0 new_start, bit 1 merkle_path);
                                    ext = [in0..in3, mmcs_index_sum, mmcs_bit, n_out (2 or 4), out0..];
                                    empty slots are P3R_NO_WITNESS (poseidon_perm/executor.rs:921-972).
                                    Under ext_degree 1 / 5 the op is a base-mode permutation (KOALA_BEAR_D1_W16 /
                                    BABY_BEAR_D1_W16, one witness per state element, executor.rs:600-700):
                                    ext = [in0..in15, mmcs_index_sum, mmcs_bit, n_out (8 or 16), out0..],
                                    b = absorb_len (the sponge length tag) */
  P3R_OP_RECOMPOSE = 10,         /* a = NonPrimitiveOpId; out; ext = D coefficient witnesses
                                    (circuit/src/ops/recompose.rs:115-170); aux = 0 (or P3R_NO_WITNESS): the `recompose` table,
                                    aux = 1: `recompose/coeff` (NpoTypeId::recompose_with_coeff_lookups,
                                    ops/npo.rs:48-60: every coefficient is a bus tuple too; a coefficient that is a
                                    hint output is created by this row with its read count, any other is named with
                                    multiplicity 0 - batch_stark_prover/recompose.rs:341-352).  A circuit may hold both kinds:
                                    the layer then proves two Recompose tables, `recompose` before `recompose/coeff`
                                    (p3r_layer_desc_counts.n_recompose_coeff). */
  P3R_OP_POSEIDON2_W32_PERM = 11 /* ABI version 8.  A permutation of the width-32 table (`poseidon2_perm/<field>_d4_w32`, the arity-4
                                    compression shape 4 * CAPACITY_EXT == WIDTH_EXT: eight input limbs, rate six, digests of two
                                    limbs) in a D = 4 circuit - the MMCS rows of a verifier circuit built under `--arity4`
                                    (recursion/examples/recursive_aggregation.rs:902-1046; W16 challenger rows stay
                                    P3R_OP_POSEIDON2_PERM).  a = NonPrimitiveOpId; aux = flags (bit 0 new_start, bit 1
                                    merkle_path); ext = [in0..in7, mmcs_index_sum (must be P3R_NO_WITNESS: the arity-4 table has
                                    no index accumulator bus), mmcs_bit, mmcs_bit2, n_out (6 or 8), out0..].  Semantics of
                                    PoseidonPermExecutor::execute for `is_arity4()` (circuit/src/ops/poseidon_perm/
                                    executor.rs:92-235,290-303,493-561,947-966): a sponge row chains the whole previous normal
                                    output and mirrors its own output into the Merkle chain state; a Merkle row places the
                                    previous Merkle-state digest (output limbs 0, 1) into chunk pos = mmcs_bit + 2 * mmcs_bit2,
                                    fills the other three chunks from its private data in ascending order, then overwrites
                                    every limb that names a witness.  Both direction bits are required on a Merkle row.  The
                                    preprocessed rows are Poseidon2PreprocessedRow<8, 6> (executor.rs:777-884: every named input
                                    limb is a bus read, Merkle rows included; the accumulator slots carry the two bit
                                    witnesses, both read). */
};

typedef struct p3r_op {
  uint32_t kind;
  uint32_t a, b, c, out, aux;
  uint32_t ext_off, ext_len; /* slice of p3r_circuit_desc.ext */
} p3r_op;

typedef struct p3r_circuit_desc {
  uint32_t witness_count;
  size_t n_ops;     const p3r_op* ops;                     /* execution order */
  size_t n_ext;     const uint32_t* ext;
  size_t n_public;  const uint32_t* public_rows;           /* witness of public input i */
  size_t n_private; const uint32_t* private_input_rows;
  size_t n_rewrite; const uint32_t* witness_rewrite;       /* pairs (duplicate, canonical) */
  uint32_t public_lanes, alu_lanes, horner_packed_steps, recompose_lanes, min_trace_height;
} p3r_circuit_desc;

typedef struct p3r_circuit_inputs {
  const uint32_t* public_values;   /* n_public x 4, canonical */
  const uint32_t* private_values;  /* n_private x 4 */
  size_t n_private_data;                 /* set_private_data: Poseidon2PermPrivateData { sibling } */
  const uint32_t* private_data_op_ids;   /* n_private_data NonPrimitiveOpIds */
  const uint32_t* private_data_siblings; /* n_private_data x 8: two extension limbs */
  /* ABI version 8.  Private data of P3R_OP_POSEIDON2_W32_PERM Merkle rows: the three sibling digests of an arity-4
   * level, chunk by chunk in ascending chunk order with the running-hash chunk skipped (fill_sibling_data,
   * executor.rs:166-201).  An op id of the other width in either list is an error. */
  size_t n_private_data_w32;
  const uint32_t* private_data_w32_op_ids;   /* n_private_data_w32 NonPrimitiveOpIds */
  const uint32_t* private_data_w32_siblings; /* n_private_data_w32 x 24: three chunks of two extension limbs */
} p3r_circuit_inputs;

typedef struct p3r_circuit p3r_circuit;

/* Fails (NULL + p3r_last_error) on a malformed circuit, an unclaimed private input
 * (circuit.rs:497-503) or an op the three-table backend has no table for. */
p3r_circuit* p3r_circuit_create(p3r_ctx* ctx, const p3r_circuit_desc* desc, uint32_t* commit_out);
void p3r_circuit_free(p3r_ctx* ctx, p3r_circuit* circuit);
/* The CircuitProverData the circuit was prepared into (owned by the circuit). */
const p3r_layer* p3r_circuit_layer(const p3r_circuit* circuit);
/* Op counts of the tables (five, or six with a second Recompose table), i.e. the sizes of the arrays p3r_dtraces_get returns. */
int p3r_circuit_counts(const p3r_circuit* circuit, p3r_layer_desc_counts* out);
/* Levels of the execution schedule (ops of one level have no dependencies on each other). */
int p3r_circuit_levels(const p3r_circuit* circuit, size_t* n_levels);
/* 1: the circuit was prepared on the device (preprocessed columns, ALU lane schedule and execution schedule built
 * in HBM from the uploaded op list); 0: by the host restatement of the same steps (P3R_PREP_HOST=1, or a circuit
 * the device pass handed over).  Both give the same commitment, schedule and proofs. */
int p3r_circuit_prepared_on_device(const p3r_circuit* circuit);

/* CircuitRunner::run on the device.  Errors mirror CircuitError: a witness conflict
 * (runner.rs:473-510), DivisionByZero (:378), a non-boolean mmcs_bit
 * (poseidon_perm/executor.rs:305-335), a witness that is never set (:218-221). */
p3r_dtraces* p3r_circuit_run(p3r_ctx* ctx, const p3r_circuit* circuit, const p3r_circuit_inputs* inputs);
/* run + prove_all_tables in one call.  A CircuitError of the run is what the caller gets (same code
 * and text as p3r_circuit_run), never an error the prover derived from the failed run's traces. */
int p3r_prove_next_layer(p3r_ctx* ctx, const p3r_circuit* circuit, const p3r_circuit_inputs* inputs,
                         uint32_t flags, uint8_t* proof_buf, size_t proof_cap, size_t* proof_len);

/* Inputs made resident in HBM once (set_public_inputs / set_private_inputs / set_private_data with
 * their checks, runner.rs:83-176); a run or a prove can then be repeated without PCIe. */
typedef struct p3r_dinputs p3r_dinputs;
p3r_dinputs* p3r_circuit_inputs_upload(p3r_ctx* ctx, const p3r_circuit* circuit, const p3r_circuit_inputs* inputs);
void p3r_circuit_inputs_free(p3r_ctx* ctx, p3r_dinputs* inputs);
p3r_dtraces* p3r_circuit_run_resident(p3r_ctx* ctx, const p3r_circuit* circuit, const p3r_dinputs* inputs);
int p3r_prove_next_layer_resident(p3r_ctx* ctx, const p3r_circuit* circuit, const p3r_dinputs* inputs,
                                  uint32_t flags, uint8_t* proof_buf, size_t proof_cap, size_t* proof_len);

/* Read back one array of device-resident Traces (canonical), for parity tests / inspection. */
enum p3r_traces_array {
  P3R_TRACES_CONST_VALUES = 0,    /* n_const x 4 */
  P3R_TRACES_PUBLIC_VALUES = 1,   /* n_public x 4 */
  P3R_TRACES_ALU_VALUES = 2,      /* n_alu x 16 */
  P3R_TRACES_P2_INPUT_VALUES = 3, /* n_p2 x 16 */
  P3R_TRACES_P2_FLAGS = 4,        /* n_p2 x 3: new_start, merkle_path, mmcs_bit */
  P3R_TRACES_P2_MMCS_INDEX_SUM = 5, /* n_p2 */
  P3R_TRACES_RECOMPOSE_VALUES = 6, /* n_recompose x D */
  P3R_TRACES_RECOMPOSE_COEFF_VALUES = 7, /* n_recompose_coeff x D: the second Recompose table */
  P3R_TRACES_P2W_INPUT_VALUES = 8,   /* n_p2w x 32 (ABI 8: rows of the width-32 Poseidon2 table) */
  P3R_TRACES_P2W_FLAGS = 9,          /* n_p2w x 4: new_start, merkle_path, mmcs_bit, mmcs_bit2 */
  P3R_TRACES_P2W_MMCS_INDEX_SUM = 10 /* n_p2w */
};
int p3r_dtraces_get(p3r_ctx* ctx, const p3r_layer* layer, const p3r_dtraces* traces, uint32_t which,
                    uint32_t* out, size_t out_len);

/* ---- measurement support (bench.py): run `iters` back-to-back launches of one kernel
 * family on resident data and return the mean per-launch time measured with HIP events
 * on the ctx's own stream. ---- */
int p3r_time_permute_dmat(p3r_ctx* ctx, p3r_dmat* states, int iters, double* ms_per_launch);

/* Per-kernel-family timers: while enabled, every launch of a hot kernel is bracketed by HIP
 * events on the ctx's stream; p3r_profile_read sums them per family since the last enable. */
typedef struct p3r_profile_entry {
  char name[32];
  double total_ms;
  uint64_t launches;
} p3r_profile_entry;
int p3r_profile_enable(p3r_ctx* ctx, int on);
int p3r_profile_read(p3r_ctx* ctx, p3r_profile_entry* out, size_t cap, size_t* n_out);

#ifdef __cplusplus
}
#endif
#endif /* P3R_H */
