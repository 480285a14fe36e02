// The program interpreters of the caller's-AIR seams: the instruction stream air_program.h::air_compile made of a
// p3r_air_insn program, evaluated on every row.
//
//   k_quotient_program   p3r_quotient_program_dmat: the caller's constraints on every row of the quotient domain of resident
//                        LDEs.  The prover's own k_quotient (kernels_stark.hip.h) keeps its constraint systems inlined; this
//                        kernel is the same pass with the constraints as data.
//   k_trace_program      the caller's program on every row of resident TRACES, natural order; what becomes of the values
//                        is its sink's:
//     LogupProgSink      p3r_logup_program_dmat: the fraction columns of the permutation trace and each row's total; the
//                        running sum is k_ef_scan's (kernels_stark.hip.h).  The prover's own k_logup_aux keeps the
//                        interactions of the built-in tables inlined.
//     CheckProgSink      p3r_check_program_dmat: constraints with 0 / 1 selectors - per constraint the smallest row in
//                        which it does not vanish and the number of such rows.
//     RecordSink         p3r_lookup_check_dmat, p3r_lookup_multiplicities_dmat: every term's denominator and multiplicity
//                        as canonical words, for the sort and the sums of tu_air.hip.
//     WitnessSink        p3r_witness_program_dmat: values stored as the columns of a new trace, with the value ops witness
//                        generation needs and constraints must not have (inverse-or-zero, bit fields of the canonical
//                        word, the row index).
//
// Both are one interpreter - air_run, the loop over air_step - with the sinks as a template parameter, as AuxSink /
// QuotSink share air_interactions for the built-in AIRs.
//
// One lane per row: of the quotient domain in storage (bit-reversed) order, of a trace in natural order - either way the
// read of a column at the current row is one contiguous run per wave; the next row's read is the same run bit-reversal
// (or one row) away.  The instruction stream, the column pointers and the constants are read at wave-uniform addresses
// from read-only buffers (scalar loads), and the dispatch is a wave-uniform branch: no lane ever diverges inside the loop.
//
// The slot file is LDS, [slot][word][lane]: word w of a lane is slots[w * kAirLanes + lane], so the 64 lanes of an access
// hit 64 consecutive words - every bank once per 32-lane group, conflict-free - and no register array is indexed by a
// run-time value (which would put it in scratch memory).  A lane touches its own words only: the kernels have no barrier,
// and a lane past the domain's end simply returns.
//
// Workgroup = one wave of 64 lanes.  Nothing is shared between lanes, so a larger workgroup buys nothing and only
// coarsens the LDS a CU hands out.  LDS per workgroup = air_plan's words x 64 lanes x 4 bytes = 256 bytes per live base
// value plus DC x 256 per live extension value, sized by the program (dynamic shared memory): 8 live base values are 2 KiB
// (LDS never limits occupancy), 48 are 12 KiB (13 waves per CU, 3 per SIMD), and the worst program P3R_AIR_MAX_LIVE
// admits, 48 x (5 + 1) words, is 72 KiB (2 waves per CU).  One row per lane: the decode of an instruction is a scalar load
// and a scalar branch issued beside the vector work, and rows-per-lane > 1 would multiply the slot file; it is not built.
#pragma once
#include "air_program.h"
#include "field.h"

namespace p3r {

// What a lane indexes by its chunk: in global memory (as k_quotient's job list is), because a kernel-argument array indexed
// by a lane's value would be copied to scratch memory first.
struct AirChunkTables {
  uint32_t zh[1 << kAirMaxLogChunks], zh_inv[1 << kAirMaxLogChunks];   // AirDomain's
  uint32_t* out[1 << kAirMaxLogChunks];                                // chunk c: [DC][h], natural order
};
// What every interpreter reads: the first member of every argument struct.
struct AirStream {
  const AirDevInsn* insns;         // n_insns of them
  const uint32_t* ext_consts;      // Montgomery, DC words per entry
  const uint32_t* const* cols;     // one pointer per flat column: the rows of a trace in natural order, of an LDE bit-reversed
  uint32_t n_insns;
};
struct AirProgArgs {
  AirStream prog;
  const AirChunkTables* chunks;
  int log_n;                       // log2 of the quotient domain N = h * 2^log_q
  int log_q;
  uint32_t flags;                  // 1: a selector is read (x is needed); 2: is_first_row / is_last_row (the inversions)
  uint32_t shift, w_n, g_inv;      // AirDomain's
  uint32_t alpha[kMaxAirDC];
};

// A lane's slot file: word w is s[w * kAirLanes].
template <class PP, int DC>
struct AirSlots {
  using F = Fp<PP>;
  using E = typename Chal<PP, DC>::type;
  uint32_t* s;
  __device__ __forceinline__ F ld(uint32_t w) const { return F::raw(s[w * kAirLanes]); }
  __device__ __forceinline__ void st(uint32_t w, F v) const { s[w * kAirLanes] = v.v; }
  __device__ __forceinline__ E lde(uint32_t w) const {
    E e;
#pragma unroll
    for (int k = 0; k < DC; ++k) e.c[k] = F::raw(s[(w + k) * kAirLanes]);
    return e;
  }
  __device__ __forceinline__ void ste(uint32_t w, const E& e) const {
#pragma unroll
    for (int k = 0; k < DC; ++k) s[(w + k) * kAirLanes] = e.c[k].v;
  }
};

// read-only buffers at wave-uniform addresses; readfirstlane says so where the compiler cannot see it, so that the
// dispatch is a scalar branch and the slot offsets are scalar
__device__ __forceinline__ AirDevInsn air_fetch(gptr<const AirDevInsn> insns, uint32_t pc) {
  AirDevInsn in;
  in.op = __builtin_amdgcn_readfirstlane(insns[pc].op);
  in.dst = __builtin_amdgcn_readfirstlane(insns[pc].dst);
  in.a = __builtin_amdgcn_readfirstlane(insns[pc].a);
  in.b = __builtin_amdgcn_readfirstlane(insns[pc].b);
  return in;
}

// One instruction of a lane whose current / next rows are j / j_next of every column: the value ops here, the rest
// (selectors, ASSERT_ZERO; lookup terms and column ends) in the sink.
template <class PP, int DC, class Sink>
__device__ __forceinline__ void air_step(const AirDevInsn& in, const AirSlots<PP, DC>& sl, gptr<const uint32_t> ext_consts,
                                         gptr<const uint32_t* const> cols, size_t j, size_t j_next, Sink& sink) {
  using F = Fp<PP>;
  using E = typename Chal<PP, DC>::type;
  uint32_t* s = sl.s;
  switch (in.op) {
    case AIR_D_CONST: sl.st(in.dst, F::raw(in.a)); break;
    case AIR_D_CONST_EXT:
#pragma unroll
      for (int k = 0; k < DC; ++k) s[(in.dst + k) * kAirLanes] = ext_consts[in.a + k];
      break;
    case AIR_D_LOAD: sl.st(in.dst, F::raw(as_global(cols[in.a])[in.b ? j_next : j])); break;
    case AIR_D_LOAD_EXT: {
      const size_t r = in.b ? j_next : j;
#pragma unroll
      for (int k = 0; k < DC; ++k) s[(in.dst + k) * kAirLanes] = as_global(cols[in.a + k])[r];
      break;
    }
    case AIR_D_ADD_BB: sl.st(in.dst, sl.ld(in.a) + sl.ld(in.b)); break;
    case AIR_D_ADD_EE: sl.ste(in.dst, sl.lde(in.a) + sl.lde(in.b)); break;
    case AIR_D_ADD_EB: { E e = sl.lde(in.a); e.c[0] += sl.ld(in.b); sl.ste(in.dst, e); break; }
    case AIR_D_SUB_BB: sl.st(in.dst, sl.ld(in.a) - sl.ld(in.b)); break;
    case AIR_D_SUB_EE: sl.ste(in.dst, sl.lde(in.a) - sl.lde(in.b)); break;
    case AIR_D_SUB_EB: { E e = sl.lde(in.a); e.c[0] -= sl.ld(in.b); sl.ste(in.dst, e); break; }
    case AIR_D_SUB_BE: { E e = -sl.lde(in.b); e.c[0] += sl.ld(in.a); sl.ste(in.dst, e); break; }
    case AIR_D_MUL_BB: sl.st(in.dst, sl.ld(in.a) * sl.ld(in.b)); break;
    case AIR_D_MUL_EE: sl.ste(in.dst, sl.lde(in.a) * sl.lde(in.b)); break;
    case AIR_D_MUL_EB: sl.ste(in.dst, sl.lde(in.a) * sl.ld(in.b)); break;
    case AIR_D_NEG_B: sl.st(in.dst, -sl.ld(in.a)); break;
    case AIR_D_NEG_E: sl.ste(in.dst, -sl.lde(in.a)); break;
    default: sink.step(in, sl); break;
  }
}

// A whole stream over one lane's slots (lane_slots: word 0 of the lane), current / next rows j / j_next, into `sink`.
template <class PP, int DC, class Sink>
__device__ __forceinline__ void air_run(const AirStream& prog, uint32_t* lane_slots, size_t j, size_t j_next, Sink& sink) {
  const AirSlots<PP, DC> sl{lane_slots};
  const gptr<const AirDevInsn> insns = as_global(prog.insns);
  const gptr<const uint32_t> ext_consts = as_global(prog.ext_consts);
  const gptr<const uint32_t* const> cols = as_global(prog.cols);
  for (uint32_t pc = 0; pc < prog.n_insns; ++pc) air_step<PP, DC>(air_fetch(insns, pc), sl, ext_consts, cols, j, j_next, sink);
}

// The selectors of a lane's row.  On the quotient domain they are k_quotient_program's values at the lane's point; on the
// trace domain 0 / 1 by the row (DebugConstraintBuilder's).  The three ops that store them stay case labels of each sink's
// one switch: served from here - by a nested switch, or by a test before the sink's switch - the interpreters of these
// sinks ran 10 to 15 % slower (profiles/r22/program_seams.txt), and a select between the members put them into scratch.
template <class PP, int DC>
struct AirSelectors {
  using F = Fp<PP>;
  F is_first, is_last, is_transition;
  __device__ __forceinline__ void of_trace_row(size_t r, size_t h) {
    is_first = r == 0 ? F::one() : F::zero();
    is_last = r == h - 1 ? F::one() : F::zero();
    is_transition = r == h - 1 ? F::zero() : F::one();
  }
};

// The sinks of a constraint program: the selectors of the lane's point, and the Horner fold of the asserted values.
template <class PP, int DC>
struct QuotProgSink {
  using F = Fp<PP>;
  using E = typename Chal<PP, DC>::type;
  AirSelectors<PP, DC> sel;
  E alpha, acc;
  __device__ __forceinline__ void step(const AirDevInsn& in, const AirSlots<PP, DC>& sl) {
    switch (in.op) {
      case AIR_D_FIRST: sl.st(in.dst, sel.is_first); break;
      case AIR_D_LAST: sl.st(in.dst, sel.is_last); break;
      case AIR_D_TRANS: sl.st(in.dst, sel.is_transition); break;
      case AIR_D_ASSERT_B: acc = acc * alpha; acc.c[0] += sl.ld(in.a); break;
      case AIR_D_ASSERT_E: acc = acc * alpha + sl.lde(in.a); break;
      default: break;   // air_compile emits nothing else for a constraint program
    }
  }
};

template <class PP, int DC>
__global__ void __launch_bounds__(kAirLanes) k_quotient_program(AirProgArgs a) {
  using F = Fp<PP>;
  using E = typename Chal<PP, DC>::type;
  extern __shared__ uint32_t air_slots[];
  const size_t n_rows = size_t(1) << a.log_n;
  const size_t j = (size_t)blockIdx.x * kAirLanes + threadIdx.x;   // storage row
  if (j >= n_rows) return;
  const uint32_t i = bit_reverse((uint32_t)j, a.log_n);            // natural index on the quotient coset
  const uint32_t n_chunks = 1u << a.log_q;
  const uint32_t c = i & (n_chunks - 1);
  const size_t j_next = bit_reverse((uint32_t)((i + n_chunks) & (n_rows - 1)), a.log_n);
  const gptr<const AirChunkTables> chunks = as_global(a.chunks);
  QuotProgSink<PP, DC> sink;
  AirSelectors<PP, DC>& sel = sink.sel;
  sel.is_first = sel.is_last = sel.is_transition = F::zero();
  if (a.flags & 1u) {
    const F x = F::raw(a.shift) * F::raw(a.w_n).pow(i);
    sel.is_transition = x - F::raw(a.g_inv);
    if (a.flags & 2u) {
      // x - 1 and x - w_h^-1 are roots of x^h - 1, which has no zero in the domain (air_domain): one shared inversion
      const F xm1 = x - F::one();
      const F t = (xm1 * sel.is_transition).inv() * F::raw(chunks->zh[c]);
      sel.is_first = t * sel.is_transition;
      sel.is_last = t * xm1;
    }
  }
  sink.acc = E::zero();
#pragma unroll
  for (int k = 0; k < DC; ++k) sink.alpha.c[k] = F::raw(a.alpha[k]);

  air_run<PP, DC>(a.prog, air_slots + threadIdx.x, j, j_next, sink);
  const E quot = sink.acc * F::raw(chunks->zh_inv[c]);
  const size_t h = n_rows >> a.log_q, r = i >> a.log_q;
  uint32_t* out = chunks->out[c];
#pragma unroll
  for (int k = 0; k < DC; ++k) as_global(out)[(size_t)k * h + r] = quot.c[k].v;
}

// A program on the rows of TRACES in natural order, the next row wrapping at the height.  The sink brings its argument
// struct (Args: an AirStream `prog`, `log_h`, and what it writes to), how it starts on a row (init) and what it writes after
// the last instruction (done: the LogUp sink's row total, nothing elsewhere).  A lane past the end returns before its sink
// exists: with h < 64 the check sink's ballots see the active lanes only.
template <class PP, int DC, template <class, int> class Sink>
__global__ void __launch_bounds__(kAirLanes) k_trace_program(typename Sink<PP, DC>::Args a) {
  extern __shared__ uint32_t air_slots[];
  const size_t h = size_t(1) << a.log_h;
  const size_t r = (size_t)blockIdx.x * kAirLanes + threadIdx.x;
  if (r >= h) return;
  Sink<PP, DC> sink;
  sink.init(a, r, h);
  air_run<PP, DC>(a.prog, air_slots + threadIdx.x, r, (r + 1) & (h - 1), sink);
  sink.done(a);
}

// The sinks of a lookup program.  The open column's fraction is kept as num / den in registers: a term m / d does
// num <- num * d + m * den, den <- den * d, and the end of the column the one inversion f = num * den^-1 - one per
// column, not per term.  f goes to words [col * DC + k][row] of the output (consecutive lanes, consecutive words) and
// into the row's total.  A lane whose den is zero - upstream divides by zero there - records its row in *bad_row
// (the smallest wins) and writes zeros; the host refuses the call then (tu_air.hip).
struct AirLogupArgs {
  AirStream prog;
  int log_h;
  uint32_t* out;                   // [DC * (1 + G)][h]: the fraction columns are written here, the first DC by k_ef_scan
  uint32_t* rowsum;                // [DC][h]: sum_g f_g of the row
  uint32_t* bad_row;               // one word, 0xffffffff before the launch: the smallest row with a zero denominator
};
template <class PP, int DC>
struct LogupProgSink {
  using Args = AirLogupArgs;
  using F = Fp<PP>;
  using E = typename Chal<PP, DC>::type;
  gptr<uint32_t> out;
  uint32_t* bad_row;
  size_t h, row;
  E num, den, total;
  __device__ __forceinline__ void init(const Args& a, size_t r, size_t h_) {
    out = as_global(a.out);
    bad_row = a.bad_row;
    h = h_;
    row = r;
    num = total = E::zero();
    den = E::one();
  }
  __device__ __forceinline__ void done(const Args& a) const {
    const gptr<uint32_t> rowsum = as_global(a.rowsum);
#pragma unroll
    for (int k = 0; k < DC; ++k) rowsum[(size_t)k * h + row] = total.c[k].v;
  }
  __device__ __forceinline__ void step(const AirDevInsn& in, const AirSlots<PP, DC>& sl) {
    switch (in.op) {
      case AIR_D_TERM_BB: { const F m = sl.ld(in.a), d = sl.ld(in.b); num = num * d + den * m; den = den * d; break; }
      case AIR_D_TERM_BE: { const F m = sl.ld(in.a); const E d = sl.lde(in.b); num = num * d + den * m; den = den * d; break; }
      case AIR_D_TERM_EB: { const E m = sl.lde(in.a); const F d = sl.ld(in.b); num = num * d + m * den; den = den * d; break; }
      case AIR_D_TERM_EE: { const E m = sl.lde(in.a), d = sl.lde(in.b); num = num * d + m * den; den = den * d; break; }
      case AIR_D_COL_END: {
        E f = E::zero();
        if (den.is_zero()) atomicMin(bad_row, (uint32_t)row);
        else f = num * den.inv();
#pragma unroll
        for (int k = 0; k < DC; ++k) out[((size_t)in.a * DC + k) * h + row] = f.c[k].v;
        total += f;
        num = E::zero();
        den = E::one();
        break;
      }
      default: break;   // air_compile emits nothing else for a lookup program
    }
  }
};

// The sinks of a constraint program on the trace domain (DebugConstraintBuilder): the selectors are 0 / 1 by the lane's
// row, and an asserted value is looked at, not folded.  Every lane of the wave stands at the same ASSERT (the instruction
// stream is wave-uniform), so one ballot of "not zero" over the wave's active lanes says whether any row failed; only then
// does ONE lane - the lowest failing one - add the popcount to the constraint's counter and offer the wave's smallest
// failing row to its first_row.  At most two atomics per wave and constraint, none at all on a satisfying trace.
// The constraint's ordinal is counted here: one ASSERT, one increment, the same in every lane.
struct AirCheckArgs {
  AirStream prog;
  int log_h;
  uint32_t* first_row;             // [n_constraints], 0xffffffff before the launch
  unsigned long long* n_failed;    // [n_constraints], 0 before the launch
};
template <class PP, int DC>
struct CheckProgSink {
  using Args = AirCheckArgs;
  AirSelectors<PP, DC> sel;
  uint32_t* first_row;
  unsigned long long* n_failed;
  uint32_t wave_row;   // the row of the wave's lane 0
  uint32_t k;          // constraints met so far
  __device__ __forceinline__ void init(const Args& a, size_t r, size_t h) {
    sel.of_trace_row(r, h);
    first_row = a.first_row;
    n_failed = a.n_failed;
    wave_row = blockIdx.x * (uint32_t)kAirLanes;
    k = 0;
  }
  __device__ __forceinline__ void done(const Args&) const {}
  __device__ __forceinline__ void vote(bool bad) {
    const uint64_t failing = __ballot(bad);
    if (failing) {
      const uint32_t low = (uint32_t)__ffsll((unsigned long long)failing) - 1u;
      if (threadIdx.x == low) {
        atomicAdd(n_failed + k, (unsigned long long)__popcll(failing));
        atomicMin(first_row + k, wave_row + low);
      }
    }
    ++k;
  }
  __device__ __forceinline__ void step(const AirDevInsn& in, const AirSlots<PP, DC>& sl) {
    switch (in.op) {
      case AIR_D_FIRST: sl.st(in.dst, sel.is_first); break;
      case AIR_D_LAST: sl.st(in.dst, sel.is_last); break;
      case AIR_D_TRANS: sl.st(in.dst, sel.is_transition); break;
      case AIR_D_ASSERT_B: vote(sl.ld(in.a).v != 0); break;
      case AIR_D_ASSERT_E: vote(!sl.lde(in.a).is_zero()); break;
      default: break;   // air_compile emits nothing else for a constraint program
    }
  }
};

// The sinks of a lookup program whose terms are recorded, not summed: term t of row r is slot base + r * n_terms + t of
// the call - the slots of a call are its records in record order (instance, row, term) - and writes the canonical words
// of its denominator and multiplicity, both lifted, to [word][slot], and whether the multiplicity is not zero to
// mark[slot].  Nothing is inverted and a column end does nothing.  The lanes of a wave write n_terms words apart; the
// n_terms writes of a row fill the lines between.  The term's ordinal is counted here, as CheckProgSink counts constraints.
struct AirRecordArgs {
  AirStream prog;
  int log_h;
  uint32_t n_terms;                // LOOKUPs of the program
  uint32_t* den;                   // [DC][n_slots], canonical
  uint32_t* mul;                   // [DC][n_slots], canonical
  uint32_t* mark;                  // [n_slots]
  size_t n_slots;                  // of the whole call
  size_t base;                     // first slot of this instance
};
template <class PP, int DC>
struct RecordSink {
  using Args = AirRecordArgs;
  using E = typename Chal<PP, DC>::type;
  gptr<uint32_t> den, mul, mark;
  size_t n_slots, slot;   // slot: of the row's next term
  __device__ __forceinline__ void init(const Args& a, size_t r, size_t) {
    den = as_global(a.den);
    mul = as_global(a.mul);
    mark = as_global(a.mark);
    n_slots = a.n_slots;
    slot = a.base + r * a.n_terms;
  }
  __device__ __forceinline__ void done(const Args&) const {}
  __device__ __forceinline__ void put(const E& m, const E& d) {
#pragma unroll
    for (int k = 0; k < DC; ++k) {
      den[(size_t)k * n_slots + slot] = d.c[k].to_canonical();
      mul[(size_t)k * n_slots + slot] = m.c[k].to_canonical();
    }
    mark[slot] = m.is_zero() ? 0u : 1u;
    ++slot;
  }
  __device__ __forceinline__ void step(const AirDevInsn& in, const AirSlots<PP, DC>& sl) {
    switch (in.op) {
      case AIR_D_TERM_BB: put(E::from_base(sl.ld(in.a)), E::from_base(sl.ld(in.b))); break;
      case AIR_D_TERM_BE: put(E::from_base(sl.ld(in.a)), sl.lde(in.b)); break;
      case AIR_D_TERM_EB: put(sl.lde(in.a), E::from_base(sl.ld(in.b))); break;
      case AIR_D_TERM_EE: put(sl.lde(in.a), sl.lde(in.b)); break;
      default: break;   // COL_END: the grouping into columns does not matter to the balance
    }
  }
};

// The sinks of a witness program: values become columns.  The selectors are CheckProgSink's 0 / 1.  INV is the field's own
// inverse - Fp::inv is x^(p-2) and the extension inverses multiply by the inverse of a norm, so 0 comes out as 0 with no
// guard: the try_inverse().unwrap_or_default() of an is-zero witness.  BITS leaves Montgomery form (one multiplication
// by 1), shifts and masks the canonical word, and re-enters (one multiplication by R^2); ROW enters the same way (a row is
// below 2^TWO_ADICITY < p).  A STORE writes word out[col * h + row]: the 64 lanes of the wave write 64 consecutive words of
// one column, plain vector stores; air_plan has seen to it that every column below the output's width has one writer.
struct AirWitnessArgs {
  AirStream prog;
  int log_h;
  uint32_t* out;                   // [W][h]: the stored columns
};
template <class PP, int DC>
struct WitnessSink {
  using Args = AirWitnessArgs;
  using F = Fp<PP>;
  using E = typename Chal<PP, DC>::type;
  AirSelectors<PP, DC> sel;
  gptr<uint32_t> out;
  size_t h, row;
  __device__ __forceinline__ void init(const Args& a, size_t r, size_t h_) {
    sel.of_trace_row(r, h_);
    out = as_global(a.out);
    h = h_;
    row = r;
  }
  __device__ __forceinline__ void done(const Args&) const {}
  __device__ __forceinline__ void step(const AirDevInsn& in, const AirSlots<PP, DC>& sl) {
    switch (in.op) {
      case AIR_D_FIRST: sl.st(in.dst, sel.is_first); break;
      case AIR_D_LAST: sl.st(in.dst, sel.is_last); break;
      case AIR_D_TRANS: sl.st(in.dst, sel.is_transition); break;
      case AIR_D_INV_B: sl.st(in.dst, sl.ld(in.a).inv()); break;
      case AIR_D_INV_E: sl.ste(in.dst, sl.lde(in.a).inv()); break;
      case AIR_D_BITS: {
        const uint32_t lo = in.b & 0xffu, n = in.b >> 8;   // 1 <= n, lo + n <= 31 (air_plan)
        sl.st(in.dst, F::from_canonical((sl.ld(in.a).to_canonical() >> lo) & ((1u << n) - 1u)));
        break;
      }
      case AIR_D_ROW: sl.st(in.dst, F::from_canonical((uint32_t)row)); break;
      case AIR_D_STORE_B: out[(size_t)in.b * h + row] = sl.ld(in.a).v; break;
      case AIR_D_STORE_E: {
        const E e = sl.lde(in.a);
#pragma unroll
        for (int k = 0; k < DC; ++k) out[((size_t)in.b + k) * h + row] = e.c[k].v;
        break;
      }
      default: break;   // air_compile emits nothing else for a witness program
    }
  }
};

}  // namespace p3r
