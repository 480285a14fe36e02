// The constraint-program interpreter of the quotient seam (p3r_quotient_program_dmat): the caller's AIR, as the
// instruction stream air_program.h::air_compile made of it, evaluated on every row of the quotient domain of resident
// LDEs.  The prover's own k_quotient (kernels_stark.hip.h) keeps its constraint systems inlined; this kernel is the
// same pass with the constraints as data.
//
// One lane per quotient-domain row, in storage (bit-reversed) order, so that the read of a column at the current row is
// one contiguous run per wave, as in k_quotient; the next row's read is the same run bit-reversal away.  The
// instruction stream, the column pointers and the constants are read at wave-uniform addresses from read-only buffers
// (scalar loads), and the dispatch is a wave-uniform branch: no lane ever diverges inside the loop.
//
// The slot file is LDS, [slot][word][lane]: word w of a lane is slots[w * kAirLanes + lane], so the 64 lanes of an access
// hit 64 consecutive words - every bank once per 32-lane group, conflict-free - and no register array is indexed by a
// run-time value (which would put it in scratch memory).  A lane touches its own words only: the kernel has no barrier,
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
struct AirProgArgs {
  const AirDevInsn* insns;         // n_insns of them
  const uint32_t* ext_consts;      // Montgomery, DC words per entry
  const uint32_t* const* cols;     // one pointer per flat column: H words, bit-reversed rows
  const AirChunkTables* chunks;
  uint32_t n_insns;
  int log_n;                       // log2 of the quotient domain N = h * 2^log_q
  int log_q;
  uint32_t flags;                  // 1: a selector is read (x is needed); 2: is_first_row / is_last_row (the inversions)
  uint32_t shift, w_n, g_inv;      // AirDomain's
  uint32_t alpha[kMaxAirDC];
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
  F is_first = F::zero(), is_last = F::zero(), is_transition = F::zero();
  if (a.flags & 1u) {
    const F x = F::raw(a.shift) * F::raw(a.w_n).pow(i);
    is_transition = x - F::raw(a.g_inv);
    if (a.flags & 2u) {
      // x - 1 and x - w_h^-1 are roots of x^h - 1, which has no zero in the domain (air_domain): one shared inversion
      const F xm1 = x - F::one();
      const F t = (xm1 * is_transition).inv() * F::raw(chunks->zh[c]);
      is_first = t * is_transition;
      is_last = t * xm1;
    }
  }
  E alpha, acc = E::zero();
#pragma unroll
  for (int k = 0; k < DC; ++k) alpha.c[k] = F::raw(a.alpha[k]);

  uint32_t* s = air_slots + threadIdx.x;
  auto ld = [&](uint32_t w) { return F::raw(s[w * kAirLanes]); };
  auto st = [&](uint32_t w, F v) { s[w * kAirLanes] = v.v; };
  auto lde = [&](uint32_t w) {
    E e;
#pragma unroll
    for (int k = 0; k < DC; ++k) e.c[k] = F::raw(s[(w + k) * kAirLanes]);
    return e;
  };
  auto ste = [&](uint32_t w, const E& e) {
#pragma unroll
    for (int k = 0; k < DC; ++k) s[(w + k) * kAirLanes] = e.c[k].v;
  };
  // read-only buffers at wave-uniform addresses; readfirstlane says so where the compiler cannot see it, so that the
  // dispatch is a scalar branch and the slot offsets are scalar
  const gptr<const AirDevInsn> insns = as_global(a.insns);
  const gptr<const uint32_t> ext_consts = as_global(a.ext_consts);
  const gptr<const uint32_t* const> cols = as_global(a.cols);
  for (uint32_t pc = 0; pc < a.n_insns; ++pc) {
    AirDevInsn in;
    in.op = __builtin_amdgcn_readfirstlane(insns[pc].op);
    in.dst = __builtin_amdgcn_readfirstlane(insns[pc].dst);
    in.a = __builtin_amdgcn_readfirstlane(insns[pc].a);
    in.b = __builtin_amdgcn_readfirstlane(insns[pc].b);
    switch (in.op) {
      case AIR_D_CONST: st(in.dst, F::raw(in.a)); break;
      case AIR_D_CONST_EXT:
#pragma unroll
        for (int k = 0; k < DC; ++k) s[(in.dst + k) * kAirLanes] = ext_consts[in.a + k];
        break;
      case AIR_D_LOAD: st(in.dst, F::raw(as_global(cols[in.a])[in.b ? j_next : j])); break;
      case AIR_D_LOAD_EXT: {
        const size_t r = in.b ? j_next : j;
#pragma unroll
        for (int k = 0; k < DC; ++k) s[(in.dst + k) * kAirLanes] = as_global(cols[in.a + k])[r];
        break;
      }
      case AIR_D_FIRST: st(in.dst, is_first); break;
      case AIR_D_LAST: st(in.dst, is_last); break;
      case AIR_D_TRANS: st(in.dst, is_transition); break;
      case AIR_D_ADD_BB: st(in.dst, ld(in.a) + ld(in.b)); break;
      case AIR_D_ADD_EE: ste(in.dst, lde(in.a) + lde(in.b)); break;
      case AIR_D_ADD_EB: { E e = lde(in.a); e.c[0] += ld(in.b); ste(in.dst, e); break; }
      case AIR_D_SUB_BB: st(in.dst, ld(in.a) - ld(in.b)); break;
      case AIR_D_SUB_EE: ste(in.dst, lde(in.a) - lde(in.b)); break;
      case AIR_D_SUB_EB: { E e = lde(in.a); e.c[0] -= ld(in.b); ste(in.dst, e); break; }
      case AIR_D_SUB_BE: { E e = -lde(in.b); e.c[0] += ld(in.a); ste(in.dst, e); break; }
      case AIR_D_MUL_BB: st(in.dst, ld(in.a) * ld(in.b)); break;
      case AIR_D_MUL_EE: ste(in.dst, lde(in.a) * lde(in.b)); break;
      case AIR_D_MUL_EB: ste(in.dst, lde(in.a) * ld(in.b)); break;
      case AIR_D_NEG_B: st(in.dst, -ld(in.a)); break;
      case AIR_D_NEG_E: ste(in.dst, -lde(in.a)); break;
      case AIR_D_ASSERT_B: acc = acc * alpha; acc.c[0] += ld(in.a); break;
      case AIR_D_ASSERT_E: acc = acc * alpha + lde(in.a); break;
      default: break;   // air_compile emits nothing else
    }
  }
  const E quot = acc * F::raw(chunks->zh_inv[c]);
  const size_t h = n_rows >> a.log_q, r = i >> a.log_q;
  uint32_t* out = chunks->out[c];
#pragma unroll
  for (int k = 0; k < DC; ++k) as_global(out)[(size_t)k * h + r] = quot.c[k].v;
}

}  // namespace p3r
