// gfx950 kernels of the recurrence seam (p3r_affine_scan_dmat; include/p3r.h): the columns s[r + 1] = a[r] s[r] + b[r] of
// resident traces.  Row r is the affine map x -> a[r] x + b[r]; maps compose associatively - but NOT commutatively:
// (a1, b1) then (a2, b2) is (a2 a1, a2 b1 + b2) - so the column is a scan.  Reduce, then scan, as k_ef_scan and
// device_prims.hip.h do it; no workgroup waits for another.
//
//   pass 0   grid (n_tiles, n_recs): the composite map of each tile of kAffTile rows -> agg
//   pass 1   grid (1, n_recs): one workgroup per recurrence composes the tile maps in order and applies them to init: the
//            state entering each tile -> agg, and s[h] -> last
//   pass 2   grid (n_tiles, n_recs): every thread re-reads its rows, takes the state entering its first row from the
//            tile's state and the maps of the threads before it, and steps s <- a s + b, storing before the step
//            (exclusive) or after it (inclusive)
//
// Memory.  Columns are [col][h].  A thread owns kAffItems = 4 CONSECUTIVE rows and moves them as one 16-byte access per
// column word, so a wave reads or writes 1 KiB of contiguous rows per instruction - the widest coalesced access there is -
// and a thread's rows are in scan order without a transposition through the LDS.  Heights below 4 and pointers that are
// not 16-byte aligned take the same code with 4-byte accesses (AffRec::vec == 0).  The block scan keeps the threads' maps
// in the LDS as [word][thread]: thread t touches word k at sh[k][t] and sh[k][t - off], consecutive lanes consecutive
// banks, no conflict.
//
// Forms.  A recurrence runs as one of six instances <D, MUL, ADD>, D = 1 or DC: a pure sum (no MUL) carries only B and
// multiplies nothing, a pure product (no ADD) carries only A, the affine form carries both.  The form is a word of the
// recurrence's descriptor, uniform over the workgroup (the recurrence is blockIdx.y), so one launch serves every form.
#pragma once
#include "field.h"
#include "scan_plan.h"

namespace p3r {

typedef uint32_t aff_u32x4 __attribute__((ext_vector_type(4)));   // four consecutive rows of a column word

// One recurrence of a launch, as the device reads it.
struct AffRec {
  const uint32_t* a;          // first column of a, [D][h]; not read without AFF_MUL
  const uint32_t* b;          // first column of b, [D][h]; not read without AFF_ADD
  uint32_t* out;              // first output column, [D][h]
  uint32_t* agg;              // scratch [3 D][n_tiles]: the tiles' A words, their B words, the state entering each tile
  uint32_t* last;             // [kAffMaxDC]: s[h], zero-padded, Montgomery
  uint32_t init[kAffMaxDC];   // s[0], Montgomery
  uint32_t form;              // AFF_EXT | AFF_MUL | AFF_ADD
  uint32_t inclusive;         // row r holds s[r + 1]
  uint32_t vec;               // 16-byte accesses: h % 4 == 0 and every column 16-byte aligned
};

template <class PP, int D, bool MUL, bool ADD>
struct AffOps {
  using F = Fp<PP>;
  using V = typename CircuitExt<PP, D>::type;
  static constexpr int kWords = (MUL ? D : 0) + (ADD ? D : 0);   // LDS / agg words of a map
  // x -> a x + b.  A member a form does not carry keeps its identity value and costs nothing.
  struct Map {
    V a, b;
  };
  static __device__ __forceinline__ Map identity() {
    Map m;
    m.a = V::one();
    m.b = V::zero();
    return m;
  }
  // `first`, then `then`: the order matters
  static __device__ __forceinline__ Map compose(const Map& first, const Map& then) {
    Map r = first;
    if constexpr (MUL) r.a = then.a * first.a;
    if constexpr (MUL && ADD) r.b = then.a * first.b + then.b;
    else if constexpr (ADD) r.b = first.b + then.b;
    return r;
  }
  static __device__ __forceinline__ V apply(const Map& m, const V& s) {
    if constexpr (MUL && ADD) return m.a * s + m.b;
    else if constexpr (MUL) return m.a * s;
    else return s + m.b;
  }
  // a map in the LDS, [word][thread]
  static __device__ __forceinline__ void put(uint32_t (*sh)[kAffBlock], int t, const Map& m) {
#pragma unroll
    for (int k = 0; k < D; ++k) {
      if constexpr (MUL) sh[k][t] = m.a.c[k].v;
      if constexpr (ADD) sh[(MUL ? D : 0) + k][t] = m.b.c[k].v;
    }
  }
  static __device__ __forceinline__ Map get(uint32_t (*sh)[kAffBlock], int t) {
    Map m = identity();
#pragma unroll
    for (int k = 0; k < D; ++k) {
      if constexpr (MUL) m.a.c[k] = F::raw(sh[k][t]);
      if constexpr (ADD) m.b.c[k] = F::raw(sh[(MUL ? D : 0) + k][t]);
    }
    return m;
  }
  // a tile's map in the scratch, [word][tile]: A in words [0, D), B in [D, 2 D)
  static __device__ __forceinline__ void put_agg(gptr<uint32_t> agg, size_t n_tiles, size_t tile, const Map& m) {
#pragma unroll
    for (int k = 0; k < D; ++k) {
      if constexpr (MUL) agg[(size_t)k * n_tiles + tile] = m.a.c[k].v;
      if constexpr (ADD) agg[(size_t)(D + k) * n_tiles + tile] = m.b.c[k].v;
    }
  }
  static __device__ __forceinline__ Map get_agg(gptr<const uint32_t> agg, size_t n_tiles, size_t tile) {
    Map m = identity();
#pragma unroll
    for (int k = 0; k < D; ++k) {
      if constexpr (MUL) m.a.c[k] = F::raw(agg[(size_t)k * n_tiles + tile]);
      if constexpr (ADD) m.b.c[k] = F::raw(agg[(size_t)(D + k) * n_tiles + tile]);
    }
    return m;
  }

  // rows [i, i + kAffItems) of the D columns at `col`; rows at or past h read as `fill`
  static __device__ __forceinline__ void load_items(gptr<const uint32_t> col, size_t h, size_t i, bool vec, const V& fill, V (&item)[kAffItems]) {
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const gptr<const uint32_t> c = col + (size_t)k * h;
      if (vec && i + kAffItems <= h) {
        const aff_u32x4 w = *reinterpret_cast<gptr<const aff_u32x4>>(c + i);
        item[0].c[k] = F::raw(w.x);
        item[1].c[k] = F::raw(w.y);
        item[2].c[k] = F::raw(w.z);
        item[3].c[k] = F::raw(w.w);
      } else {
#pragma unroll
        for (int q = 0; q < kAffItems; ++q) item[q].c[k] = i + q < h ? F::raw(c[i + q]) : fill.c[k];
      }
    }
  }
  static __device__ __forceinline__ void store_items(gptr<uint32_t> col, size_t h, size_t i, bool vec, const V (&item)[kAffItems]) {
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const gptr<uint32_t> c = col + (size_t)k * h;
      if (vec && i + kAffItems <= h) {
        aff_u32x4 w;
        w.x = item[0].c[k].v;
        w.y = item[1].c[k].v;
        w.z = item[2].c[k].v;
        w.w = item[3].c[k].v;
        *reinterpret_cast<gptr<aff_u32x4>>(c + i) = w;
      } else {
#pragma unroll
        for (int q = 0; q < kAffItems; ++q)
          if (i + q < h) c[i + q] = item[q].c[k].v;
      }
    }
  }
  // the maps of a thread's rows, and their composite in row order.  Rows past h are identities.
  static __device__ __forceinline__ Map load_maps(const AffRec& rec, size_t h, size_t i, Map (&loc)[kAffItems]) {
    V a[kAffItems], b[kAffItems];
    const bool vec = rec.vec != 0;
    if constexpr (MUL) load_items(as_global(rec.a), h, i, vec, V::one(), a);
    if constexpr (ADD) load_items(as_global(rec.b), h, i, vec, V::zero(), b);
    Map run = identity();
#pragma unroll
    for (int q = 0; q < kAffItems; ++q) {
      loc[q] = identity();
      if constexpr (MUL) loc[q].a = a[q];
      if constexpr (ADD) loc[q].b = b[q];
      run = compose(run, loc[q]);
    }
    return run;
  }
  // Inclusive scan of the threads' maps across the workgroup (Hillis-Steele; the earlier map is always `first`).  Returns
  // the composite of the threads BEFORE this one; sh[.][kAffBlock - 1] is then the workgroup's composite.
  static __device__ __forceinline__ Map block_scan(uint32_t (*sh)[kAffBlock], int tid, const Map& run) {
    put(sh, tid, run);
    __syncthreads();
    for (int off = 1; off < kAffBlock; off <<= 1) {
      const bool has = tid >= off;
      Map prev = identity();
      if (has) prev = get(sh, tid - off);
      const Map cur = get(sh, tid);
      __syncthreads();
      if (has) put(sh, tid, compose(prev, cur));
      __syncthreads();
    }
    return tid > 0 ? get(sh, tid - 1) : identity();
  }

  static __device__ __forceinline__ void pass0(const AffRec& rec, size_t h, size_t n_tiles, uint32_t (*sh)[kAffBlock]) {
    const int tid = threadIdx.x;
    const size_t tile = blockIdx.x, i = tile * kAffTile + (size_t)tid * kAffItems;
    Map loc[kAffItems];
    const Map run = load_maps(rec, h, i, loc);
    block_scan(sh, tid, run);
    if (tid == kAffBlock - 1) put_agg(as_global(rec.agg), n_tiles, tile, get(sh, tid));
  }

  static __device__ __forceinline__ void pass1(const AffRec& rec, size_t n_tiles, uint32_t (*sh)[kAffBlock]) {
    const int tid = threadIdx.x;
    const gptr<uint32_t> agg = as_global(rec.agg);
    const gptr<const uint32_t> agg_in = as_global(const_cast<const uint32_t*>(rec.agg));
    // thread t carries the tiles [t per, (t + 1) per)
    const size_t per = (n_tiles + kAffBlock - 1) / kAffBlock;
    const size_t lo = (size_t)tid * per < n_tiles ? (size_t)tid * per : n_tiles, hi = lo + per < n_tiles ? lo + per : n_tiles;
    Map run = identity();
    for (size_t j = lo; j < hi; ++j) run = compose(run, get_agg(agg_in, n_tiles, j));
    const Map before = block_scan(sh, tid, run);
    V s;
#pragma unroll
    for (int k = 0; k < D; ++k) s.c[k] = F::raw(rec.init[k]);
    s = apply(before, s);
    for (size_t j = lo; j < hi; ++j) {
#pragma unroll
      for (int k = 0; k < D; ++k) agg[(size_t)(2 * D + k) * n_tiles + j] = s.c[k].v;
      s = apply(get_agg(agg_in, n_tiles, j), s);
    }
    // the last thread's range ends the column (an empty range: `before` already holds every tile)
    if (tid == kAffBlock - 1) {
      const gptr<uint32_t> last = as_global(rec.last);
#pragma unroll
      for (int k = 0; k < D; ++k) last[k] = s.c[k].v;
#pragma unroll
      for (int k = D; k < kAffMaxDC; ++k) last[k] = 0u;
    }
  }

  static __device__ __forceinline__ void pass2(const AffRec& rec, size_t h, size_t n_tiles, uint32_t (*sh)[kAffBlock]) {
    const int tid = threadIdx.x;
    const size_t tile = blockIdx.x, i = tile * kAffTile + (size_t)tid * kAffItems;
    Map loc[kAffItems];
    const Map run = load_maps(rec, h, i, loc);
    const Map before = block_scan(sh, tid, run);
    const gptr<const uint32_t> agg = as_global(const_cast<const uint32_t*>(rec.agg));
    V s;
#pragma unroll
    for (int k = 0; k < D; ++k) s.c[k] = F::raw(agg[(size_t)(2 * D + k) * n_tiles + tile]);
    s = apply(before, s);
    V o[kAffItems];
    const bool inclusive = rec.inclusive != 0;
#pragma unroll
    for (int q = 0; q < kAffItems; ++q) {
      const V next = apply(loc[q], s);
      o[q] = inclusive ? next : s;
      s = next;
    }
    store_items(as_global(rec.out), h, i, rec.vec != 0, o);
  }

  template <int PASS>
  static __device__ __forceinline__ void run(const AffRec& rec, size_t h, size_t n_tiles, uint32_t (*sh)[kAffBlock]) {
    if constexpr (PASS == 0) pass0(rec, h, n_tiles, sh);
    else if constexpr (PASS == 1) pass1(rec, n_tiles, sh);
    else pass2(rec, h, n_tiles, sh);
  }
};

// One pass of every recurrence of a call.  The form is uniform over a workgroup: no divergence.
template <class PP, int DC, int PASS>
__global__ void __launch_bounds__(kAffBlock) k_affine_scan(const AffRec* __restrict__ recs, size_t h, size_t n_tiles) {
  __shared__ uint32_t sh[2 * DC][kAffBlock];
  const AffRec& rec = recs[blockIdx.y];
  switch (rec.form) {
    case AFF_ADD: AffOps<PP, 1, false, true>::template run<PASS>(rec, h, n_tiles, sh); break;
    case AFF_MUL: AffOps<PP, 1, true, false>::template run<PASS>(rec, h, n_tiles, sh); break;
    case AFF_MUL | AFF_ADD: AffOps<PP, 1, true, true>::template run<PASS>(rec, h, n_tiles, sh); break;
    case AFF_EXT | AFF_ADD: AffOps<PP, DC, false, true>::template run<PASS>(rec, h, n_tiles, sh); break;
    case AFF_EXT | AFF_MUL: AffOps<PP, DC, true, false>::template run<PASS>(rec, h, n_tiles, sh); break;
    case AFF_EXT | AFF_MUL | AFF_ADD: AffOps<PP, DC, true, true>::template run<PASS>(rec, h, n_tiles, sh); break;
    default: break;   // scan_plan admits no other form
  }
}

}  // namespace p3r
