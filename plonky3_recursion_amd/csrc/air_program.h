// The host half of the constraint-program seam (p3r_air_program_info, p3r_quotient_program_dmat; include/p3r.h) and of
// the lookup-program seam (p3r_lookup_program_info, p3r_logup_program_dmat) and of the witness seam
// (p3r_witness_program_info, p3r_witness_program_dmat): what is decided about a caller's p3r_air_insn program before
// anything touches the device.  Host only, no HIP and no context: tu_air.hip turns a plan into a launch,
// tests/air_program_host_main.cpp, tests/lookup_program_host_main.cpp and tests/witness_program_host_main.cpp walk it with
// g++ alone.
//
//   air_plan      validation, typing (base / extension), the degree walk, liveness and the assignment of values to slots;
//                 in AIR_MODE_LOOKUP the sinks are P3R_AIR_LOOKUP / P3R_AIR_LOOKUP_END instead of ASSERT_ZERO, and the
//                 degree reported is that of each auxiliary column's constraint; in AIR_MODE_WITNESS the sink is
//                 P3R_AIR_STORE, the ops INV / BITS / ROW are known, and the output columns must be stored exactly once
//   air_compile   the instruction stream the interpreter reads: operands as LDS word offsets, ops specialised by the
//                 operand types, constants and public values in Montgomery form, challenges in a side table
//   air_domain    the per-chunk constants of the quotient domain: x^h - 1 and its inverse on each of the 2^q cosets
//
// Slots.  A lane of k_quotient_program keeps the live values of its row in LDS, laid out [slot][word][lane].  Base values
// take one word, extension values DC; each kind has a region of its own (extension slots first), so a freed slot fits
// whatever is allocated next in its region and nothing fragments.  The assignment is a linear scan over last uses: the
// operands that die at an instruction are released BEFORE its result is placed (the interpreter reads both operands
// into registers first), lowest free slot first.  A region is as large as the most slots it ever held; the LDS of a
// launch is sized by the program, not by P3R_AIR_MAX_LIVE.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <queue>
#include <vector>

#include "error.h"
#include "field.h"

namespace p3r {

constexpr int kAirLanes = 64;          // lanes of a workgroup of k_quotient_program: one wave (kernels_air.hip.h)
constexpr int kMaxAirDC = 5;           // words of the widest challenge field
constexpr int kAirMaxLogChunks = 4;    // log_quotient_degree the entry takes
// the largest slot file: every slot of both regions in use (P3R_AIR_MAX_LIVE base values at one point, as many extension values at another)
constexpr size_t kAirMaxLdsBytes = (size_t)P3R_AIR_MAX_LIVE * (kMaxAirDC + 1) * kAirLanes * sizeof(uint32_t);
constexpr uint32_t kAirNoSlot = 0xffffffffu;
constexpr size_t kAirUnknownCount = ~size_t(0);   // n_public / n_challenges of p3r_air_program_info: not checked

// What a program's sinks are: the constraints of the quotient seam, the terms and columns of the lookup seam, or the
// stored columns of the witness seam.
enum AirMode { AIR_MODE_CONSTRAINTS, AIR_MODE_LOOKUP, AIR_MODE_WITNESS };

inline bool air_op_is_binary(uint32_t op) { return op == P3R_AIR_ADD || op == P3R_AIR_SUB || op == P3R_AIR_MUL; }
inline bool air_op_known(uint32_t op, AirMode mode = AIR_MODE_CONSTRAINTS) {
  return op == P3R_AIR_CONST || op == P3R_AIR_PUBLIC || (op >= P3R_AIR_CHALLENGE && op <= P3R_AIR_ASSERT_ZERO) ||
         (mode == AIR_MODE_LOOKUP && (op == P3R_AIR_LOOKUP || op == P3R_AIR_LOOKUP_END)) ||
         (mode == AIR_MODE_WITNESS && op >= P3R_AIR_LOOKUP && op <= P3R_AIR_STORE);   // the other seams' sinks: refused by name
}
// an instruction that defines no value
inline bool air_op_is_sink(uint32_t op) {
  return op == P3R_AIR_ASSERT_ZERO || op == P3R_AIR_LOOKUP || op == P3R_AIR_LOOKUP_END || op == P3R_AIR_STORE;
}
// number of value operands
inline int air_op_operands(uint32_t op) {
  return air_op_is_binary(op) || op == P3R_AIR_LOOKUP ? 2
         : (op == P3R_AIR_NEG || op == P3R_AIR_ASSERT_ZERO || op == P3R_AIR_INV || op == P3R_AIR_BITS || op == P3R_AIR_STORE) ? 1 : 0;
}

struct AirPlan {
  p3r_air_info info{};
  p3r_lookup_info lookup{};         // AIR_MODE_LOOKUP
  p3r_witness_info witness{};       // AIR_MODE_WITNESS
  std::vector<uint32_t> column_degree;   // AIR_MODE_LOOKUP: the degree of each closed column's constraint
  std::vector<uint8_t> is_ext;      // per value
  std::vector<uint32_t> slot;       // per value: its slot in the region of its kind; kAirNoSlot for a sink
  std::vector<uint32_t> last_use;   // per value: the last instruction that reads it (its own index: never read)
  uint32_t n_base_slots = 0, n_ext_slots = 0;
  bool uses_x = false;              // a selector: the lane needs its point x
  bool uses_inv = false;            // is_first_row / is_last_row: the two inversions
  // LDS word of a value's first word, and the words of a lane
  uint32_t word_of(size_t v, int dc) const { return is_ext[v] ? slot[v] * (uint32_t)dc : n_ext_slots * (uint32_t)dc + slot[v]; }
  uint32_t words(int dc) const { return n_ext_slots * (uint32_t)dc + n_base_slots; }
  size_t lds_bytes(int dc) const { return (size_t)words(dc) * kAirLanes * sizeof(uint32_t); }
};

inline uint32_t air_log_quotient_degree(uint64_t max_degree) {
  const uint64_t m = std::max<uint64_t>(max_degree, 2) - 1;
  uint32_t l = 0;
  while ((uint64_t(1) << l) < m) ++l;
  return l;
}

// What the lookup seam refuses about the height of its traces: here, so that it is checked without a device.
inline int air_trace_log_height(size_t h, int two_adicity) {
  if (h == 0 || (h & (h - 1))) fail(P3R_EINVAL, "matrix height (%zu) must be a power of two: the traces of a table live on a two-adic domain", h);
  int l = 0;
  while ((size_t(1) << l) < h) ++l;
  if (l > two_adicity) fail(P3R_EINVAL, "2^%d rows exceed the field's two-adicity (%d)", l, two_adicity);
  return l;
}

// Everything that can be refused about a program on its own.  p: the field's modulus; dc: the challenge degree;
// n_public / n_challenges: kAirUnknownCount leaves the indices unchecked; max_live: P3R_AIR_MAX_LIVE.
//
// AIR_MODE_LOOKUP: a LOOKUP (a = multiplicity, b = denominator) adds the term m / d to the open auxiliary column and
// opens one if none is open; LOOKUP_END closes it.  The constraint of a column, f * prod_k d_k - sum_k m_k prod_{l != k} d_l,
// has the degree max(1 + sum_k deg d_k, max_k(deg m_k + sum_{l != k} deg d_l)): kept per open column as the two running
// figures den_deg = sum_k deg d_k and num_deg = max_k(deg m_k + sum_{l != k} deg d_l) over the terms met so far.  A lookup
// program has no constraints of its own and no selectors.
//
// AIR_MODE_WITNESS: a STORE (a = value, b = output column) fills one column with a base value and DC with an extension
// value.  The columns 0 .. W - 1, W one past the highest stored, must each be stored exactly once; a witness program has no
// constraints and no lookups, and degrees mean nothing to it.
inline AirPlan air_plan(const p3r_air_insn* prog, size_t n, const size_t* widths, size_t n_mats, int dc, uint32_t p,
                        size_t n_public, size_t n_challenges, uint32_t max_live, AirMode mode = AIR_MODE_CONSTRAINTS) {
  const bool lookup = mode == AIR_MODE_LOOKUP, witness = mode == AIR_MODE_WITNESS;
  if (n == 0 || !prog)
    fail(P3R_EINVAL, witness ? "the program has no STORE (it is empty)"
                     : lookup ? "the program has no LOOKUP (it is empty)" : "the program has no ASSERT_ZERO (it is empty)");
  if (n > 0x7fffffffu) fail(P3R_EINVAL, "the program is too long");
  if (n_mats && !widths) fail(P3R_EINVAL, "widths is NULL");
  constexpr uint64_t kDegCap = uint64_t(1) << 40;   // saturates: a chain of squarings must not wrap
  AirPlan pl;
  pl.is_ext.assign(n, 0);
  pl.slot.assign(n, kAirNoSlot);
  pl.last_use.resize(n);
  std::vector<uint64_t> deg(n, 0);
  std::vector<uint8_t> is_assert(n, 0);   // a sink: it has no value
  uint64_t max_deg = 0;
  bool column_open = false;
  uint64_t den_deg = 0, num_deg = 0;      // of the open column
  uint32_t column_terms = 0;
  struct Store { uint64_t first, end; size_t insn; };   // output columns [first, end) of a STORE
  std::vector<Store> stores;
  for (size_t i = 0; i < n; ++i) {
    const p3r_air_insn& in = prog[i];
    pl.last_use[i] = (uint32_t)i;
    if (!air_op_known(in.op, mode)) fail(P3R_EINVAL, "instruction %zu: unknown op %u", i, in.op);
    if (lookup && in.op == P3R_AIR_ASSERT_ZERO) fail(P3R_EINVAL, "instruction %zu: ASSERT_ZERO in a lookup program, which has no constraints", i);
    if (lookup && (in.op == P3R_AIR_IS_FIRST_ROW || in.op == P3R_AIR_IS_LAST_ROW || in.op == P3R_AIR_IS_TRANSITION))
      fail(P3R_EINVAL, "instruction %zu: a selector (op %u) in a lookup program: selectors have no value on the trace domain here", i, in.op);
    if (witness && in.op == P3R_AIR_ASSERT_ZERO) fail(P3R_EINVAL, "instruction %zu: ASSERT_ZERO in a witness program, which has no constraints", i);
    if (witness && (in.op == P3R_AIR_LOOKUP || in.op == P3R_AIR_LOOKUP_END))
      fail(P3R_EINVAL, "instruction %zu: %s in a witness program, which has no lookups", i, in.op == P3R_AIR_LOOKUP ? "LOOKUP" : "LOOKUP_END");
    const int n_ops = air_op_operands(in.op);
    const uint32_t ops[2] = {in.a, in.b};
    for (int k = 0; k < n_ops; ++k) {
      if (ops[k] >= i) fail(P3R_EINVAL, "instruction %zu: operand %u is not an earlier value", i, ops[k]);
      if (is_assert[ops[k]])
        fail(P3R_EINVAL, "instruction %zu: operand %u is %s, which has no value", i, ops[k],
             witness ? "a STORE" : lookup ? "a LOOKUP or LOOKUP_END" : "an ASSERT_ZERO");
      pl.last_use[ops[k]] = (uint32_t)i;
    }
    switch (in.op) {
      case P3R_AIR_CONST:
        if (in.a >= p) fail(P3R_EINVAL, "instruction %zu: non-canonical constant %u", i, in.a);
        break;
      case P3R_AIR_PUBLIC:
        if (n_public != kAirUnknownCount && in.a >= n_public) fail(P3R_EINVAL, "instruction %zu: public value %u of %zu", i, in.a, n_public);
        break;
      case P3R_AIR_CHALLENGE:
        if (n_challenges != kAirUnknownCount && in.a >= n_challenges) fail(P3R_EINVAL, "instruction %zu: challenge %u of %zu", i, in.a, n_challenges);
        pl.is_ext[i] = 1;
        break;
      case P3R_AIR_LOCAL: case P3R_AIR_NEXT: case P3R_AIR_LOCAL_EXT: case P3R_AIR_NEXT_EXT: {
        const bool e = in.op == P3R_AIR_LOCAL_EXT || in.op == P3R_AIR_NEXT_EXT;
        if (in.a >= n_mats) fail(P3R_EINVAL, "instruction %zu: matrix %u of %zu", i, in.a, n_mats);
        if ((uint64_t)in.b + (e ? (uint64_t)dc : 1) > widths[in.a])
          fail(P3R_EINVAL, "instruction %zu: column%s %u%s of matrix %u, which has %zu", i, e ? "s" : "", in.b, e ? " .. + DC" : "", in.a, widths[in.a]);
        pl.is_ext[i] = e;
        deg[i] = 1;
        break;
      }
      case P3R_AIR_IS_FIRST_ROW: case P3R_AIR_IS_LAST_ROW:
        pl.uses_x = pl.uses_inv = true;
        deg[i] = 1;
        break;
      case P3R_AIR_IS_TRANSITION:
        pl.uses_x = true;
        break;
      case P3R_AIR_ADD: case P3R_AIR_SUB:
        pl.is_ext[i] = pl.is_ext[in.a] | pl.is_ext[in.b];
        deg[i] = std::max(deg[in.a], deg[in.b]);
        break;
      case P3R_AIR_MUL:
        pl.is_ext[i] = pl.is_ext[in.a] | pl.is_ext[in.b];
        deg[i] = std::min(deg[in.a] + deg[in.b], kDegCap);
        break;
      case P3R_AIR_NEG:
        pl.is_ext[i] = pl.is_ext[in.a];
        deg[i] = deg[in.a];
        break;
      case P3R_AIR_ASSERT_ZERO:
        is_assert[i] = 1;
        ++pl.info.n_constraints;
        max_deg = std::max(max_deg, deg[in.a]);
        break;
      case P3R_AIR_LOOKUP:   // a = m, b = d: every earlier numerator gains d, the new one is m * (the denominators so far)
        is_assert[i] = 1;
        if (!column_open) {   // the first term of a column: the numerator is m alone, the denominator product d
          column_open = true;
          num_deg = deg[in.a];
          den_deg = deg[in.b];
          column_terms = 0;
        } else {
          num_deg = std::min(std::max(num_deg + deg[in.b], deg[in.a] + den_deg), kDegCap);
          den_deg = std::min(den_deg + deg[in.b], kDegCap);
        }
        ++pl.lookup.n_terms;
        pl.lookup.max_terms_per_column = std::max(pl.lookup.max_terms_per_column, ++column_terms);
        break;
      case P3R_AIR_LOOKUP_END: {
        is_assert[i] = 1;
        if (!column_open) fail(P3R_EINVAL, "instruction %zu: LOOKUP_END with no open column", i);
        column_open = false;
        const uint64_t d = std::max(1 + den_deg, num_deg);
        pl.column_degree.push_back((uint32_t)std::min<uint64_t>(d, 0xffffffffu));
        max_deg = std::max(max_deg, d);
        ++pl.lookup.n_columns;
        break;
      }
      case P3R_AIR_INV:
        pl.is_ext[i] = pl.is_ext[in.a];
        ++pl.witness.n_inversions;
        break;
      case P3R_AIR_BITS: {
        const uint32_t lo = in.b & 0xffu, bits = in.b >> 8;
        if (pl.is_ext[in.a]) fail(P3R_EINVAL, "instruction %zu: BITS of an extension value: only a base value has a canonical word", i);
        if (bits == 0 || (uint64_t)lo + bits > 31)
          fail(P3R_EINVAL, "instruction %zu: BITS [%u, %u + %u): at least one bit, and none above bit 30 of the canonical word", i, lo, lo, bits);
        break;
      }
      case P3R_AIR_ROW:
        break;
      case P3R_AIR_STORE: {
        is_assert[i] = 1;
        const uint64_t end = (uint64_t)in.b + (pl.is_ext[in.a] ? (uint64_t)dc : 1);
        if (end > 0x7fffffffu) fail(P3R_EINVAL, "instruction %zu: output column %u: too many output columns", i, in.b);
        stores.push_back({in.b, end, i});
        ++pl.witness.n_stores;
        break;
      }
    }
  }
  if (witness) {
    if (stores.empty()) fail(P3R_EINVAL, "the program has no STORE");
    std::sort(stores.begin(), stores.end(), [](const Store& x, const Store& y) { return x.first != y.first ? x.first < y.first : x.insn < y.insn; });
    uint64_t covered = 0;   // the columns below are stored exactly once
    for (const Store& st : stores) {
      if (st.first < covered)
        fail(P3R_EINVAL, "instruction %zu: output column %llu is stored twice (the columns of an extension value are %d)", st.insn,
             (unsigned long long)st.first, dc);
      if (st.first > covered)
        fail(P3R_EINVAL, "output column %llu is stored by no instruction (the program stores up to column %llu)", (unsigned long long)covered,
             (unsigned long long)stores.back().end - 1);
      covered = st.end;
    }
    pl.witness.n_out_columns = (uint32_t)covered;
  } else if (lookup) {
    if (pl.lookup.n_terms == 0) fail(P3R_EINVAL, "the program has no LOOKUP");
    if (column_open) fail(P3R_EINVAL, "the program ends with a column still open (a LOOKUP_END is missing)");
    pl.lookup.max_constraint_degree = (uint32_t)std::min<uint64_t>(max_deg, 0xffffffffu);
  } else {
    if (pl.info.n_constraints == 0) fail(P3R_EINVAL, "the program has no ASSERT_ZERO");
    pl.info.max_degree = (uint32_t)std::min<uint64_t>(max_deg, 0xffffffffu);
    pl.info.log_quotient_degree = air_log_quotient_degree(max_deg);
  }

  // liveness and slots: a linear scan over last uses, one free list per kind, lowest slot first
  using Heap = std::priority_queue<uint32_t, std::vector<uint32_t>, std::greater<uint32_t>>;
  Heap free_slots[2];
  uint32_t* region[2] = {&pl.n_base_slots, &pl.n_ext_slots};
  uint32_t live = 0, peak = 0;
  auto release = [&](uint32_t v) {
    free_slots[pl.is_ext[v]].push(pl.slot[v]);
    --live;
  };
  for (size_t i = 0; i < n; ++i) {
    const p3r_air_insn& in = prog[i];
    const int n_ops = air_op_operands(in.op);
    if (n_ops >= 1 && pl.last_use[in.a] == i) release(in.a);
    if (n_ops == 2 && in.b != in.a && pl.last_use[in.b] == i) release(in.b);
    if (is_assert[i]) continue;
    const int kind = pl.is_ext[i];
    if (free_slots[kind].empty()) {
      pl.slot[i] = (*region[kind])++;
    } else {
      pl.slot[i] = free_slots[kind].top();
      free_slots[kind].pop();
    }
    peak = std::max(peak, ++live);
    if (pl.last_use[i] == i) release((uint32_t)i);   // never read: its slot is free again at once
  }
  pl.info.peak_live = pl.lookup.peak_live = pl.witness.peak_live = peak;
  if (peak > max_live)
    fail(P3R_EUNSUPPORTED, "the program keeps %u values alive at once; P3R_AIR_MAX_LIVE is %u", peak, max_live);
  return pl;
}

// ---- the interpreter's instruction stream
enum AirDevOp : uint32_t {
  AIR_D_CONST,       // dst <- a (a Montgomery word)
  AIR_D_CONST_EXT,   // dst <- ext_consts[a .. a + DC)
  AIR_D_LOAD,        // dst <- column a at the current (b = 0) / next (b = 1) row
  AIR_D_LOAD_EXT,    // dst <- columns a .. a + DC
  AIR_D_FIRST, AIR_D_LAST, AIR_D_TRANS,
  AIR_D_ADD_BB, AIR_D_ADD_EE, AIR_D_ADD_EB,                 // _EB: a extension, b base
  AIR_D_SUB_BB, AIR_D_SUB_EE, AIR_D_SUB_EB, AIR_D_SUB_BE,   // _BE: a base, b extension
  AIR_D_MUL_BB, AIR_D_MUL_EE, AIR_D_MUL_EB,
  AIR_D_NEG_B, AIR_D_NEG_E,
  AIR_D_ASSERT_B, AIR_D_ASSERT_E,                           // acc <- acc * alpha + a
  // the lookup seam.  A term m / d joins the open column's fraction num / den: num <- num * d + m * den, den <- den * d
  // (a = m, b = d; _BE: m base, d extension).  COL_END: f = num / den goes to the output columns a * DC .. and to the row's total
  AIR_D_TERM_BB, AIR_D_TERM_BE, AIR_D_TERM_EB, AIR_D_TERM_EE,
  AIR_D_COL_END,
  // the witness seam.  INV: dst <- a^-1, 0 for 0.  BITS: dst <- bits [b & 0xff, (b & 0xff) + (b >> 8)) of a's canonical word.
  // ROW: dst <- the lane's row.  STORE: a goes to the output column b (_E: the columns b .. b + DC)
  AIR_D_INV_B, AIR_D_INV_E,
  AIR_D_BITS,
  AIR_D_ROW,
  AIR_D_STORE_B, AIR_D_STORE_E
};
struct AirDevInsn {
  uint32_t op, dst, a, b;   // dst and value operands: LDS words of a lane
};
struct AirCompiled {
  std::vector<AirDevInsn> insns;
  std::vector<uint32_t> ext_consts;   // Montgomery, DC words per challenge the program reads
};

// publics / challenges: canonical and already checked for range.
template <class PP>
inline AirCompiled air_compile(const AirPlan& pl, const p3r_air_insn* prog, size_t n, const size_t* widths, size_t n_mats, int dc,
                               const uint32_t* publics, const uint32_t* challenges) {
  using F = Fp<PP>;
  std::vector<uint32_t> col0(n_mats + 1, 0);   // first flat column of a matrix
  for (size_t m = 0; m < n_mats; ++m) col0[m + 1] = col0[m] + (uint32_t)widths[m];
  AirCompiled out;
  out.insns.reserve(n);
  uint32_t n_closed = 0;   // lookup columns closed so far
  for (size_t i = 0; i < n; ++i) {
    const p3r_air_insn& in = prog[i];
    AirDevInsn d{};
    d.dst = air_op_is_sink(in.op) ? 0 : pl.word_of(i, dc);
    const int n_ops = air_op_operands(in.op);
    const bool ea = n_ops >= 1 && pl.is_ext[in.a], eb = n_ops == 2 && pl.is_ext[in.b];
    uint32_t wa = n_ops >= 1 ? pl.word_of(in.a, dc) : 0, wb = n_ops == 2 ? pl.word_of(in.b, dc) : 0;
    switch (in.op) {
      case P3R_AIR_CONST: d.op = AIR_D_CONST; wa = F::from_canonical(in.a).v; break;
      case P3R_AIR_PUBLIC: d.op = AIR_D_CONST; wa = F::from_canonical(publics[in.a]).v; break;
      case P3R_AIR_CHALLENGE:
        d.op = AIR_D_CONST_EXT;
        wa = (uint32_t)out.ext_consts.size();
        for (int k = 0; k < dc; ++k) out.ext_consts.push_back(F::from_canonical(challenges[(size_t)in.a * dc + k]).v);
        break;
      case P3R_AIR_LOCAL: case P3R_AIR_NEXT: d.op = AIR_D_LOAD; wa = col0[in.a] + in.b; wb = in.op == P3R_AIR_NEXT; break;
      case P3R_AIR_LOCAL_EXT: case P3R_AIR_NEXT_EXT: d.op = AIR_D_LOAD_EXT; wa = col0[in.a] + in.b; wb = in.op == P3R_AIR_NEXT_EXT; break;
      case P3R_AIR_IS_FIRST_ROW: d.op = AIR_D_FIRST; break;
      case P3R_AIR_IS_LAST_ROW: d.op = AIR_D_LAST; break;
      case P3R_AIR_IS_TRANSITION: d.op = AIR_D_TRANS; break;
      case P3R_AIR_ADD:
        d.op = ea && eb ? AIR_D_ADD_EE : ea || eb ? AIR_D_ADD_EB : AIR_D_ADD_BB;
        if (!ea && eb) std::swap(wa, wb);
        break;
      case P3R_AIR_SUB: d.op = ea && eb ? AIR_D_SUB_EE : ea ? AIR_D_SUB_EB : eb ? AIR_D_SUB_BE : AIR_D_SUB_BB; break;
      case P3R_AIR_MUL:
        d.op = ea && eb ? AIR_D_MUL_EE : ea || eb ? AIR_D_MUL_EB : AIR_D_MUL_BB;
        if (!ea && eb) std::swap(wa, wb);
        break;
      case P3R_AIR_NEG: d.op = ea ? AIR_D_NEG_E : AIR_D_NEG_B; break;
      case P3R_AIR_ASSERT_ZERO: d.op = ea ? AIR_D_ASSERT_E : AIR_D_ASSERT_B; break;
      case P3R_AIR_LOOKUP: d.op = ea ? (eb ? AIR_D_TERM_EE : AIR_D_TERM_EB) : (eb ? AIR_D_TERM_BE : AIR_D_TERM_BB); break;
      case P3R_AIR_LOOKUP_END: d.op = AIR_D_COL_END; wa = 1 + n_closed++; break;   // output column 0 is the running sum
      case P3R_AIR_INV: d.op = ea ? AIR_D_INV_E : AIR_D_INV_B; break;
      case P3R_AIR_BITS: d.op = AIR_D_BITS; wb = in.b; break;
      case P3R_AIR_ROW: d.op = AIR_D_ROW; break;
      case P3R_AIR_STORE: d.op = ea ? AIR_D_STORE_E : AIR_D_STORE_B; wb = in.b; break;
    }
    d.a = wa;
    d.b = wb;
    out.insns.push_back(d);
  }
  return out;
}

// ---- the quotient domain: N = h * 2^q points shift * w_N^i; chunk c = i mod 2^q is the coset (shift * w_N^c) * <w_h>,
// on which x^h - 1 is the constant shift^h * w_{2^q}^c - 1 (QuotientArgs::zh / zh_inv of the prover's own kernel).
struct AirDomain {
  uint32_t shift, w_n, g_inv;                       // Montgomery: the shift, w_N, w_h^-1
  uint32_t zh[1 << kAirMaxLogChunks], zh_inv[1 << kAirMaxLogChunks];
};
template <class PP>
inline AirDomain air_domain(uint32_t shift_word, int log_h, int log_q) {
  using F = Fp<PP>;
  if (shift_word >= PP::P) fail(P3R_EINVAL, "coset shift must be a canonical element (0: the field's generator)");
  if (log_q > kAirMaxLogChunks) fail(P3R_EUNSUPPORTED, "log_quotient_degree > %d is not supported", kAirMaxLogChunks);
  if (log_h + log_q > PP::TWO_ADICITY) fail(P3R_EINVAL, "a quotient domain of 2^%d points exceeds the field's two-adicity (%d)", log_h + log_q, PP::TWO_ADICITY);
  const F shift = shift_word ? F::from_canonical(shift_word) : F::generator();
  AirDomain d{};
  d.shift = shift.v;
  d.w_n = F::two_adic_generator(log_h + log_q).v;
  d.g_inv = F::two_adic_generator(log_h).inv().v;
  const F shift_h = shift.pow(uint64_t(1) << log_h), w_c = F::two_adic_generator(log_q);
  for (int c = 0; c < (1 << log_q); ++c) {
    const F zh = shift_h * w_c.pow(c) - F::one();
    if (zh.v == 0)
      fail(P3R_EINVAL, "x^h - 1 has a zero in the quotient domain: shift^h is a 2^%d-th root of unity (chunk %d)", log_q, c);
    d.zh[c] = zh.v;
    d.zh_inv[c] = zh.inv().v;
  }
  return d;
}

}  // namespace p3r
