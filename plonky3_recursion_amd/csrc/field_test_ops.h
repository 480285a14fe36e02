// The operations of field.h one at a time, behind one table that the host and the device build share: raw Montgomery
// words in, raw result words out, nothing converted on the way, so that a test decides exactly what an operation sees
// and from_canonical / to_canonical are operations under test like any other.  tests/field_host_main.cpp compiles this
// header with g++ (the host branch of reduce64), tu_field_test.hip runs it one case per lane (the device branch);
// tests/field_cases.py holds the same numbering and the operand layouts.  Not part of the product library.
#pragma once
#include "field.h"

namespace p3r {

// Operand layout (words per case) in the comments: f = one Montgomery word, r = one raw word, e = D words of an element.
enum FieldTestOp : int {
  FT_FP_ADD = 0,            // f f -> f
  FT_FP_SUB = 1,            // f f -> f
  FT_FP_NEG = 2,            // f -> f
  FT_FP_MUL = 3,            // f f -> f
  FT_FP_SQR = 4,            // f -> f
  FT_FP_DBL = 5,            // f -> f
  FT_FP_HALVE = 6,          // f -> f
  FT_FP_DOT2 = 7,           // a1 b1 a2 b2 -> f
  FT_FP_SQR_TIMES = 8,      // a x -> a*a*x
  FT_FP_CUBE = 9,           // f -> f
  FT_FP_REDUCE_LAZY = 10,   // a b -> r: reduce64_lazy(a * b), a value in [0, 2P)
  FT_FP_FROM_CANONICAL = 11,  // r (< P) -> f
  FT_FP_TO_CANONICAL = 12,  // f -> r
  FT_FP_POW = 13,           // f -> f, exponent in aux
  FT_FP_INV = 14,           // f -> f
  FT_FP_TWO_ADIC_GEN = 15,  // r (bits) -> f
  FT_BIT_REVERSE = 16,      // r (x) r (bits) -> r

  FT_FP4_ADD = 32,          // e e -> e
  FT_FP4_SUB = 33,          // e e -> e
  FT_FP4_NEG = 34,          // e -> e
  FT_FP4_MUL = 35,          // e e -> e
  FT_FP4_MUL_BASE = 36,     // e f -> e
  FT_FP4_DOT2_BASE = 37,    // a1 (e) b1 (f) a2 (e) b2 (f) -> e
  FT_FP4_SQR = 38,          // e -> e
  FT_FP4_DBL = 39,          // e -> e
  FT_FP4_HALVE = 40,        // e -> e
  FT_FP4_POW = 41,          // e -> e, exponent in aux
  FT_FP4_NORM = 42,         // e -> n0 n1 d
  FT_FP4_INV_GIVEN = 43,    // e d -> a.inv_given(a.norm(), d)
  FT_FP4_INV = 44,          // e -> e

  FT_FP5_ADD = 64,          // e e -> e
  FT_FP5_SUB = 65,          // e e -> e
  FT_FP5_NEG = 66,          // e -> e
  FT_FP5_MUL = 67,          // e e -> e
  FT_FP5_MUL_BASE = 68,     // e f -> e
  FT_FP5_DOT2_BASE = 69,    // a1 (e) b1 (f) a2 (e) b2 (f) -> e
  FT_FP5_SQR = 70,          // e -> e
  FT_FP5_FROBENIUS1 = 71,   // e -> e
  FT_FP5_FROBENIUS2 = 72,   // e -> e
  FT_FP5_MUL_C0 = 73,       // e e -> f
  FT_FP5_NORM_COFACTOR = 74,  // e -> e
  FT_FP5_POW = 75,          // e -> e, exponent in aux
  FT_FP5_INV = 76,          // e -> e
  FT_FP5_DBL = 77,          // e -> e
  FT_FP5_HALVE = 78,        // e -> e

  FT_FP1_MUL = 96,          // e e -> e
  FT_FP1_INV = 97,          // e -> e
};

// Words a case of `op` reads and writes; false for a number that is no operation.
P3R_HD bool field_test_shape(int op, int* words_in, int* words_out) {
  int wi = 0, wo = 0;
  switch (op) {
    case FT_FP_ADD: case FT_FP_SUB: case FT_FP_MUL: case FT_FP_SQR_TIMES: case FT_FP_REDUCE_LAZY: case FT_BIT_REVERSE:
      wi = 2, wo = 1; break;
    case FT_FP_NEG: case FT_FP_SQR: case FT_FP_DBL: case FT_FP_HALVE: case FT_FP_CUBE: case FT_FP_FROM_CANONICAL:
    case FT_FP_TO_CANONICAL: case FT_FP_POW: case FT_FP_INV: case FT_FP_TWO_ADIC_GEN:
      wi = 1, wo = 1; break;
    case FT_FP_DOT2: wi = 4, wo = 1; break;
    case FT_FP4_ADD: case FT_FP4_SUB: case FT_FP4_MUL: wi = 8, wo = 4; break;
    case FT_FP4_NEG: case FT_FP4_SQR: case FT_FP4_DBL: case FT_FP4_HALVE: case FT_FP4_POW: case FT_FP4_INV: wi = 4, wo = 4; break;
    case FT_FP4_MUL_BASE: case FT_FP4_INV_GIVEN: wi = 5, wo = 4; break;
    case FT_FP4_DOT2_BASE: wi = 10, wo = 4; break;
    case FT_FP4_NORM: wi = 4, wo = 3; break;
    case FT_FP5_ADD: case FT_FP5_SUB: case FT_FP5_MUL: wi = 10, wo = 5; break;
    case FT_FP5_NEG: case FT_FP5_SQR: case FT_FP5_FROBENIUS1: case FT_FP5_FROBENIUS2: case FT_FP5_NORM_COFACTOR:
    case FT_FP5_POW: case FT_FP5_INV: case FT_FP5_DBL: case FT_FP5_HALVE:
      wi = 5, wo = 5; break;
    case FT_FP5_MUL_BASE: wi = 6, wo = 5; break;
    case FT_FP5_DOT2_BASE: wi = 12, wo = 5; break;
    case FT_FP5_MUL_C0: wi = 10, wo = 1; break;
    case FT_FP1_MUL: wi = 2, wo = 1; break;
    case FT_FP1_INV: wi = 1, wo = 1; break;
    default: return false;
  }
  *words_in = wi;
  *words_out = wo;
  return true;
}
// The quintic extension exists over KoalaBear only (kHasQuintic).
P3R_HD bool field_test_is_quintic(int op) { return op >= FT_FP5_ADD && op <= FT_FP5_HALVE; }

template <class E, int D>
P3R_HD E field_test_load(const uint32_t* in) {
  E e;
  for (int i = 0; i < D; ++i) e.c[i].v = in[i];
  return e;
}
template <class E, int D>
P3R_HD void field_test_store(uint32_t* out, const E& e) {
  for (int i = 0; i < D; ++i) out[i] = e.c[i].v;
}

// One case: field_test_shape(op) words from `in`, the result words to `out`.  False (nothing written) for a number that
// is no operation of this field.
template <class PP>
P3R_HD bool field_test_apply(int op, const uint32_t* in, uint32_t* out, uint32_t aux) {
  using F = Fp<PP>;
  using E4 = Fp4<PP>;
  using E1 = Fp1<PP>;
  auto f = [&](int i) { return F::raw(in[i]); };
  auto e4 = [&](int i) { return field_test_load<E4, 4>(in + i); };
  auto put4 = [&](const E4& e) { field_test_store<E4, 4>(out, e); };
  switch (op) {
    case FT_FP_ADD: out[0] = (f(0) + f(1)).v; return true;
    case FT_FP_SUB: out[0] = (f(0) - f(1)).v; return true;
    case FT_FP_NEG: out[0] = (-f(0)).v; return true;
    case FT_FP_MUL: out[0] = (f(0) * f(1)).v; return true;
    case FT_FP_SQR: out[0] = f(0).sqr().v; return true;
    case FT_FP_DBL: out[0] = f(0).dbl().v; return true;
    case FT_FP_HALVE: out[0] = f(0).halve().v; return true;
    case FT_FP_DOT2: out[0] = F::dot2(f(0), f(1), f(2), f(3)).v; return true;
    case FT_FP_SQR_TIMES: out[0] = f(0).sqr_times(f(1)).v; return true;
    case FT_FP_CUBE: out[0] = f(0).cube().v; return true;
    case FT_FP_REDUCE_LAZY: out[0] = F::reduce64_lazy((uint64_t)in[0] * in[1]); return true;
    case FT_FP_FROM_CANONICAL: out[0] = F::from_canonical(in[0]).v; return true;
    case FT_FP_TO_CANONICAL: out[0] = f(0).to_canonical(); return true;
    case FT_FP_POW: out[0] = f(0).pow(aux).v; return true;
    case FT_FP_INV: out[0] = f(0).inv().v; return true;
    case FT_FP_TWO_ADIC_GEN: out[0] = F::two_adic_generator((int)in[0]).v; return true;
    case FT_BIT_REVERSE: out[0] = bit_reverse(in[0], (int)in[1]); return true;

    case FT_FP4_ADD: put4(e4(0) + e4(4)); return true;
    case FT_FP4_SUB: put4(e4(0) - e4(4)); return true;
    case FT_FP4_NEG: put4(-e4(0)); return true;
    case FT_FP4_MUL: put4(e4(0) * e4(4)); return true;
    case FT_FP4_MUL_BASE: put4(e4(0) * f(4)); return true;
    case FT_FP4_DOT2_BASE: put4(E4::dot2_base(e4(0), f(4), e4(5), f(9))); return true;
    case FT_FP4_SQR: put4(e4(0).sqr()); return true;
    case FT_FP4_DBL: put4(e4(0).dbl()); return true;
    case FT_FP4_HALVE: put4(e4(0).halve()); return true;
    case FT_FP4_POW: put4(e4(0).pow(aux)); return true;
    case FT_FP4_NORM: {
      const typename E4::Norm nm = e4(0).norm();
      out[0] = nm.n0.v, out[1] = nm.n1.v, out[2] = nm.d.v;
      return true;
    }
    case FT_FP4_INV_GIVEN: {
      const E4 a = e4(0);
      put4(a.inv_given(a.norm(), f(4)));
      return true;
    }
    case FT_FP4_INV: put4(e4(0).inv()); return true;

    case FT_FP1_MUL: field_test_store<E1, 1>(out, field_test_load<E1, 1>(in) * field_test_load<E1, 1>(in + 1)); return true;
    case FT_FP1_INV: field_test_store<E1, 1>(out, field_test_load<E1, 1>(in).inv()); return true;
    default: break;
  }
  if constexpr (kHasQuintic<PP>) {
    using E5 = Fp5<PP>;
    auto e5 = [&](int i) { return field_test_load<E5, 5>(in + i); };
    auto put5 = [&](const E5& e) { field_test_store<E5, 5>(out, e); };
    switch (op) {
      case FT_FP5_ADD: put5(e5(0) + e5(5)); return true;
      case FT_FP5_SUB: put5(e5(0) - e5(5)); return true;
      case FT_FP5_NEG: put5(-e5(0)); return true;
      case FT_FP5_MUL: put5(e5(0) * e5(5)); return true;
      case FT_FP5_MUL_BASE: put5(e5(0) * f(5)); return true;
      case FT_FP5_DOT2_BASE: put5(E5::dot2_base(e5(0), f(5), e5(6), f(11))); return true;
      case FT_FP5_SQR: put5(e5(0).sqr()); return true;
      case FT_FP5_FROBENIUS1: put5(e5(0).template frobenius<1>()); return true;
      case FT_FP5_FROBENIUS2: put5(e5(0).template frobenius<2>()); return true;
      case FT_FP5_MUL_C0: out[0] = E5::mul_c0(e5(0), e5(5)).v; return true;
      case FT_FP5_NORM_COFACTOR: put5(e5(0).norm_cofactor()); return true;
      case FT_FP5_POW: put5(e5(0).pow(aux)); return true;
      case FT_FP5_INV: put5(e5(0).inv()); return true;
      case FT_FP5_DBL: put5(e5(0).dbl()); return true;
      case FT_FP5_HALVE: put5(e5(0).halve()); return true;
      default: break;
    }
  }
  return false;
}

}  // namespace p3r
