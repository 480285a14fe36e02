// Poseidon2 width-16 permutation in FP64: the throughput form used by MMCS leaf hashing and the wide 2-to-1 layers (one
// permutation per lane).  The arithmetic also builds on the host (P3R_HD; tools/microbench/host_p2f_check.cpp compares
// it with the integer permutation of poseidon2.h there).
//
// Why FP64 for an integer permutation.  gfx950 issues v_add_f64 / v_mul_f64 / v_fma_f64 at the
// full DP rate (tools/microbench: profiles/r02/op_rates.txt), and an integer-valued double holds
// 53 bits, so the linear layers need NO modular reduction: a field addition is ONE instruction
// instead of three (add, sub, min on a 31-bit modulus in a 32-bit word has one bit of headroom),
// `d*s + sum` with a small integer d is one FMA, and so is `s * 2^-k + sum` for the inverse powers of two of the internal
// diagonal (exact dyadic values, brought back to integers only every few rounds: see the partial rounds below).  Only
// the S-box reduces in the full rounds, and its reduction also absorbs whatever the linear layers accumulated.  Same
// round structure and constants as poseidon2.h; values are exact throughout, so the result is the same field element.
//
// Representation: a state element is a double holding an INTEGER congruent to the CANONICAL value
// (not the Montgomery form: the plain product of two Montgomery forms is not one), of either sign,
// magnitude < 2^53; inside the partial rounds some lanes hold dyadic rationals x / 2^m instead (2^m | P - 1).
// p2f_load / p2f_store convert from / to the Montgomery u32 of field.h.
//
// Exactness (every step below is exact arithmetic, |.| 2^m < 2^53 for a value with denominator 2^m):
//   a * b mod P:    p2f_mulmod_k below: the quotient from a * (b / P), the remainder through P = P_HI + 1 with P_HI a
//                   7-bit (4-bit) multiple of 2^24 (2^27), so q * P_HI is exact; needs |a b| < 2^76; |result| < 0.7 P.
//   x mod P:        p2f_reduce: q = rint(x / P) (as x / P + 1.5 2^52 - 1.5 2^52); r = fma(-q, P, x) is exact because
//                   x - q P is a small integer.  Precondition: x is an INTEGER-valued double (any exact integer below
//                   2^53 qualifies; the magic-number rounding itself holds up to |x / P| < 2^51).  The quotient is off
//                   x / P by at most 1/2 + |x| 2^-53 / P, so |r| <= P / 2 + 1 for every |x| < 2^53.  (The "|x| < 2^51"
//                   stated here before was only a sufficient bound; this is the precondition p2f_partial_walk uses.)
//   x / 2^k:        for 2^k | P - 1 and ANY integer x:  x / 2^k  =  t - frac(t) * P  with t = x * 2^-k
//                   (x = 2^k F + low  =>  x / 2^k = F - low (P-1) / 2^k  mod P,  frac(t) = low / 2^k):
//                   v_mul_f64, v_fract_f64, v_fma_f64.  |result| <= |x| / 2^k + P.  The same fix-up t - frac(t) P
//                   turns any dyadic t with denominator 2^m, 2^m | P - 1, into an integer congruent to it.
//   growth:         the partial rounds' per-lane schedule and its bounds: p2f_lane / p2f_partial_walk below.
#pragma once
#include <utility>

#include "poseidon2.h"

#if defined(__FAST_MATH__) || defined(__FINITE_MATH_ONLY__) && __FINITE_MATH_ONLY__
#error "poseidon2_f64.hip.h relies on exact IEEE-754 double arithmetic (error-free products, magic-number rounding): do not build with -ffast-math / -Ofast"
#endif

namespace p3r {

template <class PP>
struct P2F64 {
  static constexpr double P = (double)PP::P;
  static constexpr double INVP = 1.0 / (double)PP::P;
  // x + MAGIC - MAGIC = x rounded to the nearest integer for |x| < 2^51: two instructions, the first one fused with the
  // product that forms x (v_rndne_f64 is full-rate on gfx950 too - tools/microbench/int_rates - and would be the same
  // count: v_mul_f64 + v_rndne_f64); p2f_mulmod_k never subtracts it back.
  static constexpr double MAGIC = 0x1.8p52;
  // P = P_HI + 1 with P_HI = c * 2^m (127 * 2^24, 15 * 2^27): q * P_HI is an exact double for q < 2^46
  static constexpr double P_HI = (double)(PP::P - 1);
};
#pragma clang fp contract(off)

template <class PP>
P3R_HD double p2f_quot(double x) {
  return __builtin_fma(x, P2F64<PP>::INVP, P2F64<PP>::MAGIC) - P2F64<PP>::MAGIC;
}

// x - floor(x), exact for every double: v_fract_f64 on the device (its clamp below 1.0 never acts on the dyadic
// values of this file, whose fractions are multiples of 2^-27), the same subtraction on the host
P3R_HD double p2f_fract(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_fract(x);
#else
  return x - __builtin_floor(x);
#endif
}

// x mod P, |result| <= 0.5 P (+ rounding slack)
template <class PP>
P3R_HD double p2f_reduce(double x) {
  const double q = p2f_quot<PP>(x);
  return __builtin_fma(-q, P2F64<PP>::P, x);
}
// x * m mod P where m = +-2^-k, 2^k | P - 1
template <class PP>
P3R_HD double p2f_mul_2exp_neg(double x, double m) {
  const double t = x * m;
  const double f = p2f_fract(t);
  return __builtin_fma(-f, P2F64<PP>::P, t);
}
// x * m + a mod P for an INTEGER a: the addend rides in the first FMA, which is exact while |x| + 2^k |a| < 2^53 (the
// value in units of 2^-k; frac(t) is then the fraction of x * 2^-k alone).  |result| < |x| / 2^k + |a| + P.  The only
// caller is the width-32 kernel, with k <= 12: p2wf_partial_walk (poseidon2_w32_f64.hip.h) checks that precondition and
// the fixed value's bound at every round of its schedule.
template <class PP>
P3R_HD double p2f_mul_2exp_neg_add(double x, double m, double a) {
  const double t = __builtin_fma(x, m, a);
  const double f = p2f_fract(t);
  return __builtin_fma(-f, P2F64<PP>::P, t);
}

// a * b mod P given c = b / P (rounded; c is shared by every product with the same b: the S-box multiplies by x twice or
// three times).  Until round 5 in five instructions:
//   q = fma(a, c, MAGIC) - MAGIC = rint(a c);  t = q * P_HI;  e = fma(a, b, -t) = (a b - q P) + q exactly (an integer below
//   2^47, because q * P_HI is exact);  result = e - q.  Needs |a b| < 2^76 (q < 2^46); |result| < 0.7 P.
// Now in FOUR: the rounding constant is never subtracted from the quotient, it rides through the chain and cancels in the
// last step.
//   qm = fma(a, c, MAGIC)            = MAGIC + q exactly, q = rint(a c)                        (|q| < 2^46)
//   t  = fma(qm, P_HI, -MAGIC * P)   = q P_HI - MAGIC exactly: qm P_HI = MAGIC P_HI + q P_HI, and MAGIC P = MAGIC P_HI + MAGIC;
//                                      the result is a multiple of 2^24 below 2^77, 53 significant bits
//   e  = fma(a, b, -t)               = (a b - q P) + q + MAGIC exactly: an integer below 2^47 on top of MAGIC, inside [2^52, 2^53)
//   e - qm                           = a b - q P
// MAGIC P = 3 P 2^51 is a 33-bit constant.  The three constants must sit in registers (one scalar operand per instruction
// on gfx9, no 64-bit literals in the three-address forms): `k` = -MAGIC P in a vector register pair, P_HI and MAGIC in scalar
// ones, pinned by p2f_sbox_consts so that the compiler does not fold them back into literals (see P2FDiag below for what
// that costs).  Two instructions fewer per S-box of degree 3, four per S-box of degree 7.
template <class PP>
struct P2FSboxK {
  double k, p_hi, magic;
};
template <class PP>
P3R_HD P2FSboxK<PP> p2f_sbox_consts() {
  P2FSboxK<PP> K;
  K.k = -(P2F64<PP>::MAGIC * P2F64<PP>::P);
  K.p_hi = P2F64<PP>::P_HI;
  K.magic = P2F64<PP>::MAGIC;
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(K.k), "+s"(K.p_hi), "+s"(K.magic));
#endif
  return K;
}
template <class PP>
P3R_HD double p2f_mulmod_k(double a, double b, double c, const P2FSboxK<PP>& K) {
  const double qm = __builtin_fma(a, c, K.magic);
  const double t = __builtin_fma(qm, K.p_hi, K.k);
  const double e = __builtin_fma(a, b, -t);
  return e - qm;
}

// |x| < 2^38 (p2f_mulmod_k needs |a b| < 2^76).  (Until round 5 there was a second, "wide" form on the two-product
// p2f_mulmod for lanes that arrived unreduced; every caller reduces such lanes first now, which is cheaper.)
template <class PP>
P3R_HD double p2f_sbox(double x, const P2FSboxK<PP>& K) {
  const double c = x * P2F64<PP>::INVP;
  const double x2 = p2f_mulmod_k<PP>(x, x, c, K);
  const double x3 = p2f_mulmod_k<PP>(x2, x, c, K);
  if (PP::SBOX_DEGREE == 3) return x3;
  const double x6 = p2f_mulmod_k<PP>(x3, x3, x3 * P2F64<PP>::INVP, K);
  return p2f_mulmod_k<PP>(x6, x, c, K);
}

P3R_HD void p2f_mat4(double& x0, double& x1, double& x2, double& x3) {
  const double t01 = x0 + x1, t23 = x2 + x3;
  const double t0123 = t01 + t23;
  const double t01123 = t0123 + x1;
  const double t01233 = t0123 + x3;
  const double n3 = __builtin_fma(x0, 2.0, t01233);
  const double n1 = __builtin_fma(x2, 2.0, t01123);
  const double n0 = t01123 + t01;
  const double n2 = t01233 + t23;
  x0 = n0; x1 = n1; x2 = n2; x3 = n3;
}
// |out| <= 35 max|in|
P3R_HD void p2f_external_linear(double* s) {
#pragma unroll
  for (int i = 0; i < P2_WIDTH; i += 4) p2f_mat4(s[i], s[i + 1], s[i + 2], s[i + 3]);
  double sum[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) sum[k] = (s[k] + s[4 + k]) + (s[8 + k] + s[12 + k]);
#pragma unroll
  for (int i = 0; i < P2_WIDTH; ++i) s[i] += sum[i & 3];
}

// ---- partial rounds: the internal diagonal as per-lane forms fixed at compile time
//
// Exact FP64 arithmetic on dyadic rationals (integers times 2^-m) maps onto F_P as a ring homomorphism (1/2 -> 2^-1
// mod P), so a lane multiplied by 2^-k does not have to be brought back to an integer every round: `s * 2^-k + sum` is
// ONE exact FMA, and the fix-up t - frac(t) P (an integer congruent to t: frac(t) P maps to 0) works for any denominator
// 2^m with 2^m | P - 1, m <= 24 (KoalaBear) / 27 (BabyBear).  A lane carries its fraction until the fix-up, which
// runs only when the next round would take it past what stays exact.  Per lane:
//   P2F_SBOX    lane 0, factor -2: the S-box reduces it every round.
//   P2F_INT     a small integer factor: one FMA; reduced (p2f_reduce) before the lane sum of its scheduled rounds.
//   P2F_DYADIC  +-2^-k: one FMA; fixed (p2f_fract + FMA) right after the FMA of its scheduled rounds and of the last one.
//   P2F_WRAP    +-2^-24 (-+2^-27), applied as the INTEGER factor -+127 (-+15): 127 2^24 = P - 1 = -1, so 2^-24 = -127
//               (15 2^27 = P - 1, 2^-27 = -15); one FMA, reduced like an integer lane, every third (fourth) round.
// The lane sum is two partial sums: the integer lanes, and the dyadic ones, whose sum is fixed to an integer (two
// instructions, skipped in a round where no dyadic lane carries a fraction) before the two are added and reduced.
// The schedule (`first`, `every`: the rounds first, first + every, ..; every = 0: first only; first < 0: never) is checked
// by p2f_partial_walk below, step by step, for both fields.  (A runtime form per lane was 2.3 x slower in the width-32
// kernel, poseidon2_w32_f64.hip.h: everything here is resolved at compile time, the partial rounds are unrolled.)
enum P2FForm : int { P2F_SBOX, P2F_INT, P2F_DYADIC, P2F_WRAP };
struct P2FLane {
  int form;
  int d;       // P2F_SBOX / P2F_INT / P2F_WRAP: the integer factor;  P2F_DYADIC: the sign of +-2^-k
  int k;       // P2F_DYADIC: k
  int first, every;
};
// diagonals of poseidon2.h: p2_internal_linear
//  KoalaBear: [-2, 1, 2, 1/2, 3, 4, -1/2, -3, -4, 1/2^8, 1/8, 1/2^24, -1/2^8, -1/8, -1/16, -1/2^24]
//  BabyBear : [-2, 1, 2, 1/2, 3, 4, -1/2, -3, -4, 1/2^8, 1/4, 1/8, 1/2^27, -1/2^8, -1/16, -1/2^27]
template <class PP>
constexpr P2FLane p2f_lane(int i) {
  constexpr P2FLane kb[P2_WIDTH] = {
      {P2F_SBOX, -2, 0, -1, 0}, {P2F_INT, 1, 0, -1, 0},   {P2F_INT, 2, 0, 10, 0},    {P2F_DYADIC, 1, 1, 9, 10},
      {P2F_INT, 3, 0, 9, 0},    {P2F_INT, 4, 0, 6, 8},    {P2F_DYADIC, -1, 1, 9, 10}, {P2F_INT, -3, 0, 10, 0},
      {P2F_INT, -4, 0, 7, 8},   {P2F_DYADIC, 1, 8, 1, 2}, {P2F_DYADIC, 1, 3, 4, 5},   {P2F_WRAP, -127, 0, 1, 3},
      {P2F_DYADIC, -1, 8, 1, 2}, {P2F_DYADIC, -1, 3, 4, 5}, {P2F_DYADIC, -1, 4, 3, 4}, {P2F_WRAP, 127, 0, 1, 3}};
  constexpr P2FLane bb[P2_WIDTH] = {
      {P2F_SBOX, -2, 0, -1, 0}, {P2F_INT, 1, 0, -1, 0},   {P2F_INT, 2, 0, -1, 0},     {P2F_DYADIC, 1, 1, -1, 0},
      {P2F_INT, 3, 0, 6, 0},    {P2F_INT, 4, 0, 6, 0},    {P2F_DYADIC, -1, 1, -1, 0}, {P2F_INT, -3, 0, 7, 0},
      {P2F_INT, -4, 0, 7, 0},   {P2F_DYADIC, 1, 8, 0, 2}, {P2F_DYADIC, 1, 2, 6, 6},   {P2F_DYADIC, 1, 3, 5, 7},
      {P2F_WRAP, -15, 0, 4, 4}, {P2F_DYADIC, -1, 8, 0, 2}, {P2F_DYADIC, -1, 4, 2, 5}, {P2F_WRAP, 15, 0, 4, 4}};
  return PP::FIELD_ID == 0 ? kb[i] : bb[i];
}
// INT / WRAP: reduced before the lane sum of round r;  DYADIC: fixed after its FMA of round r
template <class PP>
constexpr bool p2f_lane_hits(int i, int r) {
  const P2FLane L = p2f_lane<PP>(i);
  if (L.form == P2F_DYADIC && r == PP::PARTIAL_ROUNDS - 1) return true;   // every lane leaves the partial rounds an integer
  if (L.form == P2F_SBOX || L.first < 0 || r < L.first) return false;
  return L.every == 0 ? r == L.first : (r - L.first) % L.every == 0;
}
// an INT / WRAP lane with |d| > 1 that is not reduced before the last round's sum is reduced after the partial rounds
// (the d = 1 lane adds one reduced sum a round: below 2^37 after them, never reduced)
template <class PP>
constexpr bool p2f_lane_reduce_after(int i) {
  const P2FLane L = p2f_lane<PP>(i);
  return (L.form == P2F_INT || L.form == P2F_WRAP) && L.d != 1 && !p2f_lane_hits<PP>(i, PP::PARTIAL_ROUNDS - 1);
}
// a DYADIC lane's denominator exponent at the lane sum of round r (0 for the other lanes)
template <class PP>
constexpr int p2f_lane_denom(int i, int r) {
  const P2FLane L = p2f_lane<PP>(i);
  if (L.form != P2F_DYADIC) return 0;
  int last = -1;
  for (int j = 0; j < r; ++j)
    if (p2f_lane_hits<PP>(i, j)) last = j;
  return L.k * (r - 1 - last);
}
template <class PP>
constexpr int p2f_frac_denom(int r) {
  int m = 0;
  for (int i = 0; i < P2_WIDTH; ++i) m = p2f_lane_denom<PP>(i, r) > m ? p2f_lane_denom<PP>(i, r) : m;
  return m;
}
// the lane's factor as an FP64 value
template <class PP>
constexpr double p2f_lane_factor(int i) {
  const P2FLane L = p2f_lane<PP>(i);
  if (L.form != P2F_DYADIC) return (double)L.d;
  double m = 1.0;
  for (int j = 0; j < L.k; ++j) m *= 0.5;
  return L.d < 0 ? -m : m;
}
constexpr double p2f_abs(double x) { return x < 0 ? -x : x; }
// The factors that are not inline constants of the ISA (3, 127 / 15 and the inverse powers of two below 1/2) are SCALAR
// REGISTER values, one pair per magnitude (the sign is a source modifier).  Written as literals they are only encodable
// in the two-address v_fmac_f64 form, whose addend register is overwritten: every `x * m + sum` then starts with a copy
// of `sum` (v_mov_b64).  From a register the three-address v_fma_f64 takes them.
template <class PP>
constexpr bool p2f_lane_inline(int i) {
  const double a = p2f_abs(p2f_lane_factor<PP>(i));
  return a == 0.5 || a == 1.0 || a == 2.0 || a == 4.0;
}
template <class PP>
constexpr int p2f_lane_rep(int i) {
  for (int j = 0; j < i; ++j)
    if (p2f_abs(p2f_lane_factor<PP>(j)) == p2f_abs(p2f_lane_factor<PP>(i))) return j;
  return i;
}
template <class PP, int I>
P3R_HD void p2f_pin_factor(double* mk) {
  if constexpr (p2f_lane_rep<PP>(I) == I && !p2f_lane_inline<PP>(I)) {
    mk[I] = p2f_abs(p2f_lane_factor<PP>(I));
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+s"(mk[I]));
#endif
  }
}

// ---- the bound walker: every step of the partial rounds on worst-case magnitudes, for the schedule above
//
// Per lane a bound M >= |x| (an integer) and the denominator exponent m (x 2^m is an integer).  What it checks:
//   exactness        every value and every partial sum is exact: M 2^m < 2^53 (a sum of integers is bounded by the sum
//                    of the bounds, so every partial sum of the two lane sums, in any order, is exact too);
//   fix-ups          m <= TWO_ADICITY where a fraction is fixed (2^m | P - 1), and the fixed value M + P < 2^53;
//   S-box domain     |x + rc| < 2^38 at every S-box (p2f_mulmod_k needs |a b| < 2^76), here and in the full rounds after;
//   p2f_reduce       the input is an integer below 2^53 (that is its precondition, see there), the output <= P / 2 + 1;
//   the outputs      < 2^36 after the last full rounds, what p2f_store (< 2^40) and a carried lane's p2f_reduce accept.
// Entry: the full rounds leave |x| <= 35 max |S-box out| = 35 * 0.7 P (p2f_external_linear; p2f_mulmod_k: < 0.7 P).
// Returns 0, or 1000 (round + 1) + 10 lane + what, naming the first step that fails.
template <class PP>
constexpr int p2f_partial_walk() {
  using u64 = unsigned long long;
  constexpr u64 EXACT = u64(1) << 53, SBOX_IN = u64(1) << 38, P = PP::P;
  constexpr u64 SBOX_OUT = (7 * P + 9) / 10, RED = P / 2 + 2;
  u64 M[P2_WIDTH] = {};
  int m[P2_WIDTH] = {};
  for (int i = 0; i < P2_WIDTH; ++i) M[i] = 35 * SBOX_OUT;
  for (int r = 0; r < PP::PARTIAL_ROUNDS; ++r) {
    const int at = 1000 * (r + 1);
    if (M[0] + (P - 1) >= SBOX_IN) return at + 1;
    M[0] = SBOX_OUT;
    for (int i = 0; i < P2_WIDTH; ++i) {
      const P2FLane L = p2f_lane<PP>(i);
      if ((L.form == P2F_INT || L.form == P2F_WRAP) && p2f_lane_hits<PP>(i, r)) {
        if (M[i] >= EXACT) return at + 10 * i + 2;
        M[i] = RED;
      }
    }
    u64 I = 0, F = 0;
    int mF = 0;
    for (int i = 0; i < P2_WIDTH; ++i) {
      if (p2f_lane<PP>(i).form == P2F_DYADIC) {
        F += M[i];
        mF = m[i] > mF ? m[i] : mF;
        if (m[i] != p2f_lane_denom<PP>(i, r)) return at + 10 * i + 3;   // the code's own count of the denominators
      } else {
        I += M[i];
      }
    }
    if (mF != p2f_frac_denom<PP>(r) || mF > PP::TWO_ADICITY) return at + 4;
    if (I >= EXACT || F >= (EXACT >> mF)) return at + 5;
    const u64 Fi = mF > 0 ? F + P : F;
    if (I + Fi >= EXACT) return at + 6;
    const u64 S = RED;
    for (int i = 0; i < P2_WIDTH; ++i) {
      const P2FLane L = p2f_lane<PP>(i);
      if (L.form == P2F_DYADIC) {
        M[i] = ((M[i] + (u64(1) << L.k) - 1) >> L.k) + S;
        m[i] += L.k;
        if (M[i] >= (EXACT >> m[i])) return at + 10 * i + 7;
        if (p2f_lane_hits<PP>(i, r)) {
          if (m[i] > PP::TWO_ADICITY || M[i] + P >= EXACT) return at + 10 * i + 8;
          M[i] += P;
          m[i] = 0;
        }
      } else {
        M[i] = u64(L.d < 0 ? -L.d : L.d) * M[i] + S;
        if (M[i] >= EXACT) return at + 10 * i + 9;
      }
    }
  }
  for (int i = 0; i < P2_WIDTH; ++i) {
    if (p2f_lane_reduce_after<PP>(i)) M[i] = RED;
    if (m[i] != 0 || M[i] + (P - 1) >= SBOX_IN) return 100000 + 10 * i;
  }
  if (35 * SBOX_OUT >= (u64(1) << 36)) return 100001;
  return 0;
}
static_assert(p2f_partial_walk<KoalaBearParams>() == 0, "KoalaBear: the partial-round schedule leaves exact FP64 arithmetic");
static_assert(p2f_partial_walk<BabyBearParams>() == 0, "BabyBear: the partial-round schedule leaves exact FP64 arithmetic");

// the sum of the lanes of one class (DYADIC or not), as a balanced tree: independent adds for the scheduler
struct P2FLaneList {
  int n;
  int lane[P2_WIDTH];
};
template <class PP>
constexpr P2FLaneList p2f_lane_list(bool dyadic) {
  P2FLaneList l = {0, {}};
  for (int i = 0; i < P2_WIDTH; ++i)
    if ((p2f_lane<PP>(i).form == P2F_DYADIC) == dyadic) l.lane[l.n++] = i;
  return l;
}
template <class PP, bool DYADIC>
P3R_HD double p2f_lane_sum(const double* s) {
  constexpr P2FLaneList L = p2f_lane_list<PP>(DYADIC);
  double v[P2_WIDTH];
#pragma unroll
  for (int i = 0; i < L.n; ++i) v[i] = s[L.lane[i]];
#pragma unroll
  for (int w = 1; w < L.n; w *= 2)
#pragma unroll
    for (int i = 0; i + w < L.n; i += 2 * w) v[i] += v[i + w];
  return v[0];
}

template <class PP, int R, int I>
P3R_HD void p2f_lane_reduce(double* s) {
  constexpr P2FLane L = p2f_lane<PP>(I);
  if constexpr ((L.form == P2F_INT || L.form == P2F_WRAP) && p2f_lane_hits<PP>(I, R)) s[I] = p2f_reduce<PP>(s[I]);
}
template <class PP, int I>
P3R_HD void p2f_lane_reduce_last(double* s) {
  if constexpr (p2f_lane_reduce_after<PP>(I)) s[I] = p2f_reduce<PP>(s[I]);
}
template <class PP, int R, int I>
P3R_HD void p2f_lane_diag(double* s, const double* mk, double sum) {
  // (constexpr variables, not calls: a call outside a constant expression is compiled)
  constexpr P2FLane L = p2f_lane<PP>(I);
  constexpr double lit = p2f_lane_factor<PP>(I);
  constexpr bool inl = p2f_lane_inline<PP>(I);
  constexpr int rep = p2f_lane_rep<PP>(I);
  constexpr bool fix = L.form == P2F_DYADIC && p2f_lane_hits<PP>(I, R);
  const double m = inl ? lit : lit < 0 ? -mk[rep] : mk[rep];
  if constexpr (lit == 1.0) {
    s[I] = s[I] + sum;
  } else if constexpr (fix) {
    const double t = __builtin_fma(s[I], m, sum);
    s[I] = __builtin_fma(-p2f_fract(t), P2F64<PP>::P, t);
  } else {
    s[I] = __builtin_fma(s[I], m, sum);
  }
}
template <class PP, int R, int... I>
P3R_HD void p2f_partial_round(double* s, const double* __restrict__ rc, const P2FSboxK<PP>& SK, const double* mk,
                              std::integer_sequence<int, I...>) {
  s[0] = p2f_sbox<PP>(s[0] + rc[R], SK);
  (p2f_lane_reduce<PP, R, I>(s), ...);
  double frac = p2f_lane_sum<PP, true>(s);
  if constexpr (p2f_frac_denom<PP>(R) > 0) frac = __builtin_fma(-p2f_fract(frac), P2F64<PP>::P, frac);
  const double sum = p2f_reduce<PP>(p2f_lane_sum<PP, false>(s) + frac);
  (p2f_lane_diag<PP, R, I>(s, mk, sum), ...);
}
template <class PP, int... R, int... I>
P3R_HD void p2f_partial_rounds(double* s, const double* __restrict__ rc, const P2FSboxK<PP>& SK,
                               std::integer_sequence<int, R...>, std::integer_sequence<int, I...> lanes) {
  double mk[P2_WIDTH];
  (p2f_pin_factor<PP, I>(mk), ...);
  (p2f_partial_round<PP, R>(s, rc, SK, mk, lanes), ...);
  (p2f_lane_reduce_last<PP, I>(s), ...);
}

// `rc`: the flat constant table of poseidon2.h as CANONICAL doubles.
// In: integers in [0, P] (p2f_load: a lazy REDC of one word), except the lanes of CARRIED (bit i = lane i), which may hold the unreduced outputs of
// a previous permutation (< 2^36) and are reduced first: three instructions per carried lane, after which EVERY S-box of
// the first full round is the narrow one (four instructions fewer per lane than the wide form that an unreduced lane,
// spread over the state by the first linear layer, used to force on all sixteen).
// Out: integers of magnitude < 2^36 (35 * 0.7 P), not reduced.
template <class PP, unsigned CARRIED = 0xFFFFu>
P3R_HD void p2f_permute(double* s, const double* __restrict__ rc) {
  const P2FSboxK<PP> SK = p2f_sbox_consts<PP>();
#pragma unroll
  for (int i = 0; i < P2_WIDTH; ++i)
    if (CARRIED >> i & 1u) s[i] = p2f_reduce<PP>(s[i]);
  p2f_external_linear(s);   // |.| <= 35 P: inside the narrow S-box's 2^38 with the round constant added
  int k = 0;
  // (two rounds per iteration: the scalar loads of the second round's constants are in flight while the first one runs)
#pragma unroll 2
  for (int r = 0; r < P2_HALF_FULL; ++r) {
#pragma unroll
    for (int i = 0; i < P2_WIDTH; ++i) s[i] = p2f_sbox<PP>(s[i] + rc[k + i], SK);
    k += P2_WIDTH;
    p2f_external_linear(s);
  }
  // Partial rounds, unrolled, every lane in its compile-time form (p2f_lane): an integer lane is reduced on its schedule
  // and, where it has grown, once after the last round; a dyadic lane is fixed on its schedule and in the last round; so
  // every lane leaves as an integer below 2^37 and every S-box of the last four full rounds is the narrow one
  // (p2f_partial_walk).  KoalaBear: 53.5 FP64 instructions per partial round where the per-round fix-ups took 64 plus
  // 2.25 in amortised reductions; BabyBear: 61.8 where they took 73 plus 2.3.  (Until round 5: 80 instructions.)
  p2f_partial_rounds<PP>(s, rc + k, SK, std::make_integer_sequence<int, PP::PARTIAL_ROUNDS>(),
                         std::make_integer_sequence<int, P2_WIDTH>());
  k += PP::PARTIAL_ROUNDS;
  // (two rounds per iteration: the scalar loads of the second round's constants are in flight while the first one runs)
#pragma unroll 2
  for (int r = 0; r < P2_HALF_FULL; ++r) {
#pragma unroll
    for (int i = 0; i < P2_WIDTH; ++i) s[i] = p2f_sbox<PP>(s[i] + rc[k + i], SK);
    k += P2_WIDTH;
    p2f_external_linear(s);
  }
}

// Montgomery u32 (field.h) -> canonical integer in a double: one REDC, one conversion.
template <class PP>
P3R_HD double p2f_load(uint32_t mont) {
  using F = Fp<PP>;
  return (double)F::reduce64_lazy((uint64_t)mont);
}
// Any state element (|x| < 2^40) -> fully reduced Montgomery u32: x * 2^32 mod P.
template <class PP>
P3R_HD uint32_t p2f_store(double x) {
  const double r = p2f_reduce<PP>(x * 0x1p32);
  const int32_t v = (int32_t)r;
  return (uint32_t)(v + ((v >> 31) & (int32_t)PP::P));
}

#pragma clang fp contract(fast)

}  // namespace p3r
