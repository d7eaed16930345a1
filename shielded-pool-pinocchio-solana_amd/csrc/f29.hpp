// f29.hpp -- BN254 field elements in an unsaturated 9 x 29-bit limb form for the MSM / NTT inner loops (host + gfx950).
//
// Fp (bn254.hpp) keeps 8 saturated 32-bit words in memory and re-slices both operands into 29-bit limbs for every
// product (and packs the result back): ~130 of the ~300 instructions of a multiplication are that re-slicing and the
// carry chains of the surrounding add/sub.  F29 stays in the 29-bit form between operations:
//   * value = sum l[k] * 2^(29k); limbs 0..7 are "normalised" when < 2^29, limb 8 carries whatever is left
//     (values here stay below 2^257, so it never exceeds 2^25);
//   * Montgomery radix R' = 2^261 (nine reduction steps of 29 bits): a product of values < 8p reduces to < 1.4 p, so
//     nothing is ever compared against p;
//   * subtraction adds a multiple of p whose limbs are pre-lifted above the subtrahend's (Pm::SUBC_kP_m: k*p with
//     every low limb >= m*(2^29-1)), so limbs never go negative and no borrow chain exists; the carry sweep that
//     brings limbs back under 2^29 is fused into the same pass where the result feeds a squaring;
//   * unsigned 64-bit column sums: 9 * A * B + 9 * 2^58 + carries < 2^64 needs A * B <= 1.5 * 2^60 for the limb
//     bounds A, B of the two operands -- every call site below states its bounds; tests/test_host_cpu.py re-derives
//     them by interval arithmetic (tests/host/f29_bounds.py) and tests/host/field_check.cpp checks the arithmetic
//     against Fp on random and extremal inputs;
//   * a product is written in one of the two forms of F29Form below.  The column form (clear / mac / reduce) is the reference and
//     what every user gets by default; the G1 table walk (msm_table.hpp) takes the product-scanning form, one running sum per product
//     whose carry is the addend of the next column's first multiply-add: 144 64-bit carry adds fewer per mixed addition and 38
//     registers fewer (k_msm_flat<Fq>: 182 -> 144 VGPRs, three waves per SIMD; profiles/f29_scan_accounting.txt).
// Reference behaviour served: the G1/G2 multi-scalar multiplications and NTTs of `sunspot prove`
// (noir_circuit/prove_linux.sh:83, scripts/generate_audit.py:680); the algorithm restated by oracle/c/groth16.c.
#pragma once
#include "bn254.hpp"

// A register the optimiser cannot see through (device builds; nothing on the host): what keeps a running column sum in the order it
// is written -- without it the compiler reassociates a product-scanning product back into separate column sums with carry adds.
#if defined(__HIP_DEVICE_COMPILE__)
#define SPP_OPAQUE(x) asm("" : "+v"(x))
#else
#define SPP_OPAQUE(x) ((void)0)
#endif

namespace spp {

// How a Montgomery product is written (both forms give the same limbs; tests/host/f29_scan_check.cpp):
//   COLUMNS : clear / mac / reduce -- 18 column sums, every reduction step adds its carry into the next column (a 64-bit shift and a
//             64-bit add per column).  The reference form, and the form of every user that has not been measured with another.
//   SCAN    : product scanning, one running sum per product with every accumulate opaque: one chain of multiply-adds per product, no
//             carry add at all.
// The forms that lost (only the carry opaque; two products in lockstep) are at commit f5e9f1a, with their numbers in
// profiles/f29_madd_chain.txt.
enum F29Form : int { F29_COLUMNS = 0, F29_SCAN = 1 };

template <class Pm>
struct F29 {
  uint32_t l[9];
  using Base = Fp<Pm>;
  typedef uint32_t (*ConstFn)(int);
  static constexpr uint32_t M = (1u << 29) - 1u;
  static constexpr uint32_t INV = Pm::INV32 & M;   // -p^-1 mod 2^29
  static SPP_HD constexpr uint32_t P9(int k) { return Base::P9(k); }

  template <ConstFn C>
  static SPP_HD F29 konst() {
    F29 r;
    SPP_UNROLL for (int i = 0; i < 9; i++) r.l[i] = C(i);
    return r;
  }
  // the same integer as 8 x 32-bit words (no domain change); words must be < 2^256
  static SPP_HD F29 from_words(const uint32_t w[8]) {
    F29 r;
    Base::to9(w, r.l);
    return r;
  }
  // normalised limbs, value < 2^256 -> 8 x 32-bit words
  SPP_HD void to_words(uint32_t w[8]) const {
    SPP_UNROLL for (int k = 0; k < 8; k++) {
      const int bit = 32 * k, i = bit / 29, o = bit % 29;
      uint32_t v = l[i] >> o;
      if (i + 1 < 9) v |= l[i + 1] << (29 - o);
      if (i + 2 < 9 && 58 - o < 32) v |= l[i + 2] << (58 - o);
      w[k] = v;
    }
  }
  // carry sweep: limbs 0..7 < 2^29 afterwards, value unchanged (input limbs <= 2^32 - 8: a limb plus the carry from below, <= 7, fits its word)
  SPP_HD F29 norm() const {
    F29 r;
    uint32_t carry = 0;
    SPP_UNROLL for (int k = 0; k < 8; k++) {
      const uint32_t t = l[k] + carry;
      r.l[k] = t & M;
      carry = t >> 29;
    }
    r.l[8] = l[8] + carry;
    return r;
  }

  // ---- column products -----------------------------------------------------------------------------
  static SPP_HD void clear(uint64_t (&c)[18]) {
    SPP_UNROLL for (int k = 0; k < 18; k++) c[k] = 0;
  }
  static SPP_HD void mac(uint64_t (&c)[18], const F29& a, const F29& b) {
    SPP_UNROLL for (int i = 0; i < 9; i++) {
      SPP_UNROLL for (int j = 0; j < 9; j++) c[i + j] += (uint64_t)a.l[i] * b.l[j];
    }
  }
  static SPP_HD void mac_sqr(uint64_t (&c)[18], const F29& a) {   // limbs of a < 2^31 (doubled in 32 bits)
    uint32_t d[9];
    SPP_UNROLL for (int i = 0; i < 9; i++) d[i] = a.l[i] << 1;
    SPP_UNROLL for (int i = 0; i < 9; i++) {
      c[2 * i] += (uint64_t)a.l[i] * a.l[i];
      SPP_UNROLL for (int j = i + 1; j < 9; j++) c[i + j] += (uint64_t)a.l[i] * d[j];
    }
  }
  // Montgomery reduction by R' = 2^261: nine steps clear 29 bits each; result normalised, < columns/R' + p
  static SPP_HD F29 reduce(uint64_t (&c)[18]) {
    SPP_UNROLL for (int k = 0; k < 9; k++) {
      const uint32_t m = ((uint32_t)c[k] * INV) & M;
      SPP_UNROLL for (int j = 0; j < 9; j++) c[k + j] += (uint64_t)m * P9(j);
      c[k + 1] += c[k] >> 29;
    }
    F29 r;
    SPP_UNROLL for (int k = 0; k < 8; k++) {
      r.l[k] = (uint32_t)c[9 + k] & M;
      c[10 + k] += c[9 + k] >> 29;
    }
    r.l[8] = (uint32_t)c[17];
    return r;
  }
  friend SPP_HD F29 operator*(const F29& a, const F29& b) {
    uint64_t c[18];
    clear(c);
    mac(c, a, b);
    return reduce(c);
  }
  SPP_HD F29 sqr() const {
    uint64_t c[18];
    clear(c);
    mac_sqr(c, *this);
    return reduce(c);
  }
  // a*b + c*d with one reduction (limb bounds: 9*(A*B + C*D) + 9*2^58 < 2^64)
  static SPP_HD F29 mul2(const F29& a, const F29& b, const F29& cc, const F29& d) {
    uint64_t c[18];
    clear(c);
    mac(c, a, b);
    mac(c, cc, d);
    return reduce(c);
  }

  // ---- product scanning ------------------------------------------------------------------------------
  // One running 64-bit sum per product: column k takes its a_i * b_(k-i), then its m_i * p_(k-i), then (k < 9) m_k and m_k * p_0;
  // shifted down 29 bits it is the carry into column k + 1 -- the addend of that column's first multiply-add, where reduce() spends a
  // shift and an add.  Every column total is the integer reduce() reaches in c[k], so the limbs are the same and the bound on a
  // column (partial sums of unsigned terms never exceed the total) is the one tests/host/f29_bounds.py certifies.  Every accumulate
  // is opaque.
  struct Scan {
    uint64_t acc = 0;
    uint32_t m[9];
    F29 r;
    SPP_HD void fma(uint32_t x, uint32_t y) {
      acc += (uint64_t)x * y;
      SPP_OPAQUE(acc);
    }
    SPP_HD void ab(int k, int i, const F29& a, const F29& b) {
      const int j = k - i;
      if (j >= 0 && j < 9) fma(a.l[i], b.l[j]);
    }
    SPP_HD void sq(int k, int i, const F29& a, const uint32_t (&d)[9]) {   // d = the limbs of a doubled (limbs of a < 2^31)
      const int j = k - i;
      if (j == i) fma(a.l[i], a.l[i]);
      else if (j > i && j < 9) fma(a.l[i], d[j]);
    }
    SPP_HD void mp(int k, int i) {
      const int j = k - i;
      if (i < k && j >= 0 && j < 9) fma(m[i], P9(j));
    }
    SPP_HD void end(int k) {
      if (k < 9) {
        m[k] = ((uint32_t)acc * INV) & M;
        fma(m[k], P9(0));
      } else {
        r.l[k - 9] = (uint32_t)acc & M;
      }
      acc >>= 29;
      SPP_OPAQUE(acc);
      if (k == 16) r.l[8] = (uint32_t)acc;
    }
  };
  // sum of NP products, one reduction (limb bounds as for mac + reduce: 9 * sum A_t * B_t + 9 * 2^58 < 2^64)
  template <int NP>
  static SPP_HD F29 dot_scan(const F29* const (&a)[NP], const F29* const (&b)[NP]) {
    Scan s;
    SPP_UNROLL for (int k = 0; k < 17; k++) {
      SPP_UNROLL for (int t = 0; t < NP; t++) {
        SPP_UNROLL for (int i = 0; i < 9; i++) s.ab(k, i, *a[t], *b[t]);
      }
      SPP_UNROLL for (int i = 0; i < 9; i++) s.mp(k, i);
      s.end(k);
    }
    return s.r;
  }
  SPP_HD F29 sqr_scan() const {
    uint32_t d[9];
    SPP_UNROLL for (int i = 0; i < 9; i++) d[i] = l[i] << 1;
    Scan s;
    SPP_UNROLL for (int k = 0; k < 17; k++) {
      SPP_UNROLL for (int i = 0; i < 9; i++) s.sq(k, i, *this, d);
      SPP_UNROLL for (int i = 0; i < 9; i++) s.mp(k, i);
      s.end(k);
    }
    return s.r;
  }
  // the products by form (F29Form): what the accumulators below call.  dot_as and sqr_as are the only places that branch on the form.
  // sum of NP products, one reduction
  template <int FORM, int NP>
  static SPP_HD F29 dot_as(const F29* const (&a)[NP], const F29* const (&b)[NP]) {
    if constexpr (FORM == F29_COLUMNS) {
      uint64_t c[18];
      clear(c);
      SPP_UNROLL for (int t = 0; t < NP; t++) mac(c, *a[t], *b[t]);
      return reduce(c);
    } else return dot_scan<NP>(a, b);
  }
  template <int FORM>
  SPP_HD F29 sqr_as() const {
    if constexpr (FORM == F29_COLUMNS) return sqr();
    else return sqr_scan();
  }
  template <int FORM>
  static SPP_HD F29 mul_as(const F29& a, const F29& b) {
    return dot_as<FORM, 1>({&a}, {&b});
  }
  template <int FORM>
  static SPP_HD F29 mul2_as(const F29& a, const F29& b, const F29& cc, const F29& d) {
    return dot_as<FORM, 2>({&a, &cc}, {&b, &d});
  }

  // ---- additive operations (C = lifted multiple of p; see gen_consts.py `lifted`) ---------------------
  // a - b + C, limbs left as they fall (each < a + C)
  template <ConstFn C>
  static SPP_HD F29 sub_lazy(const F29& a, const F29& b) {
    F29 r;
    SPP_UNROLL for (int k = 0; k < 9; k++) r.l[k] = a.l[k] + (C(k) - b.l[k]);
    return r;
  }
  template <ConstFn C>
  static SPP_HD F29 neg_lazy(const F29& b) {
    F29 r;
    SPP_UNROLL for (int k = 0; k < 9; k++) r.l[k] = C(k) - b.l[k];
    return r;
  }
  // a - b + C with the carry sweep fused in
  template <ConstFn C>
  static SPP_HD F29 sub_norm(const F29& a, const F29& b) {
    F29 r;
    uint32_t carry = 0;
    SPP_UNROLL for (int k = 0; k < 8; k++) {
      const uint32_t t = a.l[k] - b.l[k] + C(k) + carry;
      r.l[k] = t & M;
      carry = t >> 29;
    }
    r.l[8] = a.l[8] - b.l[8] + C(8) + carry;
    return r;
  }
  // a - b - 2c + C, normalised
  template <ConstFn C>
  static SPP_HD F29 sub3_norm(const F29& a, const F29& b, const F29& c2) {
    F29 r;
    uint32_t carry = 0;
    SPP_UNROLL for (int k = 0; k < 8; k++) {
      const uint32_t t = a.l[k] - b.l[k] - (c2.l[k] << 1) + C(k) + carry;
      r.l[k] = t & M;
      carry = t >> 29;
    }
    r.l[8] = a.l[8] - b.l[8] - (c2.l[8] << 1) + C(8) + carry;
    return r;
  }
  friend SPP_HD F29 add_lazy(const F29& a, const F29& b) {
    F29 r;
    SPP_UNROLL for (int k = 0; k < 9; k++) r.l[k] = a.l[k] + b.l[k];
    return r;
  }
  friend SPP_HD F29 add_norm(const F29& a, const F29& b) {
    F29 r;
    uint32_t carry = 0;
    SPP_UNROLL for (int k = 0; k < 8; k++) {
      const uint32_t t = a.l[k] + b.l[k] + carry;
      r.l[k] = t & M;
      carry = t >> 29;
    }
    r.l[8] = a.l[8] + b.l[8] + carry;
    return r;
  }

  // normalised value == k*p for some 0 <= k <= KMAX ?  The normalised form is unique, so this is a limb comparison.  The low limb
  // of k*p is k * P9(0) mod 2^29 and p is odd, so the low limb times p^-1 mod 2^29 is the only k whose multiple is left to compare:
  // one multiplication both filters (all but ~KMAX/2^29 of the non-zero cases leave here) and names the candidate.
  template <uint32_t KMAX>
  SPP_HD bool is_zero_mod_p() const {
    const uint32_t kk = (l[0] * Pm::PINV29) & M;
    if (kk > KMAX) return false;
    uint32_t diff = 0, carry = 0;
    SPP_UNROLL for (int i = 0; i < 8; i++) {
      const uint32_t t = kk * P9(i) + carry;     // KMAX * 2^29 < 2^32
      diff |= l[i] ^ (t & M);
      carry = t >> 29;
    }
    diff |= l[8] ^ (kk * P9(8) + carry);
    return diff == 0;
  }

  // ---- domain changes ---------------------------------------------------------------------------------
  // Fp (x*R, words) -> x*R'
  static SPP_HD F29 from_fp(const Base& a) { return from_words(a.l) * konst<Pm::K29_IN>(); }
  // x*R' (value < 8p) -> Fp in [0, 2p)
  SPP_HD Base to_fp() const {
    uint32_t w[8];
    SPP_UNROLL for (int i = 0; i < 8; i++) w[i] = Pm::ONE(i);
    const F29 t = *this * from_words(w);   // x*R' * R / R' = x*R, < 1.05 p
    Base r;
    t.to_words(r.l);
    return r;
  }
  // zz*R'^2/R (the scaled domain of XYZZ29::ZZ/ZZZ) -> Fp
  SPP_HD Base scaled_to_fp() const {
    const F29 t = *this * konst<Pm::K29_ZZ_OUT>();
    Base r;
    t.to_words(r.l);
    return r;
  }
};

// --------------------------------------------------------------------------------------------------------------
// XYZZ accumulator over F29 for "acc += table point" (mixed addition, 8M + 2S with 9 reductions).
//   X, Y      : x*R', y*R'                     (X normalised < 5.1 p, Y < 1.2 p)
//   ZZ, ZZZ   : zz*R'^2/R, zzz*R'^2/R          (< 1.1 p): a table coordinate x2*R (plain Fp words, < 2p) times ZZ
//               gives x2*zz*R' directly, so the table stays in the Fp format every other kernel uses.
// Limb/value bounds per line are in the comments (A x B = limb bounds of the two mul operands, in units of 2^29).
// FORM (F29Form): how the nine products of the addition are written; the values, and so the bounds, are those of F29_COLUMNS.
// --------------------------------------------------------------------------------------------------------------
template <class Pm, int FORM = F29_COLUMNS>
struct XYZZ29 {
  using F = F29<Pm>;
  using B = Fp<Pm>;
  F X, Y, ZZ, ZZZ;
  bool inf;

  static SPP_HD XYZZ29 infinity() {
    XYZZ29 r;
    SPP_UNROLL for (int i = 0; i < 9; i++) r.X.l[i] = r.Y.l[i] = r.ZZ.l[i] = r.ZZZ.l[i] = 0;
    r.inf = true;
    return r;
  }
  SPP_HD XYZZ<B> to_xyzz() const {
    if (inf) return XYZZ<B>::infinity();
    return {X.to_fp(), Y.to_fp(), ZZ.scaled_to_fp(), ZZZ.scaled_to_fp()};
  }
  static SPP_HD XYZZ29 from_xyzz(const XYZZ<B>& q) {
    XYZZ29 r;
    r.inf = q.is_inf();
    r.X = F::from_fp(q.X);
    r.Y = F::from_fp(q.Y);
    // zz*R -> zz*R' -> zz*R'^2/R (K29_IN as a plain factor); rare path (doubling fallback)
    r.ZZ = F::from_fp(q.ZZ) * F::template konst<Pm::K29_IN>();
    r.ZZZ = F::from_fp(q.ZZZ) * F::template konst<Pm::K29_IN>();
    return r;
  }

  // this += (x2, +-y2); e = table entry (Fp words, not infinity)
  SPP_HD void madd(const Affine<B>& e, bool negate) { madd_any<false>(e, negate); }
  // The same addition for a loop that keeps the same-x case out of its body (k_msm_flat): when the entry has the accumulator's x
  // -- the doubling or the cancellation, which need e = +-(the accumulated point) -- nothing is added, the accumulator keeps every
  // limb and the result is false; the caller sums that slice again with madd.  Every other case runs the statements of madd (one
  // body, madd_any), so the lazy bounds and their certificates (tests/host/f29_bounds.py) are those of madd.
  SPP_HD bool madd_distinct(const Affine<B>& e, bool negate) { return madd_any<true>(e, negate); }
  template <bool DISTINCT>
  SPP_HD bool madd_any(const Affine<B>& e, bool negate) {
    F x2 = F::from_words(e.x.l);                                         // limbs < 1, value < 2p
    F y2 = F::from_words(e.y.l);
    if (negate) y2 = F::template neg_lazy<Pm::SUBC_4P_1>(y2);            // limbs < 2 (2^30), value <= 4p
    if (inf) {
      X = x2 * F::template konst<Pm::K29_IN>();
      Y = y2 * F::template konst<Pm::K29_IN>();
      ZZ = F::template konst<Pm::K29_IN>();
      ZZZ = ZZ;
      inf = false;
      return true;
    }
    // statement order keeps few values alive at once (x2 dies first, then U2, P, PP, ...)
    const F U2 = F::template mul_as<FORM>(x2, ZZ);                       // 1 x 1
    const F Pp = F::template sub_norm<Pm::SUBC_6P_1>(U2, X);             // normalised, < 7.1 p
    if (Pp.template is_zero_mod_p<7>()) {                                // same x: doubling or cancellation (rare)
      if constexpr (DISTINCT) return false;
      const F S2 = F::template mul_as<FORM>(y2, ZZZ);
      same_x(F::template sub_norm<Pm::SUBC_2P_1>(S2, Y));
      return true;
    }
    const F PP = Pp.template sqr_as<FORM>();                             // 1 x 1 -> < 1.3 p
    const F Q = F::template mul_as<FORM>(X, PP);                         // < 1.05 p
    const F PPP = F::template mul_as<FORM>(Pp, PP);                      // < 1.06 p
    ZZ = F::template mul_as<FORM>(ZZ, PP);
    const F S2 = F::template mul_as<FORM>(y2, ZZZ);                      // 2 x 1
    const F Rr = F::template sub_norm<Pm::SUBC_2P_1>(S2, Y);             // normalised, < 3.1 p
    ZZZ = F::template mul_as<FORM>(ZZZ, PPP);
    const F R2 = Rr.template sqr_as<FORM>();                             // < 1.06 p
    X = F::template sub3_norm<Pm::SUBC_4P_3>(R2, PPP, Q);                // normalised, < 5.1 p
    const F T = F::template sub_lazy<Pm::SUBC_6P_1>(Q, X);               // limbs < 3, < 7.1 p
    const F Yn = F::template neg_lazy<Pm::SUBC_2P_1>(Y);                 // limbs < 2, <= 2p
    Y = F::template mul2_as<FORM>(Rr, T, Yn, PPP);                       // 1x3 + 2x1 -> < 1.2 p
    return true;
  }
  // the entry has the accumulator's x; Rr = y2 * ZZZ - Y, normalised: doubling when it is zero, else cancellation
  SPP_HD void same_x(const F& Rr) {
    if (Rr.template is_zero_mod_p<3>()) {
      XYZZ<B> t = to_xyzz();
      t.dbl_inplace();
      const XYZZ29 d = from_xyzz(t);
      X = d.X;
      Y = d.Y;
      ZZ = d.ZZ;
      ZZZ = d.ZZZ;
    } else {
      inf = true;
    }
  }
};

// --------------------------------------------------------------------------------------------------------------
// Fq2 = Fq[u]/(u^2+1) over F29 and the G2 accumulator.  Every component is a sum of products reduced once:
//   mul : c0 = a0*b0 + (C - a1)*b1,  c1 = a0*b1 + a1*b0            (4 products, 2 reductions)
//   sqr : c0 = (a0 + a1)*(a0 - a1 + C),  c1 = (2*a0)*a1            (2 products, 2 reductions)
// Operands are normalised (limbs < 2^29); the negations/sums made on the fly have limbs < 2^30 or 3*2^29, which keeps
// the column sums under 2^64 (sum of limb-bound products <= 6 * 2^58 per column term: tests/host/f29_bounds.py).
// CNEG_x = lifted multiple of p that dominates the component being negated (template parameter per call site).
// --------------------------------------------------------------------------------------------------------------
struct F29x2 {
  using F = F29<FqParams>;
  using Pm = FqParams;
  F c0, c1;

  static SPP_HD F29x2 from_words(const Fq2& a) { return {F::from_words(a.c0.l), F::from_words(a.c1.l)}; }
  // (a0 + a1 u)(b0 + b1 u); CA dominates a1
  template <F::ConstFn CA, int FORM = F29_COLUMNS>
  static SPP_HD F29x2 mul(const F29x2& a, const F29x2& b) {
    const F na1 = F::template neg_lazy<CA>(a.c1);
    return {F::template mul2_as<FORM>(a.c0, b.c0, na1, b.c1), F::template mul2_as<FORM>(a.c0, b.c1, a.c1, b.c0)};
  }
  // by a real constant (components scale independently)
  SPP_HD F29x2 mul_real(const F& k) const { return {c0 * k, c1 * k}; }
  // CA dominates a1
  template <F::ConstFn CA, int FORM = F29_COLUMNS>
  SPP_HD F29x2 sqr() const {
    const F s = add_lazy(c0, c1);
    const F d = F::template sub_lazy<CA>(c0, c1);
    const F t = add_lazy(c0, c0);
    return {F::template mul_as<FORM>(s, d), F::template mul_as<FORM>(t, c1)};
  }
  template <F::ConstFn C>
  static SPP_HD F29x2 sub_norm(const F29x2& a, const F29x2& b) {
    return {F::template sub_norm<C>(a.c0, b.c0), F::template sub_norm<C>(a.c1, b.c1)};
  }
  template <F::ConstFn C>
  static SPP_HD F29x2 sub3_norm(const F29x2& a, const F29x2& b, const F29x2& c2) {
    return {F::template sub3_norm<C>(a.c0, b.c0, c2.c0), F::template sub3_norm<C>(a.c1, b.c1, c2.c1)};
  }
  template <F::ConstFn C>
  static SPP_HD F29x2 neg_lazy(const F29x2& a) {
    return {F::template neg_lazy<C>(a.c0), F::template neg_lazy<C>(a.c1)};
  }
  template <uint32_t KMAX>
  SPP_HD bool is_zero_mod_p() const {
    return c0.template is_zero_mod_p<KMAX>() && c1.template is_zero_mod_p<KMAX>();
  }
  SPP_HD Fq2 to_fp() const { return {c0.to_fp(), c1.to_fp()}; }
  SPP_HD Fq2 scaled_to_fp() const { return {c0.scaled_to_fp(), c1.scaled_to_fp()}; }
  static SPP_HD F29x2 from_fp(const Fq2& a) { return {F::from_fp(a.c0), F::from_fp(a.c1)}; }
};

// G2 accumulator: same formulas and domains as XYZZ29 (X, Y in the R' domain, ZZ/ZZZ scaled by R'^2/R).
// Value bounds per component: X < 5.6 p, Y < 1.5 p, ZZ/ZZZ < 1.3 p (certificate: check_madd_g2).
// FORM (F29Form): as for XYZZ29.  XYZZ29G2 is the column form, which is also what the G2 walk runs: at two waves per SIMD the
// scanning form was not faster on the chain of additions (profiles/f29_madd_chain.txt).
template <int FORM>
struct XYZZ29G2F {
  using E = F29x2;
  using F = F29<FqParams>;
  using Pm = FqParams;
  E X, Y, ZZ, ZZZ;
  bool inf;

  static SPP_HD XYZZ29G2F infinity() {
    XYZZ29G2F r;
    SPP_UNROLL for (int i = 0; i < 9; i++) {
      r.X.c0.l[i] = r.X.c1.l[i] = r.Y.c0.l[i] = r.Y.c1.l[i] = 0;
      r.ZZ.c0.l[i] = r.ZZ.c1.l[i] = r.ZZZ.c0.l[i] = r.ZZZ.c1.l[i] = 0;
    }
    r.inf = true;
    return r;
  }
  SPP_HD XYZZ<Fq2> to_xyzz() const {
    if (inf) return XYZZ<Fq2>::infinity();
    return {X.to_fp(), Y.to_fp(), ZZ.scaled_to_fp(), ZZZ.scaled_to_fp()};
  }
  static SPP_HD XYZZ29G2F from_xyzz(const XYZZ<Fq2>& q) {
    XYZZ29G2F r;
    r.inf = q.is_inf();
    const F k = F::template konst<Pm::K29_IN>();
    r.X = E::from_fp(q.X);
    r.Y = E::from_fp(q.Y);
    r.ZZ = E::from_fp(q.ZZ).mul_real(k);
    r.ZZZ = E::from_fp(q.ZZZ).mul_real(k);
    return r;
  }

  // this += (x2, +-y2); e = table entry (Fq2 words, not infinity)
  SPP_HD void madd(const Affine<Fq2>& e, bool negate) { madd_any<false>(e, negate); }
  // as XYZZ29::madd_distinct: false and no limb changed when the entry has the accumulator's x
  SPP_HD bool madd_distinct(const Affine<Fq2>& e, bool negate) { return madd_any<true>(e, negate); }
  template <bool DISTINCT>
  SPP_HD bool madd_any(const Affine<Fq2>& e, bool negate) {
    const E x2 = E::from_words(e.x);                                     // limbs < 1, value < 2p
    const E y2 = E::from_words(e.y);
    if (inf) {
      const F k = F::template konst<Pm::K29_IN>();
      X = x2.mul_real(k);
      const E yn = E::template neg_lazy<Pm::SUBC_4P_1>(y2);               // limbs < 2, <= 4p
      E ys;
      SPP_UNROLL for (int i = 0; i < 9; i++) {
        ys.c0.l[i] = negate ? yn.c0.l[i] : y2.c0.l[i];
        ys.c1.l[i] = negate ? yn.c1.l[i] : y2.c1.l[i];
      }
      Y = ys.mul_real(k);                                                // < 1.03 p
      SPP_UNROLL for (int i = 0; i < 9; i++) {
        ZZ.c0.l[i] = k.l[i];
        ZZ.c1.l[i] = 0;
      }
      ZZZ = ZZ;
      inf = false;
      return true;
    }
    const E U2 = E::template mul<Pm::SUBC_4P_1, FORM>(x2, ZZ);                 // < 1.1 p
    const E Pp = E::template sub_norm<Pm::SUBC_6P_1>(U2, X);             // normalised, < 7.1 p
    E S2 = E::template mul<Pm::SUBC_4P_1, FORM>(y2, ZZZ);                      // < 1.1 p
    if (negate) S2 = E::template neg_lazy<Pm::SUBC_2P_1>(S2);            // limbs < 2, <= 2p
    const E Rr = E::template sub_norm<Pm::SUBC_2P_1>(S2, Y);             // normalised, < 4.1 p
    if (Pp.template is_zero_mod_p<7>()) {                                // same x: doubling or cancellation (rare)
      if constexpr (DISTINCT) return false;
      if (Rr.template is_zero_mod_p<4>()) {
        XYZZ<Fq2> t = to_xyzz();
        t.dbl_inplace();
        const XYZZ29G2F d = from_xyzz(t);
        X = d.X;
        Y = d.Y;
        ZZ = d.ZZ;
        ZZZ = d.ZZZ;
      } else {
        inf = true;
      }
      return true;
    }
    const E PP = Pp.template sqr<Pm::SUBC_8P_1, FORM>();                       // < 2.3 p
    const E Q = E::template mul<Pm::SUBC_6P_1, FORM>(X, PP);                   // < 1.2 p
    const E PPP = E::template mul<Pm::SUBC_8P_1, FORM>(Pp, PP);                // < 1.3 p
    ZZ = E::template mul<Pm::SUBC_2P_1, FORM>(ZZ, PP);
    ZZZ = E::template mul<Pm::SUBC_2P_1, FORM>(ZZZ, PPP);
    const E R2 = Rr.template sqr<Pm::SUBC_6P_1, FORM>();                       // < 1.6 p
    X = E::template sub3_norm<Pm::SUBC_4P_3>(R2, PPP, Q);                // normalised, < 5.6 p
    const E T = E::template sub_norm<Pm::SUBC_6P_1>(Q, X);               // normalised, < 7.2 p
    // Y3 = R*T - Y*PPP: eight products, two reductions
    const F nR1 = F::template neg_lazy<Pm::SUBC_6P_1>(Rr.c1);
    const F nY0 = F::template neg_lazy<Pm::SUBC_2P_1>(Y.c0);
    const F nY1 = F::template neg_lazy<Pm::SUBC_2P_1>(Y.c1);
    const F* const a0[4] = {&Rr.c0, &nR1, &nY0, &Y.c1};
    const F* const b0[4] = {&T.c0, &T.c1, &PPP.c0, &PPP.c1};
    const F* const a1[4] = {&Rr.c0, &Rr.c1, &nY0, &nY1};
    const F* const b1[4] = {&T.c1, &T.c0, &PPP.c1, &PPP.c0};
    const F y0 = F::template dot_as<FORM, 4>(a0, b0);
    Y.c1 = F::template dot_as<FORM, 4>(a1, b1);
    Y.c0 = y0;
    return true;
  }
};
using XYZZ29G2 = XYZZ29G2F<F29_COLUMNS>;

}  // namespace spp
