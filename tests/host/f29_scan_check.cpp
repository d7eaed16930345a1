// Test-only host build of csrc/f29.hpp: the product-scanning Montgomery products against clear / mac / mac_sqr / reduce, limb for
// limb, and the one-multiplication filter of is_zero_mod_p against the comparison it replaced.
//   - dot_scan<NP> for NP = 1, 2, 4, sqr_scan and the *_as<FORM> entry points (mul_as, mul2_as, dot_as<., 4>, sqr_as) in both
//     forms, for both parameter sets (Fr, Fq): random limbs under the limb bounds the call sites state, and every limb AT its bound -- 1 x 1 (operator*), 2 x 1 (y2 * ZZZ), 1x3 + 2x1 (the Y of XYZZ29), 1x1 + 2x1 (F29x2::mul), 2 x 3 and 2 x 1
//     (F29x2::sqr), 1x1 + 2x1 + 2x1 + 1x1 (the Y components of XYZZ29G2F), squares of limbs < 1 and < 2 (units of 2^29);
//   - XYZZ29<Pm, FORM> and XYZZ29G2F<FORM>, FORM = 1 (F29_SCAN): chains of madd_distinct / madd leave the limbs of FORM = 0;
//   - is_zero_mod_p<KMAX>, KMAX = 3, 4, 7: 0, p, .., (KMAX + 2) p, each with its low limb, a middle limb and the top limb moved by
//     one either way, and random values.
// Prints "OK <n checks>" or "FAIL ...".
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include "f29.hpp"
using namespace spp;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd32() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}
static long checks = 0;
#define CHECK(c, ...) do { checks++; if (!(c)) { printf("FAIL (line %d) ", __LINE__); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

template <class Pm> static bool same(const F29<Pm>& a, const F29<Pm>& b) { return memcmp(a.l, b.l, sizeof a.l) == 0; }

// limbs below bound * 2^29: mode 0 random, 1 every limb at the bound, 2 random limbs with a few at the bound
template <class Pm> static F29<Pm> limbs(uint32_t bound, int mode) {
  F29<Pm> r;
  const uint64_t top = (uint64_t)bound << 29;
  for (int i = 0; i < 9; i++) {
    uint32_t v = (uint32_t)(((uint64_t)rnd32() * top) >> 32);
    if (mode == 1 || (mode == 2 && (rnd32() & 3) == 0)) v = (uint32_t)(top - 1);
    r.l[i] = v;
  }
  return r;
}

template <class Pm, int NP> static void dot_case(const uint32_t (&ba)[NP], const uint32_t (&bb)[NP], int mode, const char* what) {
  using F = F29<Pm>;
  F a[NP], b[NP];
  const F *pa[NP], *pb[NP];
  for (int t = 0; t < NP; t++) {
    a[t] = limbs<Pm>(ba[t], mode);
    b[t] = limbs<Pm>(bb[t], mode);
    pa[t] = &a[t]; pb[t] = &b[t];
  }
  uint64_t c[18];
  F::clear(c);
  for (int t = 0; t < NP; t++) F::mac(c, a[t], b[t]);
  const F ref = F::reduce(c);
  typedef const F* const (&Ptrs)[NP];
  Ptrs ra = reinterpret_cast<Ptrs>(pa), rb = reinterpret_cast<Ptrs>(pb);
  CHECK(same(F::template dot_scan<NP>(ra, rb), ref), "%s: dot_scan<%d>", what, NP);
  CHECK(same(F::template dot_as<0, NP>(ra, rb), ref) && same(F::template dot_as<1, NP>(ra, rb), ref), "%s: dot_as<., %d>", what, NP);
  if constexpr (NP == 1) {
    CHECK(same(a[0] * b[0], ref), "%s: operator*", what);
    CHECK(same(F::template mul_as<0>(a[0], b[0]), ref) && same(F::template mul_as<1>(a[0], b[0]), ref), "%s: mul_as", what);
  }
  if constexpr (NP == 2) {
    CHECK(same(F::mul2(a[0], b[0], a[1], b[1]), ref), "%s: mul2", what);
    CHECK(same(F::template mul2_as<0>(a[0], b[0], a[1], b[1]), ref) && same(F::template mul2_as<1>(a[0], b[0], a[1], b[1]), ref), "%s: mul2_as", what);
  }
}
template <class Pm> static void sqr_case(uint32_t bound, int mode) {
  using F = F29<Pm>;
  const F a = limbs<Pm>(bound, mode);
  uint64_t c[18];
  F::clear(c);
  F::mac_sqr(c, a);
  const F ref = F::reduce(c);
  F::clear(c);
  F::mac(c, a, a);
  CHECK(same(F::reduce(c), ref), "mac_sqr against mac");
  CHECK(same(a.sqr_scan(), ref), "sqr_scan, bound %u", bound);
  CHECK(same(a.sqr(), ref), "sqr, bound %u", bound);
  CHECK(same(a.template sqr_as<0>(), ref) && same(a.template sqr_as<1>(), ref), "sqr_as, bound %u", bound);
}
template <class Pm> static void products(const char* name) {
  static const uint32_t b1[1] = {1}, b2[1] = {2}, b3[1] = {3};
  static const uint32_t y_a[2] = {1, 2}, y_b[2] = {3, 1};         // XYZZ29: Rr * T + Yn * PPP
  static const uint32_t m_a[2] = {1, 2}, m_b[2] = {1, 1};         // F29x2::mul: a0 * b0 + (C - a1) * b1
  static const uint32_t g_a[4] = {1, 2, 2, 1}, g_b[4] = {1, 1, 1, 1};   // XYZZ29G2F: Rr.c0 * T.c0 + nR1 * T.c1 + nY0 * PPP.c0 + Y.c1 * PPP.c1
  for (int mode = 0; mode < 3; mode++) {
    const int n = mode == 1 ? 1 : 200;
    for (int it = 0; it < n; it++) {
      dot_case<Pm, 1>(b1, b1, mode, name);
      dot_case<Pm, 1>(b2, b1, mode, name);
      dot_case<Pm, 1>(b2, b3, mode, name);
      dot_case<Pm, 2>(y_a, y_b, mode, name);
      dot_case<Pm, 2>(m_a, m_b, mode, name);
      dot_case<Pm, 4>(g_a, g_b, mode, name);
      sqr_case<Pm>(1, mode);
      sqr_case<Pm>(2, mode);
    }
  }
}

// ---- the accumulators by form -------------------------------------------------------------------------------------
template <class Fw> static Fw words_below_p() {   // any value < 2^253 < p
  Fw r;
  for (int i = 0; i < 8; i++) r.l[i] = rnd32();
  r.l[7] &= (1u << 29) - 1u;
  return r;
}
template <class A, class B> static bool same_g1(const A& a, const B& b) {
  return a.inf == b.inf && same(a.X, b.X) && same(a.Y, b.Y) && same(a.ZZ, b.ZZ) && same(a.ZZZ, b.ZZZ);
}
template <class A, class B> static bool same_g2(const A& a, const B& b) {
  return a.inf == b.inf && same(a.X.c0, b.X.c0) && same(a.X.c1, b.X.c1) && same(a.Y.c0, b.Y.c0) && same(a.Y.c1, b.Y.c1) && same(a.ZZ.c0, b.ZZ.c0) &&
         same(a.ZZ.c1, b.ZZ.c1) && same(a.ZZZ.c0, b.ZZZ.c0) && same(a.ZZZ.c1, b.ZZZ.c1);
}
// the formulas are polynomial identities in the coordinates: the entries need not lie on a curve for the forms to agree
template <class Pm> static void g1_chains(const char* name) {
  using Fw = Fp<Pm>;
  for (int trial = 0; trial < 20; trial++) {
    XYZZ29<Pm, 0> a0 = XYZZ29<Pm, 0>::infinity();
    XYZZ29<Pm, 1> a1 = XYZZ29<Pm, 1>::infinity();
    for (int s = 0; s < 30; s++) {
      const Affine<Fw> e{words_below_p<Fw>(), words_below_p<Fw>()};
      const bool neg = rnd32() & 1, distinct = rnd32() & 1;
      if (distinct) {
        const bool d0 = a0.madd_distinct(e, neg), d1 = a1.madd_distinct(e, neg);
        CHECK(d0 && d1, "%s: madd_distinct refused a random entry", name);
      } else {
        a0.madd(e, neg); a1.madd(e, neg);
      }
      CHECK(same_g1(a0, a1), "%s: accumulator limbs differ between forms at step %d", name, s);
    }
  }
}
static void g2_chains() {
  for (int trial = 0; trial < 20; trial++) {
    XYZZ29G2F<0> a0 = XYZZ29G2F<0>::infinity();
    XYZZ29G2F<1> a1 = XYZZ29G2F<1>::infinity();
    for (int s = 0; s < 30; s++) {
      const Affine<Fq2> e{{words_below_p<Fq>(), words_below_p<Fq>()}, {words_below_p<Fq>(), words_below_p<Fq>()}};
      const bool neg = rnd32() & 1, distinct = rnd32() & 1;
      if (distinct) {
        const bool d0 = a0.madd_distinct(e, neg), d1 = a1.madd_distinct(e, neg);
        CHECK(d0 && d1, "g2: madd_distinct refused a random entry");
      } else {
        a0.madd(e, neg); a1.madd(e, neg);
      }
      CHECK(same_g2(a0, a1), "g2: accumulator limbs differ between forms at step %d", s);
    }
  }
}

// ---- is_zero_mod_p ------------------------------------------------------------------------------------------------
// the comparison before the filter: the low limb against that of every multiple in turn
template <class Pm, uint32_t KMAX> static bool is_zero_by_compares(const F29<Pm>& v) {
  using F = F29<Pm>;
  uint32_t kk = 0xffffffffu;
  for (uint32_t k = 0; k <= KMAX; k++)
    if (v.l[0] == ((k * F::P9(0)) & F::M)) kk = k;
  if (kk == 0xffffffffu) return false;
  uint32_t diff = 0, carry = 0;
  for (int i = 0; i < 8; i++) {
    const uint32_t t = kk * F::P9(i) + carry;
    diff |= v.l[i] ^ (t & F::M);
    carry = t >> 29;
  }
  diff |= v.l[8] ^ (kk * F::P9(8) + carry);
  return diff == 0;
}
template <class Pm, uint32_t KMAX> static void zero_case(const F29<Pm>& v, int expect, const char* what) {
  const bool got = v.template is_zero_mod_p<KMAX>(), old = is_zero_by_compares<Pm, KMAX>(v);
  CHECK(got == old, "%s: is_zero_mod_p<%u> = %d, by compares %d", what, KMAX, (int)got, (int)old);
  if (expect >= 0) CHECK(got == (expect != 0), "%s: is_zero_mod_p<%u> = %d, expected %d", what, KMAX, (int)got, expect);
}
template <class Pm, uint32_t KMAX> static void zero_checks(const char* name) {
  using F = F29<Pm>;
  F p, kp;
  for (int i = 0; i < 9; i++) { p.l[i] = F::P9(i); kp.l[i] = 0; }
  CHECK(((uint64_t)F::P9(0) * Pm::PINV29 & F::M) == 1, "%s: PINV29 is not the inverse of the low limb of p", name);
  for (uint32_t k = 0; k <= KMAX + 2; k++) {
    zero_case<Pm, KMAX>(kp, k <= KMAX, name);
    static const int moved[3] = {0, 5, 8};
    for (int w = 0; w < 3; w++) {
      for (int dir = -1; dir <= 1; dir += 2) {
        F v = kp;
        v.l[moved[w]] = moved[w] < 8 ? (v.l[moved[w]] + (uint32_t)dir) & F::M : v.l[8] + (uint32_t)dir;   // stays a normalised form
        zero_case<Pm, KMAX>(v, 0, name);
      }
    }
    kp = add_norm(kp, p);
  }
  for (int it = 0; it < 2000; it++) {
    F v = limbs<Pm>(1, 0);
    zero_case<Pm, KMAX>(v, 0, name);
    v.l[0] = (rnd32() % (KMAX + 3) * F::P9(0)) & F::M;    // passes (or just misses) the filter, fails the comparison
    zero_case<Pm, KMAX>(v, -1, name);
  }
}

int main() {
  products<FrParams>("Fr");
  products<FqParams>("Fq");
  g1_chains<FrParams>("Fr");
  g1_chains<FqParams>("Fq");
  g2_chains();
  zero_checks<FrParams, 3>("Fr");
  zero_checks<FrParams, 4>("Fr");
  zero_checks<FrParams, 7>("Fr");
  zero_checks<FqParams, 3>("Fq");
  zero_checks<FqParams, 4>("Fq");
  zero_checks<FqParams, 7>("Fq");
  printf("OK %ld checks\n", checks);
  return 0;
}
