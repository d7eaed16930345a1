// Test-only host build of csrc/f29.hpp: XYZZ29::madd_distinct and XYZZ29G2::madd_distinct, the mixed addition of the flat table
// walk that refuses the same-x case instead of doubling, against madd.
//   - entry with another x than the accumulator: true, and every limb of the accumulator equals what madd leaves (random chains,
//     accumulators with extremal limbs, the first addition from infinity);
//   - entry = +-(the accumulated point): false, and no limb and no flag of the accumulator changed.
// Prints "OK <n checks>" or "FAIL ...".
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <vector>
#include "f29.hpp"
using namespace spp;

static uint64_t rng_state = 0x2545F4914F6CDD1Dull;
static uint32_t rnd32() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}
static int checks = 0;
#define CHECK(c, msg) do { checks++; if (!(c)) { printf("FAIL %s (line %d)\n", msg, __LINE__); exit(1); } } while (0)

static bool same(const F29<FqParams>& a, const F29<FqParams>& b) { return memcmp(a.l, b.l, sizeof a.l) == 0; }
static bool same(const F29x2& a, const F29x2& b) { return same(a.c0, b.c0) && same(a.c1, b.c1); }
template <class A> static bool same_acc(const A& a, const A& b) {
  return a.inf == b.inf && same(a.X, b.X) && same(a.Y, b.Y) && same(a.ZZ, b.ZZ) && same(a.ZZZ, b.ZZZ);
}

static Fq fq_hex(const char* h) {
  uint32_t c[8];
  for (int i = 0; i < 8; i++) {
    char buf[9];
    memcpy(buf, h + 8 * i, 8);
    buf[8] = 0;
    c[7 - i] = (uint32_t)strtoul(buf, nullptr, 16);
  }
  return Fq::from_canonical(c);
}
template <class Aff> static std::vector<Aff> multiples(const Aff& G, int n) {
  std::vector<Aff> pts;
  for (int i = 0; i < n; i++) {
    uint32_t k[8];
    for (int j = 0; j < 8; j++) k[j] = rnd32();
    k[7] &= 0x0fffffff;
    pts.push_back(scalar_mul(G, k).to_affine());
  }
  return pts;
}

// one step on two copies: madd on `ref`, madd_distinct on `acc`; `same_x` says which outcome is due
template <class A, class Aff> static void step(A& acc, const Aff& e, bool neg, bool same_x, const char* what) {
  A ref = acc;
  const A before = acc;
  ref.madd(e, neg);
  const bool done = acc.madd_distinct(e, neg);
  if (same_x) {
    CHECK(!done, what);
    CHECK(same_acc(acc, before), "refused addition changed the accumulator");
    acc = ref;                         // go on from the complete addition's result (the doubled point, or infinity)
  } else {
    CHECK(done, what);
    CHECK(same_acc(acc, ref), "madd_distinct differs from madd");
  }
}

// Acc: XYZZ29<FqParams> with G1Affine / G1XYZZ, or XYZZ29G2 with G2Affine / G2XYZZ
template <class Acc, class Aff, class Ref> static void chains(const std::vector<Aff>& pts, int trials, const char* name) {
  for (int trial = 0; trial < trials; trial++) {
    Acc acc = Acc::infinity();
    for (int s = 0; s < 40; s++) {
      const int mode = rnd32() % 8;
      bool neg = rnd32() & 1;
      Aff e = pts[rnd32() % pts.size()];
      bool same_x = false;
      if (mode <= 1 && !acc.inf) {     // the accumulated point itself (doubling) or its negative (cancellation), either sign of the flag
        const Ref r = acc.to_xyzz();
        e = r.to_affine();
        if (mode == 1) e.y = e.y.neg();
        same_x = true;
      } else if (!acc.inf) {
        const Aff a = acc.to_xyzz().to_affine();
        same_x = a.x == e.x;           // a random pick that happens to be the sum so far (12-24 points: it does happen)
      }
      step(acc, e, neg, same_x, name);
    }
  }
  // the first addition from infinity, both signs, every point
  for (const Aff& e : pts)
    for (int neg = 0; neg < 2; neg++) {
      Acc acc = Acc::infinity();
      step(acc, e, neg != 0, false, "first addition from infinity");
      CHECK(!acc.inf, "finite after the first addition");
      step(acc, e, neg != 0, true, "the same entry again: doubling refused");
      Acc again = Acc::infinity();
      again.madd(e, neg != 0);
      step(again, e, neg == 0, true, "the negated entry: cancellation refused");
      CHECK(again.inf, "cancelled by madd");
    }
}

// Extremal limbs: the same residues with the largest limbs the accumulator's invariants allow.  Adding a multiple of p to a
// coordinate keeps the point; X may be up to 5.1 p (G2: 5.6 p), so the reduced residue + 4 p is a legal accumulator with the largest
// top limbs madd meets.  madd_distinct must track madd limb for limb on it, and refuse on it.
static F29<FqParams> plus_kp(const F29<FqParams>& a, uint32_t k) {
  using F = F29<FqParams>;
  F r;
  uint32_t carry = 0;
  for (int i = 0; i < 8; i++) {
    const uint32_t t = a.l[i] + k * F::P9(i) + carry;
    r.l[i] = t & F::M;
    carry = t >> 29;
  }
  r.l[8] = a.l[8] + k * F::P9(8) + carry;
  return r;
}
static void extremal_g1(const std::vector<G1Affine>& pts) {
  using X29 = XYZZ29<FqParams>;
  for (size_t i = 0; i + 1 < pts.size(); i++) {
    X29 acc = X29::infinity();
    acc.madd(pts[i], false);
    acc.madd(pts[i + 1], true);
    acc.X = plus_kp(F29<FqParams>::from_fp(acc.X.to_fp()), 4);     // the residue below 1.06 p, + 4 p: under the 5.1 p of the invariant
    for (int neg = 0; neg < 2; neg++) {
      X29 a = acc;
      step(a, pts[(i + 2) % pts.size()], neg != 0, false, "extremal X, distinct entry");
      X29 b = acc;
      G1Affine self = acc.to_xyzz().to_affine();
      step(b, self, neg != 0, true, "extremal X, own point");
    }
  }
}
static void extremal_g2(const std::vector<G2Affine>& pts) {
  for (size_t i = 0; i + 1 < pts.size(); i++) {
    XYZZ29G2 acc = XYZZ29G2::infinity();
    acc.madd(pts[i], false);
    acc.madd(pts[i + 1], true);
    acc.X.c0 = plus_kp(F29<FqParams>::from_fp(acc.X.c0.to_fp()), 4);
    acc.X.c1 = plus_kp(F29<FqParams>::from_fp(acc.X.c1.to_fp()), 4);
    for (int neg = 0; neg < 2; neg++) {
      XYZZ29G2 a = acc;
      step(a, pts[(i + 2) % pts.size()], neg != 0, false, "g2 extremal X, distinct entry");
      XYZZ29G2 b = acc;
      G2Affine self = acc.to_xyzz().to_affine();
      step(b, self, neg != 0, true, "g2 extremal X, own point");
    }
  }
}

int main() {
  const G1Affine G1{Fq::one(), Fq::one().dbl()};
  // BN254 G2 generator (EIP-197), x = x0 + x1 u, y = y0 + y1 u
  const G2Affine G2{{fq_hex("1800deef121f1e76426a00665e5c4479674322d4f75edadd46debd5cd992f6ed"),
                     fq_hex("198e9393920d483a7260bfb731fb5d25f1aa493335a9e71297e485b7aef312c2")},
                    {fq_hex("12c85ea5db8c6deb4aab71808dcb408fe3d1e7690c43d37b4ce6cc0166fa7daa"),
                     fq_hex("090689d0585ff075ec9e99ad690c3395bc4b313370b38ef355acdadcd122975b")}};
  const std::vector<G1Affine> p1 = multiples(G1, 24);
  const std::vector<G2Affine> p2 = multiples(G2, 12);
  chains<XYZZ29<FqParams>, G1Affine, G1XYZZ>(p1, 50, "g1 chain");
  printf("g1 chains ok\n");
  chains<XYZZ29G2, G2Affine, G2XYZZ>(p2, 20, "g2 chain");
  printf("g2 chains ok\n");
  extremal_g1(p1);
  extremal_g2(p2);
  printf("extremal ok\n");
  printf("OK %d\n", checks);
  return 0;
}
