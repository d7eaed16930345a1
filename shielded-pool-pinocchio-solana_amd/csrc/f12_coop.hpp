// Wave-cooperative Fq12 arithmetic: one Fq12 product spread over the 64 lanes of a wave, operands and results in LDS.
// Used by the once-per-group tail of the random-linear-combination verifier (verify_rlc.hpp, kernels_verify_rlc.hip), the
// batch form of `sunspot verify` (noir_circuit/prove_linux.sh:86-87): a chain of ~900 dependent Fq12 products, each of them
// 144 independent Fq products, which one lane (pairing_fast.hpp) would run for longer than the whole lanes phase in front.
//
// Scheme (the minimum one): the schoolbook product of two 12-coefficient polynomials in w has 23 columns; column k goes to
// lane k, which sums its <= 12 products and writes t[k]; after a barrier lane c < 12 folds with w^12 = 18 w^6 - 82 in closed
// form,
//     w^(12+j) = 18 w^(6+j) - 82 w^j            (j = 0..5)
//     w^(18+j) = 242 w^(6+j) - 1476 w^j         (j = 0..4;  242 = 18^2 - 82, 1476 = 18 * 82)
//     out[c]   = t[c]   -  82 t[12+c] - 1476 t[18+c]      (c = 0..5, t[23] = 0)
//     out[6+c] = t[6+c] +  18 t[12+c] +  242 t[18+c]
// so a product costs the wave 12 + 2 Fq products of latency instead of 166, with no cross-lane reduction.
//
// Everything is written as PHASE functions: f(lane) touches only the shared arrays it is given, and a barrier separates two
// phases.  The executor X decides what a phase is: on the device x.phase(f) runs f for this lane and waits at the barrier
// (CoopWave, kernels_verify_rlc.hip); on the host it runs f for lanes 0..63 one after another (CoopEmu, below), which is how
// tests/host/verify_rlc_check.cpp compares every routine with its one-lane counterpart of pairing_fast.hpp.  A phase never
// reads what another lane writes in the same phase (the emulation would see the sequential order, a wave would not).
// Control flow is uniform across the wave: loops run the same trip count on every lane and a lane without work multiplies
// zeros.  Functions with loops are small and out of line, their Fq products are calls (the hazard at scalar_mul_rolled).
#pragma once
#include "pairing_fast.hpp"

namespace spp {

SPP_HDN Fq fq_mul_call(const Fq& a, const Fq& b) { return a * b; }

struct CoopConsts {
  Fq k18, k82, k242, k1476, one;
  Fq FA[12], FB[12];
};
SPP_HD CoopConsts make_coop_consts(const PairingFastConsts& pc) {
  CoopConsts c;
  c.k18 = pc.k18;
  c.k82 = pc.k82;
  c.k242 = pc.k18 * pc.k18 - pc.k82;
  c.k1476 = pc.k18 * pc.k82;
  c.one = pc.one;
  for (int i = 0; i < 12; i++) {
    c.FA[i] = pc.FA[i];
    c.FB[i] = pc.FB[i];
  }
  return c;
}

// what the cooperative routines share (LDS on the device): the 23 columns, scratch elements, the constants
struct CoopShared {
  CoopConsts cc;
  Fq t[23];
  F12 u, v;          // temporaries of frob chains and of pow_x
  Fq ninv;           // the one inversion of the final exponentiation
  uint32_t flag[12];
};

// host emulation of a wave: the lanes of a phase one after another
struct CoopEmu {
  template <class Fn>
  void phase(Fn f) {
    for (uint32_t lane = 0; lane < 64; lane++) f(lane);
  }
};

// ---- phases ------------------------------------------------------------------------------------------------------------
// column `lane` of a (12 coefficients) times b (12 coefficients)
SPP_HDN void coop_cols_full(uint32_t lane, const Fq* a, const Fq* b, Fq* t) {
  Fq acc = Fq::zero();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (uint32_t j = 0; j < 12; j++) {
    const uint32_t i = lane - j;                       // wraps for j > lane: not < 12 then
    const bool live = i < 12 && lane < 23;
    const Fq x = live ? a[live ? i : 0] : Fq::zero();
    acc = acc + fq_mul_call(x, b[j]);
  }
  if (lane < 23) t[lane] = acc;
}
// column `lane` of f times the sparse line  l[0] + l[1] w + l[2] w^3 + l[3] w^6 + l[4] w^7 + l[5] w^9
SPP_HDN void coop_cols_line(uint32_t lane, const Fq* f, const Fq* l, Fq* t) {
  Fq acc = Fq::zero();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (uint32_t s = 0; s < 6; s++) {
    const uint32_t off = s == 0 ? 0u : s == 1 ? 1u : s == 2 ? 3u : s == 3 ? 6u : s == 4 ? 7u : 9u;
    const uint32_t i = lane - off;
    const bool live = i < 12 && lane < 23;
    const Fq x = live ? f[live ? i : 0] : Fq::zero();
    acc = acc + fq_mul_call(x, l[s]);
  }
  if (lane < 23) t[lane] = acc;
}
// lane c < 12: coefficient c of the folded product
SPP_HDN void coop_fold(uint32_t lane, const Fq* t, Fq* out, const CoopConsts& cc) {
  const uint32_t c = lane < 12 ? lane : 0, j = c < 6 ? c : c - 6;
  const Fq hi = j < 5 ? t[18 + j] : Fq::zero();
  const Fq m1 = fq_mul_call(t[12 + j], c < 6 ? cc.k82 : cc.k18);
  const Fq m2 = fq_mul_call(hi, c < 6 ? cc.k1476 : cc.k242);
  const Fq r = c < 6 ? t[c] - m1 - m2 : t[c] + m1 + m2;
  if (lane < 12) out[lane] = r;
}
SPP_HDN void coop_frob_lane(uint32_t lane, const Fq* a, Fq* out, const CoopConsts& cc) {
  const uint32_t i = lane < 12 ? lane : 0;
  const Fq r = fq_mul_call(a[i], cc.FA[i]) + fq_mul_call(a[(i + 6) % 12], cc.FB[i]);
  if (lane < 12) out[lane] = r;
}

// ---- routines: sequences of phases ----------------------------------------------------------------------------------------
// out = a * b; out may be a or b (the fold reads the columns only)
template <class X>
SPP_HD void coop_f12_mul(X& x, CoopShared& sh, const F12& a, const F12& b, F12& out) {
  x.phase([&](uint32_t lane) { coop_cols_full(lane, a.c, b.c, sh.t); });
  x.phase([&](uint32_t lane) { coop_fold(lane, sh.t, out.c, sh.cc); });
}
// out = f * (l0 + l1 w + l3 w^3 + l6 w^6 + l7 w^7 + l9 w^9), the six coefficients in l[0..5] (shared); out may be f
template <class X>
SPP_HD void coop_f12_mul_line(X& x, CoopShared& sh, const F12& f, const Fq* l, F12& out) {
  x.phase([&](uint32_t lane) { coop_cols_line(lane, f.c, l, sh.t); });
  x.phase([&](uint32_t lane) { coop_fold(lane, sh.t, out.c, sh.cc); });
}
// out = a^p; out must not be a
template <class X>
SPP_HD void coop_f12_frob(X& x, CoopShared& sh, const F12& a, F12& out) {
  x.phase([&](uint32_t lane) { coop_frob_lane(lane, a.c, out.c, sh.cc); });
}
// a = a^(p^6) in place
template <class X>
SPP_HD void coop_f12_conj6(X& x, F12& a) {
  x.phase([&](uint32_t lane) {
    if (lane < 12 && (lane & 1)) a.c[lane] = a.c[lane].neg();
  });
}
template <class X>
SPP_HD void coop_f12_copy(X& x, const F12& a, F12& out) {
  x.phase([&](uint32_t lane) {
    if (lane < 12) out.c[lane] = a.c[lane];
  });
}
// out = y^x, x = BN_X; out must not be y
template <class X>
SPP_HDN void coop_f12_pow_x(X& x, CoopShared& sh, const F12& y, F12& out) {
  coop_f12_copy(x, y, out);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int b = 61; b >= 0; b--) {
    coop_f12_mul(x, sh, out, out, out);
    if ((BN_X >> b) & 1) coop_f12_mul(x, sh, out, y, out);
  }
}

// the fixed-table Miller loop over five tables (miller_multi(5, tabs, Ps, false, ..., extra) of pairing_fast.hpp):
// f = prod_k l_k(Ps[k]) over the ate loop, times `extra`.  tabs, Ps, extra and f are shared; a pair whose P is at infinity
// contributes 1.  line[6] is shared scratch.
struct CoopMiller {
  const LineStep* tab[5];
  G1Affine P[5];
  uint32_t live[5];     // P[k] is not at infinity
  Fq line[6];
};
template <class X>
SPP_HDN void coop_fixed_lines(X& x, CoopShared& sh, CoopMiller& m, uint32_t idx, F12& f) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (uint32_t k = 0; k < 5; k++) {
    if (!m.live[k]) continue;                          // uniform: shared word
    x.phase([&](uint32_t lane) {                       // the line of mul_table_line, one coefficient per lane
      if (lane >= 6) return;
      const LineStep& s = m.tab[k][idx];
      const G1Affine& P = m.P[k];
      Fq v;
      if (lane == 0) v = P.y;
      else if (lane == 1) v = fq_mul_call(P.x.neg(), s.a1);
      else if (lane == 2) v = s.a3;
      else if (lane == 3) v = Fq::zero();
      else if (lane == 4) v = fq_mul_call(P.x.neg(), s.b1);
      else v = s.b3;
      m.line[lane] = v;
    });
    coop_f12_mul_line(x, sh, f, m.line, f);
  }
}
template <class X>
SPP_HDN void coop_miller5(X& x, CoopShared& sh, CoopMiller& m, const F12& extra, F12& f) {
  x.phase([&](uint32_t lane) {
    if (lane < 12) f.c[lane] = lane == 0 ? sh.cc.one : Fq::zero();
    if (lane >= 16 && lane < 21) m.live[lane - 16] = m.P[lane - 16].is_inf() ? 0u : 1u;
  });
  uint32_t idx = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int i = 63; i >= 0; i--) {
    coop_f12_mul(x, sh, f, f, f);
    coop_fixed_lines(x, sh, m, idx++, f);
    if ((ATE_LO >> i) & 1) coop_fixed_lines(x, sh, m, idx++, f);
  }
  coop_fixed_lines(x, sh, m, idx++, f);
  coop_fixed_lines(x, sh, m, idx++, f);
  coop_f12_mul(x, sh, f, extra, f);
}

// final_exp_is_one of pairing_fast.hpp, product by product; the temporaries are shared
struct CoopFinal {
  F12 g, t, y, fx, fx2, fx3, a, b, c, B, C, A;
};
template <class X>
SPP_HDN void coop_frob_n(X& x, CoopShared& sh, const F12& a, uint32_t n, F12& out) {   // out = a^(p^n), n = 1..3; out != a
  coop_f12_frob(x, sh, a, n == 1 ? out : sh.u);
  if (n == 2) coop_f12_frob(x, sh, sh.u, out);
  if (n == 3) {
    coop_f12_frob(x, sh, sh.u, sh.v);
    coop_f12_frob(x, sh, sh.v, out);
  }
}
template <class X>
SPP_HDN void coop_final_easy(X& x, CoopShared& sh, CoopFinal& w, const F12& f) {   // w.y = f^((p^6-1)(p^2+1))
  // inverse through the norm: t = f^p * ... * f^(p^11), f * t in Fq
  coop_f12_frob(x, sh, f, w.g);
  coop_f12_copy(x, w.g, w.t);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int i = 2; i <= 11; i++) {
    coop_f12_frob(x, sh, w.g, w.a);
    coop_f12_copy(x, w.a, w.g);
    coop_f12_mul(x, sh, w.t, w.g, w.t);
  }
  coop_f12_mul(x, sh, f, w.t, w.a);
  x.phase([&](uint32_t lane) {
    if (lane == 0) sh.ninv = w.a.c[0].inv();          // the one inversion stays on one lane
  });
  x.phase([&](uint32_t lane) {
    const Fq r = fq_mul_call(w.t.c[lane < 12 ? lane : 0], sh.ninv);
    if (lane < 12) w.t.c[lane] = r;                    // t = f^-1
  });
  coop_f12_copy(x, f, w.a);
  coop_f12_conj6(x, w.a);
  coop_f12_mul(x, sh, w.a, w.t, w.y);
  coop_frob_n(x, sh, w.y, 2, w.a);
  coop_f12_mul(x, sh, w.a, w.y, w.y);
}
template <class X>
SPP_HDN bool coop_final_exp_is_one(X& x, CoopShared& sh, CoopFinal& w, const F12& f) {
  coop_final_easy(x, sh, w, f);
  // hard part (y is unitary now: y^-1 = conj6(y)), the chain of final_exp_is_one
  coop_f12_pow_x(x, sh, w.y, w.fx);
  coop_f12_pow_x(x, sh, w.fx, w.fx2);
  coop_f12_pow_x(x, sh, w.fx2, w.fx3);
  coop_f12_mul(x, sh, w.fx, w.fx, w.a);          // a = fx^2
  coop_f12_mul(x, sh, w.fx2, w.fx2, w.b);        // b = fx2^2
  coop_f12_mul(x, sh, w.b, w.b, w.g);
  coop_f12_mul(x, sh, w.g, w.b, w.b);            // b = fx2^6
  coop_f12_mul(x, sh, w.fx3, w.fx3, w.c);
  coop_f12_mul(x, sh, w.c, w.c, w.c);            // c = fx3^4
  coop_f12_mul(x, sh, w.c, w.c, w.g);
  coop_f12_mul(x, sh, w.g, w.c, w.c);            // c = fx3^12
  coop_f12_mul(x, sh, w.a, w.a, w.g);            // g = fx^4
  coop_f12_mul(x, sh, w.c, w.b, w.B);
  coop_f12_mul(x, sh, w.B, w.g, w.B);            // B = y^l1
  coop_f12_mul(x, sh, w.B, w.a, w.C);            // C = y^l2
  coop_f12_mul(x, sh, w.C, w.b, w.A);
  coop_f12_mul(x, sh, w.A, w.y, w.A);            // A = y^l0
  coop_f12_conj6(x, w.y);
  coop_f12_mul(x, sh, w.y, w.B, w.y);            // y = D = y^l3
  coop_frob_n(x, sh, w.B, 1, w.g);
  coop_f12_mul(x, sh, w.A, w.g, w.A);
  coop_frob_n(x, sh, w.C, 2, w.g);
  coop_f12_mul(x, sh, w.A, w.g, w.A);
  coop_frob_n(x, sh, w.y, 3, w.g);
  coop_f12_mul(x, sh, w.A, w.g, w.A);
  x.phase([&](uint32_t lane) {
    if (lane < 12) sh.flag[lane] = (lane == 0 ? w.A.c[0] == sh.cc.one : w.A.c[lane].is_zero()) ? 1u : 0u;
  });
  uint32_t ok = 1;
  for (int i = 0; i < 12; i++) ok &= sh.flag[i];
  return ok != 0;
}

}  // namespace spp
