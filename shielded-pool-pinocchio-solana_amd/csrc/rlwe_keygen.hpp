// RLWE key generation and the key check (scripts/rlwe_keygen.py:98-127): the per-lane phases around the 1024-point transform of
// rlwe_ntt.hpp.  One wavefront per key, lane t owns the coefficients t + 64 j, field 0 (= q) only: the public key is needed mod q,
// so there is no second field and no CRT.
//
//   b = e - a * sk  mod (X^1024 + 1, q)                                 k_rlwe_keygen       (rlwe_keygen.py:104-116)
//   max |centred(b + a * sk)|, max |centred(sk)|                        k_rlwe_key_noise    (what a holder of the key can check)
//
// The product  a * s  is  NTT^-1( NTT(a psi^j) . NTT(s psi^j) / 1024 ) psi^-j.  Bound argument of the chain, in units of p = q
// (rn_mul: ANY int32 times a constant |c| < p comes out in (-p, p); 2^31 / q = 12.8):
//   twist            rn_mul(a_i, psi^i), rn_mul(s_i, psi^i)   a_i in [0, q), s_i any int32 (signed key coefficients go in as
//                                                             they are; a key reduced mod q is in [0, q))          -> (-1, 1)
//   two transforms   rn_ntt1<true>: inputs (-1, 1) as rn_dft16 asks, at most 9 inside (rlwe_ntt.hpp), outputs of pass 3   <= 4
//   rk_pointwise     NEITHER factor is a constant below p any more.  S' = rn_mul(S, scale) with scale = 2^64 / 1024 mod p (the
//                    `one` of the tables scaled by 1/1024, RnHostTables::pk_scale) is S / 1024 in Montgomery form   -> (-1, 1)
//                    rn_mul(A, S') with |A| <= 4 as the free operand                                                -> (-1, 1)
//   inverse          rn_ntt1<true> with w^-1                                                                         <= 4
//   untwist          rn_mul(x, psi^-i)                                                                              -> (-1, 1)
//   rk_public_b      canon(e) - canon(prod) in (-1, 1), then rn_canon                                               -> [0, 1)
// tests/host/rlwe_keygen_check.cpp runs exactly these functions lane by lane against the schoolbook product and reports the
// largest magnitude any of them produced.
// Nothing here branches on, or indexes by, a value: every selection is arithmetic on the sign bit.
#pragma once
#include "rlwe_ntt.hpp"

namespace spp {

// x[j] <- x[j] * psi^(lane + 64 j); x any int32
RN_HD void rk_twist(uint32_t lane, int32_t (&x)[16], const int32_t* psi, const RnField& f) {
#pragma unroll
  for (int j = 0; j < 16; j++) x[j] = rn_mul(x[j], psi[lane + 64 * j], f);
}
// A[j] <- A[j] * S[j] / 1024 for two transform outputs (|.| <= 4p); scale = RnHostTables::pk_scale
RN_HD void rk_pointwise(int32_t (&A)[16], const int32_t (&S)[16], int32_t scale, const RnField& f) {
#pragma unroll
  for (int j = 0; j < 16; j++) A[j] = rn_mul(A[j], rn_mul(S[j], scale, f), f);
}
// (e - prod) mod p in [0, p) for prod in (-p, p) and a small signed e
RN_HD uint32_t rk_public_b(int32_t prod, int32_t e, const RnField& f) {
  return (uint32_t)rn_canon(rn_canon(e, f) - rn_canon(prod, f), f);
}
// |centred(v)| for v in [0, p): min(v, p - v)
RN_HD uint32_t rk_abs_centred(uint32_t v, const RnField& f) {
  const int32_t d = (int32_t)(2 * v) - f.p;          // > 0: v is above p / 2 (p is odd: never 0)
  const int32_t up = ~(d >> 31);                     // all ones when v > p / 2
  return (uint32_t)(((int32_t)v & ~up) | ((f.p - (int32_t)v) & up));
}
// |centred((b + prod) mod p)| for b in [0, p), prod in (-p, p)
RN_HD uint32_t rk_noise(uint32_t b, int32_t prod, const RnField& f) {
  int32_t v = (int32_t)b + rn_canon(prod, f) - f.p;  // [0, 2p) - p
  return rk_abs_centred((uint32_t)rn_canon(v, f), f);
}
RN_HD uint32_t rk_max(uint32_t a, uint32_t b) {
  const uint32_t m = 0u - (uint32_t)(a < b);
  return (a & ~m) | (b & m);
}

}  // namespace spp
