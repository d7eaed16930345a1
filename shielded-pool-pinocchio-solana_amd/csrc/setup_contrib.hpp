// A contribution to the delta of a Groth16 proving key (phase 2 of a setup ceremony) and what its verifier reads off the files:
// one scalar times many G1 points (kernels_setup.hip), the point check that runs before caller data reaches an MSM, and the byte
// layout of the SPPK container as far as "what may a contribution change" goes (spp_ceremony_api.cpp).
//
// What depends on delta (spp_setup.cpp): delta1, delta2, the K section (the private wires, scaled by 1/delta) and the n - 1 Z
// points tau^i t(tau) / delta.  A contribution with secret d sets delta' = d * delta and K' = K / d, Z' = Z / d and copies every
// other byte.  The scalar 1/d is the SAME for all ~62 K points of the audit key, so it is recoded ONCE, on the host, to its
// non-adjacent form, and the digits reach the kernel through memory that every lane reads at the same index: each add / skip
// decision is taken by the wave, not by the lane (the bit loop of g1_scalar_mul, kernels_msm.hip, brings the scalar to canonical
// form and tests a bit per lane).  No table of multiples per lane: NAF has ~254 doublings and ~85 mixed additions (weight 1/3); a
// 4-bit table would be 8 XYZZ points = 1 KB per lane, that is scratch.
//
// The addition: XYZZ::madd (bn254.hpp) tests U2 == X and then S2 == Y and doubles or returns infinity, so acc = +-P is summed
// correctly wherever it occurs.  It does occur for 0 < k < r on a point of order r: r = 1 mod 4, so k = r - 2 ends with the
// digit -1 on the accumulator (r - 1) P = -P, a doubling inside the addition (the tests carry r - 1, r - 2, (r +- 1) / 2).  A
// point of another order (a caller's) only changes WHICH step meets the case, not whether the product is right.
//
// The conversion to affine is per lane (to_affine).  Measured at the audit key's 61 474 points: 1.81 ms with it against 1.70 ms for
// the same loop storing XYZZ and inverting nothing, so 0.11 ms (6 %) is all a block-wide batched inversion through LDS could save
// before its own products and barriers; and the points are 970 waves on 1 024 SIMDs -- less than one wave per SIMD, no wave
// waits for another's inversion.  DESIGN.md has the figures.
//
// Host and device: the recoding, the scaling and the point check are SPP_HD, so that a host program pins them against big
// integers (tests/host/setup_contrib_check.cpp); the layout functions read bytes only.
#pragma once
#include <string.h>
#include "bn254.hpp"

namespace spp {

static constexpr uint32_t SC_MAX_DIGITS = 256;   // NAF of a value below 2^254 has at most 255 digits

// Non-adjacent form of the canonical scalar k (8 limbs, least significant first, k < 2^255): dig[i] in {-1, 0, 1}, least
// significant first, sum_i dig[i] 2^i = k, no two neighbours both non-zero, the top digit +1.  Returns the number of digits
// (0 for k = 0); dig[] beyond it is zero.
SPP_HD uint32_t sc_naf_recode(const uint32_t k[8], int8_t dig[SC_MAX_DIGITS]) {
  uint32_t v[8];
  for (int i = 0; i < 8; i++) v[i] = k[i];
  uint32_t len = 0;
  for (uint32_t i = 0; i < SC_MAX_DIGITS; i++) {
    int d = 0;
    if (v[0] & 1u) {
      d = 2 - (int)(v[0] & 3u);   // +1 if v = 1 mod 4, -1 if v = 3 mod 4
      if (d > 0) {
        v[0] -= 1u;               // v is odd: no borrow
      } else {
        uint32_t c = 1;           // v + 1
        for (int j = 0; j < 8; j++) v[j] = addc32(v[j], 0u, c);
      }
    }
    dig[i] = (int8_t)d;
    if (d) len = i + 1;
    for (int j = 0; j < 7; j++) v[j] = (v[j] >> 1) | (v[j + 1] << 31);
    v[7] >>= 1;
  }
  return len;
}

// k * p from the digits of sc_naf_recode, most significant first.  `dig` is read at indices that do not depend on the lane.
// (F = Fq: the ceremony's K | Z and CS points; F = Fq2: the 1 / n of the group transform over G2, ptau.hpp)
template <class F>
SPP_HD XYZZ<F> sc_scale_point(const Affine<F>& p, const int8_t* dig, uint32_t len) {
  XYZZ<F> acc = XYZZ<F>::infinity();
  const Affine<F> np = p.neg();
#if defined(__HIPCC__)
#pragma unroll 1
#endif
  for (uint32_t i = len; i-- > 0;) {
    acc.dbl_inplace();
    const int d = dig[i];
    if (d != 0) acc.madd(d > 0 ? p : np);
  }
  return acc;
}

// One G1 point as the files hold it (X | Y, 32 B big-endian each; 64 zero bytes: the point at infinity), read as 16 words.
static constexpr uint32_t SC_POINT_BAD = 0, SC_POINT_OK = 1, SC_POINT_INF = 2;
SPP_HD uint32_t sc_load_be32(const uint8_t* b) { return ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3]; }
// SC_POINT_OK: both coordinates below q and y^2 = x^3 + 3; SC_POINT_INF: all zero; else SC_POINT_BAD.  *out: the point in
// Montgomery form (infinity unless SC_POINT_OK), what the MSM and the scaling kernel read.
SPP_HD uint32_t sc_decode_point(const uint8_t raw[64], Affine<Fq>* out) {
  uint32_t x[8], y[8], any = 0;
  for (int i = 0; i < 8; i++) {
    x[7 - i] = sc_load_be32(raw + 4 * i);
    y[7 - i] = sc_load_be32(raw + 32 + 4 * i);
    any |= x[7 - i] | y[7 - i];
  }
  *out = Affine<Fq>::infinity();
  if (any == 0) return SC_POINT_INF;
  if (Fq::geq_mod(x) || Fq::geq_mod(y)) return SC_POINT_BAD;
  const Fq fx = Fq::from_canonical(x), fy = Fq::from_canonical(y);
  if (!(fy.sqr() == fx.sqr() * fx + Fq::from_u64(3))) return SC_POINT_BAD;
  *out = Affine<Fq>{fx, fy};
  return SC_POINT_OK;
}

// ----------------------------------------------------------------------------------------------------------------------
// The SPPK container (written by sppk_write.hpp only) as byte ranges.
//   header 7 words | alpha1 beta1 delta1 (64 B each) | beta2 delta2 (128 B each) | A: count, wires, points | B1: the same |
//   B2: count, wires, 128 B points | K: count, wires, points | Z: count, points | CB: count, wires, points | CS: the same
// ----------------------------------------------------------------------------------------------------------------------
struct SppkLayout {
  size_t delta1 = 0, delta2 = 0;       // offsets of delta1 (64 B) and delta2 (128 B)
  size_t k_points = 0, z_points = 0;   // offsets of the first K point and the first Z point
  uint32_t n_k = 0, n_z = 0;
  size_t cs_points = 0;                // offset of the first CS point (the sigma contributions' section), n_cs of them
  uint32_t n_cs = 0;
};
inline bool sppk_layout(const uint8_t* b, size_t len, SppkLayout* L) {
  size_t p = 0;
  bool ok = true;
  auto u32 = [&]() -> uint32_t {
    if (len - p < 4) { ok = false; return 0; }
    const uint32_t v = (uint32_t)b[p] | ((uint32_t)b[p + 1] << 8) | ((uint32_t)b[p + 2] << 16) | ((uint32_t)b[p + 3] << 24);
    p += 4;
    return v;
  };
  auto skip = [&](uint64_t n) {
    if (!ok || n > (uint64_t)(len - p)) { ok = false; return; }
    p += (size_t)n;
  };
  if (len < 28) return false;
  if (u32() != 0x4b505053u || u32() != 1) return false;
  skip(20);
  skip(128);
  L->delta1 = p; skip(64);
  skip(128);
  L->delta2 = p; skip(128);
  { const uint32_t n = u32(); skip((uint64_t)n * 4); skip((uint64_t)n * 64); }
  { const uint32_t n = u32(); skip((uint64_t)n * 4); skip((uint64_t)n * 64); }
  { const uint32_t n = u32(); skip((uint64_t)n * 4); skip((uint64_t)n * 128); }
  L->n_k = u32(); skip((uint64_t)L->n_k * 4); L->k_points = p; skip((uint64_t)L->n_k * 64);
  L->n_z = u32(); L->z_points = p; skip((uint64_t)L->n_z * 64);
  { const uint32_t n = u32(); skip((uint64_t)n * 4); skip((uint64_t)n * 64); }
  L->n_cs = u32(); skip((uint64_t)L->n_cs * 4); L->cs_points = p; skip((uint64_t)L->n_cs * 64);
  return ok && p == len;
}
// The gnark raw verifying key: alpha1 beta1 | beta2 gamma2 | delta1 (at 384) delta2 (at 448) | count (big-endian) | K | 12 B | two G2
static constexpr size_t VK_DELTA1 = 384, VK_DELTA2 = 448, VK_FIXED = 576;
inline bool vk_layout_ok(const uint8_t* b, size_t len) {
  if (len < VK_FIXED + 4) return false;
  const uint64_t nk = sc_load_be32(b + VK_FIXED);
  return nk >= 2 && (uint64_t)len == VK_FIXED + 4 + nk * 64 + 12 + 256;
}

// Verdict of the structural comparison (step 1 of the verifier): SC_DIFF_FORMAT when a key does not parse, SC_DIFF_OTHER when the
// two differ anywhere outside delta1, delta2, the K points and the Z points (lengths and counts included), else SC_DIFF_OK with
// *L = the layout both share.
static constexpr int SC_DIFF_OK = 0, SC_DIFF_FORMAT = 1, SC_DIFF_OTHER = 2;
inline int sppk_delta_diff(const uint8_t* before, size_t nb, const uint8_t* after, size_t na, SppkLayout* L) {
  SppkLayout A;
  if (!sppk_layout(before, nb, L) || !sppk_layout(after, na, &A)) return SC_DIFF_FORMAT;
  if (na != nb) return SC_DIFF_OTHER;
  // the ranges a contribution may change, in file order; everything between them must be equal (the counts and wire lists with it)
  const size_t lo[4] = {L->delta1, L->delta2, L->k_points, L->z_points};
  const size_t hi[4] = {L->delta1 + 64, L->delta2 + 128, L->k_points + (size_t)L->n_k * 64, L->z_points + (size_t)L->n_z * 64};
  size_t at = 0;
  for (int s = 0; s < 4; s++) {
    if (memcmp(before + at, after + at, lo[s] - at) != 0) return SC_DIFF_OTHER;
    at = hi[s];
  }
  if (memcmp(before + at, after + at, nb - at) != 0) return SC_DIFF_OTHER;
  return SC_DIFF_OK;
}
// The same for the verifying keys: true when `after` has the layout and equals `before` outside delta1 | delta2
inline bool vk_delta_diff_ok(const uint8_t* before, size_t nb, const uint8_t* after, size_t na) {
  if (!vk_layout_ok(before, nb) || !vk_layout_ok(after, na) || na != nb) return false;
  return memcmp(before, after, VK_DELTA1) == 0 && memcmp(before + VK_FIXED, after + VK_FIXED, nb - VK_FIXED) == 0;
}

}  // namespace spp
