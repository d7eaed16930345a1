// Threshold opening of an audit ciphertext, host + gfx950: the per-lane pieces of k_rlwe_partial and k_rlwe_combine
// (kernels_witness.hip) and of the host check tests/host/partial_decrypt_check.cpp.  Each of t auditors holds one Shamir share
// s_i of the RLWE secret key (1024 values of Fr, rlwe_keygen.py:51-65) and nobody rebuilds the key: with lambda_i the Lagrange
// coefficient at 0 of the participating set, sk = sum_i lambda_i s_i coefficient by coefficient over Fr, and the negacyclic
// product is linear, so
//     sum_i lambda_i (s_i * c1)[k] = (sk * c1)[k]   over Fr, for the 64 message slots k.
// The right side is an integer of absolute value below 2^66 (a key below q: 1024 * 2^28 * 2^28), so its centred lift from Fr is
// the exact product and its residue mod q is what ao_decrypt_slot (audit_open.hpp) sums.  Nothing is approximated.
//
//   scaled share   u[j] = lambda_i s_i[j], canonical in [0, r)                                      rp_scaled_share
//   partial        p_i[k] = (u * c1)[k] + blind_i[k]  mod r                                          rp_dot_slot + rp_blind_slot
//   blind          e + q rho + sum_{j in S, j != i} sgn(x_i, x_j) M(seed_ij, ct_commitment, k)      e int32, rho uint64: the caller's
//   combination    w = sum_i p_i[k] over Fr, centred; |w| < 2^104 or the slot is inconsistent;        rp_combine_residue
//                  (w mod q, c0[k]) -> the byte by ao_round_slot
// The pairwise masks M cancel in the sum over S (sgn(x_i, x_j) = -sgn(x_j, x_i), both ends hold seed_ij), q rho vanishes mod q,
// and e joins the ciphertext's noise.  Honest partials sum to |w| < 2^66 + 64 (2^31 + q 2^64) < 2^99.
//
// The wide dot product (rp_dot_slot).  Slot k of u * c1 mod X^1024 + 1 is P - N with
//     P = sum_{j <= k} u[k - j] c1[j],   N = sum_{j > k} u[1024 + k - j] c1[j],
// both taken as unreduced integers and reduced mod r once.  The table is limb-major, U[1024 i + j] = limb i (32 bits) of u[j]:
// lane k of a wave reads index (k - j) mod 1024 at step j, so the 64 lanes read 64 consecutive words of one limb row -- 64
// different LDS banks -- and c1[j] is one address for the whole wave.  Bounds, with u < 2^254 in eight 32-bit limbs and
// c1[j] < 2^28:
//   - a column a[i] (64 bits) takes limb_i * c1[j] < (2^32 - 1)(2^28 - 1) < 2^60 - 2^32 per term;
//   - rp_wide_fold, every RP_FOLD = 16 terms, moves a[i] >> 32 into a[i + 1] and leaves a[i] < 2^32 (i = 0..8; a[9] is the
//     top and is never cut).  A column therefore holds at most  2^32 (kept) + 2^32 (carry in) + 16 (2^60 - 2^32) < 2^64
//     before the next fold: the carries stay lazy for 16 terms and never wrap;
//   - P, N < 1024 * 2^254 * 2^28 = 2^292: ten limbs, a[9] < 2^4 after the last fold;
//   - rp_wide_to_fr: limbs 0..7 as a 256-bit value (Fr::from_u256) plus limbs 8..9 (< 2^36, canonical as they stand) times
//     2^256 -- the split fr_from_wide48 (sha256.hpp) makes.
// For j < 64 the lanes of a wave disagree on the side a term belongs to (j <= k or not), so both sides run there, one of
// them with c1[j] replaced by 0: 64 doubled terms of 1024, and one instruction stream for the wave.
#pragma once
#include "audit_open.hpp"
#include "sha256.hpp"

namespace spp {

static constexpr uint32_t RP_LIMBS = 8, RP_ACC = 10, RP_FOLD = 16;
static constexpr uint32_t RP_TABLE_WORDS = RP_LIMBS * AO_N;              // 32 KB
static constexpr uint32_t RP_PARTIAL_LEN = 32;
static constexpr uint32_t RP_MAX_T = 64;
static constexpr uint32_t RP_BAD_PARTIALS = 8;                           // SPP_AUDIT_BAD_PARTIALS
static constexpr uint32_t RP_COOP_SPONGE_MAX = 2048;                     // records up to which k_rlwe_partial hashes its own ciphertext
static constexpr uint32_t RP_SMALL_BITS = 104;                           // a combined slot is an integer below 2^104 in absolute value
static_assert(AO_N % RP_FOLD == 0 && AO_SLOTS % RP_FOLD == 0, "whole folds on both sides of slot 63");

// the tag of the pairwise masks: a random-oracle domain of its own (sha256.hpp lists the other two)
struct DstPartial { static SPP_HD constexpr uint32_t b(int i) { constexpr char d[17] = "spp-partial-mask"; return (uint32_t)(uint8_t)d[i]; } };

// u = lambda * s as canonical limbs; s_be: 32 B big-endian, canonical (the caller refuses anything else)
SPP_HD void rp_scaled_share(const Fr& lambda, const uint8_t* s_be, uint32_t u[RP_LIMBS]) {
  (lambda * Fr::from_bytes_be(s_be)).to_canonical(u);
}

struct RpWide {
  unsigned long long a[RP_ACC];
};
SPP_HD void rp_wide_zero(RpWide& w) {
  SPP_UNROLL for (uint32_t i = 0; i < RP_ACC; i++) w.a[i] = 0;
}
// one term: limb i of table entry idx times c (< 2^28) into column i
SPP_HD void rp_wide_madd(RpWide& w, const uint32_t* U, uint32_t idx, uint32_t c) {
  SPP_UNROLL for (uint32_t i = 0; i < RP_LIMBS; i++) w.a[i] += (unsigned long long)U[AO_N * i + idx] * c;
}
SPP_HD void rp_wide_fold(RpWide& w) {
  SPP_UNROLL for (uint32_t i = 0; i + 1 < RP_ACC; i++) {
    w.a[i + 1] += w.a[i] >> 32;
    w.a[i] &= 0xffffffffull;
  }
}
// the value mod r; w folded, below 2^292
SPP_HD Fr rp_wide_to_fr(const RpWide& w) {
  uint32_t lo[8], hi[8];
  SPP_UNROLL for (int i = 0; i < 8; i++) {
    lo[i] = (uint32_t)w.a[i];
    hi[i] = 0;
  }
  hi[0] = (uint32_t)w.a[8];
  hi[1] = (uint32_t)w.a[9];
  return Fr::from_u256(lo) + Fr::from_canonical(hi) * Fr::r2();
}

// (u * c1 mod X^1024 + 1)[k] mod r for slot k < 64.  U: the limb-major table of u (RP_TABLE_WORDS), c1[1024] below 2^28.
SPP_HD Fr rp_dot_slot(const uint32_t* U, const uint32_t* c1, uint32_t k) {
  RpWide P, N;
  rp_wide_zero(P);
  rp_wide_zero(N);
  for (uint32_t j0 = 0; j0 < AO_SLOTS; j0 += RP_FOLD) {          // both sides: lanes differ in where j <= k ends
    for (uint32_t j = j0; j < j0 + RP_FOLD; j++) {
      const uint32_t c = c1[j], idx = (k - j) & (AO_N - 1);
      const bool pos = j <= k;
      rp_wide_madd(P, U, idx, pos ? c : 0u);
      rp_wide_madd(N, U, idx, pos ? 0u : c);
    }
    rp_wide_fold(P);
    rp_wide_fold(N);
  }
  for (uint32_t j0 = AO_SLOTS; j0 < AO_N; j0 += RP_FOLD) {        // j > 63 >= k: the subtracted side only
    SPP_UNROLL for (uint32_t jj = 0; jj < RP_FOLD; jj++) rp_wide_madd(N, U, (k - (j0 + jj)) & (AO_N - 1), c1[j0 + jj]);
    rp_wide_fold(N);
  }
  return rp_wide_to_fr(P) - rp_wide_to_fr(N);
}

// the 64-byte message of one mask as sixteen big-endian words: seed_ij (32 B) | bytes 4..31 of the canonical big-endian
// ct_commitment (28 B) | k (4 B).  The commitment is the one recomputed from the c0 and c1 in hand: a mask is never reused for
// another c1.  (Bytes 0..3 of a canonical field element hold under 30 bits; the 224 that are kept leave 2^-112 for a collision.)
SPP_HD void rp_mask_message(const uint8_t* seed, const uint8_t* ct_be, uint32_t k, uint32_t m[16]) {
  for (int i = 0; i < 8; i++)
    m[i] = ((uint32_t)seed[4 * i] << 24) | ((uint32_t)seed[4 * i + 1] << 16) | ((uint32_t)seed[4 * i + 2] << 8) | seed[4 * i + 3];
  for (int i = 0; i < 7; i++) {
    const uint8_t* p = ct_be + 4 + 4 * i;
    m[8 + i] = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
  }
  m[15] = k;
}
SPP_HD Fr rp_mask(const uint8_t* seed, const uint8_t* ct_be, uint32_t k) {
  uint32_t m[16];
  rp_mask_message(seed, ct_be, k, m);
  return hash64_to_fr<DstPartial>(m);
}
// e + q rho mod r
SPP_HD Fr rp_smudge(int32_t e, unsigned long long rho) {
  const Fr v = Fr::from_u64(rho) * Fr::from_u64(AO_Q);
  return e >= 0 ? v + Fr::from_u64((unsigned long long)e) : v - Fr::from_u64((unsigned long long)(-(long long)e));
}
// the blinding of slot k for auditor `self` of the set xs[t]; seeds: t * 32 B in xs order (entry `self` is not read) or
// nullptr for no masks; the mask of a pair is added by the end with the smaller x and subtracted by the other
SPP_HD Fr rp_blind_slot(int32_t e, unsigned long long rho, uint32_t t, const uint32_t* xs, uint32_t self, const uint8_t* seeds,
                        const uint8_t* ct_be, uint32_t k) {
  Fr b = rp_smudge(e, rho);
  if (seeds)
    for (uint32_t j = 0; j < t; j++) {
      if (j == self) continue;
      const Fr m = rp_mask(seeds + 32 * (size_t)j, ct_be, k);
      b = xs[self] < xs[j] ? b + m : b - m;
    }
  return b;
}

// one combined slot: w = the canonical limbs of sum_i p_i[k].  Returns the centred value mod q, in [0, q), which is
// (sk * c1)[k] + E mod q for honest partials; *bad is raised when the centred value is not below 2^104 in absolute value -- a
// wrong share, another set, another record.  The residue is computed whatever the size (ao_centred_mod_q reduces any value).
SPP_HD uint32_t rp_combine_residue(const uint32_t w[8], bool& bad) {
  uint32_t m[8];
  if (canonical_gt_half<FrParams>(w)) canonical_negate<FrParams>(w, m);
  else { SPP_UNROLL for (int i = 0; i < 8; i++) m[i] = w[i]; }
  static_assert(RP_SMALL_BITS == 3 * 32 + 8, "limbs 0..2 and the low byte of limb 3");
  if ((m[3] >> 8) | m[4] | m[5] | m[6] | m[7]) bad = true;
  return ao_centred_mod_q(w);
}

}  // namespace spp
