// Batch verification by random linear combination (RLC), host + gfx950: the reference form of the whole scheme.
// Serves `sunspot verify <vk> <proof> <pw>` (noir_circuit/prove_linux.sh:86-87, audit_circuit/prove_audit.sh:98-99) for many
// proofs against one key, like verify_one.hpp, whose decisions it reproduces except with probability about 2^-127 per call.
//
// With secret 128-bit scalars r_i, s_i per proof, the stage-2 (Pedersen proof of knowledge) and stage-4 (Groth16) equations of
// all proofs of a group hold iff (up to that probability)
//     prod_i e(r_i Ar_i, Bs_i) * e(-(sum r_i) alpha, beta) * e(-Kagg, gamma) * e(-sum r_i Krs_i, delta)
//       * e(sum s_i PoK_i, G) * e(sum s_i Cm_i, GSigmaNeg) == 1
//     Kagg = (sum r_i) K[0] + sum_k (sum_i r_i pub_ik) K[k+1] + (sum_i r_i c_i) K[nk-1] + sum r_i Cm_i
// c_i the BSB22 challenge of Cm_i.  Per proof that leaves the format / curve / subgroup checks, one dynamic-pair Miller loop,
// five 128-bit G1 scalar multiplications and a few Fr products (rlc_term); the five key-side pairings and the final
// exponentiation are paid once per group (rlc_final_serial here on one lane, f12_coop.hpp wave-wide).
//
// A term is 28 + nk elements of 32 bytes (RlcLayout): the Miller value, the four points r Krs, r Cm, s Cm, s PoK in XYZZ, and
// the Fr words r, r pub_k, r c.  Element e of proof i sits at ws[e * stride + i] (batch-minor); a folded group has stride 1.
#pragma once
#include "verify_one.hpp"

namespace spp {

struct W256 {
  uint32_t l[8];
};
// the beta pair of the combined equation, beside VerifyKeyDev (k_verify's argument stays what it is)
struct RlcKeyDev {
  const LineStep* tab_beta;   // line table of beta2
  G1Affine neg_alpha;         // -alpha1
};
struct RlcSeed {
  uint8_t b[32];
};
static constexpr uint32_t RLC_E_MILLER = 0, RLC_E_POINTS = 12, RLC_E_WORDS = 28;   // element offsets of a term
static constexpr uint32_t RLC_P_RKRS = 0, RLC_P_RCM = 1, RLC_P_SCM = 2, RLC_P_SPOK = 3;
static constexpr uint32_t RLC_MAX_NK = 36;                                         // a term is at most 64 elements
SPP_HD uint32_t rlc_elems(uint32_t nk) { return RLC_E_WORDS + nk; }

template <class F>
SPP_HD W256 w256_of(const F& a) {
  W256 w;
  for (int i = 0; i < 8; i++) w.l[i] = a.l[i];
  return w;
}
template <class F>
SPP_HD F w256_as(const W256& w) {
  F a;
  for (int i = 0; i < 8; i++) a.l[i] = w.l[i];
  return a;
}
SPP_HD void rlc_put_point(W256* out, size_t stride, uint32_t which, const G1XYZZ& p) {
  W256* o = out + (size_t)(RLC_E_POINTS + 4 * which) * stride;
  o[0] = w256_of(p.X);
  o[stride] = w256_of(p.Y);
  o[2 * stride] = w256_of(p.ZZ);
  o[3 * stride] = w256_of(p.ZZZ);
}
SPP_HD G1XYZZ rlc_get_point(const W256* in, size_t stride, uint32_t which) {
  const W256* o = in + (size_t)(RLC_E_POINTS + 4 * which) * stride;
  return {w256_as<Fq>(o[0]), w256_as<Fq>(o[stride]), w256_as<Fq>(o[2 * stride]), w256_as<Fq>(o[3 * stride])};
}

// (r_i, s_i): the two 128-bit halves of SHA-256(seed[32] || be32(i) || "spp-rlc-scalars1"), little-endian limbs; a zero half -> 1
SPP_HDN void rlc_scalars(const uint8_t seed[32], uint32_t index, uint32_t r[4], uint32_t s[4]) {
  constexpr char tag[17] = "spp-rlc-scalars1";
  uint32_t blk[16];
  for (int i = 0; i < 8; i++) blk[i] = be32_at(seed + 4 * i);
  blk[8] = index;
  for (int i = 0; i < 4; i++)
    blk[9 + i] = ((uint32_t)(uint8_t)tag[4 * i] << 24) | ((uint32_t)(uint8_t)tag[4 * i + 1] << 16) | ((uint32_t)(uint8_t)tag[4 * i + 2] << 8) |
                 (uint32_t)(uint8_t)tag[4 * i + 3];
  blk[13] = 0x80000000u;
  blk[14] = 0;
  blk[15] = 52 * 8;
  Sha256 h;
  h.init();
  h.compress(blk);
  for (int i = 0; i < 4; i++) {
    r[i] = h.h[3 - i];
    s[i] = h.h[7 - i];
  }
  if ((r[0] | r[1] | r[2] | r[3]) == 0) r[0] = 1;
  if ((s[0] | s[1] | s[2] | s[3]) == 0) s[0] = 1;
}
// scalar_mul_rolled for a 128-bit scalar
SPP_HDN G1XYZZ g1_scalar_mul128(const G1Affine& p, const uint32_t k[4]) {
  G1XYZZ acc = G1XYZZ::infinity();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int w = 3; w >= 0; w--) {
    const uint32_t kw = w == 3 ? k[3] : w == 2 ? k[2] : w == 1 ? k[1] : k[0];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int b = 31; b >= 0; b--) {
      xyzz_dbl_call(acc);
      if ((kw >> b) & 1) xyzz_madd_call(acc, p);
    }
  }
  return acc;
}
SPP_HDN void g1_add_call(G1XYZZ& a, const G1XYZZ& b) { a.add(b); }
SPP_HDN G1Affine g1_to_affine_call(const G1XYZZ& a) { return a.to_affine(); }

// One proof's term.  Makes the checks of verify_one steps 0-1 unchanged; a proof that fails them is DROPPED: false, nothing
// written.  Points at infinity behave as in miller_multi / madd: a pair with Ar or Bs at infinity contributes 1, a point at
// infinity adds nothing to its sum.
SPP_HDN bool rlc_term(const VerifyKeyDev& vk, const uint8_t* proof, const uint8_t* pw, const uint8_t seed[32], uint32_t index, W256* out,
                      size_t stride) {
  const PairingFastConsts& pc = vk.pc;
  const uint32_t npub = vk.nk - 2;
  if (be32_at(proof + 256) != 1) return false;
  if (be32_at(pw) != npub || be32_at(pw + 4) != 0 || be32_at(pw + 8) != npub) return false;
  for (int o = 0; o < 388; o += 32) {
    if (o == 256) o = 260;
    if (!be_is_canonical<FqParams>(proof + o)) return false;
  }
  for (uint32_t k = 0; k < npub; k++)
    if (!be_is_canonical<FrParams>(pw + 12 + 32 * k)) return false;
  const G1Affine Ar = g1_from_raw_hd(proof), Krs = g1_from_raw_hd(proof + 192), Cm = g1_from_raw_hd(proof + 260),
                 Pok = g1_from_raw_hd(proof + 324);
  const G2Affine Bs = g2_from_raw_hd(proof + 64);
  if (!g1_on_curve_hd(Ar, pc) || !g1_on_curve_hd(Krs, pc) || !g1_on_curve_hd(Cm, pc) || !g1_on_curve_hd(Pok, pc)) return false;
  if (!g2_on_curve_hd(Bs, vk.twist_b) || !g2_in_subgroup(Bs)) return false;

  uint32_t r[4], s[4];
  rlc_scalars(seed, index, r, s);
  {
    const G1Affine rAr = g1_to_affine_call(g1_scalar_mul128(Ar, r));
    const F12 m = miller_multi(0, nullptr, nullptr, true, rAr, Bs, f12_one(pc), pc);
    for (int i = 0; i < 12; i++) out[(size_t)(RLC_E_MILLER + i) * stride] = w256_of(m.c[i]);
  }
  rlc_put_point(out, stride, RLC_P_RKRS, g1_scalar_mul128(Krs, r));
  rlc_put_point(out, stride, RLC_P_RCM, g1_scalar_mul128(Cm, r));
  rlc_put_point(out, stride, RLC_P_SCM, g1_scalar_mul128(Cm, s));
  rlc_put_point(out, stride, RLC_P_SPOK, g1_scalar_mul128(Pok, s));
  uint32_t lim[8];
  for (int i = 0; i < 8; i++) lim[i] = i < 4 ? r[i] : 0;
  const Fr rf = Fr::from_canonical(lim);
  uint32_t m16[16];
  for (int k = 0; k < 16; k++) m16[k] = be32_at(proof + 260 + 4 * k);
  W256* words = out + (size_t)RLC_E_WORDS * stride;
  words[0] = w256_of(rf);
  for (uint32_t k = 0; k < npub; k++) {
    uint8_t t[32];
    for (int b = 0; b < 32; b++) t[b] = pw[12 + 32 * k + b];
    words[(size_t)(1 + k) * stride] = w256_of(rf * Fr::from_bytes_be(t));
  }
  words[(size_t)(1 + npub) * stride] = w256_of(rf * bsb22_challenge(m16));
  return true;
}

// The product of the Miller values and the sums of the points and words of the live terms first .. first + n - 1
// (live[i] != 0), as one term with stride 1.  No live term: the neutral term.
inline void rlc_fold(const VerifyKeyDev& vk, const W256* ws, size_t stride, const uint32_t* live, size_t first, size_t n, W256* folded) {
  const PairingFastConsts& pc = vk.pc;
  F12 m = f12_one(pc);
  G1XYZZ pt[4] = {G1XYZZ::infinity(), G1XYZZ::infinity(), G1XYZZ::infinity(), G1XYZZ::infinity()};
  Fr words[RLC_MAX_NK];
  for (uint32_t k = 0; k < vk.nk; k++) words[k] = Fr::zero();
  for (size_t i = first; i < first + n; i++) {
    if (!live[i]) continue;
    const W256* t = ws + i;
    F12 mi;
    for (int e = 0; e < 12; e++) mi.c[e] = w256_as<Fq>(t[(size_t)(RLC_E_MILLER + e) * stride]);
    m = f12_mul(m, mi, pc);
    for (uint32_t p = 0; p < 4; p++) pt[p].add(rlc_get_point(t, stride, p));
    for (uint32_t k = 0; k < vk.nk; k++) words[k] = words[k] + w256_as<Fr>(t[(size_t)(RLC_E_WORDS + k) * stride]);
  }
  for (int e = 0; e < 12; e++) folded[RLC_E_MILLER + e] = w256_of(m.c[e]);
  for (uint32_t p = 0; p < 4; p++) rlc_put_point(folded, 1, p, pt[p]);
  for (uint32_t k = 0; k < vk.nk; k++) folded[RLC_E_WORDS + k] = w256_of(words[k]);
}

// the G1 arguments of the five key-side pairings, in table order gamma, delta, G, GSigmaNeg, beta; kparts[k] = S_k K[k] for
// k < nk and kparts[nk] = S_0 (-alpha) are the scalar multiplications (one lane each in the group kernel)
SPP_HDN void rlc_key_scalar_mul(const VerifyKeyDev& vk, const RlcKeyDev& rk, const W256* folded, uint32_t k, G1XYZZ& out) {
  const Fr s = w256_as<Fr>(folded[RLC_E_WORDS + (k < vk.nk ? k : 0)]);
  out = g1_scalar_mul_fr(k < vk.nk ? vk.K[k] : rk.neg_alpha, s);
}
SPP_HDN void rlc_tail_point(const W256* folded, const G1XYZZ& kagg, const G1XYZZ& alpha_r, uint32_t k, G1Affine& out) {
  const G1XYZZ p = k == 0 ? kagg.neg() : k == 1 ? rlc_get_point(folded, 1, RLC_P_RKRS).neg() : k == 2 ? rlc_get_point(folded, 1, RLC_P_SPOK)
                 : k == 3 ? rlc_get_point(folded, 1, RLC_P_SCM) : alpha_r;
  out = g1_to_affine_call(p);
}
// One lane: Kagg and (sum r)(-alpha), the five-table Miller loop with the folded Miller value as `extra`, the final exponentiation.
// The yardstick of the cooperative tail.
SPP_HDN bool rlc_final_serial(const VerifyKeyDev& vk, const RlcKeyDev& rk, const W256* folded) {
  const PairingFastConsts& pc = vk.pc;
  G1XYZZ kagg = rlc_get_point(folded, 1, RLC_P_RCM), part, alpha_r;
  for (uint32_t k = 0; k < vk.nk; k++) {
    rlc_key_scalar_mul(vk, rk, folded, k, part);
    g1_add_call(kagg, part);
  }
  rlc_key_scalar_mul(vk, rk, folded, vk.nk, alpha_r);
  const LineStep* tabs[5] = {vk.tab[0], vk.tab[1], vk.tab[2], vk.tab[3], rk.tab_beta};
  G1Affine Ps[5];
  for (uint32_t k = 0; k < 5; k++) rlc_tail_point(folded, kagg, alpha_r, k, Ps[k]);
  F12 extra;
  for (int e = 0; e < 12; e++) extra.c[e] = w256_as<Fq>(folded[RLC_E_MILLER + e]);
  const F12 f = miller_multi(5, tabs, Ps, false, G1Affine::infinity(), G2Affine::infinity(), extra, pc);
  return final_exp_is_one(f, pc);
}

}  // namespace spp
