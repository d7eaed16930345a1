// Publicly checkable (Pedersen) sharing of the auditors' RLWE key: the two generators, the common polynomial a from a seed, the
// fixed-base window table, the commitment c G + c' H read off that table, and the receiver's check of one value
// (kernels_vss.hip has the kernels, spp_vss_api.cpp the calls, include/spp.h the protocol).
//
// A dealing of n values with threshold t publishes C_k[v] = c_k[v] G + c'_k[v] H, k < t, and sends receiver x the evaluations
// y = sum_k c_k x^k, y' = sum_k c'_k x^k (two launches of the Shamir kernel).  The receiver accepts iff
// y G + y' H == sum_k x^k C_k.  Every scalar on the left of both equations is full size and per lane, and the two bases never
// change, so nothing is doubled at run time: the table holds d 2^(8 w) B for both bases B, the 32 byte positions w and the 255
// non-zero bytes d, in affine form (2 * 32 * 255 = 16 320 points of 64 B, 1 020 KB: it stays in L2).  A commitment is then at
// most 64 mixed additions; pt_mul_each (ptau.hpp) would pay 2 x (254 doublings + ~254 additions) for it, some lane of a wave
// adding in almost every step.  A scalar arrives as the 32 big-endian bytes of the ABI, and byte 31 - w of it IS window w:
// nothing is recoded.  A zero byte adds nothing.
//
// The addition is XYZZ::madd (bn254.hpp), which doubles for an accumulator equal to the entry and returns infinity for the
// opposite one; the accumulator starts at infinity and may come back to it (c = c' = 0 is the point at infinity, 64 zero bytes).
// The right side of the check is Horner over points: acc <- x acc + C_k from k = t - 1 down.  x is a 32-bit share index, so the
// product is an MSB-first double-and-add of x's own bit length over XYZZ::add, the same in every lane of a launch (x is the
// receiver's).  Crafted dealings make the accumulator meet its next term (C_0 = +-x C_1) or make a C_k infinity: add and madd
// take their equal / opposite / infinity branches there, and tests/host/vss_check.cpp pins that.
//
// The table is indexed by bytes of secret scalars, so the addresses a dealing reads depend on them.
//
// The last section is the committee's view of the same commitments and the hand-over of the key to a new committee.
//
// Host and device: everything below is SPP_HD or plain C++, so that tests/host/vss_check.cpp and tests/host/reshare_check.cpp pin
// it against big integers.
#pragma once
#include <string.h>
#include "bn254.hpp"
#include "ptau.hpp"
#include "sha256.hpp"
#include "setup_contrib.hpp"

namespace spp {

static constexpr uint32_t VSS_WINDOW_BITS = 8, VSS_WINDOWS = 32, VSS_DIGITS = 255;
static constexpr uint32_t VSS_BASE_G = 0, VSS_BASE_H = 1;
static constexpr uint32_t VSS_TABLE_POINTS = 2 * VSS_WINDOWS * VSS_DIGITS;   // 16 320
static constexpr uint32_t VSS_FLAG_BAD_POINT = 1, VSS_FLAG_BAD_SHARE = 2, VSS_FLAG_NOT_ZERO = 4;   // SPP_VSS_* of include/spp.h
static constexpr uint32_t VSS_RLWE_N = 1024, VSS_RLWE_Q = 167772161u;

// ----------------------------------------------------------------------------------------------------------------------
// generators (host only)
// ----------------------------------------------------------------------------------------------------------------------
inline G1Affine vss_generator_g() { return {Fq::from_u64(1), Fq::from_u64(2)}; }
// H: x = SHA-256("spp-vss-pedersen-h" | ctr, 4 bytes big-endian) mod p for ctr = 0, 1, ... until x^3 + 3 is a square;
// y = the smaller root.  p = 3 mod 4, so a root of v is v^((p + 1) / 4) when there is one.  *ctr_out: the counter that gave it (1).
inline G1Affine vss_generator_h(uint32_t* ctr_out = nullptr) {
  uint32_t e[8];   // (p + 1) / 4
  for (int i = 0; i < 8; i++) e[i] = FqParams::MOD(i);
  e[0] += 1;       // p ends in ...47: no carry
  for (int i = 0; i < 7; i++) e[i] = (e[i] >> 2) | (e[i + 1] << 30);
  e[7] >>= 2;
  for (uint32_t ctr = 0;; ctr++) {
    uint8_t msg[22], dig[32];
    memcpy(msg, "spp-vss-pedersen-h", 18);
    for (int i = 0; i < 4; i++) msg[18 + i] = (uint8_t)(ctr >> (24 - 8 * i));
    sha256_bytes(msg, sizeof msg, dig);
    const Fq x = Fq::from_bytes_be(dig);   // reduces mod p
    const Fq v = x.sqr() * x + Fq::from_u64(3);
    Fq y = Fq::one(), b = v;
    for (int w = 0; w < 8; w++)
      for (int i = 0; i < 32; i++) {
        if ((e[w] >> i) & 1u) y = y * b;
        b = b.sqr();
      }
    if (!(y.sqr() == v)) continue;
    uint32_t c[8];
    y.to_canonical(c);
    if (canonical_gt_half<FqParams>(c)) y = y.neg();
    if (ctr_out) *ctr_out = ctr;
    return {x, y};
  }
}

// ----------------------------------------------------------------------------------------------------------------------
// the common a of a joint key (host only)
// ----------------------------------------------------------------------------------------------------------------------
// SHA-256("spp-dkg-a" | seed | ctr, 4 bytes big-endian), ctr = 0, 1, ...: each digest is eight big-endian words, masked to 28 bits,
// kept when below q; the first 1024 kept are a
inline void vss_a_from_seed(const uint8_t seed[32], uint32_t a[VSS_RLWE_N]) {
  uint8_t msg[9 + 32 + 4], dig[32];
  memcpy(msg, "spp-dkg-a", 9);
  memcpy(msg + 9, seed, 32);
  uint32_t got = 0;
  for (uint32_t ctr = 0; got < VSS_RLWE_N; ctr++) {
    for (int i = 0; i < 4; i++) msg[41 + i] = (uint8_t)(ctr >> (24 - 8 * i));
    sha256_bytes(msg, sizeof msg, dig);
    for (int w = 0; w < 8 && got < VSS_RLWE_N; w++) {
      const uint32_t v = sc_load_be32(dig + 4 * w) & 0x0fffffffu;
      if (v < VSS_RLWE_Q) a[got++] = v;
    }
  }
}

// ----------------------------------------------------------------------------------------------------------------------
// the window table
// ----------------------------------------------------------------------------------------------------------------------
SPP_HD uint32_t vss_table_index(uint32_t base, uint32_t w, uint32_t d) { return (base * VSS_WINDOWS + w) * VSS_DIGITS + (d - 1u); }
// the 64 window bases 2^(8 w) B, G's first then H's (host: 8 doublings each; the device multiplies them by d)
inline void vss_window_bases(G1Affine out[2 * VSS_WINDOWS]) {
  const G1Affine gen[2] = {vss_generator_g(), vss_generator_h()};
  for (uint32_t b = 0; b < 2; b++) {
    G1XYZZ run = G1XYZZ::from_affine(gen[b]);
    for (uint32_t w = 0; w < VSS_WINDOWS; w++) {
      out[b * VSS_WINDOWS + w] = run.to_affine();
      for (uint32_t i = 0; i < VSS_WINDOW_BITS; i++) run.dbl_inplace();
    }
  }
}
// entry i of the table from the window bases: d * 2^(8 w) B, 1 <= d <= 255, by the bit loop of ptau.hpp on d's eight bits
SPP_HD G1Affine vss_table_entry(const G1Affine* wbases, uint32_t i) {
  const uint32_t d = i % VSS_DIGITS + 1u;
  return pt_mul_bits(wbases[i / VSS_DIGITS], &d, VSS_WINDOW_BITS).to_affine();
}

// ----------------------------------------------------------------------------------------------------------------------
// c G + c' H off the table
// ----------------------------------------------------------------------------------------------------------------------
// acc += k B for the scalar whose 32 big-endian bytes are at k_be (k < r is the caller's check; any 256-bit value is summed right)
SPP_HD void vss_add_fixed(G1XYZZ& acc, const G1Affine* table, uint32_t base, const uint8_t* k_be) {
#if defined(__HIPCC__)
#pragma unroll 1
#endif
  for (uint32_t w = 0; w < VSS_WINDOWS; w++) {
    const uint32_t d = k_be[31u - w];
    if (d) acc.madd(table[vss_table_index(base, w, d)]);
  }
}
SPP_HD G1XYZZ vss_commit(const G1Affine* table, const uint8_t* c_be, const uint8_t* cb_be) {
  G1XYZZ acc = G1XYZZ::infinity();
  vss_add_fixed(acc, table, VSS_BASE_G, c_be);
  vss_add_fixed(acc, table, VSS_BASE_H, cb_be);
  return acc;
}
// X | Y big-endian, 64 zero bytes for infinity (what sc_decode_point reads back)
SPP_HD void vss_store_point(const G1XYZZ& p, uint8_t out[64]) {
  const G1Affine a = p.to_affine();
  if (a.is_inf()) {
    for (int i = 0; i < 64; i++) out[i] = 0;
    return;
  }
  a.x.to_bytes_be(out);
  a.y.to_bytes_be(out + 32);
}

// ----------------------------------------------------------------------------------------------------------------------
// the receiver's check of one value of one dealer
// ----------------------------------------------------------------------------------------------------------------------
SPP_HD bool vss_same_point(const G1XYZZ& a, const G1XYZZ& b) {
  if (a.is_inf() || b.is_inf()) return a.is_inf() && b.is_inf();
  return a.X * b.ZZ == b.X * a.ZZ && a.Y * b.ZZZ == b.Y * a.ZZZ;
}
SPP_HD uint32_t vss_bit_length(uint32_t x) {
  uint32_t n = 0;
  while (n < 32 && (x >> n)) n++;
  return n;
}
// x * p, MSB-first over x's own bits; xbits = vss_bit_length(x) >= 1
SPP_HD G1XYZZ vss_mul_small(const G1XYZZ& p, uint32_t x, uint32_t xbits) {
  G1XYZZ r = p;   // the top bit
#if defined(__HIPCC__)
#pragma unroll 1
#endif
  for (uint32_t b = xbits - 1u; b-- > 0;) {
    r.dbl_inplace();
    if ((x >> b) & 1u) r.add(p);
  }
  return r;
}
// commitments: C_k of this value at commitments + k * stride (64 B each), k < t; y_be, yb_be: the sub-share and its blind;
// zero_be: the published constant-term blind of a refresh, or nullptr.  Returns the VSS_FLAG_* bits; a commitment that is no
// point ends the check (VSS_FLAG_BAD_POINT alone).
// The Horner walk both the receiver's check and the share commitments use: *acc = sum_k x^k C_k, *c0 = C_0; false (and nothing
// more read) at the first commitment that is no point.
SPP_HD bool vss_eval_commitments(uint32_t t, uint32_t x, const uint8_t* commitments, size_t stride, G1XYZZ* acc_out, G1Affine* c0) {
  const uint32_t xbits = vss_bit_length(x);
  G1XYZZ acc = G1XYZZ::infinity();
  G1Affine c;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
  for (uint32_t k = t; k-- > 0;) {
    if (sc_decode_point(commitments + (size_t)k * stride, &c) == SC_POINT_BAD) return false;
    if (!acc.is_inf()) acc = vss_mul_small(acc, x, xbits);
    acc.madd(c);
  }
  *acc_out = acc;
  *c0 = c;
  return true;
}
SPP_HD uint32_t vss_check_value(const G1Affine* table, uint32_t t, uint32_t x, const uint8_t* commitments, size_t stride, const uint8_t* y_be,
                                const uint8_t* yb_be, const uint8_t* zero_be) {
  G1XYZZ acc;
  G1Affine c;
  if (!vss_eval_commitments(t, x, commitments, stride, &acc, &c)) return VSS_FLAG_BAD_POINT;
  uint32_t flags = 0;
  if (!vss_same_point(vss_commit(table, y_be, yb_be), acc)) flags |= VSS_FLAG_BAD_SHARE;
  if (zero_be) {   // c holds C_0
    G1XYZZ zh = G1XYZZ::infinity();
    vss_add_fixed(zh, table, VSS_BASE_H, zero_be);
    if (!vss_same_point(zh, G1XYZZ::from_affine(c))) flags |= VSS_FLAG_NOT_ZERO;
  }
  return flags;
}

// ----------------------------------------------------------------------------------------------------------------------
// the committee's commitments, and handing the key to a new committee
// ----------------------------------------------------------------------------------------------------------------------
// D_k[v] = sum_i C_{i,k}[v] commits to coefficient k of the ONE polynomial whose value at 0 is the key and at x_j auditor j's
// share; E_x[v] = sum_k x^k D_k[v] (vss_eval_commitments) is what share_j G + blind_j H must equal.  A member j of a set S of t old
// members deals (share_j, blind_j) to the new committee, so its C'_{j,0} is E_{x_j}; the new committee's commitments are
// D'_k[v] = sum_{j in S} lambda_j C'_{j,k}[v] with lambda_j the Lagrange coefficient at 0 of x_j in S.
//
// That last sum is the only one here with full-size scalars on variable points, and its scalars are the same for every output
// point: the weight of dealer d does not depend on (k, v).  So the lanes of a wave share ONE MSB-first scan over the 254 bits:
// one doubling per bit, and for each dealer whose bit is set one mixed addition of the lane's own point of that dealer.  The
// weights are read through a pointer that is the same in every lane (scalar loads), every branch on a bit is the wave's, and
// nothing diverges but the equal / opposite / infinity branches inside madd.  pt_mul_each per dealer would pay the 254 doublings
// `dealers` times over, and a general addition per dealer on top.  weights == nullptr is the sum itself (the committee of a key
// or of a refresh round): `dealers` mixed additions and no scan.  A weight of 0 has no bit set and adds nothing.
static constexpr uint32_t VSS_FLAG_NOT_SHARE = 8;   // SPP_VSS_NOT_SHARE
static constexpr uint32_t VSS_LINCOMB_MAX = 64;      // dealers of a weighted sum

// raw[64] -> Montgomery form for the sums below; SPP_VSS_BAD_POINT (and infinity in *out) when it is no point, else 0
SPP_HD uint32_t vss_decode(const uint8_t raw[64], G1Affine* out) {
  return sc_decode_point(raw, out) == SC_POINT_BAD ? VSS_FLAG_BAD_POINT : 0u;
}
// base (optional) + sum_d w_d points[d * stride]; weights: dealers * 8 canonical words, least significant first, or nullptr (all 1)
SPP_HD G1XYZZ vss_lincomb(uint32_t dealers, const uint32_t* weights, const G1Affine* points, size_t stride, const G1Affine* base) {
  G1XYZZ acc = G1XYZZ::infinity();
  if (weights) {
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (uint32_t b = 254; b-- > 0;) {   // r < 2^254
      acc.dbl_inplace();
#if defined(__HIPCC__)
#pragma unroll 1
#endif
      for (uint32_t d = 0; d < dealers; d++)
        if ((weights[8u * d + (b >> 5)] >> (b & 31u)) & 1u) acc.madd(points[(size_t)d * stride]);
    }
  } else {
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (uint32_t d = 0; d < dealers; d++) acc.madd(points[(size_t)d * stride]);
  }
  if (base) acc.madd(*base);
  return acc;
}
// the new member's extra check of old member x_old's dealing: is its constant term C'_0 (c0_raw) the public share commitment
// E_{x_old} under the old committee's commitments?  0 or VSS_FLAG_NOT_SHARE; a committee entry or a C'_0 that is no point: BAD_POINT
SPP_HD uint32_t vss_is_share(uint32_t t_old, uint32_t x_old, const uint8_t* committee, size_t stride, const uint8_t* c0_raw) {
  G1XYZZ e;
  G1Affine d0, c0;
  if (!vss_eval_commitments(t_old, x_old, committee, stride, &e, &d0)) return VSS_FLAG_BAD_POINT;
  if (sc_decode_point(c0_raw, &c0) == SC_POINT_BAD) return VSS_FLAG_BAD_POINT;
  return vss_same_point(e, G1XYZZ::from_affine(c0)) ? 0u : VSS_FLAG_NOT_SHARE;
}
// lambda_j = prod_{i != j} x_i / (x_i - x_j) for distinct non-zero xs (host only)
inline void vss_lagrange_at_zero(const uint32_t* xs, uint32_t count, Fr* out) {
  for (uint32_t j = 0; j < count; j++) {
    Fr num = Fr::one(), den = Fr::one();
    for (uint32_t i = 0; i < count; i++)
      if (i != j) {
        num = num * Fr::from_u64(xs[i]);
        den = den * (Fr::from_u64(xs[i]) - Fr::from_u64(xs[j]));
      }
    out[j] = num * den.inv();
  }
}
// out = sum_d w_d y_d mod r over big-endian values `stride` bytes apart
SPP_HD void vss_weighted_sum(uint32_t dealers, const Fr* weights, const uint8_t* ys_be, size_t stride, uint8_t out_be[32]) {
  uint8_t buf[32];
  Fr acc = Fr::zero();
  for (uint32_t d = 0; d < dealers; d++) {
    for (int i = 0; i < 32; i++) buf[i] = ys_be[(size_t)d * stride + i];
    acc = acc + weights[d] * Fr::from_bytes_be(buf);
  }
  acc.to_bytes_be(out_be);
}

}  // namespace spp
