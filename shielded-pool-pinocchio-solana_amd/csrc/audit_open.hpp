// Opening one audit record, host + gfx950: the per-lane pieces of k_audit_open (kernels_witness.hip) and of
// the host check tests/host/audit_open_check.cpp.  A record is what the prover of an audit proof hands to the chain and the
// auditor: (proof, public witness, ciphertext) -- scripts/generate_audit.py:590-606 writes the ciphertext next to the proof,
// scripts/rlwe_decrypt.py:61-149 opens it.  Three independent decisions (include/spp.h, SPP_AUDIT_*):
//   bit 1  the proof does not verify                                   (k_verify / verify_one.hpp; not decided here)
//   bit 2  a coefficient >= q, or sponge(pack(c0) ++ pack(c1)) != the public witness's ct_commitment
//   bit 4  the decrypted owner is not a pair of field elements on Grumpkin, or H(owner_x, owner_y) != its wa_commitment
// The two hashes themselves (Poseidon2 sponge, Poseidon t = 3) are computed by the caller -- on the device by poseidon2_permute /
// poseidon_permute29 -- and compared here, bytewise, with the words of the public witness.
#pragma once
#include "bn254.hpp"

namespace spp {

static constexpr uint32_t AO_Q = 167772161u, AO_DELTA = 655360u;      // q, Delta = q / 256 (generate_audit.py:24-33)
static constexpr uint32_t AO_N = 1024, AO_SLOTS = 64;
static constexpr uint32_t AO_CT_WORDS = AO_SLOTS + AO_N;                // one ciphertext: c0[64] then c1[1024]
static constexpr uint32_t AO_PACK_WIDTH = 7;                            // coefficients per packed field, 32 bits each
static constexpr uint32_t AO_FIELDS_C0 = 10, AO_FIELDS = 157;           // ceil(64 / 7) + ceil(1024 / 7)
static constexpr uint32_t AO_PW_WA = 12, AO_PW_CT = 44;                 // offsets of the two public words in the 76-byte .pw
static constexpr uint32_t AO_BAD_PROOF = 1, AO_BAD_CIPHERTEXT = 2, AO_BAD_IDENTITY = 4;

// a coefficient as the arithmetic below wants it; *bad is raised when it was not below q (the record then carries bit 2)
SPP_HD uint32_t ao_coeff(uint32_t v, bool& bad) {
  if (v >= AO_Q) {
    bad = true;
    v %= AO_Q;
  }
  return v;
}

// little-endian 32-bit word jw (0..7) of packed field f (0..156) of a ciphertext c0[64], c1[1024]: pack_values
// (generate_audit.py:154-163) puts coefficient 7 i + j of a polynomial at bits [32 j, 32 j + 32) of its field i; c0 fills fields
// 0..9, c1 fields 10..156.  A coefficient >= q goes in as its residue (the record carries bit 2 whatever it hashes to).
SPP_HD uint32_t ao_packed_word(const uint32_t* c0, const uint32_t* c1, uint32_t f, uint32_t jw) {
  if (jw >= AO_PACK_WIDTH) return 0;
  bool bad = false;
  if (f < AO_FIELDS_C0) {
    const uint32_t idx = AO_PACK_WIDTH * f + jw;
    return idx < AO_SLOTS ? ao_coeff(c0[idx], bad) : 0u;
  }
  const uint32_t idx = AO_PACK_WIDTH * (f - AO_FIELDS_C0) + jw;
  return idx < AO_N ? ao_coeff(c1[idx], bad) : 0u;
}
// the same field as an element of Fr (< 2^224: canonical as it stands)
SPP_HD Fr ao_packed_field(const uint32_t* c0, const uint32_t* c1, uint32_t f) {
  uint32_t w[8];
  SPP_UNROLL for (uint32_t j = 0; j < 8; j++) w[j] = ao_packed_word(c0, c1, f, j);
  return Fr::from_canonical(w);
}

// sk2[i] = sk[i], sk2[1024 + i] = (q - sk[i]) mod q: the negacyclic wrap as a second half of the table
SPP_HD void ao_sk2_entry(uint32_t s, uint32_t& lo, uint32_t& hi) {
  lo = s;
  hi = s ? AO_Q - s : 0u;
}
// the rounding tail of one slot, shared by ao_decrypt_slot and the threshold path (rlwe_partial.hpp):
//   round(centred(c0[t] + prod) / Delta) mod 256 -- floor division, then Python's round(): half to even.
// c0_t and prod = (sk * c1)[t] mod q: both below q.
SPP_HD uint8_t ao_round_slot(uint32_t c0_t, uint32_t prod) {
  const long long q = (long long)AO_Q, delta = (long long)AO_DELTA;
  long long noisy = ((long long)c0_t + (long long)prod) % q;
  if (noisy > q / 2) noisy -= q;                              // centered_mod (rlwe_decrypt.py:54-58)
  long long k = noisy / delta, rem = noisy % delta;
  if (rem < 0) {
    rem += delta;
    k -= 1;
  }
  if (2 * rem > delta || (2 * rem == delta && (k & 1))) k += 1;
  return (uint8_t)(((k % 256) + 256) % 256);
}
// message slot t of rlweDecrypt (rlwe_decrypt.py:101-118, shamir.ts:134-169), as k_rlwe_decrypt computes it:
//   (sk * c1)[t] = sum_j sk2[(t - j) mod 2048] * c1[j]   -- 28 x 28-bit products, the 64-bit sum folded mod q every 128 terms;
//   round(centred(c0[t] + (sk * c1)[t]) / Delta) mod 256 -- floor division, then Python's round(): half to even.
// c1[1024] and c0_t = c0[t]: coefficients below q.
SPP_HD uint8_t ao_decrypt_slot(const uint32_t* sk2, const uint32_t* c1, uint32_t c0_t, uint32_t t) {
  unsigned long long acc = 0, total = 0;
  for (uint32_t j = 0; j < AO_N; j++) {
    acc += (unsigned long long)sk2[(t - j) & 2047u] * c1[j];
    if ((j & 127u) == 127u) {
      total += acc % (unsigned long long)AO_Q;
      acc = 0;
    }
  }
  return ao_round_slot(c0_t, (uint32_t)(total % (unsigned long long)AO_Q));
}

// one reconstructed key coefficient as k_shamir_combine hands it to the decryption (reconstructSk, shamir.ts:97-120 /
// rlwe_decrypt.py:73-91): c, the canonical limbs of a value v of Fr, stands for v when v <= (r - 1) / 2 and for v - r above
// that; the result is that integer mod q in [0, q).  An honest coefficient has |v| <= 3; any other value is reduced all the
// same: |v| mod q by Horner over the eight limbs (the remainder stays below q < 2^28, so remainder * 2^32 + limb < 2^60), then
// q minus that on the negative side.
SPP_HD uint32_t ao_centred_mod_q(const uint32_t c[8]) {
  const bool neg = canonical_gt_half<FrParams>(c);
  uint32_t m[8];
  if (neg) canonical_negate<FrParams>(c, m);
  else { SPP_UNROLL for (int i = 0; i < 8; i++) m[i] = c[i]; }
  unsigned long long r = 0;
  for (int i = 7; i >= 0; i--) r = ((r << 32) | m[i]) % (unsigned long long)AO_Q;
  return neg ? (r ? (uint32_t)(AO_Q - (uint32_t)r) : 0u) : (uint32_t)r;
}

// where slot t of the message lands in the 64-byte owner record owner_x | owner_y, each 32 B big-endian: the slots are the
// little-endian bytes of owner_x (0..31) then of owner_y (32..63) (generate_audit.py:489-496, rlwe_decrypt.py:127-132)
SPP_HD uint32_t ao_owner_byte(uint32_t t) { return t < 32 ? 31 - t : 95 - t; }
// the two 256-bit integers as little-endian 32-bit limbs
SPP_HD void ao_owner_limbs(const uint8_t* msg, uint32_t x[8], uint32_t y[8]) {
  SPP_UNROLL for (int i = 0; i < 8; i++) {
    x[i] = (uint32_t)msg[4 * i] | ((uint32_t)msg[4 * i + 1] << 8) | ((uint32_t)msg[4 * i + 2] << 16) | ((uint32_t)msg[4 * i + 3] << 24);
    y[i] = (uint32_t)msg[32 + 4 * i] | ((uint32_t)msg[32 + 4 * i + 1] << 8) | ((uint32_t)msg[32 + 4 * i + 2] << 16) |
           ((uint32_t)msg[32 + 4 * i + 3] << 24);
  }
}
// both coordinates below r and y^2 = x^3 - 17 (Grumpkin, noir_circuit/src/main.nr:54-59): an identity key is never the point at
// infinity, so (0, 0) fails here like any other pair off the curve.  *px, *py: the coordinates as field elements when in range.
SPP_HD bool ao_owner_on_curve(const uint32_t x[8], const uint32_t y[8], Fr* px, Fr* py) {
  if (Fr::geq_mod(x) || Fr::geq_mod(y)) return false;
  const Fr fx = Fr::from_canonical(x), fy = Fr::from_canonical(y);
  *px = fx;
  *py = fy;
  return fy.sqr() == fx.sqr() * fx - Fr::from_u64(17);
}

SPP_HD bool ao_bytes_equal32(const uint8_t* a, const uint8_t* b) {
  uint32_t o = 0;
  for (int i = 0; i < 32; i++) o |= (uint32_t)(a[i] ^ b[i]);
  return o == 0;
}
// bits 2 and 4 of one record.  coeff_bad: some coefficient was >= q; ct_be: the sponge over the 157 packed fields, canonical
// 32 B big-endian; point_ok: ao_owner_on_curve; wa_be: H(owner_x, owner_y) likewise (read only when point_ok); pw: the 76-byte
// public witness (header | wa_commitment | ct_commitment, submit_audit.rs:19-21).  The header is the verifier's business.
SPP_HD uint32_t ao_decide(bool coeff_bad, const uint8_t* ct_be, bool point_ok, const uint8_t* wa_be, const uint8_t* pw) {
  uint32_t f = 0;
  if (coeff_bad || !ao_bytes_equal32(ct_be, pw + AO_PW_CT)) f |= AO_BAD_CIPHERTEXT;
  if (!point_ok || !ao_bytes_equal32(wa_be, pw + AO_PW_WA)) f |= AO_BAD_IDENTITY;
  return f;
}

}  // namespace spp
