// Host-side helpers shared by the units of the setup ceremony (spp_ceremony_api.cpp: the delta contributions; spp_ptau_api.cpp: the
// powers-of-tau transcript, the derivation of a key from it and the sigma contributions): clearing secrets on every return path,
// fr.Hash, validity of raw points, the generators, the pairing-product test, the device point check and the Horner over the
// window sums of the resident-buffer Pippenger.  Included after spp_internal.hpp, by those two units only.
#pragma once
#include "spp_internal.hpp"
#include "setup_contrib.hpp"

namespace {
// overwrites on every return path; the volatile stores are not removed as dead
struct Wipe {
  void* p;
  size_t n;
  ~Wipe() {
    volatile uint8_t* q = (volatile uint8_t*)p;
    for (size_t i = 0; i < n; i++) q[i] = 0;
  }
};
// the same for a device buffer, declared AFTER the DevBuf it clears (so it runs before the buffer is released)
struct DevWipe {
  DevBuf& b;
  size_t n;
  hipStream_t st;
  ~DevWipe() {
    if (!b.p) return;
    hipMemsetAsync(b.p, 0, n, st);
    hipStreamSynchronize(st);
  }
};

// count values of fr.Hash(msg, dst): 48 bytes per element, as the toxic waste of spp_setup
inline void hash_to_fr(const uint8_t* msg, size_t len, const char* dst, Fr* out, int count) {
  std::vector<uint8_t> u((size_t)48 * count);
  Wipe wu{u.data(), u.size()};
  expand_message_xmd(msg, len, (const uint8_t*)dst, strlen(dst), u.data(), u.size());
  for (int i = 0; i < count; i++) {
    uint32_t w[12];
    Wipe ww{w, sizeof w};
    for (int k = 0; k < 12; k++) w[k] = sc_load_be32(u.data() + 48 * i + 4 * k);
    out[i] = fr_from_wide48(w);
  }
}
// 32 bytes of the caller's entropy, or of the operating system's when entropy is NULL
inline bool ceremony_seed(const uint8_t* entropy, uint8_t seed[32]) {
  if (entropy) {
    memcpy(seed, entropy, 32);
    return true;
  }
  FILE* f = fopen("/dev/urandom", "rb");
  const bool got = f && fread(seed, 1, 32, f) == 32;
  if (f) fclose(f);
  return got;
}
inline bool g1_raw_valid(const uint8_t* raw, G1Affine* out) { return sc_decode_point(raw, out) != SC_POINT_BAD; }
// a G2 point of the order-r subgroup with canonical coordinates, not infinity
inline bool g2_raw_valid(const uint8_t* raw, G2Affine* out) {
  for (int o = 0; o < 128; o += 32)
    if (!be_is_canonical<FqParams>(raw + o)) return false;
  *out = g2_from_raw(raw);
  return !out->is_inf() && g2_on_curve(*out) && g2_in_subgroup(*out);
}
inline G1Affine g1_generator() { return G1Affine{Fq::from_u64(1), Fq::from_u64(2)}; }
inline G2Affine g2_generator() {
  auto dec = [](const char* s) {
    Fq acc = Fq::zero(), ten = Fq::from_u64(10);
    for (; *s; s++) acc = acc * ten + Fq::from_u64((uint64_t)(*s - '0'));
    return acc;
  };
  G2Affine g;
  g.x.c0 = dec("10857046999023057135944570762232829481370756359578518086990519993285655852781");
  g.x.c1 = dec("11559732032986387107991004021392285783925812861821192530917403151452391805634");
  g.y.c0 = dec("8495653923123431417604973247489272438418190587263600148770280649306958101930");
  g.y.c1 = dec("4082367875863433681332203403145435568316851327593401208105741076214120093531");
  return g;
}
// prod e(P, Q) == 1 for pairs whose Q are valid; a pair with P = infinity contributes 1
inline bool pairing_is_one(std::vector<std::pair<G1Affine, G2Affine>> pairs) {
  std::vector<std::pair<G1Affine, G2Affine>> live;
  for (auto& pq : pairs)
    if (!pq.first.is_inf()) live.push_back(pq);
  return live.empty() || pairing_product_is_one(live);
}
inline bool write_bytes(const char* path, const uint8_t* p, size_t n) {
  FILE* f = fopen(path, "wb");
  if (!f) return false;
  const bool ok = fwrite(p, 1, n, f) == n;
  return fclose(f) == 0 && ok;
}
// z * base == T + c * base_after: the equation of a Schnorr receipt (base | base_after | T as the challenge hashed them)
inline bool schnorr_holds(const G1Affine& base, const G1Affine& base_after, const G1Affine& T, const Fr& c, const uint8_t z_be[32]) {
  uint32_t zl[8], cl[8];
  Fr::from_bytes_be(z_be).to_canonical(zl);
  c.to_canonical(cl);
  G1XYZZ rhs = scalar_mul(base_after, cl);
  rhs.madd(T);
  const G1Affine lhs = scalar_mul(base, zl).to_affine(), r = rhs.to_affine();
  return lhs.is_inf() == r.is_inf() && lhs.x == r.x && lhs.y == r.y;
}

// raw[n * 64] -> d_pts (Montgomery form) and flags (host) by k_g1_decode_check.  ctx->mu held, device set.
inline int decode_points(hipStream_t st, const uint8_t* raw, size_t n, DevBuf& d_pts, std::vector<uint32_t>& flags) {
  DevBuf d_raw, d_flags;
  UP(d_raw, raw, n * 64);
  HIP_TRY(d_pts.alloc(n * sizeof(G1Affine)));
  HIP_TRY(d_flags.alloc(n * sizeof(uint32_t)));
  launch_g1_decode_check(st, d_raw.as<uint8_t>(), (uint32_t)n, d_pts.as<G1Affine>(), d_flags.as<uint32_t>());
  HIP_TRY(hipGetLastError());
  flags.resize(n);
  if (n) HIP_TRY(hipMemcpyAsync(flags.data(), d_flags.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return SPP_OK;
}
// sum_j 2^(16 j) W_j over the window sums launch_pippenger_g1 / _g2 left on the device, after the stream was synchronised
template <class F>
inline int pippenger_sum(const XYZZ<F>* d_windows, Affine<F>* out) {
  std::vector<XYZZ<F>> w(pippenger_windows());
  HIP_TRY(hipMemcpy(w.data(), d_windows, sizeof(XYZZ<F>) * w.size(), hipMemcpyDeviceToHost));
  XYZZ<F> r = XYZZ<F>::infinity();
  for (int j = (int)w.size() - 1; j >= 0; j--) {
    for (int k = 0; k < 16; k++) r.dbl_inplace();
    r.add(w[j]);
  }
  *out = r.to_affine();
  return SPP_OK;
}
}  // namespace
