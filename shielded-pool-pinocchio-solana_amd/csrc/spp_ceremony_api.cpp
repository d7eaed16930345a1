// libspp C ABI, the setup ceremony: a contribution to the delta of a proving key, its receipt and the verifier of one link of a
// chain of contributions; the same pair for sigma, the trapdoor of the commitment's proof of knowledge (include/spp.h has the
// protocols; setup_contrib.hpp the kernel's method and the container's byte ranges).
#include "spp_internal.hpp"
#include "ceremony_host.hpp"

#include <chrono>

namespace {
Fr schnorr_challenge(const uint8_t pk_hash[32], const uint8_t* delta1, const uint8_t* delta1_after, const uint8_t* T) {
  uint8_t m[32 + 3 * 64];
  memcpy(m, pk_hash, 32);
  memcpy(m + 32, delta1, 64);
  memcpy(m + 96, delta1_after, 64);
  memcpy(m + 160, T, 64);
  Fr c;
  hash_to_fr(m, sizeof m, "spp-groth16-contribute-c1", &c, 1);
  return c;
}
// out[i] = k * points[i] (raw in, raw out) for the canonical limbs k != 0; *bad = index of the first point that is not on the
// curve (then nothing is written), else n.  The digits are cleared in host and device memory on every path.  kernel_ms
// (optional): the scaling kernel alone, between two events.
int scale_raw_points(spp_ctx* ctx, const uint8_t* points, size_t n, const uint32_t k[8], uint8_t* out, size_t* bad, float* kernel_ms = nullptr) {
  hipStream_t st = ctx->stream;
  int8_t dig[SC_MAX_DIGITS];
  Wipe wd{dig, sizeof dig};
  const uint32_t len = sc_naf_recode(k, dig);
  *bad = n;
  if (n == 0) return SPP_OK;
  DevBuf d_pts, d_out, d_dig;
  std::vector<uint32_t> flags;
  if (int e = decode_points(st, points, n, d_pts, flags)) return e;
  for (size_t i = 0; i < n; i++)
    if (flags[i] == SC_POINT_BAD) { *bad = i; return SPP_OK; }
  HIP_TRY(d_out.alloc(n * sizeof(G1Affine)));
  HIP_TRY(d_dig.alloc(sizeof dig));
  DevWipe dw{d_dig, sizeof dig, st};
  HIP_TRY(hipMemcpyAsync(d_dig.p, dig, sizeof dig, hipMemcpyHostToDevice, st));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (kernel_ms) {
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    hipEventRecord(e0, st);
  }
  launch_g1_scale(st, d_pts.as<G1Affine>(), (uint32_t)n, d_dig.as<int8_t>(), len, d_out.as<G1Affine>());
  if (kernel_ms) hipEventRecord(e1, st);
  const hipError_t launched = hipGetLastError();
  std::vector<G1Affine> res(n);
  hipError_t done = hipMemcpyAsync(res.data(), d_out.p, n * sizeof(G1Affine), hipMemcpyDeviceToHost, st);
  if (done == hipSuccess) done = hipStreamSynchronize(st);
  if (kernel_ms) {
    if (launched == hipSuccess && done == hipSuccess) hipEventElapsedTime(kernel_ms, e0, e1);
    hipEventDestroy(e0);
    hipEventDestroy(e1);
  }
  HIP_TRY(launched);
  HIP_TRY(done);
  for (size_t i = 0; i < n; i++) g1_to_raw(res[i], out + 64 * i);
  return SPP_OK;
}
// the K points and the Z points of a key, concatenated
std::vector<uint8_t> kz_points(const std::vector<uint8_t>& pk, const SppkLayout& L) {
  std::vector<uint8_t> o;
  o.insert(o.end(), pk.begin() + L.k_points, pk.begin() + L.k_points + (size_t)L.n_k * 64);
  o.insert(o.end(), pk.begin() + L.z_points, pk.begin() + L.z_points + (size_t)L.n_z * 64);
  return o;
}
}  // namespace

extern "C" int spp_g1_scale_points(spp_ctx* ctx, const uint8_t* points, size_t n, const uint8_t scalar_be[32], uint8_t* out) {
  return spp_g1_scale_points_timed(ctx, points, n, scalar_be, out, nullptr, 0, nullptr);
}
extern "C" int spp_g1_scale_points_timed(spp_ctx* ctx, const uint8_t* points, size_t n, const uint8_t scalar_be[32], uint8_t* out, float* kernel_ms,
                                         size_t host_points, float* host_ms) {
  if (!ctx || !scalar_be || (n && (!points || !out))) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (n >= (1u << 31)) return fail(SPP_ERR_BAD_INPUT, "too many points");
  if (!be_is_canonical<FrParams>(scalar_be)) return fail(SPP_ERR_BAD_INPUT, "the scalar is not below r");
  uint32_t k[8];
  Wipe wk{k, sizeof k};
  uint32_t any = 0;
  for (int i = 0; i < 8; i++) any |= k[7 - i] = sc_load_be32(scalar_be + 4 * i);
  if (!any) return fail(SPP_ERR_BAD_INPUT, "the scalar is zero");
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  size_t bad = n;
  if (kernel_ms) *kernel_ms = 0;
  if (int e = scale_raw_points(ctx, points, n, k, out, &bad, kernel_ms)) return e;
  if (bad != n) return fail(SPP_ERR_BAD_INPUT, "point %zu is not on the curve", bad);
  if (host_ms) {   // one thread, the double-and-add of bn254.hpp, conversion to affine included; must give the kernel's bytes
    *host_ms = 0;
    const size_t m = std::min(host_points, n);
    std::vector<G1Affine> pts(m);
    for (size_t i = 0; i < m; i++) sc_decode_point(points + 64 * i, &pts[i]);
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<G1Affine> res(m);
    for (size_t i = 0; i < m; i++) res[i] = scalar_mul(pts[i], k).to_affine();
    *host_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (size_t i = 0; i < m; i++) {
      uint8_t b[64];
      g1_to_raw(res[i], b);
      if (memcmp(b, out + 64 * i, 64) != 0) return fail(SPP_ERR_HIP, "internal: point %zu differs between the kernel and the host loop", i);
    }
  }
  return SPP_OK;
}

extern "C" int spp_setup_contribute(spp_ctx* ctx, const char* pk_in, const char* vk_in, const uint8_t entropy[32], const char* pk_out,
                                    const char* vk_out, uint8_t receipt[SPP_CONTRIB_RECEIPT_LEN]) {
  if (!ctx || !pk_in || !vk_in || !pk_out || !vk_out || !receipt) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  std::vector<uint8_t> pk, vk;
  if (!read_file(pk_in, pk)) return fail(SPP_ERR_IO, "cannot read %s", pk_in);
  if (!read_file(vk_in, vk)) return fail(SPP_ERR_IO, "cannot read %s", vk_in);
  SppkLayout L;
  if (!sppk_layout(pk.data(), pk.size(), &L)) return fail(SPP_ERR_FORMAT, "%s is not a proving key", pk_in);
  if (!vk_layout_ok(vk.data(), vk.size())) return fail(SPP_ERR_FORMAT, "%s is not a verifying key", vk_in);
  if (memcmp(vk.data() + VK_DELTA1, pk.data() + L.delta1, 64) || memcmp(vk.data() + VK_DELTA2, pk.data() + L.delta2, 128))
    return fail(SPP_ERR_BAD_INPUT, "%s and %s do not hold the same delta", pk_in, vk_in);
  G1Affine delta1;
  G2Affine delta2;
  if (!g1_raw_valid(pk.data() + L.delta1, &delta1) || delta1.is_inf() || !g2_raw_valid(pk.data() + L.delta2, &delta2))
    return fail(SPP_ERR_FORMAT, "%s holds an invalid delta", pk_in);

  // the secrets: d (the contribution), k (the nonce of the receipt), 1/d and their limbs; all cleared on every path
  uint8_t seed[32];
  Fr dk[2], dinv;
  uint32_t dl[8], kl[8], il[8];
  Wipe w0{seed, sizeof seed}, w1{dk, sizeof dk}, w2{&dinv, sizeof dinv}, w3{dl, sizeof dl}, w4{kl, sizeof kl}, w5{il, sizeof il};
  if (entropy) memcpy(seed, entropy, 32);
  else {
    FILE* f = fopen("/dev/urandom", "rb");
    const bool got = f && fread(seed, 1, 32, f) == 32;
    if (f) fclose(f);
    if (!got) return fail(SPP_ERR_IO, "no randomness from the operating system");
  }
  hash_to_fr(seed, 32, "spp-groth16-contribute-v1", dk, 2);
  if (dk[0].is_zero()) return fail(SPP_ERR_BAD_INPUT, "the entropy gives the contribution zero: use another");
  dinv = dk[0].inv();
  dk[0].to_canonical(dl);
  dk[1].to_canonical(kl);
  dinv.to_canonical(il);

  // K and Z by 1/d on the device, one launch over both
  const std::vector<uint8_t> before = kz_points(pk, L);
  const size_t n = (size_t)L.n_k + L.n_z;
  std::vector<uint8_t> after(before.size());
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    size_t bad = n;
    if (int e = scale_raw_points(ctx, before.data(), n, il, after.data(), &bad)) return e;
    if (bad != n) return fail(SPP_ERR_FORMAT, "%s: point %zu of K | Z is not on the curve", pk_in, bad);
  }
  // delta1', delta2' and the receipt on the host
  uint8_t d1[64], d2[128], T[64], pk_hash[32];
  g1_to_raw(scalar_mul(delta1, dl).to_affine(), d1);
  g2_to_raw(scalar_mul(delta2, dl).to_affine(), d2);
  g1_to_raw(scalar_mul(delta1, kl).to_affine(), T);
  sha256_bytes(pk.data(), pk.size(), pk_hash);
  const Fr c = schnorr_challenge(pk_hash, pk.data() + L.delta1, d1, T);
  const Fr z = dk[1] + c * dk[0];   // public
  memcpy(receipt, d1, 64);
  memcpy(receipt + 64, T, 64);
  z.to_bytes_be(receipt + 128);

  memcpy(pk.data() + L.delta1, d1, 64);
  memcpy(pk.data() + L.delta2, d2, 128);
  memcpy(pk.data() + L.k_points, after.data(), (size_t)L.n_k * 64);
  memcpy(pk.data() + L.z_points, after.data() + (size_t)L.n_k * 64, (size_t)L.n_z * 64);
  memcpy(vk.data() + VK_DELTA1, d1, 64);
  memcpy(vk.data() + VK_DELTA2, d2, 128);
  if (!write_bytes(pk_out, pk.data(), pk.size())) return fail(SPP_ERR_IO, "cannot write %s", pk_out);
  if (!write_bytes(vk_out, vk.data(), vk.size())) return fail(SPP_ERR_IO, "cannot write %s", vk_out);
  return SPP_OK;
}

extern "C" int spp_setup_verify_contribution(spp_ctx* ctx, const char* pk_before, const char* vk_before, const char* pk_after,
                                             const char* vk_after, const uint8_t receipt[SPP_CONTRIB_RECEIPT_LEN], int* ok, uint32_t* reason) {
  if (!ctx || !pk_before || !vk_before || !pk_after || !vk_after || !receipt || !ok || !reason) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  *ok = 0;
  *reason = SPP_CONTRIB_FORMAT;
  std::vector<uint8_t> pb, vb, pa, va;
  for (auto f : {std::make_pair(pk_before, &pb), std::make_pair(vk_before, &vb), std::make_pair(pk_after, &pa), std::make_pair(vk_after, &va)})
    if (!read_file(f.first, *f.second)) return fail(SPP_ERR_IO, "cannot read %s", f.first);
  auto refuse = [&](uint32_t why) { *reason = why; return SPP_OK; };

  // 1. the files parse, and the proving keys differ in delta1, delta2, the K points and the Z points only
  SppkLayout L;
  const int diff = sppk_delta_diff(pb.data(), pb.size(), pa.data(), pa.size(), &L);
  if (diff == SC_DIFF_FORMAT || !vk_layout_ok(vb.data(), vb.size()) || !vk_layout_ok(va.data(), va.size())) return refuse(SPP_CONTRIB_FORMAT);
  if (diff != SC_DIFF_OK) return refuse(SPP_CONTRIB_NOT_A_DELTA_CHANGE);

  // 2. every point a contribution may change is a point: K | Z of both keys, delta1, delta1' through the device check, the two
  //    delta2 on the host (twist, subgroup)
  const size_t n = (size_t)L.n_k + L.n_z;
  std::vector<uint8_t> raw = kz_points(pb, L);
  {
    const std::vector<uint8_t> kz_after = kz_points(pa, L);
    raw.insert(raw.end(), kz_after.begin(), kz_after.end());
    raw.insert(raw.end(), pb.begin() + L.delta1, pb.begin() + L.delta1 + 64);
    raw.insert(raw.end(), pa.begin() + L.delta1, pa.begin() + L.delta1 + 64);
  }
  if (2 * n + 2 >= (1u << 31)) return refuse(SPP_CONTRIB_FORMAT);
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf d_pts;
  std::vector<uint32_t> flags;
  if (int e = decode_points(st, raw.data(), 2 * n + 2, d_pts, flags)) return e;
  for (size_t i = 0; i < 2 * n + 2; i++)
    if (flags[i] == SC_POINT_BAD) return refuse(SPP_CONTRIB_POINT_INVALID);
  for (size_t i = 0; i < n; i++)
    if (flags[n + i] == SC_POINT_INF && flags[i] != SC_POINT_INF) return refuse(SPP_CONTRIB_POINT_INVALID);
  if (flags[2 * n] != SC_POINT_OK || flags[2 * n + 1] != SC_POINT_OK) return refuse(SPP_CONTRIB_POINT_INVALID);
  G1Affine delta1, delta1a, T;
  G2Affine delta2, delta2a;
  g1_raw_valid(pb.data() + L.delta1, &delta1);
  g1_raw_valid(pa.data() + L.delta1, &delta1a);
  if (!g2_raw_valid(pb.data() + L.delta2, &delta2) || !g2_raw_valid(pa.data() + L.delta2, &delta2a)) return refuse(SPP_CONTRIB_POINT_INVALID);

  // 3. the receipt: knowledge of d with delta1' = d * delta1, bound to the key it was applied to
  uint8_t hb[32], ha[32];
  sha256_bytes(pb.data(), pb.size(), hb);
  sha256_bytes(pa.data(), pa.size(), ha);
  {
    if (memcmp(receipt, pa.data() + L.delta1, 64) != 0) return refuse(SPP_CONTRIB_RECEIPT);
    if (sc_decode_point(receipt + 64, &T) == SC_POINT_BAD || !be_is_canonical<FrParams>(receipt + 128)) return refuse(SPP_CONTRIB_RECEIPT);
    const Fr c = schnorr_challenge(hb, pb.data() + L.delta1, receipt, receipt + 64);
    uint32_t zl[8], cl[8];
    Fr::from_bytes_be(receipt + 128).to_canonical(zl);
    c.to_canonical(cl);
    G1XYZZ rhs = scalar_mul(delta1a, cl);
    rhs.madd(T);
    const G1Affine lhs = scalar_mul(delta1, zl).to_affine(), r = rhs.to_affine();
    if (lhs.is_inf() != r.is_inf() || !(lhs.x == r.x) || !(lhs.y == r.y)) return refuse(SPP_CONTRIB_RECEIPT);
  }

  // 4. delta1' and delta2' hide the same scalar
  const G1Affine g1{Fq::from_u64(1), Fq::from_u64(2)};
  if (!pairing_is_one({{delta1a, g2_generator()}, {g1.neg(), delta2a}})) return refuse(SPP_CONTRIB_DELTA_PAIR);

  // 5. K' | Z' = (K | Z) / d, all points at once: P = sum rho_i (K | Z)_i, P' the same over the key after, and
  //    e(P', delta2') e(-P, delta2) = 1.  rho_i: the first 16 bytes of SHA256(hash before | hash after | i as 8 bytes big-endian)
  if (n) {
    std::vector<Fr> rho(n);
    uint8_t m[72], dg[32];
    memcpy(m, hb, 32);
    memcpy(m + 32, ha, 32);
    for (size_t i = 0; i < n; i++) {
      for (int b = 0; b < 8; b++) m[64 + b] = (uint8_t)((uint64_t)i >> (8 * (7 - b)));
      sha256_bytes(m, sizeof m, dg);
      uint32_t w[8] = {sc_load_be32(dg + 12), sc_load_be32(dg + 8), sc_load_be32(dg + 4), sc_load_be32(dg), 0, 0, 0, 0};
      rho[i] = Fr::from_canonical(w);
    }
    DevBuf d_rho, d_ws;
    UP(d_rho, rho.data(), n * sizeof(Fr));
    HIP_TRY(d_ws.alloc(pippenger_workspace_bytes((uint32_t)n)));
    G1Affine sum[2];
    for (int side = 0; side < 2; side++) {
      G1XYZZ* win = nullptr;
      launch_pippenger_g1(st, d_pts.as<G1Affine>() + side * n, d_rho.as<Fr>(), (uint32_t)n, d_ws.p, &win, nullptr, nullptr);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipStreamSynchronize(st));
      sum[side] = pippenger_finish(win);
    }
    if (!pairing_is_one({{sum[1], delta2a}, {sum[0].neg(), delta2}})) return refuse(SPP_CONTRIB_SCALING);
  }

  // 6. the verifying key follows: the same bytes but delta1 | delta2, which are the proving key's
  if (!vk_delta_diff_ok(vb.data(), vb.size(), va.data(), va.size()) || memcmp(va.data() + VK_DELTA1, pa.data() + L.delta1, 64) != 0 ||
      memcmp(va.data() + VK_DELTA2, pa.data() + L.delta2, 128) != 0)
    return refuse(SPP_CONTRIB_VK);
  *ok = 1;
  *reason = SPP_CONTRIB_OK;
  return SPP_OK;
}

// -----------------------------------------------------------------------------------------------------
// sigma contributions: the trapdoor of the commitment's proof of knowledge (CS = sigma CB, the vk's last G2 point -rho sigma G2)
// -----------------------------------------------------------------------------------------------------
namespace {
Fr sigma_challenge(const uint8_t pk_hash[32], const uint8_t* cs0, const uint8_t* cs0_after, const uint8_t* T) {
  uint8_t m[32 + 3 * 64];
  memcpy(m, pk_hash, 32);
  memcpy(m + 32, cs0, 64);
  memcpy(m + 96, cs0_after, 64);
  memcpy(m + 160, T, 64);
  Fr c;
  hash_to_fr(m, sizeof m, "spp-groth16-sigma-c1", &c, 1);
  return c;
}
// the vk's last G2 point
size_t vk_sigma_point(size_t vk_len) { return vk_len - 128; }
}  // namespace

extern "C" int spp_setup_contribute_sigma(spp_ctx* ctx, const char* pk_in, const char* vk_in, const uint8_t entropy[32], const char* pk_out,
                                          const char* vk_out, uint8_t receipt[SPP_CONTRIB_RECEIPT_LEN]) {
  if (!ctx || !pk_in || !vk_in || !pk_out || !vk_out || !receipt) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  std::vector<uint8_t> pk, vk;
  if (!read_file(pk_in, pk)) return fail(SPP_ERR_IO, "cannot read %s", pk_in);
  if (!read_file(vk_in, vk)) return fail(SPP_ERR_IO, "cannot read %s", vk_in);
  SppkLayout L;
  if (!sppk_layout(pk.data(), pk.size(), &L)) return fail(SPP_ERR_FORMAT, "%s is not a proving key", pk_in);
  if (!vk_layout_ok(vk.data(), vk.size())) return fail(SPP_ERR_FORMAT, "%s is not a verifying key", vk_in);
  if (L.n_cs == 0) return fail(SPP_ERR_BAD_INPUT, "%s has no committed wires: there is no sigma to contribute to", pk_in);
  G1Affine cs0;
  G2Affine H;
  if (sc_decode_point(pk.data() + L.cs_points, &cs0) != SC_POINT_OK || !g2_raw_valid(vk.data() + vk_sigma_point(vk.size()), &H))
    return fail(SPP_ERR_FORMAT, "%s / %s hold an invalid commitment key", pk_in, vk_in);

  // the secrets: s (the contribution), k (the nonce of the receipt) and their limbs; all cleared on every path
  uint8_t seed[32];
  Fr sk[2];
  uint32_t sl[8], kl[8];
  Wipe w0{seed, sizeof seed}, w1{sk, sizeof sk}, w2{sl, sizeof sl}, w3{kl, sizeof kl};
  if (!ceremony_seed(entropy, seed)) return fail(SPP_ERR_IO, "no randomness from the operating system");
  hash_to_fr(seed, 32, "spp-groth16-sigma-v1", sk, 2);
  if (sk[0].is_zero()) return fail(SPP_ERR_BAD_INPUT, "the entropy gives the contribution zero: use another");
  sk[0].to_canonical(sl);
  sk[1].to_canonical(kl);

  // CS by s on the device
  std::vector<uint8_t> after((size_t)L.n_cs * 64);
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    size_t bad = L.n_cs;
    if (int e = scale_raw_points(ctx, pk.data() + L.cs_points, L.n_cs, sl, after.data(), &bad)) return e;
    if (bad != L.n_cs) return fail(SPP_ERR_FORMAT, "%s: point %zu of CS is not on the curve", pk_in, bad);
  }
  // the vk's point and the receipt on the host
  uint8_t T[64], pk_hash[32];
  g1_to_raw(scalar_mul(cs0, kl).to_affine(), T);
  sha256_bytes(pk.data(), pk.size(), pk_hash);
  const Fr c = sigma_challenge(pk_hash, pk.data() + L.cs_points, after.data(), T);
  const Fr z = sk[1] + c * sk[0];   // public
  memcpy(receipt, after.data(), 64);
  memcpy(receipt + 64, T, 64);
  z.to_bytes_be(receipt + 128);
  memcpy(pk.data() + L.cs_points, after.data(), after.size());
  g2_to_raw(scalar_mul(H, sl).to_affine(), vk.data() + vk_sigma_point(vk.size()));
  if (!write_bytes(pk_out, pk.data(), pk.size())) return fail(SPP_ERR_IO, "cannot write %s", pk_out);
  if (!write_bytes(vk_out, vk.data(), vk.size())) return fail(SPP_ERR_IO, "cannot write %s", vk_out);
  return SPP_OK;
}

extern "C" int spp_setup_verify_sigma_contribution(spp_ctx* ctx, const char* pk_before, const char* vk_before, const char* pk_after,
                                                   const char* vk_after, const uint8_t receipt[SPP_CONTRIB_RECEIPT_LEN], int* ok, uint32_t* reason) {
  if (!ctx || !pk_before || !vk_before || !pk_after || !vk_after || !receipt || !ok || !reason) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  *ok = 0;
  *reason = SPP_SIGMA_FORMAT;
  std::vector<uint8_t> pb, vb, pa, va;
  for (auto f : {std::make_pair(pk_before, &pb), std::make_pair(vk_before, &vb), std::make_pair(pk_after, &pa), std::make_pair(vk_after, &va)})
    if (!read_file(f.first, *f.second)) return fail(SPP_ERR_IO, "cannot read %s", f.first);
  auto refuse = [&](uint32_t why) { *reason = why; return SPP_OK; };

  // 1. the files parse; 2. they differ in the CS points and the vk's last G2 point only
  SppkLayout L, La;
  if (!sppk_layout(pb.data(), pb.size(), &L) || !sppk_layout(pa.data(), pa.size(), &La) || !vk_layout_ok(vb.data(), vb.size()) ||
      !vk_layout_ok(va.data(), va.size()))
    return refuse(SPP_SIGMA_FORMAT);
  if (L.n_cs == 0) return fail(SPP_ERR_BAD_INPUT, "%s has no committed wires: there is no sigma to contribute to", pk_before);
  const size_t n = L.n_cs, cs_end = L.cs_points + n * 64, hp = vk_sigma_point(vb.size());
  if (pa.size() != pb.size() || va.size() != vb.size() || memcmp(pb.data(), pa.data(), L.cs_points) != 0 ||
      memcmp(pb.data() + cs_end, pa.data() + cs_end, pb.size() - cs_end) != 0 || memcmp(vb.data(), va.data(), hp) != 0)
    return refuse(SPP_SIGMA_NOT_A_SIGMA_CHANGE);

  // 3. every CS point of both keys is a point (the device's check), the first ones are not infinity, the two G2 points are in the group
  std::vector<uint8_t> raw(pb.begin() + L.cs_points, pb.begin() + cs_end);
  raw.insert(raw.end(), pa.begin() + L.cs_points, pa.begin() + cs_end);
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf d_pts;
  std::vector<uint32_t> flags;
  if (int e = decode_points(st, raw.data(), 2 * n, d_pts, flags)) return e;
  for (size_t i = 0; i < 2 * n; i++)
    if (flags[i] == SC_POINT_BAD) return refuse(SPP_SIGMA_POINT_INVALID);
  for (size_t i = 0; i < n; i++)
    if (flags[n + i] == SC_POINT_INF && flags[i] != SC_POINT_INF) return refuse(SPP_SIGMA_POINT_INVALID);
  if (flags[0] != SC_POINT_OK || flags[n] != SC_POINT_OK) return refuse(SPP_SIGMA_POINT_INVALID);
  G1Affine cs0, cs0a, T;
  G2Affine H, Ha;
  sc_decode_point(pb.data() + L.cs_points, &cs0);
  sc_decode_point(pa.data() + L.cs_points, &cs0a);
  if (!g2_raw_valid(vb.data() + hp, &H) || !g2_raw_valid(va.data() + hp, &Ha)) return refuse(SPP_SIGMA_POINT_INVALID);

  // 4. the receipt: knowledge of s with CS'_0 = s CS_0, bound to the key it was applied to
  uint8_t hb[32], ha[32];
  sha256_bytes(pb.data(), pb.size(), hb);
  sha256_bytes(pa.data(), pa.size(), ha);
  if (memcmp(receipt, pa.data() + L.cs_points, 64) != 0) return refuse(SPP_SIGMA_RECEIPT);
  if (sc_decode_point(receipt + 64, &T) == SC_POINT_BAD || !be_is_canonical<FrParams>(receipt + 128)) return refuse(SPP_SIGMA_RECEIPT);
  if (!schnorr_holds(cs0, cs0a, T, sigma_challenge(hb, pb.data() + L.cs_points, receipt, receipt + 64), receipt + 128)) return refuse(SPP_SIGMA_RECEIPT);

  // 5., 6. the scaling is tested against the G2 point the vk carries, so that point is tied to the receipt's s first: a vk whose
  //    point is not s H (e(CS'_0, H) != e(CS_0, H')) is SPP_SIGMA_VK, whatever the CS points are; with it, all points at once:
  //    e(sum rho_i CS'_i, H) = e(sum rho_i CS_i, H'), rho_i as in the delta verifier
  if (!pairing_is_one({{cs0a, H}, {cs0.neg(), Ha}})) return refuse(SPP_SIGMA_VK);
  std::vector<Fr> rho(n);
  uint8_t m[72], dg[32];
  memcpy(m, hb, 32);
  memcpy(m + 32, ha, 32);
  for (size_t i = 0; i < n; i++) {
    for (int b = 0; b < 8; b++) m[64 + b] = (uint8_t)((uint64_t)i >> (8 * (7 - b)));
    sha256_bytes(m, sizeof m, dg);
    uint32_t w[8] = {sc_load_be32(dg + 12), sc_load_be32(dg + 8), sc_load_be32(dg + 4), sc_load_be32(dg), 0, 0, 0, 0};
    rho[i] = Fr::from_canonical(w);
  }
  DevBuf d_rho, d_ws;
  UP(d_rho, rho.data(), n * sizeof(Fr));
  HIP_TRY(d_ws.alloc(pippenger_workspace_bytes((uint32_t)n)));
  G1Affine sum[2];
  for (int side = 0; side < 2; side++) {
    G1XYZZ* win = nullptr;
    launch_pippenger_g1(st, d_pts.as<G1Affine>() + side * n, d_rho.as<Fr>(), (uint32_t)n, d_ws.p, &win, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    sum[side] = pippenger_finish(win);
  }
  if (!pairing_is_one({{sum[1], H}, {sum[0].neg(), Ha}})) return refuse(SPP_SIGMA_SCALING);
  *ok = 1;
  *reason = SPP_SIGMA_OK;
  return SPP_OK;
}
