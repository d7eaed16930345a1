// A gnark verifying key made ready for k_verify: parsed and validated on the host, then its line tables, K points and the
// VerifyKeyDev descriptor uploaded on a stream.  Shared by spp_verify_batch (spp_verify_api.cpp) and spp_audit_open_batch
// (spp_audit_api.cpp), which runs the same kernel in front of k_audit_open.
// The struct is unit-local on purpose (anonymous namespace): it holds DevBuf members, and DevBuf is itself a unit-local type of
// spp_internal.hpp, so a struct with external linkage would name a different type in every unit that includes this header.
#pragma once
#include "spp_internal.hpp"

namespace {
struct VerifyKeyPrep {
  uint32_t nk = 0;                       // K points: public inputs + 2 (the constant, the commitment challenge)
  G1Affine alpha1;
  G2Affine q[4], beta2;                  // gamma2, delta2, pedG, pedGS: the key-side points of the four table-driven pairings
  std::vector<G1Affine> K;
  std::vector<LineStep> tabs_host[4];    // the sources of the asynchronous uploads: this object outlives the caller's synchronise
  VerifyKeyDev h;
  DevBuf dtab[4], dK, dvk;
  // host only.  pw_len: the length the caller's public witnesses have (0: not checked here)
  int parse(const uint8_t* vk, size_t vk_len, size_t pw_len) {
    auto be32 = [](const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; };
    if (vk_len < 576 + 4) return fail(SPP_ERR_FORMAT, "verifying key too short");
    nk = be32(vk + 576);
    size_t off = 580;
    if (nk < 2 || vk_len != off + (size_t)nk * 64 + 12 + 256) return fail(SPP_ERR_FORMAT, "verifying key has the wrong length");
    if (pw_len && pw_len != 12 + 32 * (size_t)(nk - 2)) return fail(SPP_ERR_FORMAT, "public witness length does not match the verifying key");
    alpha1 = g1_from_raw(vk);
    beta2 = g2_from_raw(vk + 128);
    q[0] = g2_from_raw(vk + 256);
    q[1] = g2_from_raw(vk + 448);
    K.resize(nk);
    for (uint32_t i = 0; i < nk; i++) K[i] = g1_from_raw(vk + off + 64 * (size_t)i);
    off += (size_t)nk * 64;
    if (be32(vk + off) != 1 || be32(vk + off + 4) != 0 || be32(vk + off + 8) != 1) return fail(SPP_ERR_FORMAT, "unsupported commitment layout");
    q[2] = g2_from_raw(vk + off + 12);
    q[3] = g2_from_raw(vk + off + 12 + 128);
    for (const G2Affine* p : {&beta2, &q[0], &q[1], &q[2], &q[3]})
      if (p->is_inf() || !g2_on_curve(*p)) return fail(SPP_ERR_FORMAT, "verifying key holds an invalid G2 point");
    if (!pairing_fast_consts_consistent()) return fail(SPP_ERR_HIP, "internal: Frobenius constants are not two-term");
    return SPP_OK;
  }
  // per-key preparation on the host (line tables of the four key-side G2 points, e(-alpha, beta), constants) and its upload
  int upload(hipStream_t st) {
    h.pc = make_pairing_fast_consts();
    h.e_alpha_beta = f12_from(miller_loop(alpha1.neg(), beta2));
    h.twist_b = twist_b();
    h.nk = nk;
    for (int k = 0; k < 4; k++) {
      tabs_host[k] = build_line_table(q[k]);
      UP(dtab[k], tabs_host[k].data(), tabs_host[k].size() * sizeof(LineStep));
      h.tab[k] = dtab[k].as<LineStep>();
    }
    UP(dK, K.data(), K.size() * sizeof(G1Affine));
    h.K = dK.as<G1Affine>();
    HIP_TRY(dvk.alloc(sizeof h));
    HIP_TRY(hipMemcpyAsync(dvk.p, &h, sizeof h, hipMemcpyHostToDevice, st));
    return SPP_OK;
  }
  const VerifyKeyDev* dev() { return dvk.as<VerifyKeyDev>(); }
};
}  // namespace
