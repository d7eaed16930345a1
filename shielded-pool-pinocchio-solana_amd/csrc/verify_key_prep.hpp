// A gnark verifying key made ready for k_verify: parsed and validated on the host, then its line tables, K points and the
// VerifyKeyDev descriptor uploaded on a stream.  Shared by spp_verify_batch (spp_verify_api.cpp) and spp_audit_open_batch
// (spp_audit_api.cpp), which runs the same kernel in front of k_audit_open.
// The struct is unit-local on purpose (anonymous namespace): it holds DevBuf members, and DevBuf is itself a unit-local type of
// spp_internal.hpp, so a struct with external linkage would name a different type in every unit that includes this header.
// Below it, what the callers of the random-linear-combination verifier share (spp_verify_batch_rlc, spp_audit_open_batch_rlc, the
// pool ledger in mode SPP_POOL_VERIFY_RLC): the beta pair, the seed, the group argument, the workspace and the slicing of a dense batch.
#pragma once
#include "spp_internal.hpp"
#include "verify_rlc.hpp"
#include "verify_rlc_list.hpp"

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

// the beta pair of the combined equation: a fifth line table and -alpha1, beside VerifyKeyDev
struct RlcKeyPrep {
  std::vector<LineStep> tab_host;        // the source of the asynchronous upload, like VerifyKeyPrep::tabs_host
  RlcKeyDev h;
  DevBuf dtab, drk;
  int upload(hipStream_t st, const VerifyKeyPrep& key) {
    tab_host = build_line_table(key.beta2);
    UP(dtab, tab_host.data(), tab_host.size() * sizeof(LineStep));
    h = RlcKeyDev{dtab.as<LineStep>(), key.alpha1.neg()};
    UP(drk, &h, sizeof h);
    return SPP_OK;
  }
  const RlcKeyDev* dev() { return drk.as<RlcKeyDev>(); }
};

constexpr uint32_t RLC_DEFAULT_GROUP = 256;       // profiles/verify_rlc_probe.json: 64 / 256 / 1024 at 2^15 proofs = 59.3 / 61.2 / 74.6 ms
// 0 -> the default; a multiple of 64 in [64, 4096]
inline int rlc_group_arg(uint32_t& group) {
  if (group == 0) group = RLC_DEFAULT_GROUP;
  if (group < 64 || group > 4096 || group % 64) return fail(SPP_ERR_BAD_INPUT, "group must be a multiple of 64 in [64, 4096]");
  return SPP_OK;
}
// 32 bytes from the operating system: one seed per verifier launch, never reused (include/spp.h has the rule)
inline int rlc_os_seed(RlcSeed& seed) {
  FILE* f = fopen("/dev/urandom", "rb");
  const bool got = f && fread(seed.b, 1, 32, f) == 32;
  if (f) fclose(f);
  if (!got) return fail(SPP_ERR_BAD_INPUT, "no randomness from the operating system");
  return SPP_OK;
}
// the workspace of one slice, the live words and the fallback list, for a batch (or a list) of at most `count` proofs
struct RlcScratch {
  DevBuf ws, live, list;
  int alloc(uint32_t nk, size_t count, uint32_t group) {
    const size_t n = std::min(count, (size_t)rlc_slice_len(group));
    HIP_TRY(ws.alloc(n * rlc_elems(nk) * sizeof(W256)));
    HIP_TRY(live.alloc(n * sizeof(uint32_t)));
    HIP_TRY(list.alloc(n * sizeof(uint32_t)));
    return SPP_OK;
  }
};
// a dense batch in slices of at most 2^18 proofs, a multiple of the group.  d_stats: 4 words that are added to (1..3 by the
// kernels), d_nfb: the length of the fallback list, 0 on entry and reset per slice; the groups are rlc_dense_groups, known to the host
inline int rlc_verify_dense(hipStream_t st, const VerifyKeyDev* vk, const RlcKeyDev* rk, const uint8_t* dproofs, const uint8_t* dpws, size_t pw_len,
                            size_t count, const RlcSeed& seed, uint32_t group, uint32_t flags, RlcScratch& sc, int32_t* dok, uint32_t* d_stats,
                            uint32_t* d_nfb) {
  const size_t slice = rlc_slice_len(group);
  for (size_t at = 0; at < count; at += slice) {
    const uint32_t n = (uint32_t)std::min(slice, count - at);
    if (at) HIP_TRY(hipMemsetAsync(d_nfb, 0, sizeof(uint32_t), st));
    launch_verify_rlc(st, vk, rk, dproofs + at * SPP_PROOF_LEN, dpws + at * pw_len, (uint32_t)pw_len, n, seed, (uint32_t)at, group, flags,
                      sc.ws.as<W256>(), sc.live.as<uint32_t>(), dok + at, sc.list.as<uint32_t>(), d_nfb, d_stats);
  }
  return SPP_OK;
}
inline uint32_t rlc_dense_groups(size_t count, uint32_t group) {
  const size_t slice = rlc_slice_len(group);
  uint32_t g = 0;
  for (size_t at = 0; at < count; at += slice) g += (uint32_t)((std::min(slice, count - at) + group - 1) / group);
  return g;
}
}  // namespace
