// libspp C ABI, auditor side of a batch of audit records: spp_audit_open_batch, spp_audit_open_batch_rlc (the same with the
// random-linear-combination verifier, verify_rlc.hpp, in front of the open kernel) and spp_audit_open_batch_partials (the same
// from t auditors' partial decryptions instead of the key, rlwe_partial.hpp).  One upload of (proofs, public witnesses,
// ciphertexts), k_verify as spp_verify_batch runs it, then k_audit_open (kernels_witness.hip, audit_open.hpp) on the same
// stream, one download of owners and flags.  Replaces scripts/rlwe_decrypt.py:61-149 for many records and adds what that
// script leaves to the reader: is this ciphertext the one the proof commits to, is the decrypted identity the one it commits to.
#include "spp_internal.hpp"
#include "verify_key_prep.hpp"

// rlc: the verifier in front of k_audit_open is the dense random-linear-combination one (group checked by the caller, a fresh seed
// from the operating system, slices and workspace as in spp_verify_batch_rlc); stats: its four counters, or nullptr.
// partials (with t): the threshold form -- no key; k_rlwe_combine turns the t partials of every record into the residues of
// sk * c1 the open kernel rounds, and into bit 8 (rlwe_partial.hpp); sk_mod_q is then nullptr
static int audit_open(spp_ctx* ctx, const uint8_t* vk, size_t vk_len, const uint32_t* sk_mod_q, uint32_t t, const uint8_t* partials, size_t count,
                      const uint8_t* proofs, const uint8_t* pws, const uint32_t* c0, const uint32_t* c1, uint8_t* owners, uint32_t* flags, bool rlc,
                      uint32_t group, uint32_t* stats) {
  const bool threshold = sk_mod_q == nullptr && t != 0;
  if (!ctx || (!threshold && !sk_mod_q) || (count && (!pws || !c0 || !c1 || !owners || !flags || (threshold && !partials))))
    return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if ((vk == nullptr) != (vk_len == 0)) return fail(SPP_ERR_BAD_INPUT, "vk and vk_len must both be given or both be absent");
  if (vk && count && !proofs) return fail(SPP_ERR_BAD_INPUT, "NULL argument: proofs (needed with a verifying key)");
  if (count > (1u << 24)) return fail(SPP_ERR_BAD_INPUT, "too many records in one call (%zu; at most 2^24)", count);
  if (threshold) {
    if (int e = spp_check_partials(t, count, partials)) return e;
  } else {
    for (int i = 0; i < 1024; i++)
      if (sk_mod_q[i] >= 167772161u) return fail(SPP_ERR_BAD_INPUT, "secret key coefficient %d not in [0, q)", i);
  }
  VerifyKeyPrep key;
  if (vk) {
    if (int e = key.parse(vk, vk_len, 0)) return e;
    if (key.nk != 4) return fail(SPP_ERR_FORMAT, "the verifying key has %u public inputs, an audit proof has 2 (wa_commitment, ct_commitment)", key.nk - 2);
  }
  if (count == 0) return SPP_OK;
  RlcSeed seed;
  if (rlc && vk)
    if (int e = rlc_os_seed(seed)) return e;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  if (int e = spp_ensure_ctx_consts(ctx)) return e;
  hipStream_t st = ctx->stream;
  DevBuf dsk, dproofs, dpws, d0, d1, dok, downers, dflags, dcnt, dparts, dbad;
  RlcKeyPrep rkey;
  RlcScratch sc;
  if (threshold) {
    UP(dparts, partials, (size_t)t * count * 64 * SPP_PARTIAL_LEN);
    HIP_TRY(dsk.alloc(count * 64 * sizeof(uint32_t)));      // the residues, in the key's place
    HIP_TRY(dbad.alloc(count * sizeof(uint32_t)));
  } else {
    UP(dsk, sk_mod_q, 4096);
  }
  UP(dpws, pws, count * (size_t)SPP_AUDIT_PW_LEN);
  UP(d0, c0, count * 64 * 4);
  UP(d1, c1, count * 1024 * 4);
  HIP_TRY(downers.alloc(count * 64));
  HIP_TRY(dflags.alloc(count * sizeof(uint32_t)));
  if (vk) {
    if (int e = key.upload(st)) return e;
    UP(dproofs, proofs, count * (size_t)SPP_PROOF_LEN);
    HIP_TRY(dok.alloc(count * sizeof(int32_t)));
    if (rlc) {
      if (int e = rkey.upload(st, key)) return e;
      if (int e = sc.alloc(key.nk, count, group)) return e;
      HIP_TRY(dcnt.alloc(5 * sizeof(uint32_t)));            // stats[4], then the length of the fallback list
      HIP_TRY(hipMemsetAsync(dcnt.p, 0, 5 * sizeof(uint32_t), st));
      if (int e = rlc_verify_dense(st, key.dev(), rkey.dev(), dproofs.as<uint8_t>(), dpws.as<uint8_t>(), SPP_AUDIT_PW_LEN, count, seed, group, 0, sc,
                                   dok.as<int32_t>(), dcnt.as<uint32_t>(), dcnt.as<uint32_t>() + 4))
        return e;
    } else {
      launch_verify(st, key.dev(), dproofs.as<uint8_t>(), dpws.as<uint8_t>(), SPP_AUDIT_PW_LEN, (uint32_t)count, dok.as<int32_t>());
    }
  }
  if (threshold) {
    launch_rlwe_combine(st, t, dparts.as<uint8_t>(), nullptr, dsk.as<uint32_t>(), nullptr, dbad.as<uint32_t>(), (uint32_t)count);
    launch_audit_open_partials(st, ctx->hc, dsk.as<uint32_t>(), dbad.as<uint32_t>(), d0.as<uint32_t>(), d1.as<uint32_t>(), dpws.as<uint8_t>(),
                               vk ? dok.as<int32_t>() : nullptr, downers.as<uint8_t>(), dflags.as<uint32_t>(), (uint32_t)count);
  } else {
    launch_audit_open(st, ctx->hc, dsk.as<uint32_t>(), d0.as<uint32_t>(), d1.as<uint32_t>(), dpws.as<uint8_t>(), vk ? dok.as<int32_t>() : nullptr,
                      downers.as<uint8_t>(), dflags.as<uint32_t>(), (uint32_t)count);
  }
  HIP_TRY(hipMemcpyAsync(owners, downers.p, count * 64, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(flags, dflags.p, count * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  if (stats && rlc && vk) {
    HIP_TRY(hipMemcpy(stats, dcnt.p, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    stats[0] += rlc_dense_groups(count, group);
  }
  return SPP_OK;
}

extern "C" int spp_audit_open_batch(spp_ctx* ctx, const uint8_t* vk, size_t vk_len, const uint32_t* sk_mod_q, size_t count,
                                    const uint8_t* proofs, const uint8_t* pws, const uint32_t* c0, const uint32_t* c1, uint8_t* owners,
                                    uint32_t* flags) {
  return audit_open(ctx, vk, vk_len, sk_mod_q, 0, nullptr, count, proofs, pws, c0, c1, owners, flags, false, 0, nullptr);
}

extern "C" int spp_audit_open_batch_partials(spp_ctx* ctx, const uint8_t* vk, size_t vk_len, uint32_t t, const uint8_t* partials, size_t count,
                                             const uint8_t* proofs, const uint8_t* pws, const uint32_t* c0, const uint32_t* c1, uint8_t* owners,
                                             uint32_t* flags) {
  if (int e = spp_check_share_set(t, nullptr)) return e;
  return audit_open(ctx, vk, vk_len, nullptr, t, partials, count, proofs, pws, c0, c1, owners, flags, false, 0, nullptr);
}

extern "C" int spp_audit_open_batch_rlc(spp_ctx* ctx, const uint8_t* vk, size_t vk_len, const uint32_t* sk_mod_q, size_t count,
                                        const uint8_t* proofs, const uint8_t* pws, const uint32_t* c0, const uint32_t* c1, uint32_t group,
                                        uint8_t* owners, uint32_t* flags, uint32_t stats[4]) {
  if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
  if (int e = rlc_group_arg(group)) return e;
  return audit_open(ctx, vk, vk_len, sk_mod_q, 0, nullptr, count, proofs, pws, c0, c1, owners, flags, true, group, stats);
}
