// libspp C ABI, threshold opening of audit ciphertexts (rlwe_partial.hpp): an auditor's partial decryptions from its own Shamir
// share (spp_rlwe_partial_decrypt_batch), their combination by a party that holds no share (spp_rlwe_combine_partials), and the
// smudging noise an auditor adds (spp_rlwe_sample_smudge).  The RLWE secret key is never rebuilt: the place of
// spp_shamir_reconstruct + spp_rlwe_decrypt_batch (scripts/rlwe_decrypt.py:61-132) for auditors who do not trust one machine
// with every record.  spp_audit_open_batch_partials, the opening of whole records from partials, is in spp_audit_api.cpp.
#include "spp_internal.hpp"
#include "rlwe_partial.hpp"
#include "secret_buffers.hpp"

namespace {
const size_t PARTIAL_MAX_RECORDS = (size_t)1 << 24;
const uint32_t SMUDGE_MAX_BOUND = 1u << 20;
}  // namespace

// t in [1, 64], every x nonzero and distinct: the participating set as all three calls take it
int spp_check_share_set(uint32_t t, const uint32_t* xs) {
  if (t == 0 || t > spp::RP_MAX_T) return fail(SPP_ERR_BAD_INPUT, "threshold %u is not in [1, 64]", t);
  if (!xs) return SPP_OK;
  for (uint32_t i = 0; i < t; i++) {
    if (xs[i] == 0) return fail(SPP_ERR_BAD_INPUT, "xs[%u] is 0: that share would be the secret", i);
    for (uint32_t j = 0; j < i; j++)
      if (xs[i] == xs[j]) return fail(SPP_ERR_BAD_INPUT, "xs[%u] repeats xs[%u] = %u", i, j, xs[i]);
  }
  return SPP_OK;
}
// every partial a canonical field element, named by auditor, record and slot
int spp_check_partials(uint32_t t, size_t count, const uint8_t* partials) {
  const size_t n = (size_t)t * count * 64;
  for (size_t i = 0; i < n; i++)
    if (!be_is_canonical<FrParams>(partials + 32 * i))
      return fail(SPP_ERR_BAD_INPUT, "partial %zu (auditor %zu, record %zu, slot %zu) is not a canonical field element", i, i / (count * 64),
                  i / 64 % count, i % 64);
  return SPP_OK;
}

extern "C" int spp_rlwe_sample_smudge(size_t n, uint32_t bound, int32_t* e, uint64_t* rho) {
  if (!e || !rho) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (bound > SMUDGE_MAX_BOUND) return fail(SPP_ERR_BAD_INPUT, "bound %u: at most 2^20", bound);
  if (n > PARTIAL_MAX_RECORDS * 64) return fail(SPP_ERR_BAD_INPUT, "n %zu: at most 2^30 values in one call", n);
  OsRandom rnd;
  const uint64_t range = 2 * (uint64_t)bound + 1, limit = ((uint64_t)1 << 32) - (((uint64_t)1 << 32) % range);   // words below `limit` are uniform mod range
  for (size_t i = 0; i < n;) {
    uint8_t w[4];
    if (!rnd.next(w, 4)) return fail(SPP_ERR_IO, "cannot read /dev/urandom");
    const uint64_t v = (uint32_t)w[0] | (uint32_t)w[1] << 8 | (uint32_t)w[2] << 16 | (uint32_t)w[3] << 24;
    if (v < limit) e[i++] = (int32_t)((int64_t)(v % range) - (int64_t)bound);
  }
  for (size_t i = 0; i < n; i++) {
    uint8_t w[8];
    if (!rnd.next(w, 8)) return fail(SPP_ERR_IO, "cannot read /dev/urandom");
    uint64_t v = 0;
    for (int b = 0; b < 8; b++) v |= (uint64_t)w[b] << (8 * b);
    rho[i] = v;
  }
  return SPP_OK;
}

extern "C" int spp_rlwe_partial_decrypt_batch(spp_ctx* ctx, uint32_t t, const uint32_t* xs, uint32_t self, const uint8_t* share_be, size_t count,
                                              const uint32_t* c0, const uint32_t* c1, const int32_t* e, const uint64_t* rho,
                                              const uint8_t* pair_seeds, uint8_t* partials, uint8_t* ct_commitments) {
  if (!ctx || !xs || !share_be || (count && (!c0 || !c1 || !partials))) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (int rc = spp_check_share_set(t, xs)) return rc;
  if (self >= t) return fail(SPP_ERR_BAD_INPUT, "self %u: the set has %u members", self, t);
  if (count > PARTIAL_MAX_RECORDS) return fail(SPP_ERR_BAD_INPUT, "too many records in one call (%zu; at most 2^24)", count);
  for (uint32_t i = 0; i < spp::AO_N; i++)
    if (!be_is_canonical<FrParams>(share_be + 32 * i)) return fail(SPP_ERR_BAD_INPUT, "share value %u is not a canonical field element", i);
  for (size_t k = 0; k < count; k++) {
    for (uint32_t i = 0; i < spp::AO_SLOTS; i++)
      if (c0[k * 64 + i] >= spp::AO_Q) return fail(SPP_ERR_BAD_INPUT, "ciphertext %zu: c0[%u] not in [0, q)", k, i);
    for (uint32_t i = 0; i < spp::AO_N; i++)
      if (c1[k * 1024 + i] >= spp::AO_Q) return fail(SPP_ERR_BAD_INPUT, "ciphertext %zu: c1[%u] not in [0, q)", k, i);
  }
  if (count == 0) return SPP_OK;
  // Lagrange coefficient at 0 of this auditor in the set: prod_{j != self} (-x_j) / (x_self - x_j)   (rlwe_decrypt.py:38-51)
  Fr num = Fr::one(), den = Fr::one();
  for (uint32_t j = 0; j < t; j++) {
    if (j == self) continue;
    num = num * Fr::from_u64(xs[j]).neg();
    den = den * (Fr::from_u64(xs[self]) - Fr::from_u64(xs[j]));
  }
  const Fr lambda = num * den.inv();
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  if (int rc = spp_ensure_ctx_consts(ctx)) return rc;
  hipStream_t st = ctx->stream;
  const size_t slots = count * 64;
  WipedDevBuf dshare, du, dseeds;
  DevBuf dxs, d0, d1, de, drho, dout, dct;
  UP_SECRET(dshare, share_be, (size_t)spp::AO_N * 32);
  du.bytes = spp::RP_TABLE_WORDS * sizeof(uint32_t);
  du.st = st;
  HIP_TRY(du.alloc(du.bytes));
  if (pair_seeds) UP_SECRET(dseeds, pair_seeds, (size_t)t * 32);
  UP(dxs, xs, (size_t)t * sizeof(uint32_t));
  UP(d0, c0, slots * 4);
  UP(d1, c1, count * 1024 * 4);
  if (e) UP(de, e, slots * sizeof(int32_t));
  if (rho) UP(drho, rho, slots * sizeof(uint64_t));
  HIP_TRY(dout.alloc(slots * SPP_PARTIAL_LEN));
  HIP_TRY(dct.alloc(count * 32));
  launch_partial_scale(st, lambda, dshare.as<uint8_t>(), du.as<uint32_t>());
  launch_rlwe_partial(st, ctx->hc, du.as<uint32_t>(), t, dxs.as<uint32_t>(), self, pair_seeds ? dseeds.as<uint8_t>() : nullptr, d0.as<uint32_t>(),
                      d1.as<uint32_t>(), e ? de.as<int32_t>() : nullptr, rho ? drho.as<uint64_t>() : nullptr, dout.as<uint8_t>(),
                      dct.as<uint8_t>(), (uint32_t)count);
  HIP_TRY(hipMemcpyAsync(partials, dout.p, slots * SPP_PARTIAL_LEN, hipMemcpyDeviceToHost, st));
  if (ct_commitments) HIP_TRY(hipMemcpyAsync(ct_commitments, dct.p, count * 32, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return SPP_OK;
}

extern "C" int spp_rlwe_combine_partials(spp_ctx* ctx, uint32_t t, size_t count, const uint8_t* partials, const uint32_t* c0, uint8_t* msg,
                                         uint32_t* flags) {
  if (!ctx || (count && (!partials || !c0 || !msg))) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (int rc = spp_check_share_set(t, nullptr)) return rc;
  if (count > PARTIAL_MAX_RECORDS) return fail(SPP_ERR_BAD_INPUT, "too many records in one call (%zu; at most 2^24)", count);
  if (count == 0) return SPP_OK;
  if (int rc = spp_check_partials(t, count, partials)) return rc;
  for (size_t i = 0; i < count * 64; i++)      // the rounding adds c0 to a residue: both below q (ao_round_slot)
    if (c0[i] >= spp::AO_Q) return fail(SPP_ERR_BAD_INPUT, "ciphertext %zu: c0[%zu] not in [0, q)", i / 64, i % 64);
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf dp, d0, dm, df;
  UP(dp, partials, (size_t)t * count * 64 * SPP_PARTIAL_LEN);
  UP(d0, c0, count * 64 * 4);
  HIP_TRY(dm.alloc(count * 64));
  HIP_TRY(df.alloc(count * sizeof(uint32_t)));
  launch_rlwe_combine(st, t, dp.as<uint8_t>(), d0.as<uint32_t>(), nullptr, dm.as<uint8_t>(), df.as<uint32_t>(), (uint32_t)count);
  HIP_TRY(hipMemcpyAsync(msg, dm.p, count * 64, hipMemcpyDeviceToHost, st));
  if (flags) HIP_TRY(hipMemcpyAsync(flags, df.p, count * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return SPP_OK;
}
