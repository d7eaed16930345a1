// libspp C ABI, deposit proofs: the rows of the deposit circuit from the resident tree (spp_deposit_rows_from_tree; k_deposit_rows,
// deposit_rows.hpp) and the check of a log of proved deposits (spp_verify_deposit_chain).  The proving entry points,
// spp_prove_deposits(_device), sit with the other batch entry points in spp_prove.cpp, whose workspaces they use.
// The reference has no counterpart: its program checks nothing about a deposit (shielded_pool_program/src/instructions/
// deposit.rs:31-36,73).
#include "spp_internal.hpp"
#include "deposit_rows.hpp"
#include "verify_key_prep.hpp"

static_assert(SPP_DEPOSIT_INPUTS == DEPOSIT_ROW_FIXED + SPP_TREE_DEPTH && SPP_DEPOSIT_PW_LEN == 12 + 5 * 32,
              "include/spp.h and deposit_rows.hpp disagree");

// the host entry points' record check: every field canonical, secret_key != 0.  An amount >= 2^64 passes: the circuit refuses it in place
int spp_check_deposit_records(size_t count, const uint8_t* deposits) {
  static const char* const field_name[3] = {"secret_key", "amount", "randomness"};
  for (size_t i = 0; i < count; i++) {
    const uint8_t* d = deposits + SPP_DEPOSIT_LEN * i;
    for (int f = 0; f < 3; f++)
      if (!be_is_canonical<FrParams>(d + 32 * f))
        return fail(SPP_ERR_BAD_INPUT, "deposit %zu: %s is not a canonical field element", i, field_name[f]);
    bool sk_zero = true;
    for (int b = 0; b < 32; b++) sk_zero &= d[b] == 0;
    if (sk_zero) return fail(SPP_ERR_BAD_INPUT, "deposit %zu: secret_key is 0", i);
  }
  return SPP_OK;
}
// ctx->mu held: the leaves asked for are in the tree
int spp_check_deposit_range(const spp_merkle_tree* t, uint64_t first_index, size_t count) {
  if (first_index > t->n_leaves || count > t->n_leaves - first_index)
    return fail(SPP_ERR_BAD_INPUT, "deposits %llu .. %llu are not all in the tree (%llu leaves)", (unsigned long long)first_index,
                (unsigned long long)(first_index + count - 1), (unsigned long long)t->n_leaves);
  return SPP_OK;
}

extern "C" int spp_deposit_rows_from_tree(spp_merkle_tree* t, uint64_t first_index, size_t count, const uint8_t* deposits, uint8_t* rows) {
  if (!t || (count && (!deposits || !rows))) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (count > (1u << 24)) return fail(SPP_ERR_BAD_INPUT, "too many deposits in one call (%zu; at most 2^24)", count);
  if (int e = spp_check_deposit_records(count, deposits)) return e;
  spp_ctx* ctx = t->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (int e = spp_check_deposit_range(t, first_index, count)) return e;
  if (count == 0) return SPP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  if (int e = spp_ensure_ctx_consts(ctx)) return e;
  hipStream_t st = ctx->stream;
  const size_t row_bytes = (size_t)(DEPOSIT_ROW_FIXED + t->depth) * 32;
  DevBuf dd, dr;
  UP(dd, deposits, count * SPP_DEPOSIT_LEN);
  HIP_TRY(dr.alloc(count * row_bytes));
  launch_deposit_rows(st, ctx->gk_table, ctx->hc, t->dev, first_index, dd.as<uint8_t>(), dr.as<uint8_t>(), (uint32_t)count);
  HIP_TRY(hipMemcpyAsync(rows, dr.p, count * row_bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return SPP_OK;
}

// The chain.  Proof verification does not depend on the position in the log, so it is one spp_verify_batch call (k_verify, one lane per
// proof) for the whole batch.  What is left is a scan that carries 40 bytes of state through 76 bytes per instruction, each step
// depending on whether the one before was accepted: no parallel structure worth a kernel, so it runs here after the one download of
// the flags that spp_verify_batch makes.
extern "C" int spp_verify_deposit_chain(spp_ctx* ctx, const uint8_t* vk, size_t vk_len, size_t count, const uint8_t* proofs, const uint8_t* pws,
                                        const uint64_t* lamports, const uint8_t start_root[32], uint64_t start_index, uint32_t* codes,
                                        uint8_t end_root[32], uint64_t* end_index) {
  if (!ctx || !vk || !start_root || (count && (!proofs || !pws || !codes))) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (count > (1u << 24)) return fail(SPP_ERR_BAD_INPUT, "too many instructions in one call (%zu; at most 2^24)", count);
  VerifyKeyPrep key;   // parsed here as well, so that the refusals do not depend on the count
  if (int e = key.parse(vk, vk_len, 0)) return e;
  if (key.nk != 5 + 2) return fail(SPP_ERR_FORMAT, "the verifying key has %u public inputs, a deposit proof has 5", key.nk - 2);
  std::vector<int32_t> ok(count);
  if (count)
    if (int e = spp_verify_batch(ctx, vk, vk_len, count, proofs, pws, SPP_DEPOSIT_PW_LEN, ok.data(), nullptr)) return e;
  uint8_t root[32];
  memcpy(root, start_root, 32);
  uint64_t n = start_index;
  bool wrapped = false;   // the counter passed 2^64 - 1: no 32-byte index word the circuit accepts equals it any more
  for (size_t i = 0; i < count; i++) {
    const uint8_t* w = pws + SPP_DEPOSIT_PW_LEN * i + 12;   // old_root | new_root | commitment | amount | index
    uint8_t want[32] = {0};
    uint32_t code = SPP_DEPOSIT_OK;
    if (lamports) {
      for (int b = 0; b < 8; b++) want[24 + b] = (uint8_t)(lamports[i] >> (8 * (7 - b)));
      if (memcmp(w + 96, want, 32) != 0) code = SPP_DEPOSIT_BAD_AMOUNT;
    }
    if (!code && memcmp(w, root, 32) != 0) code = SPP_DEPOSIT_STALE_ROOT;
    if (!code) {
      for (int b = 0; b < 8; b++) want[24 + b] = (uint8_t)(n >> (8 * (7 - b)));
      if (wrapped || memcmp(w + 128, want, 32) != 0) code = SPP_DEPOSIT_BAD_INDEX;
    }
    if (!code && ok[i] != 1) code = SPP_DEPOSIT_BAD_PROOF;
    codes[i] = code;
    if (!code) {
      memcpy(root, w + 32, 32);
      if (++n == 0) wrapped = true;
    }
  }
  if (end_root) memcpy(end_root, root, 32);
  if (end_index) *end_index = n;
  return SPP_OK;
}
