// libspp C ABI, the withdrawal plan: spp_withdrawal_audit_plan, and the stream-ordered form spp_prove_withdrawals (spp_prove.cpp) runs
// over the wa_commitment words of its withdraw rows.  Which notes of a batch still need an audit record: one per identity the pool
// does not hold yet (the record is keyed by wa_commitment, shielded_pool_program/src/instructions/submit_audit.rs:65-73).  What a lane
// does and why the result does not depend on scheduling or on the salt is withdrawal_plan.hpp; the launches are
// kernels_withdrawals.hip.  One upload, five launches on ctx->stream -- ordered with the pool's commits and the tree's inserts --,
// one download.  The pool is read and never written.
#include "spp_internal.hpp"
#include "withdrawal_plan.hpp"

static_assert(SPP_AUDIT_RESIDENT == WPLAN_RESIDENT && SPP_WITHDRAWALS_MAX == WPLAN_MAX, "include/spp.h and withdrawal_plan.hpp disagree");

// the scratch of one plan: [slots | rep | pos | tile_counts | tile_base | resident]
static size_t plan_words(uint32_t count) { return (size_t)pool_slots_for(count) + 2 * (size_t)count + 2 * WPLAN_MAX_TILES; }
size_t spp_withdrawal_plan_scratch_bytes(size_t count) { return plan_words((uint32_t)count) * sizeof(uint32_t) + count; }

static int plan_salt(spp_pool* pool, PoolSet* audits, uint64_t* salt) {
  if (pool) {
    PoolSet sets[2];
    spp_pool_view(pool, sets, salt);
    *audits = sets[SPP_POOL_AUDIT_RECORDS];
    return SPP_OK;
  }
  FILE* f = fopen("/dev/urandom", "rb");
  if (!f || fread(salt, 1, sizeof *salt, f) != sizeof *salt) {
    if (f) fclose(f);
    return fail(SPP_ERR_IO, "cannot read /dev/urandom");
  }
  fclose(f);
  return SPP_OK;
}

int spp_withdrawal_plan_enqueue(spp_ctx* ctx, spp_pool* pool, const uint8_t* d_keys, size_t stride, size_t count, void* d_scratch,
                                uint32_t* d_audit_of, uint32_t* d_audit_note, uint32_t* d_n_audits) {
  PoolSet audits{};
  uint64_t salt = 0;
  if (int e = plan_salt(pool, &audits, &salt)) return e;
  hipStream_t st = ctx->stream;
  const uint32_t n = (uint32_t)count, slots_n = pool_slots_for(count);
  uint32_t* slots = (uint32_t*)d_scratch;
  uint32_t *rep = slots + slots_n, *pos = rep + n, *tile_counts = pos + n, *tile_base = tile_counts + WPLAN_MAX_TILES;
  uint8_t* resident = (uint8_t*)(tile_base + WPLAN_MAX_TILES);
  HIP_TRY(hipMemsetAsync(slots, 0xFF, (size_t)slots_n * sizeof(uint32_t), st));
  launch_withdrawal_plan(st, pool ? &audits : nullptr, salt, slots, slots_n - 1, d_keys, stride, n, resident, rep, pos, tile_counts, tile_base,
                         d_audit_of, d_audit_note, d_n_audits);
  return SPP_OK;
}

extern "C" int spp_withdrawal_audit_plan(spp_ctx* ctx, spp_pool* pool, size_t count, const uint8_t* wa, uint32_t* audit_of, uint32_t* audit_note,
                                         uint32_t* n_audits) {
  if (!ctx || !wa || !audit_of || !audit_note || !n_audits) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (count > WPLAN_MAX) return fail(SPP_ERR_BAD_INPUT, "too many keys in one call (%zu; at most 2^20)", count);
  if (pool && spp_pool_view(pool, nullptr, nullptr) != ctx) return fail(SPP_ERR_BAD_INPUT, "the pool belongs to another spp_ctx");
  *n_audits = 0;
  if (count == 0) return SPP_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf dkeys, dscratch, dout;
  UP(dkeys, wa, count * 32);
  HIP_TRY(dscratch.alloc(spp_withdrawal_plan_scratch_bytes(count)));
  HIP_TRY(dout.alloc((2 * count + 1) * sizeof(uint32_t)));
  uint32_t *d_of = dout.as<uint32_t>(), *d_note = d_of + count, *d_n = d_note + count;
  if (int e = spp_withdrawal_plan_enqueue(ctx, pool, dkeys.as<uint8_t>(), 32, count, dscratch.p, d_of, d_note, d_n)) return e;
  uint32_t n = 0;
  std::vector<uint32_t> note(count);   // entries past n_audits are not part of the result: the caller's stay as they were
  HIP_TRY(hipMemcpyAsync(audit_of, d_of, count * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(note.data(), d_note, count * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&n, d_n, sizeof n, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  memcpy(audit_note, note.data(), (size_t)n * sizeof(uint32_t));
  *n_audits = n;
  return SPP_OK;
}
