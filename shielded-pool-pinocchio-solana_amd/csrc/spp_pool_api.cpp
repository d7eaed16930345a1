// libspp C ABI, the pool ledger: spp_pool_*.  A device-resident restatement of the state the pool program decides on --
// ShieldedPoolState's root ring (shielded_pool_program/src/state.rs:6-46) and the two sets of accounts whose existence it tests,
// spent nullifiers and audit records -- and the settling of a batch of submit_audit / withdraw instructions with the decisions
// the program makes processing them one after another (instructions/submit_audit.rs, withdraw.rs).  What a lane does and why the
// parallel resolution of duplicates equals the sequential one is in pool_table.hpp; the launches are in kernels_pool.hip.
// One call = one upload, screen -> verify (compacted list) -> claim -> settle -> commit on ctx->stream, one download.
#include "spp_internal.hpp"
#include "verify_key_prep.hpp"
#include "pool_table.hpp"

struct spp_pool {
  spp_ctx* ctx = nullptr;
  uint64_t capacity = 0, salt = 0;
  bool compact = true;              // env SPP_POOL_COMPACT=0 (profiling aid): verify every proof of a batch, not the compacted list
  VerifyKeyPrep key[2];             // [0] withdraw (5 public inputs), [1] audit (2): parsed once, line tables resident
  PoolState state;                  // host copy of the ring; add_roots changes it here and uploads it
  PoolState* d_state = nullptr;
  PoolSet set[2]{};                 // SPP_POOL_NULLIFIERS, SPP_POOL_AUDIT_RECORDS: device pointers
  uint32_t* d_counts = nullptr;     // keys per set, advanced by the commit kernel
  uint64_t counts[2] = {0, 0};      // as downloaded at the end of the last call that could change them
};

static_assert(SPP_POOL_STATE_LEN == POOL_STATE_LEN && SPP_POOL_OK == POOL_OK && SPP_POOL_AUDIT_EXISTS == POOL_AUDIT_EXISTS &&
                  SPP_POOL_NO_AUDIT_RECORD == POOL_NO_AUDIT_RECORD && SPP_POOL_BAD_ROOT == POOL_BAD_ROOT &&
                  SPP_POOL_NULLIFIER_USED == POOL_NULLIFIER_USED && SPP_POOL_BAD_RECIPIENT == POOL_BAD_RECIPIENT &&
                  SPP_POOL_BAD_PROOF == POOL_BAD_PROOF && SPP_PROOF_LEN == POOL_PROOF && SPP_WITHDRAW_PW_LEN == POOL_WITHDRAW_PW &&
                  SPP_AUDIT_PW_LEN == POOL_AUDIT_PW,
              "include/spp.h and pool_table.hpp disagree");

static constexpr size_t POOL_MAX_BATCH = (size_t)1 << 24;
static constexpr uint64_t POOL_MAX_CAPACITY = (uint64_t)1 << 30;   // slot indices are 32-bit

static int pool_salt(uint64_t* salt) {
  if (const char* env = getenv("SPP_POOL_SALT")) {
    char* end = nullptr;
    *salt = strtoull(env, &end, 16);
    if (end == env || *end) return fail(SPP_ERR_BAD_INPUT, "SPP_POOL_SALT is not a hexadecimal number");
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

extern "C" void spp_pool_free(spp_pool* p) {
  if (!p) return;
  hipSetDevice(p->ctx->device);
  hipStreamSynchronize(p->ctx->stream);
  for (PoolSet& s : p->set) {
    if (s.claim) hipFree(s.claim);
    if (s.keys) hipFree(s.keys);
  }
  if (p->d_state) hipFree(p->d_state);
  if (p->d_counts) hipFree(p->d_counts);
  delete p;
}

extern "C" int spp_pool_new(spp_ctx* ctx, const uint8_t* withdraw_vk, size_t withdraw_vk_len, const uint8_t* audit_vk, size_t audit_vk_len,
                            uint64_t capacity, spp_pool** out) {
  if (!ctx || !withdraw_vk || !audit_vk || !out) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (capacity == 0 || capacity > POOL_MAX_CAPACITY) return fail(SPP_ERR_BAD_INPUT, "capacity must be 1..2^30 keys per set");
  spp_pool* p = new spp_pool();
  p->ctx = ctx;
  auto bail = [&](int e) { spp_pool_free(p); return e; };
  if (int e = p->key[0].parse(withdraw_vk, withdraw_vk_len, 0)) return bail(e);
  if (p->key[0].nk != 7)
    return bail(fail(SPP_ERR_FORMAT, "the withdraw verifying key has %u public inputs, a withdraw proof has 5", p->key[0].nk - 2));
  if (int e = p->key[1].parse(audit_vk, audit_vk_len, 0)) return bail(e);
  if (p->key[1].nk != 4)
    return bail(fail(SPP_ERR_FORMAT, "the audit verifying key has %u public inputs, an audit proof has 2", p->key[1].nk - 2));
  if (int e = pool_salt(&p->salt)) return bail(e);
  if (const char* env = getenv("SPP_POOL_COMPACT")) p->compact = atoi(env) != 0;
  p->capacity = capacity;
  pool_state_init(p->state);

  std::lock_guard<std::mutex> lk(ctx->mu);
  if (hipSetDevice(ctx->device) != hipSuccess) return bail(fail(SPP_ERR_HIP, "hipSetDevice"));
  hipStream_t st = ctx->stream;
  const uint32_t slots = pool_slots_for(capacity);
  bool ok = hipMalloc((void**)&p->d_state, sizeof(PoolState)) == hipSuccess && hipMalloc((void**)&p->d_counts, 2 * sizeof(uint32_t)) == hipSuccess;
  for (PoolSet& s : p->set) {
    s.mask = slots - 1;
    ok = ok && hipMalloc((void**)&s.claim, (size_t)slots * sizeof(uint32_t)) == hipSuccess && hipMalloc((void**)&s.keys, (size_t)slots * 32) == hipSuccess;
    ok = ok && hipMemsetAsync(s.claim, 0, (size_t)slots * sizeof(uint32_t), st) == hipSuccess;
  }
  if (!ok) return bail(fail(SPP_ERR_HIP, "hipMalloc (two sets of %u slots)", slots));
  ok = hipMemsetAsync(p->d_counts, 0, 2 * sizeof(uint32_t), st) == hipSuccess &&
       hipMemcpyAsync(p->d_state, &p->state, sizeof(PoolState), hipMemcpyHostToDevice, st) == hipSuccess;
  if (!ok) return bail(fail(SPP_ERR_HIP, "initialising the pool state"));
  for (VerifyKeyPrep& k : p->key)
    if (int e = k.upload(st)) return bail(e);
  if (hipStreamSynchronize(st) != hipSuccess) return bail(fail(SPP_ERR_HIP, "hipStreamSynchronize"));
  *out = p;
  return SPP_OK;
}

// state.add_root (state.rs:28-33) for `count` deposits in order
extern "C" int spp_pool_add_roots(spp_pool* p, size_t count, const uint8_t* roots) {
  if (!p || (count && !roots)) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (count == 0) return SPP_OK;
  if (count > POOL_MAX_BATCH) return fail(SPP_ERR_BAD_INPUT, "too many roots in one call (%zu; at most 2^24)", count);
  spp_ctx* ctx = p->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  for (size_t i = 0; i < count; i++) pool_add_root(p->state, roots + 32 * i);
  HIP_TRY(hipMemcpyAsync(p->d_state, &p->state, sizeof(PoolState), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return SPP_OK;
}

extern "C" int spp_pool_state(spp_pool* p, uint8_t state[SPP_POOL_STATE_LEN]) {
  if (!p || !state) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  std::lock_guard<std::mutex> lk(p->ctx->mu);
  pool_state_bytes(p->state, state);
  return SPP_OK;
}

extern "C" int spp_pool_counts(spp_pool* p, uint64_t counts[2]) {
  if (!p || !counts) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  std::lock_guard<std::mutex> lk(p->ctx->mu);
  counts[0] = p->counts[0];
  counts[1] = p->counts[1];
  return SPP_OK;
}

// the set counts as the device has them, into the host copy; enqueued behind the commit kernel, complete after the synchronise
static int pool_fetch_counts(spp_pool* p, hipStream_t st, uint32_t host[2]) {
  HIP_TRY(hipMemcpyAsync(host, p->d_counts, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  return SPP_OK;
}
static int pool_room(const spp_pool* p, int which, size_t count) {
  if (p->counts[which] + count > p->capacity)
    return fail(SPP_ERR_BAD_INPUT, "the %s set holds %llu of %llu keys: a call with %zu more could overflow it",
                which == SPP_POOL_NULLIFIERS ? "nullifier" : "audit-record", (unsigned long long)p->counts[which],
                (unsigned long long)p->capacity, count);
  return SPP_OK;
}
// the per-call resolve table: >= 2 x count words, all empty
static int pool_resolve_table(hipStream_t st, size_t count, DevBuf& slots, uint32_t* mask) {
  const uint32_t n = pool_slots_for(count);
  HIP_TRY(slots.alloc((size_t)n * sizeof(uint32_t)));
  HIP_TRY(hipMemsetAsync(slots.p, 0xFF, (size_t)n * sizeof(uint32_t), st));
  *mask = n - 1;
  return SPP_OK;
}

extern "C" int spp_pool_import_keys(spp_pool* p, int which, size_t count, const uint8_t* keys) {
  if (!p || (count && !keys)) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (which != SPP_POOL_NULLIFIERS && which != SPP_POOL_AUDIT_RECORDS) return fail(SPP_ERR_BAD_INPUT, "which: SPP_POOL_NULLIFIERS or SPP_POOL_AUDIT_RECORDS");
  if (count == 0) return SPP_OK;
  if (count > POOL_MAX_BATCH) return fail(SPP_ERR_BAD_INPUT, "too many keys in one call (%zu; at most 2^24)", count);
  spp_ctx* ctx = p->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (int e = pool_room(p, which, count)) return e;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf dkeys, dprov, dresult, dslots;
  uint32_t rmask = 0, cnt[2];
  UP(dkeys, keys, count * 32);
  HIP_TRY(dprov.alloc(count * sizeof(int32_t)));
  HIP_TRY(dresult.alloc(count * sizeof(int32_t)));
  if (int e = pool_resolve_table(st, count, dslots, &rmask)) return e;
  launch_pool_screen_import(st, p->set[which], p->salt, dkeys.as<uint8_t>(), (uint32_t)count, dprov.as<int32_t>());
  launch_pool_resolve(st, dslots.as<uint32_t>(), rmask, p->salt, dkeys.as<uint8_t>(), 32, (uint32_t)count, dprov.as<int32_t>(), nullptr,
                      POOL_AUDIT_EXISTS, dresult.as<int32_t>());
  launch_pool_commit(st, p->set[which], p->salt, dkeys.as<uint8_t>(), 32, (uint32_t)count, dresult.as<int32_t>(), p->d_counts + which);
  if (int e = pool_fetch_counts(p, st, cnt)) return e;
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  p->counts[0] = cnt[0];
  p->counts[1] = cnt[1];
  return SPP_OK;
}

extern "C" int spp_pool_contains(spp_pool* p, int which, size_t count, const uint8_t* keys, uint8_t* present) {
  if (!p || (count && (!keys || !present))) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (which != SPP_POOL_NULLIFIERS && which != SPP_POOL_AUDIT_RECORDS) return fail(SPP_ERR_BAD_INPUT, "which: SPP_POOL_NULLIFIERS or SPP_POOL_AUDIT_RECORDS");
  if (count == 0) return SPP_OK;
  if (count > POOL_MAX_BATCH) return fail(SPP_ERR_BAD_INPUT, "too many keys in one call (%zu; at most 2^24)", count);
  spp_ctx* ctx = p->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf dkeys, dpresent;
  UP(dkeys, keys, count * 32);
  HIP_TRY(dpresent.alloc(count));
  launch_pool_contains(st, p->set[which], p->salt, dkeys.as<uint8_t>(), (uint32_t)count, dpresent.as<uint8_t>());
  HIP_TRY(hipMemcpyAsync(present, dpresent.p, count, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return SPP_OK;
}

// screen has run and left prov, the verify list and its length; verdicts by instruction index into ok (zeroed here)
static int pool_verify(spp_pool* p, hipStream_t st, int which_key, const uint8_t* dproofs, const uint8_t* dpws, uint32_t pw_len, uint32_t count,
                       const uint32_t* dlist, const uint32_t* dnlist, DevBuf& dok) {
  HIP_TRY(dok.alloc(count * sizeof(int32_t)));
  HIP_TRY(hipMemsetAsync(dok.p, 0, count * sizeof(int32_t), st));
  if (p->compact)
    launch_verify_list(st, p->key[which_key].dev(), dproofs, dpws, pw_len, count, dlist, dnlist, dok.as<int32_t>());
  else
    launch_verify(st, p->key[which_key].dev(), dproofs, dpws, pw_len, count, dok.as<int32_t>());
  return SPP_OK;
}

extern "C" int spp_pool_submit_audit_batch(spp_pool* p, size_t count, const uint8_t* proofs, const uint8_t* pws, int32_t* result) {
  if (!p || (count && (!proofs || !pws || !result))) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (count == 0) return SPP_OK;
  if (count > POOL_MAX_BATCH) return fail(SPP_ERR_BAD_INPUT, "too many instructions in one call (%zu; at most 2^24)", count);
  spp_ctx* ctx = p->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (int e = pool_room(p, SPP_POOL_AUDIT_RECORDS, count)) return e;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const uint32_t n = (uint32_t)count;
  DevBuf dproofs, dpws, dprov, dlist, dnlist, dok, dslots, dresult;
  uint32_t rmask = 0, cnt[2];
  UP(dproofs, proofs, count * (size_t)SPP_PROOF_LEN);
  UP(dpws, pws, count * (size_t)SPP_AUDIT_PW_LEN);
  HIP_TRY(dprov.alloc(count * sizeof(int32_t)));
  HIP_TRY(dresult.alloc(count * sizeof(int32_t)));
  HIP_TRY(dlist.alloc(count * sizeof(uint32_t)));
  HIP_TRY(dnlist.alloc(sizeof(uint32_t)));
  HIP_TRY(hipMemsetAsync(dnlist.p, 0, sizeof(uint32_t), st));
  if (int e = pool_resolve_table(st, count, dslots, &rmask)) return e;
  const PoolSet& audits = p->set[SPP_POOL_AUDIT_RECORDS];
  const uint8_t* keys = dpws.as<uint8_t>() + POOL_A_WA;
  launch_pool_screen_audit(st, audits, p->salt, dpws.as<uint8_t>(), n, dprov.as<int32_t>(), dlist.as<uint32_t>(), dnlist.as<uint32_t>());
  if (int e = pool_verify(p, st, 1, dproofs.as<uint8_t>(), dpws.as<uint8_t>(), SPP_AUDIT_PW_LEN, n, dlist.as<uint32_t>(), dnlist.as<uint32_t>(), dok)) return e;
  launch_pool_resolve(st, dslots.as<uint32_t>(), rmask, p->salt, keys, SPP_AUDIT_PW_LEN, n, dprov.as<int32_t>(), dok.as<int32_t>(), POOL_AUDIT_EXISTS,
                      dresult.as<int32_t>());
  launch_pool_commit(st, audits, p->salt, keys, SPP_AUDIT_PW_LEN, n, dresult.as<int32_t>(), p->d_counts + SPP_POOL_AUDIT_RECORDS);
  HIP_TRY(hipMemcpyAsync(result, dresult.p, count * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (int e = pool_fetch_counts(p, st, cnt)) return e;
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  p->counts[0] = cnt[0];
  p->counts[1] = cnt[1];
  return SPP_OK;
}

extern "C" int spp_pool_withdraw_batch(spp_pool* p, size_t count, const uint8_t* proofs, const uint8_t* pws, const uint8_t* recipients,
                                       int32_t* result, uint64_t* amounts) {
  if (!p || (count && (!proofs || !pws || !recipients || !result))) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (count == 0) return SPP_OK;
  if (count > POOL_MAX_BATCH) return fail(SPP_ERR_BAD_INPUT, "too many instructions in one call (%zu; at most 2^24)", count);
  spp_ctx* ctx = p->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (int e = pool_room(p, SPP_POOL_NULLIFIERS, count)) return e;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const uint32_t n = (uint32_t)count;
  DevBuf dproofs, dpws, drecip, dprov, damounts, dlist, dnlist, dok, dslots, dresult;
  uint32_t rmask = 0, cnt[2];
  UP(dproofs, proofs, count * (size_t)SPP_PROOF_LEN);
  UP(dpws, pws, count * (size_t)SPP_WITHDRAW_PW_LEN);
  UP(drecip, recipients, count * 32);
  HIP_TRY(dprov.alloc(count * sizeof(int32_t)));
  HIP_TRY(dresult.alloc(count * sizeof(int32_t)));
  HIP_TRY(damounts.alloc(count * sizeof(uint64_t)));
  HIP_TRY(dlist.alloc(count * sizeof(uint32_t)));
  HIP_TRY(dnlist.alloc(sizeof(uint32_t)));
  HIP_TRY(hipMemsetAsync(dnlist.p, 0, sizeof(uint32_t), st));
  if (int e = pool_resolve_table(st, count, dslots, &rmask)) return e;
  const PoolSet& nullifiers = p->set[SPP_POOL_NULLIFIERS];
  const uint8_t* keys = dpws.as<uint8_t>() + POOL_W_NULLIFIER;
  launch_pool_screen_withdraw(st, p->d_state, p->set[SPP_POOL_AUDIT_RECORDS], nullifiers, p->salt, dpws.as<uint8_t>(), drecip.as<uint8_t>(), n,
                              dprov.as<int32_t>(), damounts.as<uint64_t>(), dlist.as<uint32_t>(), dnlist.as<uint32_t>());
  if (int e = pool_verify(p, st, 0, dproofs.as<uint8_t>(), dpws.as<uint8_t>(), SPP_WITHDRAW_PW_LEN, n, dlist.as<uint32_t>(), dnlist.as<uint32_t>(), dok)) return e;
  launch_pool_resolve(st, dslots.as<uint32_t>(), rmask, p->salt, keys, SPP_WITHDRAW_PW_LEN, n, dprov.as<int32_t>(), dok.as<int32_t>(),
                      POOL_NULLIFIER_USED, dresult.as<int32_t>());
  launch_pool_commit(st, nullifiers, p->salt, keys, SPP_WITHDRAW_PW_LEN, n, dresult.as<int32_t>(), p->d_counts + SPP_POOL_NULLIFIERS);
  HIP_TRY(hipMemcpyAsync(result, dresult.p, count * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (amounts) HIP_TRY(hipMemcpyAsync(amounts, damounts.p, count * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  if (int e = pool_fetch_counts(p, st, cnt)) return e;
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  p->counts[0] = cnt[0];
  p->counts[1] = cnt[1];
  return SPP_OK;
}
