// libspp C ABI, the pool ledger: spp_pool_*.  A device-resident restatement of the state the pool program decides on --
// ShieldedPoolState's root ring (shielded_pool_program/src/state.rs:6-46) and the two sets of accounts whose existence it tests,
// spent nullifiers and audit records -- and the settling of a batch of submit_audit / withdraw instructions with the decisions
// the program makes processing them one after another (instructions/submit_audit.rs, withdraw.rs).  What a lane does and why the
// parallel resolution of duplicates equals the sequential one is in pool_table.hpp; the launches are in kernels_pool.hip.
// One call = one upload, screen -> verify (compacted list) -> claim -> settle -> commit on ctx->stream, one download.
// Which verifier "verify" is, is the pool's mode (spp_pool_set_verifier): k_verify_list / k_verify per proof, the default, or the
// random-linear-combination verifier over the same list (verify_rlc_list.hpp; kernels_verify_rlc.hip).  Only how ok[i] is computed
// differs; screen, claim, settle and commit read ok[i] as before.
// spp_pool_settle_log takes a log in which deposits, submit_audits and withdraws alternate (state.rs:28-46,
// instructions/deposit.rs:21-37, submit_audit.rs:41-87, withdraw.rs:94-175) and settles it with a fixed number of launches.
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
  // the verifier (spp_pool_set_verifier).  The beta pairs and the counters are made when RLC is first selected and stay resident
  int verifier = SPP_POOL_VERIFY_EACH;
  uint32_t group = RLC_DEFAULT_GROUP;
  bool rlc_ready = false;
  RlcKeyPrep rkey[2];               // beside key[]
  DevBuf dvstats;                   // per key 5 words: groups, groups refused, proofs re-verified, proofs dropped | fallback-list length
  uint32_t vraw[10] = {};           // their download, and the groups of a dense launch (SPP_POOL_COMPACT=0), which only the host knows
  uint32_t dense_groups[2] = {0, 0};
  uint32_t vstats[8] = {};          // spp_pool_verify_stats: the last settling call, [0..3] withdraw key, [4..7] audit key
};

static_assert(SPP_POOL_STATE_LEN == POOL_STATE_LEN && SPP_POOL_OK == POOL_OK && SPP_POOL_AUDIT_EXISTS == POOL_AUDIT_EXISTS &&
                  SPP_POOL_NO_AUDIT_RECORD == POOL_NO_AUDIT_RECORD && SPP_POOL_BAD_ROOT == POOL_BAD_ROOT &&
                  SPP_POOL_NULLIFIER_USED == POOL_NULLIFIER_USED && SPP_POOL_BAD_RECIPIENT == POOL_BAD_RECIPIENT &&
                  SPP_POOL_BAD_PROOF == POOL_BAD_PROOF && SPP_PROOF_LEN == POOL_PROOF && SPP_WITHDRAW_PW_LEN == POOL_WITHDRAW_PW &&
                  SPP_AUDIT_PW_LEN == POOL_AUDIT_PW && SPP_INSTR_DEPOSIT == POOL_INSTR_DEPOSIT && SPP_INSTR_SUBMIT_AUDIT == POOL_INSTR_SUBMIT_AUDIT &&
                  SPP_INSTR_WITHDRAW == POOL_INSTR_WITHDRAW,
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
// ... and the verifier's counters of a settling call (mode RLC), behind its last launch; pool_stats_end after the synchronise
static int pool_fetch_stats(spp_pool* p, hipStream_t st) {
  if (p->verifier == SPP_POOL_VERIFY_RLC) HIP_TRY(hipMemcpyAsync(p->vraw, p->dvstats.p, sizeof p->vraw, hipMemcpyDeviceToHost, st));
  return SPP_OK;
}
static void pool_stats_end(spp_pool* p) {
  for (int k = 0; k < 2; k++)
    for (int j = 0; j < 4; j++)
      p->vstats[4 * k + j] = p->verifier == SPP_POOL_VERIFY_RLC ? p->vraw[5 * k + j] + (j == 0 ? p->dense_groups[k] : 0) : 0;
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

// for spp_wallet_sync (spp_witness_api.cpp), whose locate kernel reads both sets and writes neither
spp_ctx* spp_pool_view(spp_pool* p, PoolSet* sets, uint64_t* salt) {
  if (sets) {
    sets[0] = p->set[SPP_POOL_NULLIFIERS];
    sets[1] = p->set[SPP_POOL_AUDIT_RECORDS];
    *salt = p->salt;
  }
  return p->ctx;
}
void spp_pool_ring_words(spp_pool* p, uint8_t words[33 * 32]) {
  memcpy(words, p->state.current_root, 32);
  for (uint32_t k = 0; k < POOL_ROOTS; k++) memcpy(words + 32 * (1 + k), p->state.roots[k], 32);
}

extern "C" int spp_pool_set_verifier(spp_pool* p, int mode, uint32_t group) {
  if (!p) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (mode != SPP_POOL_VERIFY_EACH && mode != SPP_POOL_VERIFY_RLC) return fail(SPP_ERR_BAD_INPUT, "mode: SPP_POOL_VERIFY_EACH or SPP_POOL_VERIFY_RLC");
  if (int e = rlc_group_arg(group)) return e;
  spp_ctx* ctx = p->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (mode == SPP_POOL_VERIFY_RLC && !p->rlc_ready) {
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    RlcKeyPrep fresh[2];
    DevBuf counters;
    for (int k = 0; k < 2; k++)
      if (int e = fresh[k].upload(st, p->key[k])) return e;
    HIP_TRY(counters.alloc(sizeof p->vraw));
    HIP_TRY(hipStreamSynchronize(st));
    for (int k = 0; k < 2; k++) {                                      // complete: only now the pool takes them
      std::swap(p->rkey[k].dtab.p, fresh[k].dtab.p);
      std::swap(p->rkey[k].drk.p, fresh[k].drk.p);
    }
    std::swap(p->dvstats.p, counters.p);
    p->rlc_ready = true;
  }
  p->verifier = mode;
  p->group = group;
  return SPP_OK;
}

extern "C" int spp_pool_verify_stats(spp_pool* p, uint32_t stats[8]) {
  if (!p || !stats) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  std::lock_guard<std::mutex> lk(p->ctx->mu);
  memcpy(stats, p->vstats, sizeof p->vstats);
  return SPP_OK;
}

// the counters of a settling call: cleared in front of its first verifier launch, downloaded behind its last
static int pool_stats_begin(spp_pool* p, hipStream_t st) {
  p->dense_groups[0] = p->dense_groups[1] = 0;
  if (p->verifier == SPP_POOL_VERIFY_RLC) HIP_TRY(hipMemsetAsync(p->dvstats.p, 0, sizeof p->vraw, st));
  return SPP_OK;
}

// screen has run and left prov, the verify list and its length; verdicts by instruction index into ok (zeroed here).
// which_key: 0 withdraw, 1 audit.  Mode RLC: a seed of its own per launch, from the operating system
static int pool_verify(spp_pool* p, hipStream_t st, int which_key, const uint8_t* dproofs, const uint8_t* dpws, uint32_t pw_len, uint32_t count,
                       const uint32_t* dlist, const uint32_t* dnlist, DevBuf& dok, RlcScratch& sc) {
  HIP_TRY(dok.alloc(count * sizeof(int32_t)));
  HIP_TRY(hipMemsetAsync(dok.p, 0, count * sizeof(int32_t), st));
  if (p->verifier == SPP_POOL_VERIFY_RLC) {
    RlcSeed seed;
    if (int e = rlc_os_seed(seed)) return e;
    if (int e = sc.alloc(p->key[which_key].nk, count, p->group)) return e;
    uint32_t* cnt = p->dvstats.as<uint32_t>() + 5 * which_key;
    if (p->compact) {
      launch_verify_rlc_list(st, p->key[which_key].dev(), p->rkey[which_key].dev(), dproofs, dpws, pw_len, count, dlist, dnlist, seed, p->group,
                             sc.ws.as<W256>(), sc.live.as<uint32_t>(), dok.as<int32_t>(), sc.list.as<uint32_t>(), cnt + 4, cnt);
      return SPP_OK;
    }
    p->dense_groups[which_key] = rlc_dense_groups(count, p->group);
    return rlc_verify_dense(st, p->key[which_key].dev(), p->rkey[which_key].dev(), dproofs, dpws, pw_len, count, seed, p->group, 0, sc,
                            dok.as<int32_t>(), cnt, cnt + 4);
  }
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
  RlcScratch sc;
  uint32_t rmask = 0, cnt[2];
  UP(dproofs, proofs, count * (size_t)SPP_PROOF_LEN);
  UP(dpws, pws, count * (size_t)SPP_AUDIT_PW_LEN);
  HIP_TRY(dprov.alloc(count * sizeof(int32_t)));
  HIP_TRY(dresult.alloc(count * sizeof(int32_t)));
  HIP_TRY(dlist.alloc(count * sizeof(uint32_t)));
  HIP_TRY(dnlist.alloc(sizeof(uint32_t)));
  HIP_TRY(hipMemsetAsync(dnlist.p, 0, sizeof(uint32_t), st));
  if (int e = pool_resolve_table(st, count, dslots, &rmask)) return e;
  if (int e = pool_stats_begin(p, st)) return e;
  const PoolSet& audits = p->set[SPP_POOL_AUDIT_RECORDS];
  const uint8_t* keys = dpws.as<uint8_t>() + POOL_A_WA;
  launch_pool_screen_audit(st, audits, p->salt, dpws.as<uint8_t>(), n, dprov.as<int32_t>(), dlist.as<uint32_t>(), dnlist.as<uint32_t>());
  if (int e = pool_verify(p, st, 1, dproofs.as<uint8_t>(), dpws.as<uint8_t>(), SPP_AUDIT_PW_LEN, n, dlist.as<uint32_t>(), dnlist.as<uint32_t>(), dok, sc)) return e;
  launch_pool_resolve(st, dslots.as<uint32_t>(), rmask, p->salt, keys, SPP_AUDIT_PW_LEN, n, dprov.as<int32_t>(), dok.as<int32_t>(), POOL_AUDIT_EXISTS,
                      dresult.as<int32_t>());
  launch_pool_commit(st, audits, p->salt, keys, SPP_AUDIT_PW_LEN, n, dresult.as<int32_t>(), p->d_counts + SPP_POOL_AUDIT_RECORDS);
  HIP_TRY(hipMemcpyAsync(result, dresult.p, count * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (int e = pool_fetch_counts(p, st, cnt)) return e;
  if (int e = pool_fetch_stats(p, st)) return e;
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  pool_stats_end(p);
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
  RlcScratch sc;
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
  if (int e = pool_stats_begin(p, st)) return e;
  const PoolSet& nullifiers = p->set[SPP_POOL_NULLIFIERS];
  const uint8_t* keys = dpws.as<uint8_t>() + POOL_W_NULLIFIER;
  launch_pool_screen_withdraw(st, p->d_state, p->set[SPP_POOL_AUDIT_RECORDS], nullifiers, p->salt, dpws.as<uint8_t>(), drecip.as<uint8_t>(), n,
                              dprov.as<int32_t>(), damounts.as<uint64_t>(), dlist.as<uint32_t>(), dnlist.as<uint32_t>());
  if (int e = pool_verify(p, st, 0, dproofs.as<uint8_t>(), dpws.as<uint8_t>(), SPP_WITHDRAW_PW_LEN, n, dlist.as<uint32_t>(), dnlist.as<uint32_t>(), dok, sc)) return e;
  launch_pool_resolve(st, dslots.as<uint32_t>(), rmask, p->salt, keys, SPP_WITHDRAW_PW_LEN, n, dprov.as<int32_t>(), dok.as<int32_t>(),
                      POOL_NULLIFIER_USED, dresult.as<int32_t>());
  launch_pool_commit(st, nullifiers, p->salt, keys, SPP_WITHDRAW_PW_LEN, n, dresult.as<int32_t>(), p->d_counts + SPP_POOL_NULLIFIERS);
  HIP_TRY(hipMemcpyAsync(result, dresult.p, count * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (amounts) HIP_TRY(hipMemcpyAsync(amounts, damounts.p, count * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  if (int e = pool_fetch_counts(p, st, cnt)) return e;
  if (int e = pool_fetch_stats(p, st)) return e;
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  pool_stats_end(p);
  p->counts[0] = cnt[0];
  p->counts[1] = cnt[1];
  return SPP_OK;
}

// A log of deposit / submit_audit / withdraw instructions in one call.  Order on the stream (pool_table.hpp has the argument):
// audit screen -> verify -> audit claim + settle -> withdraw screen at each position (resident sets + the audit resolve table) ->
// verify -> nullifier claim + settle -> both commits -> scatter to log order.  A kind without instructions launches nothing.
extern "C" int spp_pool_settle_log(spp_pool* p, size_t count, const uint8_t* kinds, size_t n_deposits, const uint8_t* roots, size_t n_audits,
                                   const uint8_t* audit_proofs, const uint8_t* audit_pws, size_t n_withdraws, const uint8_t* withdraw_proofs,
                                   const uint8_t* withdraw_pws, const uint8_t* recipients, int32_t* result, uint64_t* amounts) {
  if (!p || (count && (!kinds || !result)) || (n_deposits && !roots) || (n_audits && (!audit_proofs || !audit_pws)) ||
      (n_withdraws && (!withdraw_proofs || !withdraw_pws || !recipients)))
    return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (count > POOL_MAX_BATCH) return fail(SPP_ERR_BAD_INPUT, "too many instructions in one call (%zu; at most 2^24)", count);
  if (n_deposits > count || n_audits > count || n_withdraws > count || n_deposits + n_audits + n_withdraws != count)
    return fail(SPP_ERR_BAD_INPUT, "%zu deposits, %zu submit_audits and %zu withdraws are not %zu instructions", n_deposits, n_audits, n_withdraws, count);
  // the one pass over kinds: validation, and the index arrays in one block [audit_pos | withdraw_pos | deposits_before | audits_before]
  std::vector<uint32_t> index(n_audits + 3 * n_withdraws);
  uint32_t* ix = index.data();
  size_t n[3];
  if (!pool_log_index(kinds, count, n, n_audits, n_withdraws, ix, ix + n_audits, ix + n_audits + n_withdraws, ix + n_audits + 2 * n_withdraws))
    return fail(SPP_ERR_BAD_INPUT, "kinds: SPP_INSTR_DEPOSIT, SPP_INSTR_SUBMIT_AUDIT or SPP_INSTR_WITHDRAW");
  if (n[0] != n_deposits || n[1] != n_audits || n[2] != n_withdraws)
    return fail(SPP_ERR_BAD_INPUT, "kinds holds %zu deposits, %zu submit_audits and %zu withdraws, the counts say %zu, %zu and %zu", n[0], n[1], n[2],
                n_deposits, n_audits, n_withdraws);
  if (count == 0) return SPP_OK;
  spp_ctx* ctx = p->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (int e = pool_room(p, SPP_POOL_AUDIT_RECORDS, n_audits)) return e;
  if (int e = pool_room(p, SPP_POOL_NULLIFIERS, n_withdraws)) return e;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const uint32_t na = (uint32_t)n_audits, nw = (uint32_t)n_withdraws;
  const PoolSet& audits = p->set[SPP_POOL_AUDIT_RECORDS];
  const PoolSet& nullifiers = p->set[SPP_POOL_NULLIFIERS];

  // the ring after the call, and (for the withdraws) the entries every position is a window of
  PoolState next = p->state;
  for (size_t i = 0; i < n_deposits; i++) pool_add_root(next, roots + 32 * i);
  uint8_t resident[POOL_ROOTS * 32];
  pool_ring_entries(p->state, resident);

  DevBuf dindex, dall, dall_amounts, dring;
  DevBuf aproofs, apws, aprov, alist, anlist, aok, aslots, aresult;
  DevBuf wproofs, wpws, wrecip, wprov, wamounts, wlist, wnlist, wok, wslots, wresult;
  RlcScratch asc, wsc;
  uint32_t amask = 0, wmask = 0, cnt[2];
  // upload
  UP(dindex, index.data(), index.size() * sizeof(uint32_t));
  UP(aproofs, audit_proofs, n_audits * (size_t)SPP_PROOF_LEN);
  UP(apws, audit_pws, n_audits * (size_t)SPP_AUDIT_PW_LEN);
  UP(wproofs, withdraw_proofs, n_withdraws * (size_t)SPP_PROOF_LEN);
  UP(wpws, withdraw_pws, n_withdraws * (size_t)SPP_WITHDRAW_PW_LEN);
  UP(wrecip, recipients, n_withdraws * 32);
  if (nw) {
    HIP_TRY(dring.alloc((POOL_ROOTS + n_deposits) * 32));
    HIP_TRY(hipMemcpyAsync(dring.p, resident, sizeof resident, hipMemcpyHostToDevice, st));
    if (n_deposits) HIP_TRY(hipMemcpyAsync(dring.as<uint8_t>() + sizeof resident, roots, n_deposits * 32, hipMemcpyHostToDevice, st));
  }
  HIP_TRY(dall.alloc(count * sizeof(int32_t)));
  HIP_TRY(hipMemsetAsync(dall.p, 0, count * sizeof(int32_t), st));   // SPP_POOL_OK: what a deposit gives
  if (amounts) {
    HIP_TRY(dall_amounts.alloc(count * sizeof(uint64_t)));
    HIP_TRY(hipMemsetAsync(dall_amounts.p, 0, count * sizeof(uint64_t), st));
  }
  const uint32_t* audit_pos = dindex.as<uint32_t>();
  const uint32_t* withdraw_pos = audit_pos + na;
  const uint32_t* deposits_before = withdraw_pos + nw;
  const uint32_t* audits_before = deposits_before + nw;
  const uint8_t* akeys = apws.as<uint8_t>() + POOL_A_WA;
  const uint8_t* wkeys = wpws.as<uint8_t>() + POOL_W_NULLIFIER;

  // the submit_audits among themselves; the table stays for the withdraws (all empty when there is no submit_audit)
  if (int e = pool_resolve_table(st, n_audits, aslots, &amask)) return e;
  if (int e = pool_stats_begin(p, st)) return e;
  if (na) {
    HIP_TRY(aprov.alloc(n_audits * sizeof(int32_t)));
    HIP_TRY(aresult.alloc(n_audits * sizeof(int32_t)));
    HIP_TRY(alist.alloc(n_audits * sizeof(uint32_t)));
    HIP_TRY(anlist.alloc(sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(anlist.p, 0, sizeof(uint32_t), st));
    launch_pool_screen_audit(st, audits, p->salt, apws.as<uint8_t>(), na, aprov.as<int32_t>(), alist.as<uint32_t>(), anlist.as<uint32_t>());
    if (int e = pool_verify(p, st, 1, aproofs.as<uint8_t>(), apws.as<uint8_t>(), SPP_AUDIT_PW_LEN, na, alist.as<uint32_t>(), anlist.as<uint32_t>(), aok, asc)) return e;
    launch_pool_resolve(st, aslots.as<uint32_t>(), amask, p->salt, akeys, SPP_AUDIT_PW_LEN, na, aprov.as<int32_t>(), aok.as<int32_t>(), POOL_AUDIT_EXISTS,
                        aresult.as<int32_t>());
  }
  // the withdraws, each against the ring and the audit records as of its position
  if (nw) {
    HIP_TRY(wprov.alloc(n_withdraws * sizeof(int32_t)));
    HIP_TRY(wresult.alloc(n_withdraws * sizeof(int32_t)));
    HIP_TRY(wamounts.alloc(n_withdraws * sizeof(uint64_t)));
    HIP_TRY(wlist.alloc(n_withdraws * sizeof(uint32_t)));
    HIP_TRY(wnlist.alloc(sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(wnlist.p, 0, sizeof(uint32_t), st));
    if (int e = pool_resolve_table(st, n_withdraws, wslots, &wmask)) return e;
    const PoolLogView view{dring.as<uint8_t>(), aslots.as<uint32_t>(), amask, akeys, SPP_AUDIT_PW_LEN};
    launch_pool_screen_withdraw_log(st, view, audits, nullifiers, p->salt, wpws.as<uint8_t>(), wrecip.as<uint8_t>(), deposits_before, audits_before, nw,
                                    wprov.as<int32_t>(), wamounts.as<uint64_t>(), wlist.as<uint32_t>(), wnlist.as<uint32_t>());
    if (int e = pool_verify(p, st, 0, wproofs.as<uint8_t>(), wpws.as<uint8_t>(), SPP_WITHDRAW_PW_LEN, nw, wlist.as<uint32_t>(), wnlist.as<uint32_t>(), wok, wsc)) return e;
    launch_pool_resolve(st, wslots.as<uint32_t>(), wmask, p->salt, wkeys, SPP_WITHDRAW_PW_LEN, nw, wprov.as<int32_t>(), wok.as<int32_t>(),
                        POOL_NULLIFIER_USED, wresult.as<int32_t>());
  }
  // the commits, after the last screen; then log order
  if (na) {
    launch_pool_commit(st, audits, p->salt, akeys, SPP_AUDIT_PW_LEN, na, aresult.as<int32_t>(), p->d_counts + SPP_POOL_AUDIT_RECORDS);
    launch_pool_scatter(st, audit_pos, na, aresult.as<int32_t>(), dall.as<int32_t>(), nullptr, nullptr);
  }
  if (nw) {
    launch_pool_commit(st, nullifiers, p->salt, wkeys, SPP_WITHDRAW_PW_LEN, nw, wresult.as<int32_t>(), p->d_counts + SPP_POOL_NULLIFIERS);
    launch_pool_scatter(st, withdraw_pos, nw, wresult.as<int32_t>(), dall.as<int32_t>(), wamounts.as<uint64_t>(),
                        amounts ? dall_amounts.as<uint64_t>() : nullptr);
  }
  if (n_deposits) HIP_TRY(hipMemcpyAsync(p->d_state, &next, sizeof(PoolState), hipMemcpyHostToDevice, st));
  // download
  HIP_TRY(hipMemcpyAsync(result, dall.p, count * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (amounts) HIP_TRY(hipMemcpyAsync(amounts, dall_amounts.p, count * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  if (int e = pool_fetch_counts(p, st, cnt)) return e;
  if (int e = pool_fetch_stats(p, st)) return e;
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  pool_stats_end(p);
  p->state = next;   // the host ring takes the batch's roots only now, after the stream has come through without an error
  p->counts[0] = cnt[0];
  p->counts[1] = cnt[1];
  return SPP_OK;
}
