// The pool ledger on the device: settling a batch of submit_audit / withdraw instructions with the decisions the pool program
// makes processing them one at a time in order (shielded_pool_program/src/instructions/submit_audit.rs, withdraw.rs, state.rs).
// Everything a lane does is in csrc/pool_table.hpp, where the ordering argument is written down; this file is the launch shapes.
//
//   screen    one lane per instruction: the checks that need no proof (ring, recipient, probes of the resident sets), a provisional
//             code, and the compacted list of instructions whose proof still matters (the verifier costs the same for a wave with
//             one live lane as for a full one, and a replayed log is mostly instructions whose account already exists)
//   verify    k_verify_list (kernels_verify.hip) over that list, its length read from device memory
//   claim     candidates (everything passed, proof included) claim their key in the per-call resolve table: lowest index wins
//   settle    every undecided instruction reads the winner of its key back and gets its final code
//   commit    winners only: the key goes into the resident set, the set's count goes up
// A log of all three kinds (spp_pool_settle_log) is the same steps for its submit_audits and then for its withdraws, with the
// withdraw screen reading the audit resolve table and both commits after it, and a scatter of the codes to log order.
// The resident sets are read in screen and written in commit only; the resolve table is written in claim and read in settle only:
// every dependence crosses a kernel boundary on one stream.  32-bit atomicCAS / atomicMin / atomicAdd on global memory, plain
// stores otherwise.
#include "kernels.hpp"
#include "pool_table.hpp"

namespace spp {

// appends instruction i to the verify list; the order of the list is arbitrary, the verdicts are stored by instruction index
__device__ __forceinline__ void pool_list_push(uint32_t* list, uint32_t* n_list, uint32_t i) { list[atomicAdd(n_list, 1u)] = i; }

__global__ void __launch_bounds__(256) k_pool_screen_audit(PoolSet audits, uint64_t salt, const uint8_t* __restrict__ pws, uint32_t count,
                                                           int32_t* __restrict__ prov, uint32_t* __restrict__ list, uint32_t* n_list) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int32_t c = pool_screen_audit(audits, salt, pws + (size_t)i * POOL_AUDIT_PW);
  prov[i] = c;
  if (c == POOL_PENDING_PROOF) pool_list_push(list, n_list, i);
}

__global__ void __launch_bounds__(256) k_pool_screen_withdraw(const PoolState* __restrict__ state, PoolSet audits, PoolSet nullifiers, uint64_t salt,
                                                              const uint8_t* __restrict__ pws, const uint8_t* __restrict__ recipients,
                                                              uint32_t count, int32_t* __restrict__ prov, uint64_t* __restrict__ amounts,
                                                              uint32_t* __restrict__ list, uint32_t* n_list) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint8_t* pw = pws + (size_t)i * POOL_WITHDRAW_PW;
  amounts[i] = pool_amount_u64(pw);
  const int32_t c = pool_screen_withdraw(*state, audits, nullifiers, salt, pw, recipients + (size_t)i * 32);
  prov[i] = c;
  if (c == POOL_PENDING_PROOF) pool_list_push(list, n_list, i);
}

// A withdraw of a log (spp_pool_settle_log): lane r is the withdraw of rank r, which sees the ring after deposits_before[r] of the
// batch's roots and the audit records of the submit_audits of rank < audits_before[r].  Runs after the audit claim, before any commit.
__global__ void __launch_bounds__(256) k_pool_screen_withdraw_log(PoolLogView view, PoolSet audits, PoolSet nullifiers, uint64_t salt,
                                                                  const uint8_t* __restrict__ pws, const uint8_t* __restrict__ recipients,
                                                                  const uint32_t* __restrict__ deposits_before,
                                                                  const uint32_t* __restrict__ audits_before, uint32_t count,
                                                                  int32_t* __restrict__ prov, uint64_t* __restrict__ amounts,
                                                                  uint32_t* __restrict__ list, uint32_t* n_list) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint8_t* pw = pws + (size_t)i * POOL_WITHDRAW_PW;
  amounts[i] = pool_amount_u64(pw);
  const int32_t c = pool_screen_withdraw_at(view, deposits_before[i], audits_before[i], audits, nullifiers, salt, pw, recipients + (size_t)i * 32);
  prov[i] = c;
  if (c == POOL_PENDING_PROOF) pool_list_push(list, n_list, i);
}

// the codes (and amounts, when asked for) of one kind, by rank, to their positions in the log
__global__ void __launch_bounds__(256) k_pool_scatter(const uint32_t* __restrict__ pos, uint32_t count, const int32_t* __restrict__ codes,
                                                      int32_t* __restrict__ result, const uint64_t* __restrict__ amounts,
                                                      uint64_t* __restrict__ amounts_out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  result[pos[i]] = codes[i];
  if (amounts_out) amounts_out[pos[i]] = amounts[i];
}

// import_keys: a key that is resident is done (any final code but OK); the others are candidates without a proof to check
__global__ void __launch_bounds__(256) k_pool_screen_import(PoolSet set, uint64_t salt, const uint8_t* __restrict__ keys, uint32_t count,
                                                            int32_t* __restrict__ prov) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  prov[i] = pool_set_contains(set, salt, keys + (size_t)i * 32) ? POOL_AUDIT_EXISTS : POOL_PENDING_PROOF;
}

__global__ void __launch_bounds__(256) k_pool_contains(PoolSet set, uint64_t salt, const uint8_t* __restrict__ keys, uint32_t count,
                                                       uint8_t* __restrict__ present) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  present[i] = pool_set_contains(set, salt, keys + (size_t)i * 32) ? 1 : 0;
}

// proof_ok == nullptr: no proofs in this call (import_keys), every pending instruction is a candidate
__global__ void __launch_bounds__(256) k_pool_claim(uint32_t* slots, uint32_t mask, uint64_t salt, const uint8_t* __restrict__ keys, uint32_t stride,
                                                    uint32_t count, const int32_t* __restrict__ prov, const int32_t* __restrict__ proof_ok) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  if (pool_is_candidate(prov[i], proof_ok ? proof_ok[i] != 0 : true)) pool_resolve_claim(slots, mask, salt, keys, stride, i);
}

__global__ void __launch_bounds__(256) k_pool_settle(const uint32_t* __restrict__ slots, uint32_t mask, uint64_t salt, const uint8_t* __restrict__ keys,
                                                     uint32_t stride, uint32_t count, const int32_t* __restrict__ prov,
                                                     const int32_t* __restrict__ proof_ok, int32_t dup, int32_t* __restrict__ result) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int32_t p = prov[i];
  const uint32_t w = p >= 0 ? POOL_NONE : pool_resolve_winner(slots, mask, salt, keys, stride, i);
  result[i] = pool_final_code(p, proof_ok ? proof_ok[i] != 0 : true, w, i, dup);
}

__global__ void __launch_bounds__(256) k_pool_commit(PoolSet set, uint64_t salt, const uint8_t* __restrict__ keys, uint32_t stride, uint32_t count,
                                                     const int32_t* __restrict__ result, uint32_t* set_count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  if (result[i] != POOL_OK) return;
  pool_set_insert_unique(set, salt, keys + (size_t)i * stride);
  atomicAdd(set_count, 1u);
}

static inline dim3 pool_grid(uint32_t count) { return dim3((count + 255) / 256); }

void launch_pool_screen_audit(hipStream_t st, const PoolSet& audits, uint64_t salt, const uint8_t* pws, uint32_t count, int32_t* prov, uint32_t* list,
                              uint32_t* n_list) {
  hipLaunchKernelGGL(k_pool_screen_audit, pool_grid(count), dim3(256), 0, st, audits, salt, pws, count, prov, list, n_list);
}
void launch_pool_screen_withdraw(hipStream_t st, const PoolState* state, const PoolSet& audits, const PoolSet& nullifiers, uint64_t salt,
                                 const uint8_t* pws, const uint8_t* recipients, uint32_t count, int32_t* prov, uint64_t* amounts, uint32_t* list,
                                 uint32_t* n_list) {
  hipLaunchKernelGGL(k_pool_screen_withdraw, pool_grid(count), dim3(256), 0, st, state, audits, nullifiers, salt, pws, recipients, count, prov, amounts,
                     list, n_list);
}
void launch_pool_screen_withdraw_log(hipStream_t st, const PoolLogView& view, const PoolSet& audits, const PoolSet& nullifiers, uint64_t salt,
                                     const uint8_t* pws, const uint8_t* recipients, const uint32_t* deposits_before, const uint32_t* audits_before,
                                     uint32_t count, int32_t* prov, uint64_t* amounts, uint32_t* list, uint32_t* n_list) {
  hipLaunchKernelGGL(k_pool_screen_withdraw_log, pool_grid(count), dim3(256), 0, st, view, audits, nullifiers, salt, pws, recipients, deposits_before,
                     audits_before, count, prov, amounts, list, n_list);
}
void launch_pool_scatter(hipStream_t st, const uint32_t* pos, uint32_t count, const int32_t* codes, int32_t* result, const uint64_t* amounts,
                         uint64_t* amounts_out) {
  hipLaunchKernelGGL(k_pool_scatter, pool_grid(count), dim3(256), 0, st, pos, count, codes, result, amounts, amounts_out);
}
void launch_pool_screen_import(hipStream_t st, const PoolSet& set, uint64_t salt, const uint8_t* keys, uint32_t count, int32_t* prov) {
  hipLaunchKernelGGL(k_pool_screen_import, pool_grid(count), dim3(256), 0, st, set, salt, keys, count, prov);
}
void launch_pool_contains(hipStream_t st, const PoolSet& set, uint64_t salt, const uint8_t* keys, uint32_t count, uint8_t* present) {
  hipLaunchKernelGGL(k_pool_contains, pool_grid(count), dim3(256), 0, st, set, salt, keys, count, present);
}
void launch_pool_resolve(hipStream_t st, uint32_t* slots, uint32_t mask, uint64_t salt, const uint8_t* keys, uint32_t stride, uint32_t count,
                         const int32_t* prov, const int32_t* proof_ok, int32_t dup, int32_t* result) {
  hipLaunchKernelGGL(k_pool_claim, pool_grid(count), dim3(256), 0, st, slots, mask, salt, keys, stride, count, prov, proof_ok);
  hipLaunchKernelGGL(k_pool_settle, pool_grid(count), dim3(256), 0, st, slots, mask, salt, keys, stride, count, prov, proof_ok, dup, result);
}
void launch_pool_commit(hipStream_t st, const PoolSet& set, uint64_t salt, const uint8_t* keys, uint32_t stride, uint32_t count, const int32_t* result,
                        uint32_t* set_count) {
  hipLaunchKernelGGL(k_pool_commit, pool_grid(count), dim3(256), 0, st, set, salt, keys, stride, count, result, set_count);
}

}  // namespace spp
