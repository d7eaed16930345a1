// The pool ledger, host + gfx950: the per-lane pieces of the kernels in kernels_pool.hip and of the host check
// tests/host/pool_table_check.cpp.  A device-resident restatement of what the pool program keeps and decides
// (paths relative to the reference tree, shielded_pool_program/src):
//   PoolState      ShieldedPoolState, state.rs:6-17: "poolstat", current_root, roots[32], roots_index; add_root / check_root :28-46
//   PoolSet        the accounts whose existence the program tests: the ["nullifier", n] PDAs (instructions/withdraw.rs:137-147) and
//                  the ["audit", wa_commitment] PDAs (instructions/submit_audit.rs:66-73, withdraw.rs:94-125), each as an open-
//                  addressing table of 32-byte keys
//   resolve table  duplicates INSIDE one batch, decided in parallel with the result of processing the batch in order
//
// Keys are the 32 raw bytes of a public-witness word, compared bytewise (v and v + r are two PDAs, so two keys).
//
// Resident sets.  A power-of-two number of slots >= 2 x capacity; slot s is a 32-bit claim word (0 = empty) and 32 key bytes.
// A key's home slot is pool_slot(): the low 64 bits of the key xor a per-pool salt, through the splitmix64 finaliser; probing is
// linear and wraps.  Keys are never removed (the program never closes these accounts), so a probe ends at the key or at the first
// empty slot.  The sets are READ by the screen kernel only and WRITTEN by the commit kernel only: the kernel boundary is the
// fence, no lane ever reads a key another lane of the same launch writes.  The commit kernel inserts keys that are unique and
// known to be absent, so claiming a slot with one 32-bit compare-and-swap and then writing the key with plain stores suffices.
//
// Resolve table (per call, >= 2 x count slots of 32-bit batch INDICES, 0xFFFFFFFF = empty).  The rule the program's order implies:
// among the instructions of one key that would succeed if they came first ("candidates"), the lowest index wins; every later
// instruction of that key -- candidate or not -- meets the account the winner created.  A candidate claims an empty slot with
// atomicCAS(slot, EMPTY, i); on a slot that holds index j it compares key(j) with key(i) through the immutable input buffer:
// equal -> atomicMin(slot, i), else probe on.  A slot only ever changes from EMPTY to an index and then to lower indices OF THE
// SAME KEY, so the key a slot stands for is fixed by its first claim, no key bytes are written at all, and whatever order the
// lanes arrive in the slot ends at the minimum: the result does not depend on scheduling.  A second launch reads the winner back.
#pragma once
#include "bn254.hpp"

namespace spp {

// ---- decisions (include/spp.h, SPP_POOL_*) ----
static constexpr int32_t POOL_OK = 0, POOL_AUDIT_EXISTS = 1, POOL_NO_AUDIT_RECORD = 2, POOL_BAD_ROOT = 3, POOL_NULLIFIER_USED = 4,
                         POOL_BAD_RECIPIENT = 5, POOL_BAD_PROOF = 6;
// provisional codes of the screen kernel: a final code (>= 0), or "undecided until the duplicate rule has spoken":
//   POOL_PENDING_PROOF        every check but the proof passed; the proof is on the verify list
//   pool_pending_refused(c)   the instruction fails with c whatever its proof is -- unless an earlier instruction of the batch
//                             spends the key first, which the program notices before it gets to c
static constexpr int32_t POOL_PENDING_PROOF = -1;
SPP_HD int32_t pool_pending_refused(int32_t c) { return -2 - c; }
static constexpr uint32_t POOL_NONE = 0xFFFFFFFFu;   // empty resolve slot / "no winner"

static constexpr uint32_t POOL_WITHDRAW_PW = 172, POOL_AUDIT_PW = 76, POOL_PROOF = 388;
// offsets of the public words in the two public witnesses (withdraw.rs:74-90, submit_audit.rs:41-54)
static constexpr uint32_t POOL_W_ROOT = 12, POOL_W_NULLIFIER = 44, POOL_W_RECIPIENT = 76, POOL_W_AMOUNT = 108, POOL_W_WA = 140;
static constexpr uint32_t POOL_A_WA = 12;

SPP_HD bool pool_key_equal(const uint8_t* a, const uint8_t* b) {
  uint32_t o = 0;
  for (int i = 0; i < 32; i++) o |= (uint32_t)(a[i] ^ b[i]);
  return o == 0;
}

// ---- ShieldedPoolState (state.rs:6-46) ----
static constexpr uint32_t POOL_ROOTS = 32, POOL_STATE_LEN = 1072;
struct PoolState {
  uint8_t current_root[32];
  uint8_t roots[POOL_ROOTS][32];
  uint32_t roots_index;
};
SPP_HD void pool_state_init(PoolState& s) {   // initialize.rs:65-69: everything zero
  for (int i = 0; i < 32; i++) s.current_root[i] = 0;
  for (uint32_t k = 0; k < POOL_ROOTS; k++)
    for (int i = 0; i < 32; i++) s.roots[k][i] = 0;
  s.roots_index = 0;
}
SPP_HD void pool_add_root(PoolState& s, const uint8_t* root) {   // state.rs:28-33
  const uint32_t idx = s.roots_index % POOL_ROOTS;
  for (int i = 0; i < 32; i++) s.current_root[i] = s.roots[idx][i] = root[i];
  s.roots_index += 1u;   // wrapping_add
}
SPP_HD bool pool_check_root(const PoolState& s, const uint8_t* root) {   // state.rs:36-46
  if (pool_key_equal(s.current_root, root)) return true;
  for (uint32_t k = 0; k < POOL_ROOTS; k++)
    if (pool_key_equal(s.roots[k], root)) return true;
  return false;
}
// the account bytes as bytemuck lays the struct out (state.rs:6-17)
SPP_HD void pool_state_bytes(const PoolState& s, uint8_t out[POOL_STATE_LEN]) {
  const char* tag = "poolstat";
  for (int i = 0; i < 8; i++) out[i] = (uint8_t)tag[i];
  for (int i = 0; i < 32; i++) out[8 + i] = s.current_root[i];
  for (uint32_t k = 0; k < POOL_ROOTS; k++)
    for (int i = 0; i < 32; i++) out[40 + 32 * k + i] = s.roots[k][i];
  for (int i = 0; i < 4; i++) out[1064 + i] = (uint8_t)(s.roots_index >> (8 * i));
  for (int i = 0; i < 4; i++) out[1068 + i] = 0;
}

// ---- slot function ----
SPP_HD uint64_t pool_key_low64(const uint8_t* key) {   // the low 64 bits of the big-endian word: bytes 24..31
  uint64_t v = 0;
  for (int i = 24; i < 32; i++) v = (v << 8) | key[i];
  return v;
}
SPP_HD uint64_t pool_mix64(uint64_t z) {   // splitmix64's finaliser
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
SPP_HD uint32_t pool_slot(const uint8_t* key, uint64_t salt, uint32_t mask) { return (uint32_t)pool_mix64(pool_key_low64(key) ^ salt) & mask; }
// slots for a set of `capacity` keys, or for resolving a batch of `capacity` instructions: the power of two >= 2 x capacity
SPP_HD uint32_t pool_slots_for(uint64_t capacity) {
  uint32_t n = 2;
  while ((uint64_t)n < 2 * capacity) n <<= 1;
  return n;
}

// the two read-modify-write steps: device atomics on the GPU, plain code in the (single-threaded) host check
SPP_HD uint32_t pool_cas(uint32_t* p, uint32_t expect, uint32_t val) {
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicCAS(p, expect, val);
#else
  const uint32_t old = *p;
  if (old == expect) *p = val;
  return old;
#endif
}
SPP_HD void pool_min(uint32_t* p, uint32_t val) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin(p, val);
#else
  if (val < *p) *p = val;
#endif
}

// ---- resident sets ----
struct PoolSet {
  uint32_t* claim;   // slots x 32-bit: 0 = empty, 1 = holds a key
  uint8_t* keys;     // slots x 32 B
  uint32_t mask;     // slots - 1
};
// Is `key` in the set?  Only for launches that do not insert (see the header comment).
SPP_HD bool pool_set_contains(const PoolSet& t, uint64_t salt, const uint8_t* key) {
  for (uint32_t s = pool_slot(key, salt, t.mask);; s = (s + 1) & t.mask) {
    if (t.claim[s] == 0) return false;
    if (pool_key_equal(t.keys + (size_t)s * 32, key)) return true;
  }
}
// Inserts a key that is absent and that no other lane of the launch inserts; returns its slot.  The set holds at most
// slots / 2 keys, so an empty slot is always found.
SPP_HD uint32_t pool_set_insert_unique(const PoolSet& t, uint64_t salt, const uint8_t* key) {
  for (uint32_t s = pool_slot(key, salt, t.mask);; s = (s + 1) & t.mask) {
    if (pool_cas(&t.claim[s], 0u, 1u) != 0u) continue;
    uint8_t* dst = t.keys + (size_t)s * 32;
    for (int i = 0; i < 32; i++) dst[i] = key[i];
    return s;
  }
}

// ---- resolve table ----
// keys: the input buffer; key of instruction i = keys + i * stride (stride and offset folded in by the caller)
SPP_HD void pool_resolve_claim(uint32_t* slots, uint32_t mask, uint64_t salt, const uint8_t* keys, size_t stride, uint32_t i) {
  const uint8_t* key = keys + (size_t)i * stride;
  for (uint32_t s = pool_slot(key, salt, mask);; s = (s + 1) & mask) {
    const uint32_t cur = pool_cas(&slots[s], POOL_NONE, i);
    if (cur == POOL_NONE) return;
    if (pool_key_equal(keys + (size_t)cur * stride, key)) {
      pool_min(&slots[s], i);
      return;
    }
  }
}
// after every claim of the batch has been made (the next launch): the lowest candidate index of i's key, POOL_NONE if there is none
SPP_HD uint32_t pool_resolve_winner(const uint32_t* slots, uint32_t mask, uint64_t salt, const uint8_t* keys, size_t stride, uint32_t i) {
  const uint8_t* key = keys + (size_t)i * stride;
  for (uint32_t s = pool_slot(key, salt, mask);; s = (s + 1) & mask) {
    const uint32_t cur = slots[s];
    if (cur == POOL_NONE) return POOL_NONE;
    if (cur == i || pool_key_equal(keys + (size_t)cur * stride, key)) return cur;
  }
}
// the final code of instruction i: prov from the screen, proof_ok from the verifier (read only for POOL_PENDING_PROOF), winner
// from pool_resolve_winner, dup = what the program answers when the account exists (AUDIT_EXISTS / NULLIFIER_USED)
SPP_HD bool pool_is_candidate(int32_t prov, bool proof_ok) { return prov == POOL_PENDING_PROOF && proof_ok; }
SPP_HD int32_t pool_final_code(int32_t prov, bool proof_ok, uint32_t winner, uint32_t i, int32_t dup) {
  if (prov >= 0) return prov;
  if (winner < i) return dup;
  if (prov == POOL_PENDING_PROOF) return proof_ok ? POOL_OK : POOL_BAD_PROOF;
  return -2 - prov;
}

// ---- screens (one instruction each) ----
// submit_audit.rs:41-73: an existing record answers Ok before the proof is looked at
SPP_HD int32_t pool_screen_audit(const PoolSet& audits, uint64_t salt, const uint8_t* pw) {
  return pool_set_contains(audits, salt, pw + POOL_A_WA) ? POOL_AUDIT_EXISTS : POOL_PENDING_PROOF;
}
// withdraw.rs:157-161
SPP_HD uint64_t pool_amount_u64(const uint8_t* pw) { return pool_key_low64(pw + POOL_W_AMOUNT); }
// withdraw.rs:150-154: the recipient word is 00 00 | address[0..30]
SPP_HD bool pool_recipient_matches(const uint8_t* word, const uint8_t* address) {
  uint32_t o = word[0] | word[1];
  for (int i = 0; i < 30; i++) o |= (uint32_t)(word[2 + i] ^ address[i]);
  return o == 0;
}
// withdraw.rs:94-154, the checks in program order
SPP_HD int32_t pool_screen_withdraw(const PoolState& st, const PoolSet& audits, const PoolSet& nullifiers, uint64_t salt, const uint8_t* pw,
                                    const uint8_t* address) {
  if (!pool_set_contains(audits, salt, pw + POOL_W_WA)) return POOL_NO_AUDIT_RECORD;
  if (!pool_check_root(st, pw + POOL_W_ROOT)) return POOL_BAD_ROOT;
  if (pool_set_contains(nullifiers, salt, pw + POOL_W_NULLIFIER)) return POOL_NULLIFIER_USED;
  if (!pool_recipient_matches(pw + POOL_W_RECIPIENT, address)) return pool_pending_refused(POOL_BAD_RECIPIENT);
  return POOL_PENDING_PROOF;
}

}  // namespace spp
