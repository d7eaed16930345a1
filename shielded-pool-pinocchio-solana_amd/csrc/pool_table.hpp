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
//
// A log of all three kinds in one call (spp_pool_settle_log; state.rs:28-46, instructions/deposit.rs:21-37, submit_audit.rs:41-87,
// withdraw.rs:94-175).  The dependences between kinds run one way: a deposit depends on nothing and pushes its root; a
// submit_audit depends on the audit set and on earlier submit_audits only; a withdraw reads the audit set and the ring AS OF ITS
// POSITION and the nullifier set, and nothing a withdraw does feeds back into a deposit or an audit.  So the audits are settled
// first, by the rule above over their ranks (rank = index among the instructions of one kind), and two cross-kind rules let every
// withdraw be screened on its own lane:
//   audit record at a position   the record of wa_commitment exists for a withdraw with `a` audits before it iff the key is
//                                resident or the audit resolve table's winner of that key has a rank < a: the winner is the lowest
//                                candidate, candidates are the only instructions that create the record, and a key with a resident
//                                record has no candidate at all.  The lookup is by a key of ANOTHER buffer (pool_resolve_find).
//   ring at a position           the resident ring's 32 entries in push order, oldest first (pool_ring_entries), followed by the
//                                batch's deposit roots: after the first d of them the ring holds entries d .. d+31 and
//                                current_root is entry d+31, because add_root overwrites the oldest slot (pool_check_root_at).
// With the audit-record and root checks position-exact and final, the withdraws are left coupled through their nullifiers only,
// which is the rule above over withdraw ranks.  The audit COMMIT comes after the withdraw screen: were the records inserted first, a
// withdraw that precedes its submit_audit in the log would find them.  The resident sets stay "read in screens, written in commits".
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
// The ring of a log.  entries: the 32 slots in the order add_root will overwrite them, oldest first (slots never written are zero
// and come first, which is the zero root of a fresh pool), then -- appended by the caller -- the roots the batch's deposits push.
SPP_HD void pool_ring_entries(const PoolState& s, uint8_t out[POOL_ROOTS * 32]) {
  for (uint32_t k = 0; k < POOL_ROOTS; k++) {
    const uint32_t slot = (s.roots_index + k) % POOL_ROOTS;
    for (int i = 0; i < 32; i++) out[32 * k + i] = s.roots[slot][i];
  }
}
// check_root (state.rs:36-46) on the state after `pushed` of the batch's roots: current_root is the newest entry, roots[] the 32
// newest.  On a pool that has seen no push at all both are zero, as the account is.
SPP_HD bool pool_check_root_at(const uint8_t* entries, uint32_t pushed, const uint8_t* root) {
  const uint8_t* ring = entries + (size_t)pushed * 32;
  if (pool_key_equal(ring + (POOL_ROOTS - 1) * 32, root)) return true;   // current_root
  for (uint32_t k = 0; k < POOL_ROOTS; k++)
    if (pool_key_equal(ring + k * 32, root)) return true;
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
// the same for a key that lies in another buffer (a withdraw's wa_commitment in the table its batch's submit_audits claimed)
SPP_HD uint32_t pool_resolve_find(const uint32_t* slots, uint32_t mask, uint64_t salt, const uint8_t* keys, size_t stride, const uint8_t* key) {
  for (uint32_t s = pool_slot(key, salt, mask);; s = (s + 1) & mask) {
    const uint32_t cur = slots[s];
    if (cur == POOL_NONE) return POOL_NONE;
    if (pool_key_equal(keys + (size_t)cur * stride, key)) return cur;
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

// ---- a log of all three kinds ----
// What a withdraw of a log sees of the instructions before it: the ring entries (above), how many of the batch's deposits and
// submit_audits precede it, and the resolve table the submit_audits claimed (keys: their wa_commitments, by audit rank).
struct PoolLogView {
  const uint8_t* ring;          // (32 + deposits) x 32 B
  const uint32_t* audit_slots;  // the audit resolve table, after every claim
  uint32_t audit_mask;
  const uint8_t* audit_keys;    // key of audit rank r = audit_keys + r * audit_stride
  size_t audit_stride;
};
// withdraw.rs:94-125 at a position
SPP_HD bool pool_audit_record_at(const PoolLogView& v, const PoolSet& audits, uint64_t salt, uint32_t audits_before, const uint8_t* wa) {
  if (pool_set_contains(audits, salt, wa)) return true;
  return pool_resolve_find(v.audit_slots, v.audit_mask, salt, v.audit_keys, v.audit_stride, wa) < audits_before;   // POOL_NONE is above every rank
}
// withdraw.rs:94-154 at a position, the checks in program order; the provisional codes are pool_screen_withdraw's
SPP_HD int32_t pool_screen_withdraw_at(const PoolLogView& v, uint32_t deposits_before, uint32_t audits_before, const PoolSet& audits,
                                       const PoolSet& nullifiers, uint64_t salt, const uint8_t* pw, const uint8_t* address) {
  if (!pool_audit_record_at(v, audits, salt, audits_before, pw + POOL_W_WA)) return POOL_NO_AUDIT_RECORD;
  if (!pool_check_root_at(v.ring, deposits_before, pw + POOL_W_ROOT)) return POOL_BAD_ROOT;
  if (pool_set_contains(nullifiers, salt, pw + POOL_W_NULLIFIER)) return POOL_NULLIFIER_USED;
  if (!pool_recipient_matches(pw + POOL_W_RECIPIENT, address)) return pool_pending_refused(POOL_BAD_RECIPIENT);
  return POOL_PENDING_PROOF;
}

// The index arrays of a log, on the host: the caller has to read the `count` kind bytes once anyway to validate them, and a running
// count per kind in that pass is all a scan would compute, so no device scan is spent on one byte per instruction.
//   n[k]                  instructions of kind k (0 deposit, 1 submit_audit, 2 withdraw)
//   audit_pos[r]          position in the log of the submit_audit of rank r;  withdraw_pos[r] likewise
//   deposits_before[r], audits_before[r]   of the withdraw of rank r
// The arrays hold max_audits / max_withdraws entries (0 and NULL: a counting pass); ranks past them are counted, not written, so
// a caller whose per-kind counts disagree with kinds finds out from n[] after the same pass.  false: a kind byte above 2.
static constexpr uint8_t POOL_INSTR_DEPOSIT = 0, POOL_INSTR_SUBMIT_AUDIT = 1, POOL_INSTR_WITHDRAW = 2;
inline bool pool_log_index(const uint8_t* kinds, size_t count, size_t n[3], size_t max_audits, size_t max_withdraws, uint32_t* audit_pos,
                           uint32_t* withdraw_pos, uint32_t* deposits_before, uint32_t* audits_before) {
  n[0] = n[1] = n[2] = 0;
  for (size_t i = 0; i < count; i++) {
    const uint8_t k = kinds[i];
    if (k > POOL_INSTR_WITHDRAW) return false;
    if (k == POOL_INSTR_SUBMIT_AUDIT && n[1] < max_audits) audit_pos[n[1]] = (uint32_t)i;
    if (k == POOL_INSTR_WITHDRAW && n[2] < max_withdraws) {
      withdraw_pos[n[2]] = (uint32_t)i;
      deposits_before[n[2]] = (uint32_t)n[0];
      audits_before[n[2]] = (uint32_t)n[1];
    }
    n[k]++;
  }
  return true;
}

}  // namespace spp
