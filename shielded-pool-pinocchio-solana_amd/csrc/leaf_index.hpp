// The leaf index of the resident Merkle tree, host + gfx950: the per-lane pieces of the kernels in kernels_wallet.hip and of the
// host check tests/host/leaf_index_check.cpp.  It goes from a leaf VALUE back to its POSITIONS, which is what a wallet needs that
// has lost its indices (the reference keeps them per deposit in the browser: DepositRecord.leafIndex and MerkleTreeState.leaves,
// demo-frontend/app/lib/storage.ts:9-26,45-50, carried between browsers by exportData / importDeposits :233-260).
//
// Table.  One open-addressing table of 32-bit leaf INDICES per tree, LEAF_NONE = empty, leaf_index_slots(n) = pool_slots_for(max(n,
// 32)) slots for n indexed leaves, so it is never more than half full and every probe run ends at an empty slot.  No key bytes are
// stored: the key of an entry i is level[0][i] of the tree, read through the leaf array, as the resolve table of pool_table.hpp reads
// its keys through the input buffer.  The home slot of a value is pool_slot() of its canonical 32-byte big-endian encoding under a
// per-tree 64-bit salt (leaf_home computes the same number from the canonical limbs); probing is linear and wraps.
//
// Occurrences.  EVERY leaf gets a slot of its own: leaf i claims the first empty slot of its probe run with one
// atomicCAS(slot, LEAF_NONE, i) and never compares keys while inserting.  A value that sits at several leaves therefore holds
// several slots of one run, mixed with the entries of other values that probe through the same slots.
//
// Why the answers do not depend on scheduling.  Leaves are never removed, and a claimed slot never changes again.  When all
// inserts of a launch are done, leaf i sits somewhere between its home slot and the first empty slot after it: it took the first
// empty slot it met, every slot it skipped was claimed by then and stays claimed, so there is no empty slot between home(v) and
// any entry of value v.  A query for v walks from home(v) to the first empty slot and therefore meets EVERY leaf of value v, in
// some order that depends on which lane won which slot.  What it computes -- the number of entries whose leaf equals v, and the
// minimum of those indices that are >= a start -- are functions of the SET of entries in the run, not of their order.  So the slot
// a leaf ends up in depends on scheduling; the answers do not.  (tests/host/leaf_index_check.cpp inserts the same leaves ascending,
// descending and shuffled and compares the answers.)
//
// Fence.  No launch both inserts and probes: a call first inserts leaves [indexed, n_leaves) in one launch on the context's
// stream and queries in a LATER launch, so a query never sees a run under construction.  The table grows by reallocation at the
// larger size and reinsertion of all leaves, again in a launch of its own.
//
// Cost of repeated values.  A query that wants the lowest occurrence satisfying a predicate (spp_wallet_sync: the first one whose
// nullifier is unspent) asks leaf_index_first, which evaluates the predicate on the occurrences in ascending order and re-probes
// the run once per step: k occurrences examined cost k predicate evaluations (a Poseidon hash and a set lookup each, there) and k
// walks of the run.  The number of occurrences is not capped; anyone can deposit copies of a commitment, and each copy makes the
// queries for THAT value longer, nobody else's beyond the slots the copies occupy.
#pragma once
#include "pool_table.hpp"

namespace spp {

static constexpr uint32_t LEAF_NONE = 0xFFFFFFFFu;             // an empty slot / "no such leaf"
static constexpr uint64_t LEAF_INDEX_MAX_LEAVES = (uint64_t)1 << 30;   // 2^31 slots of 4 B = 8 GiB for the table alone

struct LeafIndex {
  uint32_t* slots;   // mask + 1 words
  uint32_t mask;
  uint64_t salt;
};

SPP_HD uint32_t leaf_index_slots(uint64_t leaves) { return pool_slots_for(leaves < 32 ? 32 : leaves); }

// pool_slot() of the canonical big-endian encoding: the low 64 bits of that word are the two low canonical limbs
SPP_HD uint32_t leaf_home(const Fr& v, uint64_t salt, uint32_t mask) {
  uint32_t c[8];
  v.to_canonical(c);
  return (uint32_t)pool_mix64((((uint64_t)c[1] << 32) | c[0]) ^ salt) & mask;
}

// leaf i (i < the number of leaves, not yet in the table) takes the first empty slot of its run; returns the slot
SPP_HD uint32_t leaf_index_insert(const LeafIndex& ix, const Fr* leaves, uint32_t i) {
  for (uint32_t s = leaf_home(leaves[i], ix.salt, ix.mask);; s = (s + 1) & ix.mask)
    if (pool_cas(&ix.slots[s], LEAF_NONE, i) == LEAF_NONE) return s;
}

// The lowest index >= from whose leaf equals key, LEAF_NONE if there is none; *matches (optional) = how many leaves equal key in
// the whole table.  Only for launches that do not insert.
SPP_HD uint32_t leaf_index_lowest(const LeafIndex& ix, const Fr* leaves, const Fr& key, uint64_t from, uint32_t* matches) {
  uint32_t best = LEAF_NONE, n = 0;
  for (uint32_t s = leaf_home(key, ix.salt, ix.mask);; s = (s + 1) & ix.mask) {
    const uint32_t cur = ix.slots[s];
    if (cur == LEAF_NONE) break;
    if (leaves[cur] == key) {
      n++;
      if (cur >= from && cur < best) best = cur;
    }
  }
  if (matches) *matches = n;
  return best;
}

// The lowest index >= from whose leaf equals key and for which pred(index) holds, LEAF_NONE if there is none: the occurrences in
// ascending order, one re-probe per step (see the header comment).
template <class Pred>
SPP_HD uint32_t leaf_index_first(const LeafIndex& ix, const Fr* leaves, const Fr& key, uint64_t from, Pred pred) {
  for (;;) {
    const uint32_t i = leaf_index_lowest(ix, leaves, key, from, nullptr);
    if (i == LEAF_NONE || pred(i)) return i;
    from = (uint64_t)i + 1;
  }
}

}  // namespace spp
