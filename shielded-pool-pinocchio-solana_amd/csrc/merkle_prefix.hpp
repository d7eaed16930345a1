// The resident Merkle tree as of an earlier size, host + gfx950: which node of the tree of the first n leaves is which node of
// the tree as it stands.  The per-lane pieces of k_merkle_frontier, k_prefix_roots and the as-of forms of k_merkle_gather and
// k_withdraw_rows (kernels_witness.hip), and of the host check tests/host/merkle_prefix_check.cpp, which runs them with a toy hash.
// What it is for: the pool program pushes whatever root a deposit carries (shielded_pool_program/src/instructions/deposit.rs:31-36,
// :73; client/payroll-demo.ts:285-292 computes it locally per deposit), so the root the chain accepts is often the root of an EARLIER
// size of the leaf list than the one a prover service holds (demo-frontend/app/lib/on-chain.ts:93-125,202-235 asks the same question
// from the wallet's side).
//
// Setting.  The tree is append-only (client/merkle.ts:158-163): leaf i never changes once written, level[l][s] = H(level[l-1][2s],
// level[l-1][2s+1]) covers leaves [s 2^l, (s+1) 2^l), a child that does not exist counts as dflt[l-1] (merkle.ts:150-156), and level l
// of a tree of m leaves stores cnt_l(m) = 0 for m = 0, else ((m-1) >> l) + 1 nodes.  The prefix tree of size n <= m is the tree a
// fresh ShieldedPoolMerkleTree holds after leaves 0..n-1.
//
// The three cases.  Node (l, s) of the prefix tree of size n:
//   s >= cnt_l(n)       none of its leaves is below n: an empty subtree, dflt[l].
//   s <  cnt_l(n) - 1   (s+1) 2^l <= ((n-1) >> l) 2^l <= n-1: every leaf of the subtree is below n.  The stored node was computed
//                       from exactly those leaves when the last of them arrived; no later append reaches the subtree, so the
//                       stored value is the prefix tree's and is final: level[l][s].
//   s == cnt_l(n) - 1   the one node of the level whose subtree holds leaf n-1, the only one that can hold leaves on both sides of
//                       n.  Its stored value mixes in leaves >= n; the prefix tree's value is F[l], the frontier.
// So one node per level differs from what is stored, and everything else is a read.
//
// The frontier.  F[0] = leaf n-1.  With p = (n-1) >> l the position of the frontier node of level l, its parent is the frontier
// node of level l+1, and its sibling is
//   p odd    (l, p-1), to the left: p-1 < cnt_l(n) - 1, the second case, so stored and final:   F[l+1] = H(level[l][p-1], F[l])
//   p even   (l, p+1), to the right: p+1 >= cnt_l(n), the first case:                           F[l+1] = H(F[l], dflt[l])
// The root of the prefix tree is F[depth].  For n = 0 there is no frontier node; F[l] = dflt[l] is written so that the root is
// F[depth] for every n (no node selects the frontier then: cnt_l(0) = 0).  This is the walk of k_deposit_roots for leaf n-1.
//
// What follows from it.  A prefix root, sibling or frontier value of size n reads leaves and stored nodes of the second case only:
// values that were final when leaf n-1 was written.  So an as-of answer does not depend on leaves appended before or after the
// question, as long as n <= the size of the tree when it is asked; and R[n], the root of size n, never changes once computed.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef SPP_HD
#if defined(__HIPCC__)
#define SPP_HD __host__ __device__ __forceinline__
#else
#define SPP_HD inline
#endif
#endif
#if defined(__HIPCC__)
#define SPP_PREFIX_ROLLED _Pragma("unroll 1")   // one call site of the hash per kernel (see k_withdraw_rows on why that matters)
#else
#define SPP_PREFIX_ROLLED
#endif

namespace spp {

static constexpr uint32_t PREFIX_DEFAULT = 0, PREFIX_FRONTIER = 1, PREFIX_STORED = 2;

// nodes of level l in the tree of n leaves
SPP_HD uint64_t prefix_count(uint64_t n, uint32_t l) { return n == 0 ? 0 : ((n - 1) >> l) + 1; }

// which of the three cases node (l, s) of the prefix tree of size n is
SPP_HD uint32_t prefix_case(uint64_t n, uint32_t l, uint64_t s) {
  const uint64_t cnt = prefix_count(n, l);
  return s >= cnt ? PREFIX_DEFAULT : s + 1 == cnt ? PREFIX_FRONTIER : PREFIX_STORED;
}

// the value of node (l, s) of the prefix tree of size n.  level_l is read in the stored case only, at s < cnt_l(n) - 1
template <class Node>
SPP_HD Node prefix_node(uint64_t n, uint32_t l, uint64_t s, const Node* level_l, const Node* dflt, const Node* frontier) {
  const uint32_t c = prefix_case(n, l, s);
  return c == PREFIX_STORED ? level_l[s] : c == PREFIX_FRONTIER ? frontier[l] : dflt[l];
}

// one step of the recurrence: F[l+1] from v = F[l] (n >= 1).  level_l is read when (n-1) >> l is odd, at the position to its left
template <class Node, class Hash>
SPP_HD Node prefix_frontier_step(uint64_t n, uint32_t l, const Node* level_l, const Node* dflt, const Node& v, Hash H) {
  const uint64_t p = (n - 1) >> l;
  const bool odd = p & 1;
  return H(odd ? level_l[p - 1] : v, odd ? v : dflt[l]);
}

// The whole walk: returns the root of the prefix tree of size n and, when F is not NULL, writes F[0..depth].  level(l) gives the
// stored array of level l; n <= the number of leaves stored.
template <class Node, class Levels, class Hash>
SPP_HD Node prefix_walk(uint64_t n, uint32_t depth, Levels level, const Node* dflt, Hash H, Node* F) {
  if (n == 0) {
    if (F)
      for (uint32_t l = 0; l <= depth; l++) F[l] = dflt[l];
    return dflt[depth];
  }
  Node v = level(0)[n - 1];
  if (F) F[0] = v;
  SPP_PREFIX_ROLLED
  for (uint32_t l = 0; l < depth; l++) {
    v = prefix_frontier_step(n, l, level(l), dflt, v, H);
    if (F) F[l + 1] = v;
  }
  return v;
}

}  // namespace spp
