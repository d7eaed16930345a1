// The walk of a deposit row, host + gfx950: what k_deposit_rows (kernels_witness.hip) does per lane once it has the commitment,
// and what tests/host/deposit_rows_check.cpp runs on the host against big-integer vectors.
//
// Setting (merkle_prefix.hpp has the tree's invariants).  Leaf i of an append-only tree of m > i leaves.  The deposit circuit
// (circuit_deposit.cpp) states: slot i was empty under old_root, holds the commitment under new_root, and the siblings of the two
// paths are the same.  Those are the paths of slot i in the trees of the first i and the first i + 1 leaves.  At level l with
// p = i >> l the sibling of the path node is
//   p odd    (l, p - 1), to the left: its leaves are [(p-1) 2^l, p 2^l), all below i, so the node was final before leaf i came and
//            is the same in both trees and in the tree as it stands: level[l][p - 1], a read at p - 1 < cnt_l(i + 1) <= cnt_l(m);
//   p even   (l, p + 1), to the right: its leaves are all above i, none of them in either tree: dflt[l].
// This is the walk of k_deposit_roots (DESIGN, "Deposits from secrets") done twice over one set of siblings: from `empty` -- the
// default leaf, client/merkle.ts:152 -- it ends in the root of size i, from the commitment in the root of size i + 1.  Nothing
// stored at or to the right of the path is read, so the result does not depend on m, nor on whether the stored leaf i is the
// commitment passed in: a commitment that is not the tree's leaf gives a new_root that is not the tree's (what the chain check of
// spp_verify_deposit_chain is for).
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
#define SPP_DEPOSIT_ROLLED _Pragma("unroll 1")   // one call site of the hash per kernel (see k_withdraw_rows on why that matters)
#else
#define SPP_DEPOSIT_ROLLED
#endif

namespace spp {

static constexpr uint32_t DEPOSIT_ROW_FIXED = 8;   // old_root | new_root | commitment | amount | index | owner_x | owner_y | randomness

// level(l): the stored array of level l; i < the number of leaves stored, i < 2^depth.  sibling(l, node) receives the sibling of
// every level in order; roots[0] = old_root, roots[1] = new_root.
template <class Node, class Levels, class Hash, class Sibling>
SPP_HD void deposit_walk(uint64_t i, uint32_t depth, Levels level, const Node* dflt, const Node& empty, const Node& commitment, Hash H,
                         Sibling sibling, Node roots[2]) {
  Node v0 = empty, v1 = commitment;
  SPP_DEPOSIT_ROLLED
  for (uint32_t l = 0; l < depth; l++) {
    const uint64_t p = i >> l;
    const bool odd = p & 1;
    const Node sib = odd ? level(l)[p - 1] : dflt[l];
    sibling(l, sib);
    SPP_DEPOSIT_ROLLED
    for (int k = 0; k < 2; k++) {
      const Node cur = k ? v1 : v0;
      const Node h = H(odd ? sib : cur, odd ? cur : sib);
      if (k) v1 = h; else v0 = h;
    }
  }
  roots[0] = v0;
  roots[1] = v1;
}

}  // namespace spp
