// Ragged tables of the flat table walk (msm_table.hpp): range classes of the bases, the table layout whose 64-row blocks differ in
// length, and the split of the HBM budget over the window bits of the sets.  Host side, standard library only, like msm_plan.hpp:
// any host compiler builds it (tests/host/msm_ragged_check.cpp).
//
// Why: a base whose scalar is a bit or a byte only ever has a digit in window 0, of magnitude <= 1 or <= 255.  With one row of
// 2^(c-1) multiples for every base, 7 226 of the audit circuit's A bases and as many of its B bases kept 2 MB (G1) / 4 MB (G2)
// rows of which the walk reads entry 1, or entries 1 .. 255: 61.5 GB of the 240 GB budget.  Sized by their range those rows take
// 0.1 GB, and the budget holds 16-bit windows for all five flat sets.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "msm_plan.hpp"

namespace spp {

// ---- range classes ---------------------------------------------------------------------------------
// A class is a bound on |signed value| of the scalar (the value folded to (-p/2, p/2]); 0 = wide (no bound).

// The one spelling of "byte-ranged": a looked-up value of an OP_COUNT8 range check that is exactly one wire (coefficient 1) plus a
// small constant cst.  The log-derivative argument then holds only if the wire's value lies in [-cst, 255 - cst].  `small(coeff,
// &v)` tells whether a coefficient-table entry is a small signed integer.  Used by the small rows of the matrix evaluation
// (spp_plan.cpp) and by the range classes below.
template <class TermIt, class SmallOf>
inline bool byte_ranged_lookup(TermIt begin, TermIt end, SmallOf small, uint32_t* wire, int64_t* cst_out) {
  uint32_t w = 0, nw = 0;
  int64_t cst = 0;
  for (TermIt t = begin; t != end; ++t) {
    int64_t v;
    if (!small(t->coeff, &v)) return false;
    if (t->wire == 0) cst += v;
    else if (v == 1) { w = t->wire; nw++; }
    else return false;
  }
  if (nw != 1 || cst < -32000 || cst > 32000) return false;
  *wire = w;
  *cst_out = cst;
  return true;
}
// bound of a wire whose value plus cst is a byte: values in [-cst, 255 - cst]
inline uint32_t byte_ranged_bound(int64_t cst) {
  const int64_t lo = cst < 0 ? -cst : cst, hi = 255 - cst < 0 ? cst - 255 : 255 - cst;
  return (uint32_t)std::max<int64_t>(std::max(lo, hi), 1);
}
// a wire may be classified twice (a byte limb that is also looked up): the tighter bound holds
inline void narrow_wire(std::vector<uint32_t>& bound, uint32_t wire, uint32_t b) {
  if (wire == 0 || wire >= bound.size()) return;   // wire 0 is the constant one: its bases carry alpha / beta, wide
  if (bound[wire] == 0 || b < bound[wire]) bound[wire] = b;
}

// ---- layout ----------------------------------------------------------------------------------------
// Block b (rows 64 b .. 64 b + 63) has E_b entries per row and starts `off` units of 64 points into the table: entry d of row `row`
// lives at (off_{row/64} + d) * 64 + row % 64.  With E_b = 2^(c-1) for every block this is the uniform layout
// ((row/64) * E + d) * 64 + row % 64 bit for bit.
struct MsmBlock {
  uint64_t off;    // start of the block, in units of 64 points
  uint32_t E;      // entries per row of this block (a power of two <= 2^(c-1)): the walk adds nothing for a digit above it
  uint32_t pad_;
};
// entries a row needs for scalars of class `bound` at c-bit windows: a power of two >= bound, the full 2^(c-1) for wide ones
inline uint32_t msm_class_entries(uint32_t bound, uint32_t c) {
  const uint32_t full = 1u << (c - 1);
  if (bound == 0 || bound >= full) return full;
  uint32_t e = 1;
  while (e < bound) e <<= 1;
  return e;
}
struct MsmRagged {
  std::vector<MsmBlock> blocks;
  uint64_t units = 0;                       // total length in units of 64 points
  size_t elems() const { return (size_t)units * 64; }
  size_t index(size_t row, uint32_t d) const { return (size_t)(blocks[row >> 6].off + d) * 64 + (row & 63); }
  bool narrow(uint32_t c) const {           // any block shorter than the full row
    for (const MsmBlock& b : blocks) if (b.E != (1u << (c - 1))) return true;
    return false;
  }
};
// bound[i]: class of row i (one row per base: the flat layout).  A block is as long as its longest row.
inline MsmRagged msm_ragged_layout(const uint32_t* bound, size_t N, uint32_t c) {
  MsmRagged L;
  const size_t nb = (N + 63) / 64;
  L.blocks.resize(nb);
  for (size_t b = 0; b < nb; b++) {
    uint32_t E = 1;
    for (size_t r = b * 64; r < std::min(N, b * 64 + 64); r++) E = std::max(E, msm_class_entries(bound[r], c));
    L.blocks[b] = {L.units, E, 0};
    L.units += E;
  }
  return L;
}
// Class-major order of the bases of a flat set, stable within a class, longest rows first: blocks become homogeneous (at most one
// mixed block per class boundary), and an all-wide set keeps its order.  perm[k] = old index of the base at new position k.
inline std::vector<uint32_t> msm_class_major_order(const uint32_t* bound, size_t N, uint32_t c) {
  std::vector<uint32_t> perm(N);
  std::iota(perm.begin(), perm.end(), 0u);
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return msm_class_entries(bound[a], c) > msm_class_entries(bound[b], c); });
  return perm;
}

// ---- the HBM budget over the window bits of the sets -----------------------------------------------
// Greedy split of an HBM budget over the throughput-layout (one table row per base) MSM sets of one OR SEVERAL circuits: start
// every set at 6 bits and repeatedly widen the set whose next window bit removes the most mixed-addition work per extra byte
// (a G2 addition is weighted 3 G1 additions, as measured); `fixed` sets keep their bits.  With several circuits the unit of work
// is one proof of each (the relayer's pair: an audit proof and a withdraw proof per withdrawal), so their sets simply compete in
// one list.  A bit costs what it really costs: only the wide bases of a flat set double their rows, and only they lose a window;
// the narrow ones keep min(class entries, 2^(c-1)).
struct PlanSet {
  double n, esz, wgt;   // bases, bytes per table entry, weight of an addition (0: fixed)
  bool flat;            // one row per base (else one row per window)
  int bits;
  double narrow[3] = {0, 0, 0};   // of the n bases of a flat set: how many have rows of 1, 128 and 256 entries (PLAN_NARROW_E)
};
static constexpr double PLAN_NARROW_E[3] = {1, 128, 256};
inline double plan_wide(const PlanSet& s) { return s.flat ? s.n - s.narrow[0] - s.narrow[1] - s.narrow[2] : s.n; }
inline double plan_bytes(const PlanSet& s, int cb) {
  const double full = (double)(1u << (cb - 1));
  if (!s.flat) return s.n * s.esz * (double)msm_windows((uint32_t)cb) * full;
  double rows = plan_wide(s) * full;
  for (int k = 0; k < 3; k++) rows += s.narrow[k] * std::min(PLAN_NARROW_E[k], full);
  return rows * s.esz;
}
inline void plan_greedy(std::vector<PlanSet>& sets, double budget, int cmax) {
  double used = 0;
  for (auto& s : sets) used += plan_bytes(s, s.bits);
  for (;;) {
    int best = -1;
    double best_gain = 0;
    for (size_t i = 0; i < sets.size(); i++) {
      const PlanSet& s = sets[i];
      if (s.wgt == 0 || s.bits >= cmax || s.n == 0) continue;
      const double extra = plan_bytes(s, s.bits + 1) - plan_bytes(s, s.bits);
      if (used + extra > budget) continue;
      const double saved = s.wgt * plan_wide(s) * ((double)msm_windows((uint32_t)s.bits) - (double)msm_windows((uint32_t)s.bits + 1));
      double gain = saved / extra;
      if (saved <= 0) gain = 1e-30;   // a bit that does not change the window count yet may enable the next one
      if (gain > best_gain) { best_gain = gain; best = (int)i; }
    }
    if (best < 0) break;
    used += plan_bytes(sets[best], sets[best].bits + 1) - plan_bytes(sets[best], sets[best].bits);
    sets[best].bits++;
  }
}
static constexpr double PLAN_ESZ[7] = {64, 64, 64, 64, 64, 64, 128}, PLAN_WGT[7] = {1, 1, 1, 1, 0, 0, 3.0};   // A, B1, K, Z, CB, CS, B2
// the set of index s (order above) with `n` bases at its starting bits
inline PlanSet plan_set(int s, double n, bool flat) { return {n, PLAN_ESZ[s], PLAN_WGT[s], flat, PLAN_WGT[s] != 0 ? 6 : 9}; }
// count a base of class `bound` (0: wide) into the narrow rows of a flat set; bounds above 256 stay wide
inline void plan_count(PlanSet& s, uint32_t bound) {
  if (bound == 0 || bound > 256) return;
  s.narrow[bound <= 1 ? 0 : bound <= 128 ? 1 : 2] += 1;
}

}  // namespace spp
