// The random-linear-combination verifier (verify_rlc.hpp) over a COMPACTED LIST, host + gfx950: the index arithmetic of
// k_verify_rlc_terms_list / k_verify_rlc_group_list (kernels_verify_rlc.hip), as plain functions that a host build runs lane after
// lane (tests/host/verify_rlc_list_check.cpp).  The pool ledger's screen kernels leave the instruction indices that need a proof
// verified in list[0 .. *n_list), in the arbitrary order of their atomicAdd, and the length only in device memory.
//
//   position j of the list  <->  instruction i = list[j]
//   - proof, public witness, verdict ok[i] and the scalars (r_i, s_i) go by the INSTRUCTION index i: the weights of a proof do not
//     depend on where the scheduling of the screen kernel happened to put it;
//   - the term, its live word and the membership of a group go by the POSITION j: the workspace is as dense as the list, and the
//     fold routines of the dense kernels read it unchanged.
// A call is cut into slices of list positions (RlcListSlice: at most 2^18, a multiple of the group), which bounds the workspace; a
// slice's workspace position is j - pos0.  The host knows only max_count >= *n_list and launches for it: lanes and blocks past the
// end of the list leave at once.
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

namespace spp {

static constexpr uint32_t RLC_SLICE_MAX = 1u << 18;       // proofs (dense) or list positions per slice at most: ~1.1 KB of workspace each

struct RlcListSlice {
  uint32_t pos0, n;                                       // list positions pos0 .. pos0 + n - 1 (as far as the list goes)
};
// positions per slice for this group size: the largest multiple of `group` within `slice_max` (group <= slice_max)
SPP_HD uint32_t rlc_slice_len(uint32_t group, uint32_t slice_max = RLC_SLICE_MAX) { return slice_max / group * group; }
// slice s of a list of at most max_count positions; n == 0: past the end
SPP_HD RlcListSlice rlc_list_slice(uint32_t s, uint32_t slice_len, uint32_t max_count) {
  const uint64_t pos0 = (uint64_t)s * slice_len;
  if (pos0 >= max_count) return {max_count, 0};
  const uint32_t left = max_count - (uint32_t)pos0;
  return {(uint32_t)pos0, left < slice_len ? left : slice_len};
}
SPP_HD uint32_t rlc_list_slices(uint32_t slice_len, uint32_t max_count) { return (max_count + slice_len - 1) / slice_len; }
SPP_HD uint32_t rlc_list_blocks(uint32_t n, uint32_t group) { return (n + group - 1) / group; }   // the grid of a slice: the worst case

// terms: lane p of a slice's launch owns workspace position p and list position pos0 + p -- if the list gets that far
SPP_HD bool rlc_list_lane_active(const RlcListSlice& sl, uint32_t p, uint32_t n_list) { return p < sl.n && sl.pos0 + p < n_list; }

// groups: block b of a slice's launch covers list positions first .. first + n - 1, workspace positions first - pos0 ...;
// n == 0: the block is past the end of the list (or of the slice) and has nothing to do
struct RlcListSpan {
  uint32_t first, n;
};
SPP_HD RlcListSpan rlc_list_span(const RlcListSlice& sl, uint32_t b, uint32_t group, uint32_t n_list) {
  const uint64_t first = (uint64_t)sl.pos0 + (uint64_t)b * group;
  uint32_t end = sl.pos0 + sl.n;
  if (n_list < end) end = n_list;
  if (first >= end) return {end, 0};
  const uint32_t left = end - (uint32_t)first;
  return {(uint32_t)first, left < group ? left : group};
}

// an accepted group: lane `lane` of `lanes` gives the live positions it strides over their verdict, ok[list[j]] = 1.
// live_at: the live words of the span (workspace positions), idx: list + span.first
SPP_HD void rlc_list_accept(const uint32_t* idx, const uint32_t* live_at, uint32_t n, uint32_t lane, uint32_t lanes, int32_t* ok) {
  for (uint32_t i = lane; i < n; i += lanes)
    if (live_at[i]) ok[idx[i]] = 1;
}
// a refused group, one lane: the INSTRUCTION indices of its live positions into out[at ...], `at` reserved by the caller
// (atomicAdd of the live count on the device); returns the position behind the last one written
SPP_HD uint32_t rlc_list_refuse(const uint32_t* idx, const uint32_t* live_at, uint32_t n, uint32_t* out, uint32_t at) {
  for (uint32_t i = 0; i < n; i++)
    if (live_at[i]) out[at++] = idx[i];
  return at;
}

}  // namespace spp
