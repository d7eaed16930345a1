// lanes.hpp -- cross-lane helpers of the cooperative (one wave per instance) kernels: the solver's COOP_* items and wave-wide
// batch inversion (kernels_solve.hip) and the lane-parallel Poseidon2 permutation (poseidon2.hpp).
#pragma once
#include "bn254.hpp"

namespace spp {

__device__ __forceinline__ Fr lane_get(const Fr& v, uint32_t src) {
  Fr r;
  SPP_UNROLL for (int i = 0; i < 8; i++) r.l[i] = (uint32_t)__shfl((int)v.l[i], (int)src);
  return r;
}
// the value of one FIXED lane in every lane: v_readlane_b32 (scalar path) instead of the LDS crossbar of ds_bpermute
template <int SRC>
__device__ __forceinline__ Fr lane_bcast(const Fr& v) {
  Fr r;
  SPP_UNROLL for (int i = 0; i < 8; i++) r.l[i] = (uint32_t)__builtin_amdgcn_readlane((int)v.l[i], SRC);
  return r;
}
// lane ^ 1 / lane ^ 2 inside each quad: one DPP move per word (quad_perm [1,0,3,2] = 0xB1, [2,3,0,1] = 0x4E)
template <int CTRL>
__device__ __forceinline__ Fr lane_quad(const Fr& v) {
  Fr r;
  SPP_UNROLL for (int i = 0; i < 8; i++) r.l[i] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.l[i], CTRL, 0xF, 0xF, true);
  return r;
}
__device__ __forceinline__ Fr lane_sel(bool c, const Fr& a, const Fr& b) {
  Fr r;
  SPP_UNROLL for (int i = 0; i < 8; i++) r.l[i] = c ? a.l[i] : b.l[i];
  return r;
}

}  // namespace spp
