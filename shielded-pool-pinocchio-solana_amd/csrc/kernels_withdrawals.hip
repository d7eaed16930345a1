// The withdrawal plan on the device: which notes of a batch still need an audit record (spp_withdrawal_audit_plan,
// spp_prove_withdrawals).  Everything a lane, a wave and a tile do is in csrc/withdrawal_plan.hpp, where the ordering argument is
// written down; this file is the launch shapes.
//
//   claim     256 lanes per workgroup, one key each: probe of the resident set, claim in the resolve table
//   winners   one workgroup per tile of 1024 keys (16 waves): rep(i), the tile's number of representatives
//   scan      one workgroup of 1024 lanes: exclusive scan of at most 1024 tile counts, two levels (wave, then the 16 wave totals)
//   scatter   one workgroup per tile: audit_note and pos[] of the tile's representatives, in index order
//   assign    256 lanes per workgroup: audit_of[i] = pos[rep(i)]
// Wave64 throughout (__ballot is 64 bits wide, __shfl_up runs over 64 lanes).  No workgroup waits for another: every dependence
// between workgroups crosses a kernel boundary on one stream.  32-bit atomicCAS / atomicMin on the resolve table only.
#include "kernels.hpp"
#include "withdrawal_plan.hpp"

namespace spp {

__global__ void __launch_bounds__(256) k_wplan_claim(PoolSet audits, uint32_t has_pool, uint64_t salt, uint32_t* slots, uint32_t mask,
                                                     const uint8_t* __restrict__ keys, size_t stride, uint32_t count,
                                                     uint8_t* __restrict__ resident) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  wplan_screen_claim(has_pool ? &audits : nullptr, salt, slots, mask, keys, stride, i, resident);
}

// the flags of this lane's wave as a ballot, the counts of the tile's 16 waves in LDS; every lane of the workgroup takes part
__device__ __forceinline__ uint64_t wplan_tile_ballots(bool flag, uint32_t* wave_counts) {
  const uint64_t ballot = __ballot(flag);
  if ((threadIdx.x & (WPLAN_WAVE - 1)) == 0) wave_counts[threadIdx.x / WPLAN_WAVE] = wplan_popcount(ballot);
  __syncthreads();
  return ballot;
}

__global__ void __launch_bounds__(WPLAN_TILE) k_wplan_winners(const uint32_t* __restrict__ slots, uint32_t mask, uint64_t salt,
                                                              const uint8_t* __restrict__ keys, size_t stride, uint32_t count,
                                                              const uint8_t* __restrict__ resident, uint32_t* __restrict__ rep,
                                                              uint32_t* __restrict__ tile_counts) {
  __shared__ uint32_t wave_counts[WPLAN_TILE_WAVES];
  const uint32_t i = blockIdx.x * WPLAN_TILE + threadIdx.x;
  bool flag = false;
  if (i < count) {
    const uint32_t r = wplan_rep(slots, mask, salt, keys, stride, i, resident);
    rep[i] = r;
    flag = wplan_is_representative(r, i);
  }
  wplan_tile_ballots(flag, wave_counts);
  if (threadIdx.x == 0) tile_counts[blockIdx.x] = wplan_tile_count(wave_counts);
}

// inclusive scan over the 64 lanes of a wave
__device__ __forceinline__ uint32_t wplan_wave_scan(uint32_t v, uint32_t lane) {
  for (uint32_t d = 1; d < WPLAN_WAVE; d <<= 1) v = wplan_scan_step(v, __shfl_up(v, d, WPLAN_WAVE), lane, d);
  return v;
}

__global__ void __launch_bounds__(WPLAN_MAX_TILES) k_wplan_scan(const uint32_t* __restrict__ tile_counts, uint32_t tiles,
                                                                uint32_t* __restrict__ tile_base, uint32_t* __restrict__ n_audits) {
  __shared__ uint32_t wave_total[WPLAN_TILE_WAVES];
  const uint32_t t = threadIdx.x, lane = t & (WPLAN_WAVE - 1), wave = t / WPLAN_WAVE;
  const uint32_t own = t < tiles ? tile_counts[t] : 0;
  const uint32_t incl = wplan_wave_scan(own, lane);
  if (lane == WPLAN_WAVE - 1) wave_total[wave] = incl;
  __syncthreads();
  if (wave == 0) {   // the second level: 16 wave totals, in place, exclusive
    const uint32_t w = lane < WPLAN_TILE_WAVES ? wave_total[lane] : 0;
    const uint32_t s = wplan_wave_scan(w, lane);
    if (lane < WPLAN_TILE_WAVES) wave_total[lane] = s - w;
  }
  __syncthreads();
  const uint32_t total_incl = wave_total[wave] + incl;
  if (t < tiles) tile_base[t] = total_incl - own;
  if (t == WPLAN_MAX_TILES - 1) *n_audits = total_incl;   // lanes past `tiles` add nothing: the last lane holds the sum
}

__global__ void __launch_bounds__(WPLAN_TILE) k_wplan_scatter(const uint32_t* __restrict__ rep, uint32_t count,
                                                              const uint32_t* __restrict__ tile_base, uint32_t* __restrict__ audit_note,
                                                              uint32_t* __restrict__ pos) {
  __shared__ uint32_t wave_counts[WPLAN_TILE_WAVES];
  const uint32_t i = blockIdx.x * WPLAN_TILE + threadIdx.x;
  const bool flag = i < count && wplan_is_representative(rep[i], i);
  const uint64_t ballot = wplan_tile_ballots(flag, wave_counts);
  if (!flag) return;
  const uint32_t p = tile_base[blockIdx.x] + wplan_wave_base(wave_counts, threadIdx.x / WPLAN_WAVE) +
                     wplan_rank_in_wave(ballot, threadIdx.x & (WPLAN_WAVE - 1));
  audit_note[p] = i;   // p < n_audits <= count
  pos[i] = p;
}

__global__ void __launch_bounds__(256) k_wplan_assign(const uint32_t* __restrict__ rep, const uint32_t* __restrict__ pos, uint32_t count,
                                                      uint32_t* __restrict__ audit_of) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  audit_of[i] = wplan_audit_of(rep, pos, i);
}

// count in [1, WPLAN_MAX]; slots: mask + 1 words, all POOL_NONE; rep, pos: count words; tile_counts, tile_base: WPLAN_MAX_TILES words;
// resident: count bytes; audit_of, audit_note: count words.  audits == nullptr: no pool
void launch_withdrawal_plan(hipStream_t st, const PoolSet* audits, uint64_t salt, uint32_t* slots, uint32_t mask, const uint8_t* keys, size_t stride,
                            uint32_t count, uint8_t* resident, uint32_t* rep, uint32_t* pos, uint32_t* tile_counts, uint32_t* tile_base,
                            uint32_t* audit_of, uint32_t* audit_note, uint32_t* n_audits) {
  const dim3 lanes((count + 255) / 256), tiles(wplan_tiles(count));
  hipLaunchKernelGGL(k_wplan_claim, lanes, dim3(256), 0, st, audits ? *audits : PoolSet{}, audits ? 1u : 0u, salt, slots, mask, keys, stride, count,
                     resident);
  hipLaunchKernelGGL(k_wplan_winners, tiles, dim3(WPLAN_TILE), 0, st, slots, mask, salt, keys, stride, count, resident, rep, tile_counts);
  hipLaunchKernelGGL(k_wplan_scan, dim3(1), dim3(WPLAN_MAX_TILES), 0, st, tile_counts, tiles.x, tile_base, n_audits);
  hipLaunchKernelGGL(k_wplan_scatter, tiles, dim3(WPLAN_TILE), 0, st, rep, count, tile_base, audit_note, pos);
  hipLaunchKernelGGL(k_wplan_assign, lanes, dim3(256), 0, st, rep, pos, count, audit_of);
}

}  // namespace spp
