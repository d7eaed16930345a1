// Batch verification by random linear combination on the device: `sunspot verify <vk> <proof> <pw>`
// (noir_circuit/prove_linux.sh:86-87, audit_circuit/prove_audit.sh:98-99) for many proofs against one key, behind
// spp_verify_batch_rlc.  The scheme and its one-lane reference form are csrc/verify_rlc.hpp; the wave-wide Fq12 arithmetic of the
// once-per-group tail is csrc/f12_coop.hpp.
//   k_verify_rlc_terms   one lane per proof: format / curve / subgroup checks, one dynamic-pair Miller loop, five 128-bit G1
//                        scalar multiplications, nk Fr words -> a term in the workspace (batch-minor, 28 + nk elements of 32 B).
//                        A proof that fails a check is dropped: ok[i] = 0, live[i] = 0.
//   k_verify_rlc_group   one wave per group: folds the live terms (Miller values with the cooperative product, point sums on
//                        4 x 16 lanes, Fr sums one word per lane), builds Kagg (one K base per lane, then a sum) and runs the
//                        cooperative tail.  Accept: ok[i] = 1 for the live proofs.  Refuse: their indices go to a device list
//                        that k_verify_list settles proof by proof (or ok[i] = 0 under SPP_RLC_NO_FALLBACK).
// The same two over a compacted list whose length lives in device memory (the pool ledger; index arithmetic in verify_rlc_list.hpp):
//   k_verify_rlc_terms_list   lane p of a slice: list position pos0 + p, instruction i = list[pos0 + p]; proof, public witness and
//                             scalars by i, the term and its live word at workspace position p.  ok[i] stays as the caller cleared it.
//   k_verify_rlc_group_list   block b: the positions of rlc_list_span; same fold and tail; verdicts and the fallback list by
//                             instruction index; counts its group in stats[0], the host not knowing how many there are.
#include "../../include/spp.h"
#include "kernels.hpp"
#include "verify_rlc.hpp"
#include "verify_rlc_list.hpp"
#include "f12_coop.hpp"

namespace spp {

__global__ void __launch_bounds__(64) k_verify_rlc_terms(const VerifyKeyDev* __restrict__ vkp, const uint8_t* __restrict__ proofs,
                                                         const uint8_t* __restrict__ pws, uint32_t pw_len, uint32_t count, RlcSeed seed,
                                                         uint32_t index0, W256* __restrict__ ws, uint32_t stride, uint32_t* __restrict__ live,
                                                         int32_t* __restrict__ ok, uint32_t* __restrict__ stats) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const bool good = rlc_term(*vkp, proofs + (size_t)i * 388, pws + (size_t)i * pw_len, seed.b, index0 + i, ws + i, stride);
  live[i] = good ? 1u : 0u;
  ok[i] = 0;
  if (!good) atomicAdd(&stats[3], 1u);
}

// Whole waves past the end of the list leave at their first instruction, as in k_verify_list.
__global__ void __launch_bounds__(64) k_verify_rlc_terms_list(const VerifyKeyDev* __restrict__ vkp, const uint8_t* __restrict__ proofs,
                                                              const uint8_t* __restrict__ pws, uint32_t pw_len, const uint32_t* __restrict__ list,
                                                              const uint32_t* __restrict__ n_list, RlcListSlice sl, RlcSeed seed,
                                                              W256* __restrict__ ws, uint32_t stride, uint32_t* __restrict__ live,
                                                              uint32_t* __restrict__ stats) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (!rlc_list_lane_active(sl, p, *n_list)) return;
  const uint32_t i = list[sl.pos0 + p];
  const bool good = rlc_term(*vkp, proofs + (size_t)i * 388, pws + (size_t)i * pw_len, seed.b, i, ws + p, stride);
  live[p] = good ? 1u : 0u;
  if (!good) atomicAdd(&stats[3], 1u);
}

// the wave as the executor of f12_coop.hpp's phases: this lane's share, then the barrier
struct CoopWave {
  uint32_t lane;
  template <class Fn>
  __device__ __forceinline__ void phase(Fn f) {
    f(lane);
    __syncthreads();
  }
};

struct RlcGroupShared {
  CoopShared sh;
  CoopMiller mil;
  CoopFinal fin;
  F12 acc, term;                         // the running product of the Miller values; one term's value, later f of the tail
  G1XYZZ pts[64];
  G1XYZZ kagg;
  W256 folded[RLC_E_WORDS + RLC_MAX_NK];   // the folded group as one term (verify_rlc.hpp), what both tails read
  uint32_t n_live, verdict;
};

// acc = acc * (Miller value of live term i), i uniform
__device__ __attribute__((noinline)) void rlc_fold_miller(CoopWave& x, RlcGroupShared& S, const W256* ws, uint32_t stride, const uint32_t* live,
                                                          uint32_t first, uint32_t n) {
#pragma unroll 1
  for (uint32_t i = 0; i < n; i++) {
    if (!__builtin_amdgcn_readfirstlane(live[first + i])) continue;
    x.phase([&](uint32_t lane) {
      if (lane < 12) S.term.c[lane] = w256_as<Fq>(ws[(size_t)(RLC_E_MILLER + lane) * stride + first + i]);
    });
    coop_f12_mul(x, S.sh, S.acc, S.term, S.acc);
  }
}
// the four point sums: kind = lane / 16, sixteen partial sums each, then a tree
__device__ __attribute__((noinline)) void rlc_fold_points(CoopWave& x, RlcGroupShared& S, const W256* ws, uint32_t stride, const uint32_t* live,
                                                          uint32_t first, uint32_t n) {
  x.phase([&](uint32_t lane) {
    const uint32_t kind = lane >> 4;
    G1XYZZ a = G1XYZZ::infinity();
#pragma unroll 1
    for (uint32_t i = lane & 15; i < n; i += 16) {
      if (!live[first + i]) continue;
      const G1XYZZ p = rlc_get_point(ws + first + i, stride, kind);
      g1_add_call(a, p);
    }
    S.pts[lane] = a;
  });
#pragma unroll 1
  for (uint32_t s = 8; s >= 1; s >>= 1) {
    x.phase([&](uint32_t lane) {
      if ((lane & 15) < s) g1_add_call(S.pts[lane], S.pts[lane + s]);
    });
  }
  x.phase([&](uint32_t lane) {
    if (lane < 4) rlc_put_point(S.folded, 1, lane, S.pts[16 * lane]);
  });
}
__device__ __attribute__((noinline)) void rlc_fold_words(CoopWave& x, RlcGroupShared& S, uint32_t nk, const W256* ws, uint32_t stride,
                                                         const uint32_t* live, uint32_t first, uint32_t n) {
  x.phase([&](uint32_t lane) {
    if (lane < 12) S.folded[RLC_E_MILLER + lane] = w256_of(S.acc.c[lane]);
    if (lane >= nk) return;
    Fr a = Fr::zero();
#pragma unroll 1
    for (uint32_t i = 0; i < n; i++) {
      if (!live[first + i]) continue;
      a = a + w256_as<Fr>(ws[(size_t)(RLC_E_WORDS + lane) * stride + first + i]);
    }
    S.folded[RLC_E_WORDS + lane] = w256_of(a);
  });
}
// Kagg and (sum r)(-alpha): one scalar multiplication per lane, a sum, five inversions on five lanes; then the cooperative tail
__device__ __attribute__((noinline)) bool rlc_coop_tail(CoopWave& x, RlcGroupShared& S, const VerifyKeyDev& vk, const RlcKeyDev& rk) {
  const uint32_t nk = vk.nk;
  x.phase([&](uint32_t lane) {
    if (lane <= nk) rlc_key_scalar_mul(vk, rk, S.folded, lane, S.pts[lane]);
  });
  x.phase([&](uint32_t lane) {
    if (lane != 0) return;
    G1XYZZ kagg = rlc_get_point(S.folded, 1, RLC_P_RCM);
#pragma unroll 1
    for (uint32_t k = 0; k < nk; k++) g1_add_call(kagg, S.pts[k]);
    S.kagg = kagg;
  });
  x.phase([&](uint32_t lane) {
    if (lane < 5) {
      rlc_tail_point(S.folded, S.kagg, S.pts[nk], lane, S.mil.P[lane]);
      S.mil.tab[lane] = lane < 4 ? vk.tab[lane] : rk.tab_beta;
    }
  });
  coop_miller5(x, S.sh, S.mil, S.acc, S.term);
  return coop_final_exp_is_one(x, S.sh, S.fin, S.term);
}

// One group, the block's wave: workspace positions first .. first + n - 1.  idx == nullptr: the dense batch, the proof at position
// first + i is proof first + i; else proof idx[i] (a span of the list).
template <bool LIST>
__device__ __forceinline__ void rlc_group(RlcGroupShared& S, const VerifyKeyDev& vk, const RlcKeyDev& rk, const W256* ws, uint32_t stride,
                                          const uint32_t* live, uint32_t first, uint32_t n, const uint32_t* idx, uint32_t flags, int32_t* ok,
                                          uint32_t* list, uint32_t* n_list, uint32_t* stats) {
  CoopWave x{threadIdx.x};
  x.phase([&](uint32_t lane) {
    if (lane == 0) {
      S.sh.cc = make_coop_consts(vk.pc);
      S.n_live = 0;
      if (LIST) atomicAdd(&stats[0], 1u);
    }
    if (lane < 12) S.acc.c[lane] = lane == 0 ? vk.pc.one : Fq::zero();
  });
  x.phase([&](uint32_t lane) {
    uint32_t c = 0;
    for (uint32_t i = lane; i < n; i += 64) c += live[first + i];
    if (c) atomicAdd(&S.n_live, c);
  });
  const uint32_t n_live = S.n_live;
  if (n_live == 0) return;                                        // uniform: every proof of the group was dropped
  rlc_fold_miller(x, S, ws, stride, live, first, n);
  rlc_fold_points(x, S, ws, stride, live, first, n);
  rlc_fold_words(x, S, vk.nk, ws, stride, live, first, n);
  bool accept;
  if (flags & SPP_RLC_SERIAL_TAIL) {
    x.phase([&](uint32_t lane) {
      if (lane == 0) S.verdict = rlc_final_serial(vk, rk, S.folded) ? 1u : 0u;
    });
    accept = S.verdict != 0;
  } else {
    accept = rlc_coop_tail(x, S, vk, rk);
  }
  if (accept) {
    if (LIST) {
      rlc_list_accept(idx, live + first, n, x.lane, 64, ok);
    } else {
      for (uint32_t i = x.lane; i < n; i += 64)
        if (live[first + i]) ok[first + i] = 1;
    }
    return;
  }
  if (x.lane != 0) return;                                        // refused: the rare path, one lane
  atomicAdd(&stats[1], 1u);
  if (flags & SPP_RLC_NO_FALLBACK) return;                        // ok[i] is 0 already
  atomicAdd(&stats[2], n_live);
  uint32_t at = atomicAdd(n_list, n_live);
  if (LIST) {
    rlc_list_refuse(idx, live + first, n, list, at);
  } else {
    for (uint32_t i = 0; i < n; i++)
      if (live[first + i]) list[at++] = first + i;
  }
}

__global__ void __launch_bounds__(64) k_verify_rlc_group(const VerifyKeyDev* __restrict__ vkp, const RlcKeyDev* __restrict__ rkp,
                                                         const W256* __restrict__ ws, uint32_t stride, const uint32_t* __restrict__ live,
                                                         uint32_t count, uint32_t group, uint32_t flags, int32_t* __restrict__ ok,
                                                         uint32_t* __restrict__ list, uint32_t* __restrict__ n_list, uint32_t* __restrict__ stats) {
  __shared__ RlcGroupShared S;
  const uint32_t first = blockIdx.x * group;
  if (first >= count) return;
  const uint32_t n = count - first < group ? count - first : group;
  rlc_group<false>(S, *vkp, *rkp, ws, stride, live, first, n, nullptr, flags, ok, list, n_list, stats);
}

// the early exit is block-uniform (one word, the same for every lane) and comes before the first barrier
__global__ void __launch_bounds__(64) k_verify_rlc_group_list(const VerifyKeyDev* __restrict__ vkp, const RlcKeyDev* __restrict__ rkp,
                                                              const W256* __restrict__ ws, uint32_t stride, const uint32_t* __restrict__ live,
                                                              const uint32_t* __restrict__ in_list, const uint32_t* __restrict__ n_in, RlcListSlice sl,
                                                              uint32_t group, int32_t* __restrict__ ok, uint32_t* __restrict__ list,
                                                              uint32_t* __restrict__ n_list, uint32_t* __restrict__ stats) {
  __shared__ RlcGroupShared S;
  const RlcListSpan sp = rlc_list_span(sl, blockIdx.x, group, *n_in);
  if (sp.n == 0) return;
  rlc_group<true>(S, *vkp, *rkp, ws, stride, live, sp.first - sl.pos0, sp.n, in_list + sp.first, 0, ok, list, n_list, stats);
}

void launch_verify_rlc(hipStream_t st, const VerifyKeyDev* vk, const RlcKeyDev* rk, const uint8_t* proofs, const uint8_t* pws, uint32_t pw_len,
                       uint32_t count, const RlcSeed& seed, uint32_t index0, uint32_t group, uint32_t flags, W256* ws, uint32_t* live,
                       int32_t* ok, uint32_t* list, uint32_t* n_list, uint32_t* stats) {
  if (count == 0) return;
  hipLaunchKernelGGL(k_verify_rlc_terms, dim3((count + 63) / 64), dim3(64), 0, st, vk, proofs, pws, pw_len, count, seed, index0, ws, count,
                     live, ok, stats);
  hipLaunchKernelGGL(k_verify_rlc_group, dim3((count + group - 1) / group), dim3(64), 0, st, vk, rk, ws, count, live, count, group, flags, ok,
                     list, n_list, stats);
  if (!(flags & SPP_RLC_NO_FALLBACK)) launch_verify_list(st, vk, proofs, pws, pw_len, count, list, n_list, ok);
}

void launch_verify_rlc_list(hipStream_t st, const VerifyKeyDev* vk, const RlcKeyDev* rk, const uint8_t* proofs, const uint8_t* pws, uint32_t pw_len,
                            uint32_t max_count, const uint32_t* in_list, const uint32_t* n_in, const RlcSeed& seed, uint32_t group, W256* ws,
                            uint32_t* live, int32_t* ok, uint32_t* list, uint32_t* n_list, uint32_t* stats) {
  const uint32_t slice_len = rlc_slice_len(group), stride = max_count < slice_len ? max_count : slice_len;
  for (uint32_t s = 0; s < rlc_list_slices(slice_len, max_count); s++) {
    const RlcListSlice sl = rlc_list_slice(s, slice_len, max_count);
    hipMemsetAsync(n_list, 0, sizeof(uint32_t), st);
    hipLaunchKernelGGL(k_verify_rlc_terms_list, dim3((sl.n + 63) / 64), dim3(64), 0, st, vk, proofs, pws, pw_len, in_list, n_in, sl, seed, ws,
                       stride, live, stats);
    hipLaunchKernelGGL(k_verify_rlc_group_list, dim3(rlc_list_blocks(sl.n, group)), dim3(64), 0, st, vk, rk, ws, stride, live, in_list, n_in, sl,
                       group, ok, list, n_list, stats);
    launch_verify_list(st, vk, proofs, pws, pw_len, sl.n, list, n_list, ok);
  }
}

}  // namespace spp
