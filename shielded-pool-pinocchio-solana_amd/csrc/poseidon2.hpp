// Poseidon2 permutation (t = 4, RF = 8, RP = 56; ct_helper/src/main.nr:15-34) on the 8x32 Montgomery form, in its two device
// forms: one lane per permutation (p2_permute) and four-plus lanes of a wave per permutation (coop_p2_permute).  Both are shared
// by the solver (kernels_solve.hip: every S-box power is a witness wire) and the stand-alone sponge kernels (kernels_witness.hip:
// nothing is emitted).
#pragma once
#include "lanes.hpp"

namespace spp {

// emitter of the callers that keep no S-box powers (either form)
struct Poseidon2NoEmit {
  template <class... A>
  __device__ __forceinline__ void operator()(const A&...) const {}
};

// external matrix, rows (5,7,1,3),(4,6,1,1),(1,3,5,7),(1,1,4,6)
__device__ __forceinline__ void p2_external(Fr (&s)[4]) {
  Fr t01 = s[0] + s[1], t23 = s[2] + s[3];
  Fr d0 = s[0].dbl(), d1 = s[1].dbl(), d2 = s[2].dbl(), d3 = s[3].dbl();
  Fr q0 = d0.dbl(), q1 = d1.dbl(), q2 = d2.dbl(), q3 = d3.dbl();
  Fr n0 = q0 + s[0] + q1 + d1 + s[1] + s[2] + d3 + s[3];          // 5a+7b+c+3d
  Fr n1 = q0 + q1 + d1 + t23;                                      // 4a+6b+c+d
  Fr n2 = s[0] + d1 + s[1] + q2 + s[2] + q3 + d3 + s[3];          // a+3b+5c+7d
  Fr n3 = t01 + q2 + q3 + d3;                                      // a+b+4c+6d
  s[0] = n0; s[1] = n1; s[2] = n2; s[3] = n3;
}

// One lane per permutation, the state in registers.
// EMIT = true: x^2, x^3 = x^2 * x, x^4 = (x^2)^2, x^5 = x^4 * x of every S-box go to emit(x2, x3, x4, x5), in the order the
// circuit lays the S-boxes out (csrc/circuit.cpp sbox5); EMIT = false: x^5 only, as (x^2)^2 * x (three products).
template <bool EMIT, class Emit>
__device__ __forceinline__ void p2_permute(Fr (&s)[4], const Fr* __restrict__ rc, const Fr* __restrict__ mu, Emit emit) {
  auto sbox = [&](const Fr& x) {
    Fr x2 = x.sqr();
    if (EMIT) {
      Fr x3 = x2 * x;
      Fr x4 = x2.sqr();
      Fr x5 = x4 * x;
      emit(x2, x3, x4, x5);
      return x5;
    }
    return x2.sqr() * x;
  };
  p2_external(s);
  int k = 0;
#pragma unroll 1
  for (int r = 0; r < 4; r++) {
    SPP_UNROLL for (int i = 0; i < 4; i++) s[i] = sbox(s[i] + rc[k + i]);
    k += 4;
    p2_external(s);
  }
#pragma unroll 1
  for (int r = 0; r < 56; r++) {
    s[0] = sbox(s[0] + rc[k]);
    k++;
    Fr tot = s[0] + s[1] + s[2] + s[3];
    SPP_UNROLL for (int i = 0; i < 4; i++) s[i] = mu[i] * s[i] + tot;
  }
#pragma unroll 1
  for (int r = 0; r < 4; r++) {
    SPP_UNROLL for (int i = 0; i < 4; i++) s[i] = sbox(s[i] + rc[k + i]);
    k += 4;
    p2_external(s);
  }
}

// Lane-parallel form: lanes 0..3 hold the state, lanes 4..7 compute x^4 next to x^3 (full rounds); in a partial
// round lane 4 carries mu_0 * x alongside the S-box of lane 0, so that mu_0 * x^5 = (mu_0 * x) * x^4 is ready together with
// x^5: three dependent products per round instead of eight.  s: the state word of lanes 0..3 on entry and on return (other
// lanes: don't care).  emit(offset, x2, x3, x4, x5): called with the powers of every S-box input -- by lanes 0..3 with offset
// 16*round + 4*lane in the full rounds, by lane 0 with the running offset in the partial rounds (the solver stores them as
// witness wires; the sponge passes Poseidon2NoEmit).
template <class Emit>
__device__ __forceinline__ Fr coop_p2_permute(const Fr* __restrict__ rc, const Fr* __restrict__ mus, Fr s, uint32_t lane, Emit&& emit) {
  const uint32_t l4 = lane & 3;
  const Fr mu = mus[l4];
  auto external = [&](const Fr& mine) {   // p2_external of the state held by lanes 0..3, each lane keeping its own row
    const Fr x = lane_bcast<0>(mine), y = lane_bcast<1>(mine), z = lane_bcast<2>(mine), w = lane_bcast<3>(mine);
    const Fr t0 = x + y, t1 = z + w, t2 = y.dbl() + t1, t3 = w.dbl() + t0;
    const Fr t4 = t1.dbl().dbl() + t3, t5 = t0.dbl().dbl() + t2;
    const Fr t6 = t3 + t5, t7 = t2 + t4;
    return lane_sel(l4 < 2, lane_sel(l4 == 0, t6, t5), lane_sel(l4 == 2, t7, t4));
  };
  s = external(s);
  uint32_t k = 0, out = 0;
  auto full_round = [&]() {
    const Fr x = s + rc[k + l4];
    const Fr x2 = x * x;
    const Fr t = lane_get(x2, l4);                       // lanes 4..7: x^2 of lane - 4
    const Fr R = t * lane_sel(lane < 4, x, t);           // lanes 0..3: x^3, lanes 4..7: x^4
    const Fr x4 = lane_get(R, l4 + 4);
    const Fr x5 = x4 * x;
    if (lane < 4) emit(out + 4 * lane, x2, R, x4, x5);
    out += 16;
    k += 4;
    s = external(x5);
  };
#pragma unroll 1
  for (int r = 0; r < 4; r++) full_round();
#pragma unroll 1
  for (int r = 0; r < 56; r++) {
    const Fr x = s + rc[k];                              // lane 0
    const Fr x0 = lane_bcast<0>(x);
    const Fr R1 = lane_sel(lane == 0, x0, lane_sel(lane < 4, s, x0)) * lane_sel(lane == 0, x0, mu);
    // R1: lane 0 x^2 | lanes 1..3 mu_i * s_i | lane 4 mu_0 * x
    const Fr x2 = lane_bcast<0>(R1);
    const Fr R2 = x2 * lane_sel(lane == 0, x0, x2);      // lane 0 x^3 | lane 4 x^4
    const Fr x4 = lane_bcast<4>(R2);
    const Fr R3 = x4 * lane_sel(lane == 0, x0, R1);      // lane 0 x^5 | lane 4 mu_0 * x^5
    if (lane == 0) emit(out, R1, R2, x4, R3);
    out += 4;
    k += 1;
    const Fr val = lane_sel(lane == 0, R3, s);
    Fr tot = val + lane_quad<0xB1>(val);
    tot = tot + lane_quad<0x4E>(tot);
    const Fr m0 = lane_bcast<4>(R3);
    s = lane_sel(lane == 0, m0, R1) + tot;
  }
#pragma unroll 1
  for (int r = 0; r < 4; r++) full_round();
  return s;
}

}  // namespace spp
