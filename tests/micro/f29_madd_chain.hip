// Micro-benchmark + equality check: the chain of mixed additions of the flat table walks (XYZZ29::madd_distinct for G1,
// XYZZ29G2F::madd_distinct for G2) on register-resident operands -- no table, no gathers, no digits -- in both product forms of
// f29.hpp (F29_COLUMNS: mac + reduce, the form before product scanning; F29_SCAN) under launch bounds of 2, 3 and 4 waves per SIMD:
// 12 variants.  It ranks the forms before the walk is touched: what it leaves out is what a resident wave hides of another's gather.
//
// Every lane starts from its own point and adds the same two entries in turn (a word of the entry is mixed with the step counter,
// so that nothing of an addition is loop-invariant); the final accumulator limbs of every lane go to memory.  The program first
// checks that both forms leave the same limbs in every lane (at each occupancy), then prints one line per (group, form, occupancy):
// kernel time, additions per second over the whole chip, and cycles per addition and wave at the clock the runtime reports.
// One wave per workgroup and 4 x CUs x occupancy workgroups: one round of resident waves, as the walks are planned -- the launch bound
// sets the register budget, the size of the grid the number of waves a SIMD holds.
// Build (the flags of the translation unit to be ranked; SCHED empty or "-mllvm -amdgpu-sched-strategy=max-ilp"):
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off $SCHED -I../../shielded-pool-pinocchio-solana_amd/csrc f29_madd_chain.hip -o f29_madd_chain
// Run: ./f29_madd_chain [steps = 2000] [repeats = 3]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "f29.hpp"

using namespace spp;

#define CK(x)                                                                         \
  do {                                                                                \
    hipError_t e_ = (x);                                                              \
    if (e_ != hipSuccess) {                                                           \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_));      \
      exit(2);                                                                        \
    }                                                                                 \
  } while (0)

// words of a lane's operands: below 2^253 (top word < 2^29), so every one is a value < p whatever the other words are
__device__ __forceinline__ uint32_t mix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
__device__ __forceinline__ Fq words(uint32_t seed) {
  Fq r;
  SPP_UNROLL for (int i = 0; i < 8; i++) r.l[i] = mix(seed * 8u + (uint32_t)i);
  r.l[7] &= (1u << 29) - 1u;
  return r;
}

// the entry of a step, chosen word by word (an array indexed by the step would live in scratch memory)
__device__ __forceinline__ Fq pick(const Fq& a, const Fq& b, uint32_t second) {
  Fq r;
  SPP_UNROLL for (int i = 0; i < 8; i++) r.l[i] = second ? b.l[i] : a.l[i];
  return r;
}

template <int FORM, int WAVES>
__global__ void __launch_bounds__(64, WAVES) k_chain_g1(uint32_t* __restrict__ out, uint32_t steps, uint32_t* __restrict__ refused) {
  const uint32_t g = blockIdx.x * 64 + threadIdx.x;
  XYZZ29<FqParams, FORM> acc = XYZZ29<FqParams, FORM>::infinity();
  const Affine<Fq> e0 = {words(4 * g), words(4 * g + 1)}, e1 = {words(4 * g + 2), words(4 * g + 3)};
  acc.madd_distinct(e0, false);   // the accumulator leaves infinity
#pragma unroll 1
  for (uint32_t s = 0; s < steps; s++) {
    Affine<Fq> t;
    t.x = pick(e1.x, e0.x, s & 1);   // step 0 adds e1: the accumulator holds e0
    t.y = pick(e1.y, e0.y, s & 1);
    t.x.l[0] ^= s;
    t.y.l[1] ^= s;
    if (!acc.madd_distinct(t, (s & 2) != 0)) atomicAdd(refused, 1u);
  }
  uint32_t* o = out + (size_t)g * 36;
  SPP_UNROLL for (int i = 0; i < 9; i++) {
    o[i] = acc.X.l[i];
    o[9 + i] = acc.Y.l[i];
    o[18 + i] = acc.ZZ.l[i];
    o[27 + i] = acc.ZZZ.l[i];
  }
}
template <int FORM, int WAVES>
__global__ void __launch_bounds__(64, WAVES) k_chain_g2(uint32_t* __restrict__ out, uint32_t steps, uint32_t* __restrict__ refused) {
  const uint32_t g = blockIdx.x * 64 + threadIdx.x;
  XYZZ29G2F<FORM> acc = XYZZ29G2F<FORM>::infinity();
  const Affine<Fq2> e0 = {{words(8 * g), words(8 * g + 1)}, {words(8 * g + 2), words(8 * g + 3)}},
                    e1 = {{words(8 * g + 4), words(8 * g + 5)}, {words(8 * g + 6), words(8 * g + 7)}};
  acc.madd_distinct(e0, false);
#pragma unroll 1
  for (uint32_t s = 0; s < steps; s++) {
    Affine<Fq2> t;
    t.x = {pick(e1.x.c0, e0.x.c0, s & 1), pick(e1.x.c1, e0.x.c1, s & 1)};
    t.y = {pick(e1.y.c0, e0.y.c0, s & 1), pick(e1.y.c1, e0.y.c1, s & 1)};
    t.x.c0.l[0] ^= s;
    t.y.c1.l[1] ^= s;
    if (!acc.madd_distinct(t, (s & 2) != 0)) atomicAdd(refused, 1u);
  }
  uint32_t* o = out + (size_t)g * 72;
  const F29<FqParams>* c[8] = {&acc.X.c0, &acc.X.c1, &acc.Y.c0, &acc.Y.c1, &acc.ZZ.c0, &acc.ZZ.c1, &acc.ZZZ.c0, &acc.ZZZ.c1};
  SPP_UNROLL for (int k = 0; k < 8; k++) {
    SPP_UNROLL for (int i = 0; i < 9; i++) o[9 * k + i] = c[k]->l[i];
  }
}

typedef void (*Kern)(uint32_t*, uint32_t, uint32_t*);
struct Variant {
  const char* group;
  int form, waves;
  Kern k;
  uint32_t words_per_lane;
};
static const char* form_name(int f) {
  static const char* n[2] = {"columns", "scan"};
  return n[f];
}
#define G1(F, W) {"g1", F, W, k_chain_g1<F, W>, 36}
#define G2(F, W) {"g2", F, W, k_chain_g2<F, W>, 72}
static const Variant variants[] = {
    G1(0, 2), G1(1, 2), G1(0, 3), G1(1, 3), G1(0, 4), G1(1, 4),
    G2(0, 2), G2(1, 2), G2(0, 3), G2(1, 3), G2(0, 4), G2(1, 4),
};

int main(int argc, char** argv) {
  const uint32_t steps = argc > 1 ? (uint32_t)atoi(argv[1]) : 2000u;
  const int repeats = argc > 2 ? atoi(argv[2]) : 3;
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, 0));
  const double mhz = prop.clockRate / 1000.0;
  const uint32_t simds = (uint32_t)prop.multiProcessorCount * 4u;
  const size_t max_words = (size_t)simds * 4 * 64 * 72;
  uint32_t *d_out, *d_refused;
  CK(hipMalloc(&d_out, max_words * 4));
  CK(hipMalloc(&d_refused, 4));
  hipEvent_t ev0, ev1;
  CK(hipEventCreate(&ev0));
  CK(hipEventCreate(&ev1));
  printf("device %s, %d CUs, %.0f MHz, %u additions per lane, best of %d\n", prop.name, prop.multiProcessorCount, mhz, steps, repeats);

  // 1. equal limbs: the scanning form against the column form, over the lanes both launches have
  int bad = 0;
  std::vector<uint32_t> ref, got;
  for (const Variant& v : variants) {
    const uint32_t blocks = simds * (uint32_t)v.waves;
    const size_t n = (size_t)blocks * 64 * v.words_per_lane;
    uint32_t refused = 0;
    CK(hipMemset(d_refused, 0, 4));
    hipLaunchKernelGGL(v.k, dim3(blocks), dim3(64), 0, 0, d_out, 64u, d_refused);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(&refused, d_refused, 4, hipMemcpyDeviceToHost));
    got.resize(n);
    CK(hipMemcpy(got.data(), d_out, n * 4, hipMemcpyDeviceToHost));
    if (v.form == 0 && v.waves == 2) ref = got;   // the launch with the fewest lanes comes first in its group
    const size_t cmp_n = std::min(ref.size(), got.size());
    const bool same = memcmp(ref.data(), got.data(), cmp_n * 4) == 0;
    if (!same || refused) {
      bad++;
      printf("MISMATCH %s %s waves %d: limbs %s, %u additions refused\n", v.group, form_name(v.form), v.waves, same ? "equal" : "differ", refused);
    }
  }
  if (bad) {
    printf("equal limbs: FAILED (%d variants)\n", bad);
    return 1;
  }
  printf("equal limbs: all %zu variants leave the limbs of the column form in every lane (64 additions)\n", sizeof(variants) / sizeof(variants[0]));

  // 2. timing
  for (const Variant& v : variants) {
    const uint32_t blocks = simds * (uint32_t)v.waves;
    float best = 1e30f;
    for (int r = 0; r < repeats + 1; r++) {   // the first run warms up
      CK(hipEventRecord(ev0, 0));
      hipLaunchKernelGGL(v.k, dim3(blocks), dim3(64), 0, 0, d_out, steps, d_refused);
      CK(hipEventRecord(ev1, 0));
      CK(hipEventSynchronize(ev1));
      float ms;
      CK(hipEventElapsedTime(&ms, ev0, ev1));
      if (r > 0) best = std::min(best, ms);
    }
    const double adds = (double)blocks * 64 * steps;
    // a SIMD runs `waves` chains of `steps` additions in `best` ms
    const double cyc = best * 1e-3 * mhz * 1e6 / ((double)steps * v.waves);
    printf("%s %-11s waves/SIMD %d : %8.3f ms  %7.2f G additions/s  %7.0f cycles per addition and wave\n", v.group, form_name(v.form), v.waves, best,
           adds / (best * 1e-3) / 1e9, cyc);
  }
  return 0;
}
