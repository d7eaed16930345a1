// The lookup-inverse wires' share of the A and K sums, by byte bucket (the method and its constants: msm_lookup.hpp).  Batch-minor
// like every other kernel of the proving path: the proof is the fastest index of every array, 64 proofs to a wave.
//   inv    [256][P]                    Fr    INV[t] = 1 / (X - t)
//   bytes  [L][P]                      u8    looked-up value of lookup j (k_lookup_bytes, kernels_solve.hip)
//   bkt    [2][LKB_SLICES][256][P]     XYZZ  first-level buckets per set and slice; after the fold slice 0 holds Bkt_t and the
//                                            other slices are the scratch buckets of the second level ([window][LKB_BUCKETS][P])
//   dig    [LKB_WINDOWS][256][P]       i8    digits of INV[t]
//   win    [2][LKB_WINDOWS][P]         XYZZ  window sums, the pass sums k_msm_horner reads (Sg = 1, R = LKB_WINDOWS, c = LKB_C)
// All additions are the complete ones of bn254.hpp: this is about 1 % of the additions of a batch.
#include "kernels.hpp"
#include "msm_lookup.hpp"

namespace spp {

static_assert((LKB_SLICES - 1) * LKB_VALUES >= LKB_WINDOWS * LKB_BUCKETS, "the second level's buckets fit the slices the fold has freed");
static_assert(LKB_VALUES % 32 == 0, "k_lkb_inverses inverts chunks of 32");

// INV[t][p] = 1 / (X_p - t): lane -> (chunk of 32 values, proof), one inversion per chunk, the prefix products parked in the
// output.  X_p = t for some t < 256: that entry is 0 and the proof is refused (the parent path would divide by zero there as well
// whenever a lookup has the value t, and fail the satisfaction check).
__global__ void __launch_bounds__(64) k_lkb_inverses(const Fr* __restrict__ W, uint32_t challenge_wire, uint32_t P, Fr* __restrict__ inv,
                                                      uint32_t* __restrict__ status) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (LKB_VALUES / 32) * P) return;
  const uint32_t p = g % P, t0 = (g / P) * 32;
  const Fr X = W[(size_t)challenge_wire * P + p];
  Fr prod = Fr::one();
  bool bad = false;
#pragma unroll 1
  for (uint32_t k = 0; k < 32; k++) {
    Fr d = X - Fr::from_u64(t0 + k);
    if (d.is_zero()) {
      bad = true;
      d = Fr::one();
    }
    inv[(size_t)(t0 + k) * P + p] = prod;
    prod = prod * d;
  }
  Fr r = prod.inv();
#pragma unroll 1
  for (uint32_t k = 32; k-- > 0;) {
    Fr d = X - Fr::from_u64(t0 + k);
    const bool zero = d.is_zero();
    if (zero) d = Fr::one();
    const Fr pre = inv[(size_t)(t0 + k) * P + p];
    inv[(size_t)(t0 + k) * P + p] = zero ? Fr::zero() : r * pre;
    r = r * d;
  }
  if (bad) atomicOr(&status[p], 1u);
}

// First level: lane -> (slice, proof), blockIdx.y = set.  Every lane of a wave adds the same base -- entry 1 of its table row, one
// 64-byte line for the wave -- into the bucket of its own proof's byte.  The byte indexes 256 buckets whatever it is.
__global__ void __launch_bounds__(64) k_lkb_first(LkbSets s, const uint8_t* __restrict__ bytes, XYZZ<Fq>* __restrict__ bkt, uint32_t L, uint32_t P) {
  const uint32_t set = blockIdx.y;
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t sl = g / P, p = g % P;
  if (sl >= LKB_SLICES) return;
  const Affine<Fq>* __restrict__ table = s.table[set];
  const MsmBlock* __restrict__ blocks = s.blocks[set];
  const uint32_t* __restrict__ pos = s.pos[set];
  XYZZ<Fq>* mine = bkt + ((size_t)(set * LKB_SLICES + sl) * LKB_VALUES) * P + p;
#pragma unroll 1
  for (uint32_t j = sl; j < L; j += LKB_SLICES) {
    const uint32_t i = pos[j];
    if (i == MSM_ROW_ZERO) continue;   // the set has no base for this wire (uniform: j is the wave's)
    const Affine<Fq> e = table[(size_t)blocks[i >> 6].off * 64 + (i & 63)];
    const uint32_t v = bytes[(size_t)j * P + p];
    XYZZ<Fq> a = mine[(size_t)v * P];
    a.madd(e);
    mine[(size_t)v * P] = a;
  }
}
// Bkt_t = sum over the slices, left in slice 0: lane -> (value t, proof), blockIdx.y = set
__global__ void __launch_bounds__(64) k_lkb_fold(XYZZ<Fq>* __restrict__ bkt, uint32_t P) {
  const uint32_t set = blockIdx.y;
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= LKB_VALUES * P) return;
  XYZZ<Fq>* b0 = bkt + ((size_t)set * LKB_SLICES * LKB_VALUES) * P + g;
  XYZZ<Fq> a = *b0;
#pragma unroll 1
  for (uint32_t sl = 1; sl < LKB_SLICES; sl++) a.add(b0[(size_t)sl * LKB_VALUES * P]);
  *b0 = a;
}
// digits of INV[t][p]: lane -> (t, proof)
__global__ void __launch_bounds__(256) k_lkb_digits(const Fr* __restrict__ inv, int8_t* __restrict__ dig, uint32_t P) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= LKB_VALUES * P) return;
  int8_t d[LKB_WINDOWS];
  lkb_recode(inv[g], d);
  for (uint32_t j = 0; j < LKB_WINDOWS; j++) dig[(size_t)j * LKB_VALUES * P + g] = d[j];
}
// Second level: lane -> (window, proof), blockIdx.y = set.  The 16 scratch buckets of a lane live in the slices the fold freed.
__global__ void __launch_bounds__(64) k_lkb_windows(XYZZ<Fq>* __restrict__ bkt, const int8_t* __restrict__ dig, XYZZ<Fq>* __restrict__ win, uint32_t P) {
  const uint32_t set = blockIdx.y;
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= LKB_WINDOWS * P) return;
  const uint32_t w = g / P, p = g % P;
  const XYZZ<Fq>* pts = bkt + ((size_t)set * LKB_SLICES * LKB_VALUES) * P + p;
  XYZZ<Fq>* scratch = bkt + ((size_t)(set * LKB_SLICES + 1) * LKB_VALUES) * P + ((size_t)w * LKB_BUCKETS) * P + p;
  const int8_t* dg = dig + ((size_t)w * LKB_VALUES) * P + p;
  win[((size_t)set * LKB_WINDOWS) * P + g] =
      lkb_window_sum(scratch, P, [&](uint32_t t) { return (int)dg[(size_t)t * P]; }, [&](uint32_t t) { return pts[(size_t)t * P]; });
}
// out[set][p] += sum[set][p]: the lookup wires' share joins the set's table-walk sum
__global__ void __launch_bounds__(64) k_lkb_join(LkbSets s, const XYZZ<Fq>* __restrict__ sum, uint32_t P) {
  const uint32_t set = blockIdx.y;
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  XYZZ<Fq> a = s.out[set][p];
  a.add(sum[(size_t)set * P + p]);
  s.out[set][p] = a;
}

size_t lkb_bucket_elems(size_t P) { return (size_t)2 * LKB_SLICES * LKB_VALUES * P; }

void launch_lkb_inverses(hipStream_t st, const Fr* W, uint32_t challenge_wire, uint32_t P, Fr* inv, int8_t* dig, uint32_t* status) {
  hipLaunchKernelGGL(k_lkb_inverses, dim3(((LKB_VALUES / 32) * P + 63) / 64), dim3(64), 0, st, W, challenge_wire, P, inv, status);
  hipLaunchKernelGGL(k_lkb_digits, dim3((LKB_VALUES * P + 255) / 256), dim3(256), 0, st, inv, dig, P);
}
void launch_lkb_sums(hipStream_t st, const LkbSets& s, const uint8_t* bytes, const int8_t* dig, XYZZ<Fq>* bkt, XYZZ<Fq>* win, uint32_t L, uint32_t P) {
  (void)hipMemsetAsync(bkt, 0, sizeof(XYZZ<Fq>) * lkb_bucket_elems(P), st);   // ZZ = 0: every bucket the point at infinity
  hipLaunchKernelGGL(k_lkb_first, dim3((LKB_SLICES * P + 63) / 64, 2), dim3(64), 0, st, s, bytes, bkt, L, P);
  hipLaunchKernelGGL(k_lkb_fold, dim3((LKB_VALUES * P + 63) / 64, 2), dim3(64), 0, st, bkt, P);
  hipLaunchKernelGGL(k_lkb_windows, dim3((LKB_WINDOWS * P + 63) / 64, 2), dim3(64), 0, st, bkt, dig, win, P);
}
void launch_lkb_join(hipStream_t st, const LkbSets& s, const XYZZ<Fq>* sum, uint32_t P) {
  hipLaunchKernelGGL(k_lkb_join, dim3((P + 63) / 64, 2), dim3(64), 0, st, s, sum, P);
}

}  // namespace spp
