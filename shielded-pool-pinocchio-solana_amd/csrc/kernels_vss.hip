// The kernels of the verifiable sharing of the auditors' key (vss.hpp has the method): the window table of the two generators, the
// commitments of a dealing, the receiver's check and the sum of the accepted sub-shares.  One lane per point, one wave per
// workgroup, as kernels_ptau.hip: a dealing of the key at the largest threshold is 64 * 1024 commitments = 1 024 waves, one per SIMD.
#include "kernels.hpp"
#include "vss.hpp"

namespace spp {

// table[i] = (i % 255 + 1) * wbases[i / 255]: once per context
__global__ void __launch_bounds__(64) k_vss_table(const G1Affine* __restrict__ wbases, G1Affine* __restrict__ table) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= VSS_TABLE_POINTS) return;
  table[i] = vss_table_entry(wbases, i);
}

// commitments[(k n + v) 64 ..] = c_k[v] G + c'_k[v] H for lane k n + v < t n; c_0 = secrets, c_k = coeffs[(k - 1) n + v], the blinds alike
__global__ void __launch_bounds__(64) k_vss_commit(const G1Affine* __restrict__ table, const uint8_t* __restrict__ secrets_be,
                                                   const uint8_t* __restrict__ coeffs_be, const uint8_t* __restrict__ blinds_be,
                                                   const uint8_t* __restrict__ coeffs_blind_be, uint32_t n, uint32_t count,
                                                   uint8_t* __restrict__ commitments) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;   // count = t n
  const uint8_t* c = i < n ? secrets_be + (size_t)32 * i : coeffs_be + (size_t)32 * (i - n);
  const uint8_t* cb = i < n ? blinds_be + (size_t)32 * i : coeffs_blind_be + (size_t)32 * (i - n);
  vss_store_point(vss_commit(table, c, cb), commitments + (size_t)64 * i);
}

// flags[d n + v] = vss_check_value of dealer d's value v for the receiver at x; zero_blinds (optional): dealers * n * 32 B
__global__ void __launch_bounds__(64) k_vss_check(const G1Affine* __restrict__ table, uint32_t t, uint32_t x, uint32_t dealers, uint32_t n,
                                                  const uint8_t* __restrict__ commitments, const uint8_t* __restrict__ ys_be,
                                                  const uint8_t* __restrict__ ys_blind_be, const uint8_t* __restrict__ zero_blinds_be,
                                                  uint32_t* __restrict__ flags) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;   // dealers n <= 255 * 2^20
  if (g >= dealers * n) return;
  const uint32_t d = g / n, v = g % n;
  flags[g] = vss_check_value(table, t, x, commitments + ((size_t)d * t * n + v) * 64, (size_t)n * 64, ys_be + (size_t)32 * g,
                             ys_blind_be + (size_t)32 * g, zero_blinds_be ? zero_blinds_be + (size_t)32 * g : nullptr);
}

// out[v] = base[v] + sum_d ys[d][v] mod r, big-endian in and out; base_be optional
__global__ void __launch_bounds__(256) k_vss_sum(const uint8_t* __restrict__ base_be, const uint8_t* __restrict__ ys_be, uint32_t dealers,
                                                 uint32_t n, uint8_t* __restrict__ out_be) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  uint8_t buf[32];
  Fr acc = Fr::zero();
  if (base_be) {
    for (int i = 0; i < 32; i++) buf[i] = base_be[(size_t)32 * v + i];
    acc = Fr::from_bytes_be(buf);
  }
  for (uint32_t d = 0; d < dealers; d++) {
    for (int i = 0; i < 32; i++) buf[i] = ys_be[((size_t)d * n + v) * 32 + i];
    acc = acc + Fr::from_bytes_be(buf);
  }
  acc.to_bytes_be(buf);
  for (int i = 0; i < 32; i++) out_be[(size_t)32 * v + i] = buf[i];
}

void launch_vss_table(hipStream_t st, const G1Affine* wbases, G1Affine* table) {
  hipLaunchKernelGGL(k_vss_table, dim3((VSS_TABLE_POINTS + 63) / 64), dim3(64), 0, st, wbases, table);
}
void launch_vss_commit(hipStream_t st, const G1Affine* table, const uint8_t* secrets_be, const uint8_t* coeffs_be, const uint8_t* blinds_be,
                       const uint8_t* coeffs_blind_be, uint32_t t, uint32_t n, uint8_t* commitments) {
  const uint32_t count = t * n;   // t <= 64, n <= 2^20
  if (count) hipLaunchKernelGGL(k_vss_commit, dim3((count + 63) / 64), dim3(64), 0, st, table, secrets_be, coeffs_be, blinds_be, coeffs_blind_be, n, count, commitments);
}
void launch_vss_check(hipStream_t st, const G1Affine* table, uint32_t t, uint32_t x, uint32_t dealers, uint32_t n, const uint8_t* commitments,
                      const uint8_t* ys_be, const uint8_t* ys_blind_be, const uint8_t* zero_blinds_be, uint32_t* flags) {
  const uint32_t lanes = dealers * n;
  if (lanes) hipLaunchKernelGGL(k_vss_check, dim3((lanes + 63) / 64), dim3(64), 0, st, table, t, x, dealers, n, commitments, ys_be, ys_blind_be, zero_blinds_be, flags);
}
void launch_vss_sum(hipStream_t st, const uint8_t* base_be, const uint8_t* ys_be, uint32_t dealers, uint32_t n, uint8_t* out_be) {
  if (n) hipLaunchKernelGGL(k_vss_sum, dim3((n + 255) / 256), dim3(256), 0, st, base_be, ys_be, dealers, n, out_be);
}

}  // namespace spp
