// The kernels of the verifiable sharing of the auditors' key (vss.hpp has the method): the window table of the two generators, the
// commitments of a dealing, the receiver's check and the sum of the accepted sub-shares.  One lane per point, one wave per
// workgroup, as kernels_ptau.hip: a dealing of the key at the largest threshold is 64 * 1024 commitments = 1 024 waves, one per SIMD.
// Then the committee's commitments and the hand-over to a new committee: decoding points once, the weighted sum of the dealers'
// commitments by one scan of the weights' bits shared by the wave, the public commitments of shares, the new member's check and
// the weighted sum of its sub-shares.
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

// points[i] = raw[i * 64 ..] in Montgomery form, flags[i] = SPP_VSS_BAD_POINT or 0: what k_vss_lincomb reads
__global__ void __launch_bounds__(256) k_vss_decode(const uint8_t* __restrict__ raw, size_t count, G1Affine* __restrict__ points,
                                                    uint32_t* __restrict__ flags) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // up to 255 * 64 * 2^20
  if (i >= count) return;
  G1Affine p;
  flags[i] = vss_decode(raw + 64 * i, &p);
  points[i] = p;
}

// out[(k n + v) 64 ..] = base[k n + v] + sum_d w_d points[d * count + k n + v] for lane k n + v < count = t n (vss.hpp: one scan
// of the weights' bits shared by the wave; weights == nullptr: plain sums).  weights is the same pointer in every lane.
__global__ void __launch_bounds__(64) k_vss_lincomb(uint32_t dealers, const uint32_t* __restrict__ weights, const G1Affine* __restrict__ points,
                                                    const G1Affine* __restrict__ base, uint32_t count, uint8_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  vss_store_point(vss_lincomb(dealers, weights, points + i, count, base ? base + i : nullptr), out + (size_t)64 * i);
}

// out[(i n + v) 64 ..] = sum_k xs[i]^k D_k[v] for lane i n + v < count * n; committee: points only (the host's check)
__global__ void __launch_bounds__(64) k_vss_share_commit(uint32_t t, const uint32_t* __restrict__ xs, uint32_t count, uint32_t n,
                                                         const uint8_t* __restrict__ committee, uint8_t* __restrict__ out) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= count * n) return;   // count <= 255, n <= 2^20
  G1XYZZ e = G1XYZZ::infinity();
  G1Affine d0;
  (void)vss_eval_commitments(t, xs[g / n], committee + (size_t)64 * (g % n), (size_t)n * 64, &e, &d0);
  vss_store_point(e, out + (size_t)64 * g);
}

// flags[j n + v]: the new member at x_new checks value v of old member xs_old[j]'s dealing at threshold t_new (vss_check_value),
// then its constant term against the old committee's commitments (vss_is_share)
__global__ void __launch_bounds__(64) k_vss_reshare_check(const G1Affine* __restrict__ table, uint32_t t_old, const uint32_t* __restrict__ xs_old,
                                                          uint32_t t_new, uint32_t x_new, uint32_t n, const uint8_t* __restrict__ committee,
                                                          const uint8_t* __restrict__ commitments, const uint8_t* __restrict__ ys_be,
                                                          const uint8_t* __restrict__ ys_blind_be, uint32_t* __restrict__ flags) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;   // t_old n <= 64 * 2^20
  if (g >= t_old * n) return;
  const uint32_t j = g / n, v = g % n;
  const uint8_t* cm = commitments + ((size_t)j * t_new * n + v) * 64;
  uint32_t f = vss_check_value(table, t_new, x_new, cm, (size_t)n * 64, ys_be + (size_t)32 * g, ys_blind_be + (size_t)32 * g, nullptr);
  if (f != VSS_FLAG_BAD_POINT) f |= vss_is_share(t_old, xs_old[j], committee + (size_t)64 * v, (size_t)n * 64, cm);
  flags[g] = f;
}

// out[v] = sum_d w_d ys[d][v] mod r, big-endian in and out
__global__ void __launch_bounds__(256) k_vss_weighted_sum(const Fr* __restrict__ weights, const uint8_t* __restrict__ ys_be, uint32_t dealers,
                                                          uint32_t n, uint8_t* __restrict__ out_be) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  uint8_t buf[32];
  vss_weighted_sum(dealers, weights, ys_be + (size_t)32 * v, (size_t)n * 32, buf);
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
void launch_vss_decode(hipStream_t st, const uint8_t* raw, size_t count, G1Affine* points, uint32_t* flags) {
  if (count) hipLaunchKernelGGL(k_vss_decode, dim3((uint32_t)((count + 255) / 256)), dim3(256), 0, st, raw, count, points, flags);
}
void launch_vss_lincomb(hipStream_t st, uint32_t dealers, const uint32_t* weights, const G1Affine* points, const G1Affine* base, uint32_t count,
                        uint8_t* out) {
  if (count) hipLaunchKernelGGL(k_vss_lincomb, dim3((count + 63) / 64), dim3(64), 0, st, dealers, weights, points, base, count, out);
}
void launch_vss_share_commit(hipStream_t st, uint32_t t, const uint32_t* xs, uint32_t count, uint32_t n, const uint8_t* committee, uint8_t* out) {
  const uint32_t lanes = count * n;
  if (lanes) hipLaunchKernelGGL(k_vss_share_commit, dim3((lanes + 63) / 64), dim3(64), 0, st, t, xs, count, n, committee, out);
}
void launch_vss_reshare_check(hipStream_t st, const G1Affine* table, uint32_t t_old, const uint32_t* xs_old, uint32_t t_new, uint32_t x_new,
                              uint32_t n, const uint8_t* committee, const uint8_t* commitments, const uint8_t* ys_be, const uint8_t* ys_blind_be,
                              uint32_t* flags) {
  const uint32_t lanes = t_old * n;
  if (lanes)
    hipLaunchKernelGGL(k_vss_reshare_check, dim3((lanes + 63) / 64), dim3(64), 0, st, table, t_old, xs_old, t_new, x_new, n, committee, commitments,
                       ys_be, ys_blind_be, flags);
}
void launch_vss_weighted_sum(hipStream_t st, const Fr* weights, const uint8_t* ys_be, uint32_t dealers, uint32_t n, uint8_t* out_be) {
  if (n) hipLaunchKernelGGL(k_vss_weighted_sum, dim3((n + 255) / 256), dim3(256), 0, st, weights, ys_be, dealers, n, out_be);
}

}  // namespace spp
