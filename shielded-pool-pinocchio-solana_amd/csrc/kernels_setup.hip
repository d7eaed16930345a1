// The setup ceremony's two kernels (setup_contrib.hpp has the method): one scalar times many G1 points, and the decoding of raw
// points with their check.  One lane per point, one wave per workgroup: the audit key's 62 K points are 970 waves, fewer than the
// chip has SIMDs, so small workgroups spread them over all compute units.
#include "kernels.hpp"
#include "setup_contrib.hpp"

namespace spp {

// out[i] = k * pts[i], k by its NAF digits dig[0 .. len): every lane reads dig[] at the wave's index, so the loop's branch is uniform
__global__ void __launch_bounds__(64) k_g1_scale(const G1Affine* __restrict__ pts, uint32_t n, const int8_t* __restrict__ dig, uint32_t len,
                                                 G1Affine* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = sc_scale_point(pts[i], dig, len).to_affine();
}
// pts[i], flags[i] = sc_decode_point(raw + 64 i)
__global__ void __launch_bounds__(64) k_g1_decode_check(const uint8_t* __restrict__ raw, uint32_t n, G1Affine* __restrict__ pts,
                                                        uint32_t* __restrict__ flags) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  G1Affine p;
  const uint32_t f = sc_decode_point(raw + (size_t)64 * i, &p);
  pts[i] = p;
  flags[i] = f;
}

void launch_g1_scale(hipStream_t st, const G1Affine* pts, uint32_t n, const int8_t* dig, uint32_t len, G1Affine* out) {
  if (n) hipLaunchKernelGGL(k_g1_scale, dim3((n + 63) / 64), dim3(64), 0, st, pts, n, dig, len, out);
}
void launch_g1_decode_check(hipStream_t st, const uint8_t* raw, uint32_t n, G1Affine* pts, uint32_t* flags) {
  if (n) hipLaunchKernelGGL(k_g1_decode_check, dim3((n + 63) / 64), dim3(64), 0, st, raw, n, pts, flags);
}

}  // namespace spp
