// The kernels of the powers-of-tau transcript and of the derivation of a key from it (ptau.hpp has the method): a scalar of its own
// per point in G1 and in G2, the decoding of raw G2 points with their check, the stages of the inverse NTT over group elements, the
// column gather and the Z points.  One lane per point, one wave per workgroup, as kernels_setup.hip: a transcript for the withdraw
// circuit is 4 n - 1 = 65 535 G1 points = 1 024 waves, one per SIMD.
#include "kernels.hpp"
#include "ptau.hpp"

namespace spp {

// out[i] = sc[i] * pts[i]; sc: 8 canonical words per point, 0 < sc[i] < r (the caller's check)
__global__ void __launch_bounds__(64) k_g1_mul_each(const G1Affine* __restrict__ pts, uint32_t n, const uint32_t* __restrict__ sc,
                                                    G1Affine* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = pt_mul_each(pts[i], sc + (size_t)8 * i).to_affine();
}
__global__ void __launch_bounds__(64) k_g2_mul_each(const G2Affine* __restrict__ pts, uint32_t n, const uint32_t* __restrict__ sc,
                                                    G2Affine* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = pt_mul_each(pts[i], sc + (size_t)8 * i).to_affine();
}
// pts[i], flags[i] = pt_decode_g2(raw + 128 i)
__global__ void __launch_bounds__(64) k_g2_decode_check(const uint8_t* __restrict__ raw, uint32_t n, Fq2 twist_b, G2Affine* __restrict__ pts,
                                                        uint32_t* __restrict__ flags) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  G2Affine p;
  const uint32_t f = pt_decode_g2(raw + (size_t)128 * i, twist_b, &p);
  pts[i] = p;
  flags[i] = f;
}

// One stage of the group inverse NTT (ptau.hpp) over nbatch transforms of 2^logn elements each laid end to end, one lane per
// output element: of a transform's n lanes the first n / 2 form the sums, the others the differences and their products.  Stage 0
// reads the affine input (in != nullptr), later stages src; every stage writes dst != src.
template <class F>
__global__ void __launch_bounds__(64) k_ec_ntt_pass(const Affine<F>* __restrict__ in, const XYZZ<F>* __restrict__ src, XYZZ<F>* __restrict__ dst,
                                                    uint32_t logn, uint32_t s, uint32_t total, const uint32_t* __restrict__ tw) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;   // total = nbatch << logn
  const uint32_t lane = t & ((1u << logn) - 1u), diff = lane >> (logn - 1);
  uint32_t i0, i1, e;
  pt_bfly_index(lane & ((1u << (logn - 1)) - 1u), logn, s, &i0, &i1, &e);
  const size_t base = (size_t)(t >> logn) << logn;
  const XYZZ<F> a = in ? XYZZ<F>::from_affine(in[base + i0]) : src[base + i0], b = in ? XYZZ<F>::from_affine(in[base + i1]) : src[base + i1];
  if (diff) dst[base + i1] = pt_bfly_diff(a, b, tw + (size_t)8 * e, e == 0);
  else dst[base + i0] = pt_bfly_sum(a, b);
}
// out[bitrev(i)] = (1 / n) work[i], affine
template <class F>
__global__ void __launch_bounds__(64) k_ec_ntt_finish(const XYZZ<F>* __restrict__ work, uint32_t logn, uint32_t total, const int8_t* __restrict__ dig,
                                                      uint32_t len, Affine<F>* __restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;   // total = nbatch << logn
  const uint32_t mask = (1u << logn) - 1u;
  out[(t & ~mask) | pt_bitrev(t & mask, logn)] = pt_ntt_finish(work[t], dig, len);
}
// partial[c] = the sum of chunk c's terms; then out[j] = the sum of column j's chunks
template <class F>
__global__ void __launch_bounds__(64) k_col_gather(const Affine<F>* __restrict__ bases, const uint32_t* __restrict__ terms,
                                                   const uint32_t* __restrict__ chunk_ptr, uint32_t nchunks, const uint32_t* __restrict__ mags,
                                                   const uint32_t* __restrict__ meta, XYZZ<F>* __restrict__ partial) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nchunks) return;
  partial[c] = pt_gather_chunk(bases, terms, chunk_ptr[c], chunk_ptr[c + 1], mags, meta);
}
template <class F>
__global__ void __launch_bounds__(64) k_col_combine(const XYZZ<F>* __restrict__ partial, const uint32_t* __restrict__ col_ptr, uint32_t ncols,
                                                    Affine<F>* __restrict__ out) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= ncols) return;
  out[j] = pt_gather_combine(partial, col_ptr[j], col_ptr[j + 1]);
}
// out[i] = pts[i + n] - pts[i], i < count: the Z points tau^i (tau^n - 1) G1 of a key with delta = 1
__global__ void __launch_bounds__(64) k_g1_shifted_diff(const G1Affine* __restrict__ pts, uint32_t n, uint32_t count, G1Affine* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  G1XYZZ d = G1XYZZ::from_affine(pts[i + n]);
  d.madd(pts[i].neg());
  out[i] = d.to_affine();
}

template <class F>
void launch_ec_intt(hipStream_t st, const Affine<F>* in, XYZZ<F>* work, uint32_t logn, uint32_t nbatch, const uint32_t* tw, const int8_t* dig,
                    uint32_t len, Affine<F>* out, hipEvent_t ev_passes, hipEvent_t ev_finish) {
  const uint32_t total = nbatch << logn;
  XYZZ<F>* buf[2] = {work, work + total};   // stage s writes buf[s & 1]
  for (uint32_t s = 0; s < logn; s++)
    hipLaunchKernelGGL(k_ec_ntt_pass<F>, dim3((total + 63) / 64), dim3(64), 0, st, s == 0 ? in : (const Affine<F>*)nullptr,
                       (const XYZZ<F>*)buf[(s + 1) & 1], buf[s & 1], logn, s, total, tw);
  if (ev_passes) hipEventRecord(ev_passes, st);
  hipLaunchKernelGGL(k_ec_ntt_finish<F>, dim3((total + 63) / 64), dim3(64), 0, st, (const XYZZ<F>*)buf[(logn - 1) & 1], logn, total, dig, len, out);
  if (ev_finish) hipEventRecord(ev_finish, st);
}
template void launch_ec_intt<Fq>(hipStream_t, const G1Affine*, G1XYZZ*, uint32_t, uint32_t, const uint32_t*, const int8_t*, uint32_t, G1Affine*,
                                 hipEvent_t, hipEvent_t);
template void launch_ec_intt<Fq2>(hipStream_t, const G2Affine*, G2XYZZ*, uint32_t, uint32_t, const uint32_t*, const int8_t*, uint32_t, G2Affine*,
                                  hipEvent_t, hipEvent_t);
template <class F>
void launch_col_gather(hipStream_t st, const Affine<F>* bases, const uint32_t* terms, const uint32_t* chunk_ptr, uint32_t nchunks,
                       const uint32_t* col_ptr, uint32_t ncols, const uint32_t* mags, const uint32_t* meta, XYZZ<F>* partial, Affine<F>* out) {
  if (nchunks) hipLaunchKernelGGL(k_col_gather<F>, dim3((nchunks + 63) / 64), dim3(64), 0, st, bases, terms, chunk_ptr, nchunks, mags, meta, partial);
  if (ncols) hipLaunchKernelGGL(k_col_combine<F>, dim3((ncols + 63) / 64), dim3(64), 0, st, partial, col_ptr, ncols, out);
}
template void launch_col_gather<Fq>(hipStream_t, const G1Affine*, const uint32_t*, const uint32_t*, uint32_t, const uint32_t*, uint32_t,
                                    const uint32_t*, const uint32_t*, G1XYZZ*, G1Affine*);
template void launch_col_gather<Fq2>(hipStream_t, const G2Affine*, const uint32_t*, const uint32_t*, uint32_t, const uint32_t*, uint32_t,
                                     const uint32_t*, const uint32_t*, G2XYZZ*, G2Affine*);
void launch_g1_shifted_diff(hipStream_t st, const G1Affine* pts, uint32_t n, uint32_t count, G1Affine* out) {
  if (count) hipLaunchKernelGGL(k_g1_shifted_diff, dim3((count + 63) / 64), dim3(64), 0, st, pts, n, count, out);
}

void launch_g1_mul_each(hipStream_t st, const G1Affine* pts, uint32_t n, const uint32_t* sc, G1Affine* out) {
  if (n) hipLaunchKernelGGL(k_g1_mul_each, dim3((n + 63) / 64), dim3(64), 0, st, pts, n, sc, out);
}
void launch_g2_mul_each(hipStream_t st, const G2Affine* pts, uint32_t n, const uint32_t* sc, G2Affine* out) {
  if (n) hipLaunchKernelGGL(k_g2_mul_each, dim3((n + 63) / 64), dim3(64), 0, st, pts, n, sc, out);
}
void launch_g2_decode_check(hipStream_t st, const uint8_t* raw, uint32_t n, const Fq2& twist_b, G2Affine* pts, uint32_t* flags) {
  if (n) hipLaunchKernelGGL(k_g2_decode_check, dim3((n + 63) / 64), dim3(64), 0, st, raw, n, twist_b, pts, flags);
}

}  // namespace spp
