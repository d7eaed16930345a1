// The table-walk MSM for G1: the Fq instantiations of msm_table.hpp (the design is described there) and the kernels that exist for
// G1 only -- the digit planes of the scalars (field-independent: the G2 walk reads the same planes), the H bases in the evaluation
// basis and the column sums of the product form.  Built with the max-ilp scheduler (Makefile; why, msm_table.hpp).
#include "msm_table.hpp"

namespace spp {

template void launch_build_table<Fq>(hipStream_t, const Affine<Fq>*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, Affine<Fq>*,
                                     XYZZ<Fq>*, Fq*, const MsmBlock*, uint32_t);
template void launch_msm_accumulate<Fq>(hipStream_t, const Affine<Fq>*, const MsmBlock*, const int16_t*, XYZZ<Fq>*, uint32_t, uint32_t, uint32_t,
                                        const MsmPlan&, hipEvent_t, hipEvent_t, uint32_t*);
template void launch_msm_reduce_multi<Fq>(hipStream_t, MsmFoldSets<Fq>, uint32_t, uint32_t);
template void launch_msm_reduce<Fq>(hipStream_t, XYZZ<Fq>*, XYZZ<Fq>*, uint32_t, const MsmPlan&, uint32_t, bool);
template void launch_fixed_base_mul<Fq>(hipStream_t, const Affine<Fq>*, uint32_t, const Fr*, uint32_t, Affine<Fq>*);

// ----------------------------------------------------------------------------------------------------
// Digit planes.  One lane per (base, proof): the scalar is brought to canonical form ONCE, folded to its magnitude
// (scalars above (r-1)/2 become their negatives: the small signed noise of the audit witness stays small), recoded into
// W = ceil(254/c) signed c-bit digits and stored as int16 planes  dig[j][i][p]  (p fastest, Pp per row).  Digits lie in
// [-2^(c-1), 2^(c-1) - 1] -- for a folded (negated) scalar the recoding keeps +2^(c-1) and carries above it, so that the
// negated digit is -2^(c-1) -- which is what lets c = 16 fit int16.  The accumulate kernels then read 2 bytes per (window,
// base, proof), coalesced, with no recoder state in registers and no carry chain between windows: any window can be
// processed by any lane, which is what the window passes (msm_table.hpp) need.
// ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_msm_digits(const uint32_t* __restrict__ rows, const Fr* __restrict__ scalars,
                                                    int16_t* __restrict__ dig, uint32_t N, uint32_t P, uint32_t Pp, uint32_t c, uint32_t W) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t p = (uint32_t)(g % Pp), i = (uint32_t)(g / Pp);
  if (i >= N || p >= P) return;
  const uint32_t row = rows[i];
  if (row == 0xffffffffu) {   // MSM_ROW_ZERO: a base whose share is summed elsewhere (msm_lookup.hpp) -- the walk skips zero digits
#pragma unroll 1
    for (uint32_t j = 0; j < W; j++) dig[(size_t)j * N * Pp + (size_t)i * Pp + p] = 0;
    return;
  }
  const Fr s = scalars[(size_t)row * P + p];
  uint32_t l[8];
  s.to_canonical(l);
  const bool neg = canonical_gt_half<FrParams>(l);
  if (neg) {
    uint32_t t[8];
    canonical_negate<FrParams>(l, t);
    SPP_UNROLL for (int k = 0; k < 8; k++) l[k] = t[k];
  }
  const uint32_t mask = (1u << c) - 1u, half = 1u << (c - 1);
  uint32_t carry = 0;
  int16_t* out = dig + (size_t)i * Pp + p;
  const size_t plane = (size_t)N * Pp;
#pragma unroll 1
  for (uint32_t j = 0; j < W; j++) {
    const uint32_t d = (l[0] & mask) + carry;
    SPP_UNROLL for (int k = 0; k < 7; k++) l[k] = (l[k] >> c) | (l[k + 1] << (32 - c));
    l[7] >>= c;
    const bool over = neg ? d > half : d >= half;
    int v = over ? (int)d - (int)(1u << c) : (int)d;
    carry = over ? 1u : 0u;
    if (neg) v = -v;
    out[(size_t)j * plane] = (int16_t)v;
  }
}
void launch_msm_digits(hipStream_t st, const uint32_t* rows, const Fr* scalars, int16_t* dig, uint32_t N, uint32_t P, uint32_t c) {
  if (N == 0 || P == 0) return;
  const uint32_t Pp = msm_padded_batch(P);
  const uint64_t lanes = (uint64_t)N * Pp;
  hipLaunchKernelGGL(k_msm_digits, dim3((uint32_t)((lanes + 255) / 256)), dim3(256), 0, st, rows, scalars, dig, N, P, Pp, c, msm_windows(c));
}

// ----------------------------------------------------------------------------------------------------
// The H bases in the evaluation basis (load time).  gnark's computeH ends with an inverse coset transform that turns the
// values of h on the coset g*H into coefficients, because pk.G1.Z is a coefficient basis (Z_j = [tau^j t(tau) / delta]).
// sum_j h_j Z_j = sum_i h(g w^i) Z'_i  with  Z'_i = sum_j (g^-j / n) w^(-ij) Z_j : a DFT "in the exponent" of the n - 1 points
// (scaled, padded with the point at infinity), done ONCE when the circuit is loaded -- n + (n/2) log2 n scalar multiplications,
// ~60 ms for n = 2^15 -- and every proof saves its seventh transform (the scalars of the Z walk are the values the pointwise
// kernel leaves, natural order).  The group element is the same, so are the proof bytes.
// ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ XYZZ<Fq> g1_scalar_mul(const XYZZ<Fq>& pt, const Fr& k) {
  uint32_t c[8];
  k.to_canonical(c);
  XYZZ<Fq> acc = XYZZ<Fq>::infinity();
  if (pt.is_inf()) return acc;
#pragma unroll 1
  for (int w = 7; w >= 0; w--) {
    const uint32_t word = w == 0 ? c[0] : w == 1 ? c[1] : w == 2 ? c[2] : w == 3 ? c[3] : w == 4 ? c[4] : w == 5 ? c[5] : w == 6 ? c[6] : c[7];
#pragma unroll 1
    for (int bit = 31; bit >= 0; bit--) {
      acc.dbl_inplace();
      if ((word >> bit) & 1) acc.add(pt);
    }
  }
  return acc;
}
// x[j] = scale[j] * affine[j] (j < n_pts), infinity above
__global__ void __launch_bounds__(64) k_g1_dft_load(const G1Affine* __restrict__ pts, uint32_t n_pts, const Fr* __restrict__ scale,
                                                    G1XYZZ* __restrict__ x, uint32_t n) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  x[j] = j < n_pts ? g1_scalar_mul(G1XYZZ::from_affine(pts[j]), scale[j]) : G1XYZZ::infinity();
}
// one decimation-in-frequency stage (natural in, bit-reversed out after log2 n stages): block length len, twiddles tw[k] = w^k
__global__ void __launch_bounds__(64) k_g1_dft_stage(G1XYZZ* __restrict__ x, uint32_t n, uint32_t len, const Fr* __restrict__ tw) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n / 2) return;
  const uint32_t half = len / 2, j = g % half, b = (g / half) * len;
  G1XYZZ u = x[b + j], v = x[b + j + half];
  G1XYZZ d = u;
  d.add(v.neg());
  u.add(v);
  x[b + j] = u;
  const uint32_t e = j * (n / len);
  x[b + j + half] = e ? g1_scalar_mul(d, tw[e]) : d;
}
__global__ void __launch_bounds__(64) k_g1_to_affine(const G1XYZZ* __restrict__ x, G1Affine* __restrict__ out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = x[i].to_affine();
}
// term t: coeff[t] * base[row[t]]; then segment s = sum of terms [seg[s], seg[s+1]) as an affine point (the column sums
// X_wire = sum_i C[i][wire] * W_i of the product form of computeH, spp_load.cpp)
__global__ void __launch_bounds__(64) k_g1_terms(const G1Affine* __restrict__ base, const uint32_t* __restrict__ row, const Fr* __restrict__ coeff,
                                                 uint32_t nterms, G1XYZZ* __restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nterms) return;
  const G1XYZZ p = G1XYZZ::from_affine(base[row[t]]);
  const Fr c = coeff[t];
  if (c == Fr::one()) out[t] = p;
  else if (c == Fr::one().neg()) out[t] = p.neg();
  else out[t] = g1_scalar_mul(p, c);
}
__global__ void __launch_bounds__(64) k_g1_segsum(const G1XYZZ* __restrict__ terms, const uint32_t* __restrict__ seg, uint32_t nseg,
                                                  G1Affine* __restrict__ out) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nseg) return;
  G1XYZZ acc = G1XYZZ::infinity();
  for (uint32_t t = seg[s]; t < seg[s + 1]; t++) acc.add(terms[t]);
  out[s] = acc.to_affine();
}
void launch_g1_column_sums(hipStream_t st, const G1Affine* base, const uint32_t* row, const Fr* coeff, uint32_t nterms, const uint32_t* seg,
                           uint32_t nseg, G1XYZZ* work, G1Affine* out) {
  if (nterms) hipLaunchKernelGGL(k_g1_terms, dim3((nterms + 63) / 64), dim3(64), 0, st, base, row, coeff, nterms, work);
  if (nseg) hipLaunchKernelGGL(k_g1_segsum, dim3((nseg + 63) / 64), dim3(64), 0, st, work, seg, nseg, out);
}
// out[bitrev(i)] = Z'_i for i < n = 2^logn (the caller undoes the bit reversal); scale[j] = g^-j / n, tw_inv[k] = w^-k (k < n/2)
void launch_g1_eval_basis(hipStream_t st, const G1Affine* pts, uint32_t n_pts, uint32_t logn, const Fr* scale, const Fr* tw_inv, G1XYZZ* work,
                          G1Affine* out) {
  const uint32_t n = 1u << logn;
  hipLaunchKernelGGL(k_g1_dft_load, dim3((n + 63) / 64), dim3(64), 0, st, pts, n_pts, scale, work, n);
  for (uint32_t len = n; len >= 2; len >>= 1)
    hipLaunchKernelGGL(k_g1_dft_stage, dim3((n / 2 + 63) / 64), dim3(64), 0, st, work, n, len, tw_inv);
  hipLaunchKernelGGL(k_g1_to_affine, dim3((n + 63) / 64), dim3(64), 0, st, work, out, n);
}

}  // namespace spp
