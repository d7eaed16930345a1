// The powers-of-tau transcript (phase 1 of a setup ceremony): its byte layout, the per-point scalars of a contribution, and the
// text of the kernels in kernels_ptau.hip (spp_ptau_api.cpp has the calls, include/spp.h the protocol).
//
// SPPT: 'SPPT' | version 1 | domain_log L (u32 little-endian each), n = 2^L, then raw points as spp_setup.cpp writes them:
//   T1  tau^i G1, i < 2n - 1 (64 B each) | T2  tau^i G2, i < n (128 B each) | A1  alpha tau^i G1, i < n | B1  beta tau^i G1, i < n |
//   beta2 = beta G2.  No counts: they follow from L, and so does the file's length.
// A contribution with secrets t, a, b multiplies point i of T1 and T2 by t^i, of A1 by a t^i, of B1 by b t^i and beta2 by b.  Unlike
// the delta contribution (setup_contrib.hpp: ONE scalar, recoded once, every lane takes the same add / skip decisions) every point
// here has a scalar of its own, so the bit is the lane's: pt_mul_each doubles in every step and adds where the lane's bit is set.
// With 64 independent scalars some lane of a wave has its bit set in almost every step (2^-64 that none has), so the wave pays
// 254 doublings and ~254 additions whatever the recoding; a signed-digit form would not lower that, and a window table per lane
// (8 XYZZ points = 1 KB for G1, 2 KB for G2) is scratch.  The scalar is read one word per 32 steps from the lane's row of the
// scalar array: nothing is indexed at run time in registers.
//
// The addition is XYZZ::madd (bn254.hpp), which tests U2 == X and S2 == Y and doubles or returns infinity, so an accumulator that
// meets +-P is summed correctly wherever it occurs.  For 0 < k < r on a point of order r the binary loop never does (it would need
// k = r or r + 2); a caller's point of another order can, and the tests carry the special scalars of setup_contrib.hpp, here with a
// different one in every lane.
//
// The derivation of a key from a transcript (spp_setup_from_ptau) adds two more device steps, described where their text stands
// below: the inverse NTT over group elements, and the gather of its outputs through the columns of the R1CS matrices.
//
// Host and device: everything below is SPP_HD or plain C++, so that tests/host/ec_ntt_check.cpp pins it against big integers.
#pragma once
#include <string.h>
#include <algorithm>
#include <vector>
#include "bn254.hpp"
#include "setup_contrib.hpp"

namespace spp {

// ----------------------------------------------------------------------------------------------------------------------
// the container
// ----------------------------------------------------------------------------------------------------------------------
static constexpr uint32_t PT_MAGIC = 0x54505053u;   // 'SPPT'
static constexpr uint32_t PT_MAX_LOG = 20;
static constexpr size_t PT_HEADER = 12;
struct PtauLayout {
  uint32_t log = 0, n = 0;                    // n = 2^log
  uint32_t n_t1 = 0;                          // 2n - 1
  size_t t1 = 0, t2 = 0, a1 = 0, b1 = 0, beta2 = 0, size = 0;   // byte offsets of the sections, the file's length
};
inline bool ptau_layout_of(uint32_t log, PtauLayout* L) {
  if (log == 0 || log > PT_MAX_LOG) return false;
  L->log = log;
  L->n = 1u << log;
  L->n_t1 = 2 * L->n - 1;
  L->t1 = PT_HEADER;
  L->t2 = L->t1 + (size_t)L->n_t1 * 64;
  L->a1 = L->t2 + (size_t)L->n * 128;
  L->b1 = L->a1 + (size_t)L->n * 64;
  L->beta2 = L->b1 + (size_t)L->n * 64;
  L->size = L->beta2 + 128;
  return true;
}
inline uint32_t pt_load_le32(const uint8_t* b) { return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24); }
inline void pt_store_le32(uint8_t* b, uint32_t v) { for (int i = 0; i < 4; i++) b[i] = (uint8_t)(v >> (8 * i)); }
// true when b[0 .. len) is a transcript: magic, version, 1 <= L <= 20 and exactly the length L gives
inline bool ptau_layout(const uint8_t* b, size_t len, PtauLayout* L) {
  if (len < PT_HEADER || pt_load_le32(b) != PT_MAGIC || pt_load_le32(b + 4) != 1) return false;
  return ptau_layout_of(pt_load_le32(b + 8), L) && L->size == len;
}

// ----------------------------------------------------------------------------------------------------------------------
// a scalar per point
// ----------------------------------------------------------------------------------------------------------------------
// k * p for the canonical scalar k (least significant word first, k < 2^bits): MSB-first double-and-add from bit `bits` - 1 down.
// `k` is memory (the lane's row of the scalar array, or a row of the gather's coefficient table), read one word per 32 steps.
// pt_mul_each: a full-size scalar; the column gather passes the coefficient's own length.
template <class F>
SPP_HD XYZZ<F> pt_mul_bits(const Affine<F>& p, const uint32_t* k, uint32_t bits) {
  XYZZ<F> acc = XYZZ<F>::infinity();
  uint32_t kw = 0;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
  for (uint32_t b = bits; b-- > 0;) {
    if ((b & 31u) == 31u || b + 1 == bits) kw = k[b >> 5];
    acc.dbl_inplace();
    if ((kw >> (b & 31u)) & 1u) acc.madd(p);
  }
  return acc;
}
template <class F>
SPP_HD XYZZ<F> pt_mul_each(const Affine<F>& p, const uint32_t* k) {
  return pt_mul_bits(p, k, 254);   // r < 2^254
}
// 0 < k < r for canonical limbs
SPP_HD bool pt_scalar_ok(const uint32_t k[8]) {
  uint32_t any = 0;
  for (int i = 0; i < 8; i++) any |= k[i];
  return any != 0 && !Fr::geq_mod(k);
}

// One G2 point as the files hold it (X.c1 | X.c0 | Y.c1 | Y.c0, 32 B big-endian each; 128 zero bytes: infinity).  The flags are
// sc_decode_point's: SC_POINT_OK needs the four coordinates below q and y^2 = x^3 + 3 / (9 + u); the order-r subgroup is NOT
// tested here (the twist has a cofactor: the callers test it on the host, or on a random combination of the points).
SPP_HD uint32_t pt_decode_g2(const uint8_t raw[128], const Fq2& twist_b, Affine<Fq2>* out) {
  uint32_t c[4][8], any = 0;
  for (int f = 0; f < 4; f++)
    for (int i = 0; i < 8; i++) {
      c[f][7 - i] = sc_load_be32(raw + 32 * f + 4 * i);
      any |= c[f][7 - i];
    }
  *out = Affine<Fq2>::infinity();
  if (any == 0) return SC_POINT_INF;
  for (int f = 0; f < 4; f++)
    if (Fq::geq_mod(c[f])) return SC_POINT_BAD;
  const Fq2 x{Fq::from_canonical(c[1]), Fq::from_canonical(c[0])}, y{Fq::from_canonical(c[3]), Fq::from_canonical(c[2])};
  if (!(y.sqr() == x.sqr() * x + twist_b)) return SC_POINT_BAD;
  *out = Affine<Fq2>{x, y};
  return SC_POINT_OK;
}

// ----------------------------------------------------------------------------------------------------------------------
// the inverse NTT over group elements: Lagrange-basis points from monomial powers
// ----------------------------------------------------------------------------------------------------------------------
// L_k = (1 / n) sum_i w^(-k i) T_i: a radix-2 decimation-in-frequency transform with the root w^-1, natural order in, bit-reversed
// out, one launch per stage.  Stage s pairs (i0, i0 + half), half = n >> (s + 1), and multiplies the
// difference by w^-(j << s), j = i0 mod half.  The twiddle is the lane's own scalar, so the product is pt_mul_each on the
// difference brought to affine form first: one inversion (~40 products) against 4 more products in each of ~254 general additions.
// j = 0 needs no product; the whole last stage is j = 0, and that is where 1 / n goes (pt_ntt_finish): n products with ONE scalar,
// so the non-adjacent form of setup_contrib.hpp, whose branches the wave takes together.  Sum and difference are XYZZ::add, which
// doubles for equal operands and returns infinity for opposite ones; the transcript of tau = 1 makes every first-stage difference
// infinity and every sum a doubling.
// One lane per OUTPUT element, not per butterfly: a lane that held a, b, the sum and the difference of a G2 butterfly (64 words
// each) spilled; a lane that forms one of the two holds a, b and the addition's temporaries, and only the lanes of differences go
// on to the product.  The lanes of a transform's sums come first, then those of its differences, so whole waves do one or the other
// (from n = 128 up); the stages go from one work array to another, since the lane of the sum and the lane of the difference both
// read a and b.
template <class F>
SPP_HD XYZZ<F> pt_bfly_sum(const XYZZ<F>& a, const XYZZ<F>& b) {
  XYZZ<F> s = a;
  s.add(b);
  return s;
}
// tw * (a - b); tw: 8 canonical words in memory, not read when tw_is_one
template <class F>
SPP_HD XYZZ<F> pt_bfly_diff(const XYZZ<F>& a, const XYZZ<F>& b, const uint32_t* tw, bool tw_is_one) {
  XYZZ<F> d = a;
  d.add(b.neg());
  if (tw_is_one || d.is_inf()) return d;
  return pt_mul_each(d.to_affine(), tw);
}
SPP_HD uint32_t pt_bitrev(uint32_t v, uint32_t bits) {
  uint32_t r = 0;
  for (uint32_t i = 0; i < bits; i++) r |= ((v >> i) & 1u) << (bits - 1 - i);
  return r;
}
// butterfly u < n / 2 of stage s: the two element indices and the twiddle's exponent
SPP_HD void pt_bfly_index(uint32_t u, uint32_t logn, uint32_t s, uint32_t* i0, uint32_t* i1, uint32_t* e) {
  const uint32_t half = 1u << (logn - 1 - s), j = u & (half - 1u);
  *i0 = ((u >> (logn - 1 - s)) << (logn - s)) + j;
  *i1 = *i0 + half;
  *e = j << s;
}
// the last step of an element: 1 / n by its NAF digits, affine
template <class F>
SPP_HD Affine<F> pt_ntt_finish(const XYZZ<F>& v, const int8_t* dig, uint32_t len) {
  return sc_scale_point(v.to_affine(), dig, len).to_affine();
}

// ----------------------------------------------------------------------------------------------------------------------
// the column gather: sum_k M[k][j] * Base_k for every wire j
// ----------------------------------------------------------------------------------------------------------------------
// A coefficient c is applied as the shorter of c and r - c with a sign: c = +-1 is one mixed addition, a small integer (the audit
// rows' public-key coefficients are below 2^28) a loop of its bit length, and only the few full-size ones cost 254 steps.
// meta word: bit length of the magnitude (0: the coefficient is zero, the term adds nothing) | sign << 31.
SPP_HD uint32_t pt_signed_coeff(const uint32_t c[8], uint32_t mag[8]) {
  uint32_t any = 0;
  for (int i = 0; i < 8; i++) any |= c[i];
  const bool neg = any != 0 && canonical_gt_half<FrParams>(c);
  if (neg) canonical_negate<FrParams>(c, mag);
  else
    for (int i = 0; i < 8; i++) mag[i] = c[i];
  uint32_t bits = 0;
  for (int i = 7; i >= 0 && bits == 0; i--)
    for (int b = 31; b >= 0; b--)
      if ((mag[i] >> b) & 1u) { bits = 32u * (uint32_t)i + (uint32_t)b + 1u; break; }
  return bits | (neg ? 0x80000000u : 0u);
}
template <class F>
SPP_HD void pt_add_term(XYZZ<F>& acc, const Affine<F>& base, const uint32_t* mag, uint32_t meta) {
  const uint32_t bits = meta & 0x1ffu;
  if (bits == 0) return;
  const Affine<F> p = (meta >> 31) ? base.neg() : base;
  if (bits == 1) acc.madd(p);
  else acc.add(pt_mul_bits(p, mag, bits));
}
// the partial sum of terms [t0, t1): term t = (row, coefficient index) = terms[2 t], terms[2 t + 1]
template <class F>
SPP_HD XYZZ<F> pt_gather_chunk(const Affine<F>* bases, const uint32_t* terms, uint32_t t0, uint32_t t1, const uint32_t* mags,
                               const uint32_t* meta) {
  XYZZ<F> acc = XYZZ<F>::infinity();
#if defined(__HIPCC__)
#pragma unroll 1
#endif
  for (uint32_t t = t0; t < t1; t++) {
    const uint32_t ci = terms[2 * t + 1];
    pt_add_term(acc, bases[terms[2 * t]], mags + (size_t)8 * ci, meta[ci]);
  }
  return acc;
}
template <class F>
SPP_HD Affine<F> pt_gather_combine(const XYZZ<F>* partial, uint32_t c0, uint32_t c1) {
  XYZZ<F> acc = XYZZ<F>::infinity();
#if defined(__HIPCC__)
#pragma unroll 1
#endif
  for (uint32_t c = c0; c < c1; c++) acc.add(partial[c]);
  return acc.to_affine();
}

// The host's plan of a gather: the matrices transposed to column lists, long columns cut into chunks of PT_GATHER_CHUNK terms (a
// column of the audit circuit's constant wire has over a thousand), one lane per chunk, then one lane per column over its chunks.
static constexpr uint32_t PT_GATHER_CHUNK = 16;
struct ColEntry { uint32_t col, row, coeff; };
struct ColPlan {
  std::vector<uint32_t> terms;       // (row, coefficient index) pairs, grouped by column, a column's terms in the order given
  std::vector<uint32_t> chunk_ptr;   // chunks + 1 term offsets
  std::vector<uint32_t> col_ptr;     // columns + 1 chunk offsets; an empty column has no chunk
};
// false when an entry names a column, a row or a coefficient out of range (the kernels index with them unchecked)
inline bool col_plan(uint32_t ncols, uint32_t nrows, uint32_t ncoef, const std::vector<ColEntry>& entries, ColPlan* P) {
  std::vector<uint32_t> start(ncols + 1, 0);
  for (const ColEntry& e : entries) {
    if (e.col >= ncols || e.row >= nrows || e.coeff >= ncoef) return false;
    start[e.col + 1]++;
  }
  for (uint32_t c = 0; c < ncols; c++) start[c + 1] += start[c];
  P->terms.assign(2 * entries.size(), 0);
  std::vector<uint32_t> at(start.begin(), start.end() - 1);
  for (const ColEntry& e : entries) {
    const uint32_t t = at[e.col]++;
    P->terms[2 * t] = e.row;
    P->terms[2 * t + 1] = e.coeff;
  }
  P->chunk_ptr.assign(1, 0);
  P->col_ptr.assign(1, 0);
  for (uint32_t c = 0; c < ncols; c++) {
    for (uint32_t t = start[c]; t < start[c + 1]; t += PT_GATHER_CHUNK) P->chunk_ptr.push_back(std::min(t + PT_GATHER_CHUNK, start[c + 1]));
    P->col_ptr.push_back((uint32_t)P->chunk_ptr.size() - 1);
  }
  return true;
}

}  // namespace spp
