// arith_probe.hpp -- the raw-word probe of the arithmetic headers (spp_debug_arith, include/spp.h): one case = load the operand
// words as they are, call ONE function of bn254.hpp / f29.hpp / gnark_hints.hpp, store what it returned.  No conversion, no
// reduction, no check: the caller (tests/arith_vectors.py) chooses the word the code sees and judges the result against Python
// integers.
// The same probe_case is what the gfx950 kernels (kernels_arith_probe.hip) and the g++ twin (tests/host/arith_raw_check.cpp) run,
// so a difference between the two is a difference of the compilers, not of the harness.
#pragma once
#include "f29.hpp"
#include "gnark_hints.hpp"

namespace spp {

// X(name, code, in_words, out_words, fields): fields 0 = Fr and Fq, 1 = Fq only, 2 = Fr only.
// Fp operands are 8 words, F29 operands 9 limbs; Fq2 / F29x2 are c0 then c1.
// Scripts: in = [nsteps, 16 step words (table index | negate << 8), 8 table points (x, y as Fp words)];
//          out = [inf, affine x, y as Fp words, bit s = what step s returned, the accumulator's limbs X, Y, ZZ, ZZZ (zero padded)].
// Solver hints (gnark_hints.hpp, codes >= 128, Fr only):
//   HINT_GLV_SPLIT     in = [the 28 constant words of OP_GLV (v1x, v1y, v2x, v2y as 4 magnitude words + sign word, det 8 words), s 4 words]
//                      out = [found, s1 4 words, s2 4 words]
//   HINT_EMUL_REDUCE   dev_emulated_reduce<6, 6>: in = [a_0 .. a_5 as 8 canonical words each, q 8 words, q^-1 mod 2^256 8 words]
//                      out = [k 8 words, r 8 words, carries c_0 .. c_5 as raw Big384 (12 words each), then to_canonical(fr_from_bigs(c_i)) 8 words each]
//   HINT_GRUMPKIN_MUL  in = [k 8 words, gy as Fr words]; out = [finite, x, y as Fr words (zero when not finite)]
//   BIGS_*             Big384 operands are 12 words; LT / LOW64_ZERO return one word; ADD_SMALL_MUL: arg = m as a signed 16-bit value
//   BIG_MUL_ACC_AxB_N  in = [accumulator N words, a A words, b B words]; out = the accumulator (N words) after big_mul_acc
#define SPP_ARITH_OPS(X)                      \
  X(FP_MUL, 1, 16, 8, 0)                      \
  X(FP_SQR, 2, 8, 8, 0)                       \
  X(FP_ADD, 3, 16, 8, 0)                      \
  X(FP_SUB, 4, 16, 8, 0)                      \
  X(FP_NEG, 5, 8, 8, 0)                       \
  X(FP_DBL, 6, 8, 8, 0)                       \
  X(FP_MUL_SMALL, 7, 8, 8, 0)                 \
  X(FP_INV, 8, 8, 8, 0)                       \
  X(FP_INV_FERMAT, 9, 8, 8, 0)                \
  X(FP_TO_CANONICAL, 10, 8, 8, 0)             \
  X(FP_FROM_U256, 11, 8, 8, 0)                \
  X(FP_IS_ZERO, 12, 8, 1, 0)                  \
  X(FP_EQ, 13, 16, 1, 0)                      \
  X(FQ2_MUL, 16, 32, 16, 1)                   \
  X(FQ2_SQR, 17, 16, 16, 1)                   \
  X(FQ2_INV, 18, 16, 16, 1)                   \
  X(F29_FROM_WORDS, 32, 8, 9, 0)              \
  X(F29_TO_WORDS, 33, 9, 8, 0)                \
  X(F29_NORM, 34, 9, 9, 0)                    \
  X(F29_MUL, 35, 18, 9, 0)                    \
  X(F29_SQR, 36, 9, 9, 0)                     \
  X(F29_MUL2, 37, 36, 9, 0)                   \
  X(F29_SUB_NORM_6P_1, 38, 18, 9, 0)          \
  X(F29_SUB_NORM_2P_1, 39, 18, 9, 0)          \
  X(F29_SUB3_NORM_4P_3, 40, 27, 9, 0)         \
  X(F29_SUB_LAZY_6P_1, 41, 18, 9, 0)          \
  X(F29_NEG_LAZY_2P_1, 42, 9, 9, 0)           \
  X(F29_NEG_LAZY_4P_1, 43, 9, 9, 0)           \
  X(F29_ADD_NORM, 44, 18, 9, 0)               \
  X(F29_ADD_LAZY, 45, 18, 9, 0)               \
  X(F29_IS_ZERO_MOD_P_7, 46, 9, 1, 0)         \
  X(F29_IS_ZERO_MOD_P_3, 47, 9, 1, 0)         \
  X(F29_FROM_FP, 48, 8, 9, 0)                 \
  X(F29_TO_FP, 49, 9, 8, 0)                   \
  X(F29_SCALED_TO_FP, 50, 9, 8, 0)            \
  X(F29X2_MUL, 64, 36, 18, 1)                 \
  X(F29X2_SQR, 65, 18, 18, 1)                 \
  X(SCRIPT_G1_29, 96, 145, 54, 1)             \
  X(SCRIPT_G1_29_DISTINCT, 97, 145, 54, 1)    \
  X(SCRIPT_G1, 98, 145, 54, 1)                \
  X(SCRIPT_G2_29, 99, 273, 106, 1)            \
  X(SCRIPT_G2_29_DISTINCT, 100, 273, 106, 1)  \
  X(SCRIPT_G2, 101, 273, 106, 1)              \
  X(HINT_GLV_SPLIT, 128, 32, 9, 2)            \
  X(HINT_EMUL_REDUCE, 129, 64, 136, 2)        \
  X(HINT_GRUMPKIN_MUL, 130, 16, 17, 2)        \
  X(BIGS_ADD, 136, 24, 12, 2)                 \
  X(BIGS_SUB, 137, 24, 12, 2)                 \
  X(BIGS_NEGATE, 138, 12, 12, 2)              \
  X(BIGS_LT, 139, 24, 1, 2)                   \
  X(BIGS_SAR64, 140, 12, 12, 2)               \
  X(BIGS_LOW64_ZERO, 141, 12, 1, 2)           \
  X(BIGS_ADD_SMALL_MUL, 142, 24, 12, 2)       \
  X(BIG_MUL_ACC_4X4_12, 144, 20, 12, 2)       \
  X(BIG_MUL_ACC_2X2_12, 145, 16, 12, 2)       \
  X(BIG_MUL_ACC_8X8_8, 146, 24, 8, 2)

enum ArithOp : uint32_t {
#define X(name, code, iw, ow, fq) ARITH_##name = code,
  SPP_ARITH_OPS(X)
#undef X
};
static constexpr uint32_t ARITH_FIELD_FQ = 0x100u;   // SPP_ARITH_FQ; SPP_ARITH_FR = 0
static constexpr uint32_t ARITH_SCRIPT_STEPS = 16, ARITH_SCRIPT_POINTS = 8;
static constexpr int ARITH_FIELDS_BOTH = 0, ARITH_FIELDS_FQ = 1, ARITH_FIELDS_FR = 2;   // the last column of SPP_ARITH_OPS
static constexpr int ARITH_SMALL_MUL_MAX = 64;   // the largest |m| BIGS_ADD_SMALL_MUL takes (add_small_mul adds |m| times)

// words per case of an operation; false = no such operation for that field
inline bool arith_probe_shape(uint32_t selector, uint32_t* in_words, uint32_t* out_words) {
  if (selector & ~(ARITH_FIELD_FQ | 0xffu)) return false;
  const bool is_fq = (selector & ARITH_FIELD_FQ) != 0;
  switch (selector & 0xffu) {
#define X(name, code, iw, ow, fq) \
  case code:                      \
    if ((fq == ARITH_FIELDS_FQ && !is_fq) || (fq == ARITH_FIELDS_FR && is_fq)) return false; \
    *in_words = iw;               \
    *out_words = ow;              \
    return true;
    SPP_ARITH_OPS(X)
#undef X
  }
  return false;
}
// the args an operation knows (mul_small: the k < 2^16 of its comment; F29x2: which SUBC_kP_1 negates a1; add_small_mul: m as a
// signed 16-bit value, |m| <= 64)
inline bool arith_probe_arg_ok(uint32_t selector, uint32_t arg) {
  switch (selector & 0xffu) {
    case ARITH_FP_MUL_SMALL: return arg < (1u << 16);
    case ARITH_F29X2_MUL:
    case ARITH_F29X2_SQR: return arg == 2 || arg == 4 || arg == 6 || arg == 8;
    case ARITH_BIGS_ADD_SMALL_MUL: {
      const int m = (int16_t)(uint16_t)arg;
      return arg < (1u << 16) && m >= -ARITH_SMALL_MUL_MAX && m <= ARITH_SMALL_MUL_MAX;
    }
  }
  return true;
}

namespace arith_probe {
template <class Pm>
SPP_HD Fp<Pm> ld_fp(const uint32_t* w) {
  Fp<Pm> r;
  SPP_UNROLL for (int i = 0; i < 8; i++) r.l[i] = w[i];
  return r;
}
template <class Pm>
SPP_HD void st_fp(uint32_t* w, const Fp<Pm>& a) {
  SPP_UNROLL for (int i = 0; i < 8; i++) w[i] = a.l[i];
}
template <class Pm>
SPP_HD F29<Pm> ld_f29(const uint32_t* w) {
  F29<Pm> r;
  SPP_UNROLL for (int i = 0; i < 9; i++) r.l[i] = w[i];
  return r;
}
template <class Pm>
SPP_HD void st_f29(uint32_t* w, const F29<Pm>& a) {
  SPP_UNROLL for (int i = 0; i < 9; i++) w[i] = a.l[i];
}
SPP_HD Fq2 ld_fq2(const uint32_t* w) { return {ld_fp<FqParams>(w), ld_fp<FqParams>(w + 8)}; }
SPP_HD void st_fq2(uint32_t* w, const Fq2& a) {
  st_fp(w, a.c0);
  st_fp(w + 8, a.c1);
}
SPP_HD F29x2 ld_f29x2(const uint32_t* w) { return {ld_f29<FqParams>(w), ld_f29<FqParams>(w + 9)}; }
SPP_HD void st_f29x2(uint32_t* w, const F29x2& a) {
  st_f29(w, a.c0);
  st_f29(w + 9, a.c1);
}

// table point k of a script, and the accumulators' limbs / coordinates as words
SPP_HD G1Affine ld_point(const G1Affine*, const uint32_t* table, uint32_t k) {
  return {ld_fp<FqParams>(table + 16 * k), ld_fp<FqParams>(table + 16 * k + 8)};
}
SPP_HD G2Affine ld_point(const G2Affine*, const uint32_t* table, uint32_t k) {
  return {ld_fq2(table + 32 * k), ld_fq2(table + 32 * k + 16)};
}
SPP_HD void st_affine(uint32_t* w, const G1Affine& a) {
  st_fp(w, a.x);
  st_fp(w + 8, a.y);
}
SPP_HD void st_affine(uint32_t* w, const G2Affine& a) {
  st_fq2(w, a.x);
  st_fq2(w + 16, a.y);
}
SPP_HD void st_raw(uint32_t* w, const XYZZ29<FqParams>& a) {
  st_f29(w, a.X);
  st_f29(w + 9, a.Y);
  st_f29(w + 18, a.ZZ);
  st_f29(w + 27, a.ZZZ);
}
SPP_HD void st_raw(uint32_t* w, const XYZZ29G2& a) {
  st_f29x2(w, a.X);
  st_f29x2(w + 18, a.Y);
  st_f29x2(w + 36, a.ZZ);
  st_f29x2(w + 54, a.ZZZ);
}
SPP_HD void st_raw(uint32_t* w, const G1XYZZ& a) {
  st_fp(w, a.X);
  st_fp(w + 8, a.Y);
  st_fp(w + 16, a.ZZ);
  st_fp(w + 24, a.ZZZ);
  SPP_UNROLL for (int i = 32; i < 36; i++) w[i] = 0;
}
SPP_HD void st_raw(uint32_t* w, const G2XYZZ& a) {
  st_fq2(w, a.X);
  st_fq2(w + 16, a.Y);
  st_fq2(w + 32, a.ZZ);
  st_fq2(w + 48, a.ZZZ);
  SPP_UNROLL for (int i = 64; i < 72; i++) w[i] = 0;
}

// Acc29 = XYZZ29<FqParams> or XYZZ29G2; step count and table index are clamped, so no script reads outside its case
template <class Acc29, class A, bool DISTINCT>
SPP_HD void script29(const uint32_t* in, uint32_t* out) {
  constexpr uint32_t AW = sizeof(A) / 4;
  const uint32_t nsteps = in[0] < ARITH_SCRIPT_STEPS ? in[0] : ARITH_SCRIPT_STEPS;
  const uint32_t* table = in + 1 + ARITH_SCRIPT_STEPS;
  Acc29 acc = Acc29::infinity();
  uint32_t ret = 0;
  for (uint32_t s = 0; s < nsteps; s++) {
    const uint32_t w = in[1 + s];
    const A e = ld_point((const A*)nullptr, table, w & (ARITH_SCRIPT_POINTS - 1));
    const bool negate = (w >> 8) & 1u;
    if constexpr (DISTINCT) {
      if (acc.madd_distinct(e, negate)) ret |= 1u << s;
    } else {
      acc.madd(e, negate);
      ret |= 1u << s;
    }
  }
  out[0] = acc.inf ? 1u : 0u;
  st_affine(out + 1, acc.to_xyzz().to_affine());
  out[1 + AW] = ret;
  st_raw(out + 2 + AW, acc);
}
template <class Acc, class A>
SPP_HD void script_plain(const uint32_t* in, uint32_t* out) {
  constexpr uint32_t AW = sizeof(A) / 4;
  const uint32_t nsteps = in[0] < ARITH_SCRIPT_STEPS ? in[0] : ARITH_SCRIPT_STEPS;
  const uint32_t* table = in + 1 + ARITH_SCRIPT_STEPS;
  Acc acc = Acc::infinity();
  for (uint32_t s = 0; s < nsteps; s++) {
    const uint32_t w = in[1 + s];
    const A e = ld_point((const A*)nullptr, table, w & (ARITH_SCRIPT_POINTS - 1));
    acc.madd(((w >> 8) & 1u) ? e.neg() : e);
  }
  out[0] = acc.is_inf() ? 1u : 0u;
  st_affine(out + 1, acc.to_affine());
  out[1 + AW] = 0;
  st_raw(out + 2 + AW, acc);
}

template <F29<FqParams>::ConstFn CA>
SPP_HD void f29x2_case(bool sqr, const uint32_t* in, uint32_t* out) {
  const F29x2 a = ld_f29x2(in);
  if (sqr) {
    st_f29x2(out, a.template sqr<CA>());
  } else {
    st_f29x2(out, F29x2::template mul<CA>(a, ld_f29x2(in + 18)));
  }
}

SPP_HD Big384 ld_big(const uint32_t* w) {
  Big384 r;
  for (int i = 0; i < 12; i++) r.w[i] = w[i];
  return r;
}
SPP_HD void st_big(uint32_t* w, const Big384& a) {
  for (int i = 0; i < 12; i++) w[i] = a.w[i];
}
// big_mul_acc on an accumulator of NW words: in = [accumulator, a (NA words), b (NB words)]
template <int NW, int NA, int NB>
SPP_HD void mul_acc_case(const uint32_t* in, uint32_t* out) {
  uint32_t acc[NW], a[NA], b[NB];
  for (int i = 0; i < NW; i++) acc[i] = in[i];
  for (int i = 0; i < NA; i++) a[i] = in[NW + i];
  for (int i = 0; i < NB; i++) b[i] = in[NW + NA + i];
  big_mul_acc(acc, NW, a, NA, b, NB);
  for (int i = 0; i < NW; i++) out[i] = acc[i];
}
SPP_HD void glv_case(const uint32_t* in, uint32_t* out) {
  uint32_t kc[28], s[4], s1[4], s2[4];
  for (int i = 0; i < 28; i++) kc[i] = in[i];
  for (int i = 0; i < 4; i++) s[i] = in[28 + i];
  out[0] = dev_glv_split(kc, s, s1, s2) ? 1u : 0u;
  for (int i = 0; i < 4; i++) {
    out[1 + i] = s1[i];
    out[5 + i] = s2[i];
  }
}
SPP_HD void emul_case(const uint32_t* in, uint32_t* out) {
  uint32_t a[6][8], qc[16], kq[8], rem[8];
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 8; j++) a[i][j] = in[8 * i + j];
  for (int i = 0; i < 16; i++) qc[i] = in[48 + i];
  Big384 carry[6];
  dev_emulated_reduce<6, 6>(a, qc, kq, rem, carry);
  for (int i = 0; i < 8; i++) {
    out[i] = kq[i];
    out[8 + i] = rem[i];
  }
  for (int i = 0; i < 6; i++) {
    st_big(out + 16 + 12 * i, carry[i]);
    uint32_t c[8];
    fr_from_bigs(carry[i]).to_canonical(c);
    for (int j = 0; j < 8; j++) out[88 + 8 * i + j] = c[j];
  }
}
SPP_HD void grumpkin_case(const uint32_t* in, uint32_t* out) {
  uint32_t k[8];
  for (int i = 0; i < 8; i++) k[i] = in[i];
  Fr x = Fr::zero(), y = Fr::zero();   // what the solver stores when the result is the point at infinity
  out[0] = dev_grumpkin_mul(k, ld_fp<FrParams>(in + 8), &x, &y) ? 1u : 0u;
  st_fp(out + 1, x);
  st_fp(out + 9, y);
}
}  // namespace arith_probe

// One case of operation OP over the field Pm: `in` and `out` point at this case's words (arith_probe_shape).
template <uint32_t OP, class Pm>
SPP_HD void arith_probe_case(uint32_t arg, const uint32_t* in, uint32_t* out) {
  using namespace arith_probe;
  using B = Fp<Pm>;
  using F = F29<Pm>;
  if constexpr (OP == ARITH_FP_MUL) st_fp(out, ld_fp<Pm>(in) * ld_fp<Pm>(in + 8));
  else if constexpr (OP == ARITH_FP_SQR) st_fp(out, ld_fp<Pm>(in).sqr());
  else if constexpr (OP == ARITH_FP_ADD) st_fp(out, ld_fp<Pm>(in) + ld_fp<Pm>(in + 8));
  else if constexpr (OP == ARITH_FP_SUB) st_fp(out, ld_fp<Pm>(in) - ld_fp<Pm>(in + 8));
  else if constexpr (OP == ARITH_FP_NEG) st_fp(out, ld_fp<Pm>(in).neg());
  else if constexpr (OP == ARITH_FP_DBL) st_fp(out, ld_fp<Pm>(in).dbl());
  else if constexpr (OP == ARITH_FP_MUL_SMALL) st_fp(out, ld_fp<Pm>(in).mul_small(arg));
  else if constexpr (OP == ARITH_FP_INV) st_fp(out, ld_fp<Pm>(in).inv());
  else if constexpr (OP == ARITH_FP_INV_FERMAT) st_fp(out, ld_fp<Pm>(in).inv_fermat());
  else if constexpr (OP == ARITH_FP_TO_CANONICAL) {
    uint32_t c[8];
    ld_fp<Pm>(in).to_canonical(c);
    SPP_UNROLL for (int i = 0; i < 8; i++) out[i] = c[i];
  } else if constexpr (OP == ARITH_FP_FROM_U256) {
    uint32_t c[8];
    SPP_UNROLL for (int i = 0; i < 8; i++) c[i] = in[i];
    st_fp(out, B::from_u256(c));
  } else if constexpr (OP == ARITH_FP_IS_ZERO) out[0] = ld_fp<Pm>(in).is_zero() ? 1u : 0u;
  else if constexpr (OP == ARITH_FP_EQ) out[0] = (ld_fp<Pm>(in) == ld_fp<Pm>(in + 8)) ? 1u : 0u;
  else if constexpr (OP == ARITH_FQ2_MUL) st_fq2(out, ld_fq2(in) * ld_fq2(in + 16));
  else if constexpr (OP == ARITH_FQ2_SQR) st_fq2(out, ld_fq2(in).sqr());
  else if constexpr (OP == ARITH_FQ2_INV) st_fq2(out, ld_fq2(in).inv());
  else if constexpr (OP == ARITH_F29_FROM_WORDS) {
    uint32_t c[8];
    SPP_UNROLL for (int i = 0; i < 8; i++) c[i] = in[i];
    st_f29(out, F::from_words(c));
  } else if constexpr (OP == ARITH_F29_TO_WORDS) {
    uint32_t c[8];
    ld_f29<Pm>(in).to_words(c);
    SPP_UNROLL for (int i = 0; i < 8; i++) out[i] = c[i];
  } else if constexpr (OP == ARITH_F29_NORM) st_f29(out, ld_f29<Pm>(in).norm());
  else if constexpr (OP == ARITH_F29_MUL) st_f29(out, ld_f29<Pm>(in) * ld_f29<Pm>(in + 9));
  else if constexpr (OP == ARITH_F29_SQR) st_f29(out, ld_f29<Pm>(in).sqr());
  else if constexpr (OP == ARITH_F29_MUL2) st_f29(out, F::mul2(ld_f29<Pm>(in), ld_f29<Pm>(in + 9), ld_f29<Pm>(in + 18), ld_f29<Pm>(in + 27)));
  else if constexpr (OP == ARITH_F29_SUB_NORM_6P_1) st_f29(out, F::template sub_norm<Pm::SUBC_6P_1>(ld_f29<Pm>(in), ld_f29<Pm>(in + 9)));
  else if constexpr (OP == ARITH_F29_SUB_NORM_2P_1) st_f29(out, F::template sub_norm<Pm::SUBC_2P_1>(ld_f29<Pm>(in), ld_f29<Pm>(in + 9)));
  else if constexpr (OP == ARITH_F29_SUB3_NORM_4P_3)
    st_f29(out, F::template sub3_norm<Pm::SUBC_4P_3>(ld_f29<Pm>(in), ld_f29<Pm>(in + 9), ld_f29<Pm>(in + 18)));
  else if constexpr (OP == ARITH_F29_SUB_LAZY_6P_1) st_f29(out, F::template sub_lazy<Pm::SUBC_6P_1>(ld_f29<Pm>(in), ld_f29<Pm>(in + 9)));
  else if constexpr (OP == ARITH_F29_NEG_LAZY_2P_1) st_f29(out, F::template neg_lazy<Pm::SUBC_2P_1>(ld_f29<Pm>(in)));
  else if constexpr (OP == ARITH_F29_NEG_LAZY_4P_1) st_f29(out, F::template neg_lazy<Pm::SUBC_4P_1>(ld_f29<Pm>(in)));
  else if constexpr (OP == ARITH_F29_ADD_NORM) st_f29(out, add_norm(ld_f29<Pm>(in), ld_f29<Pm>(in + 9)));
  else if constexpr (OP == ARITH_F29_ADD_LAZY) st_f29(out, add_lazy(ld_f29<Pm>(in), ld_f29<Pm>(in + 9)));
  else if constexpr (OP == ARITH_F29_IS_ZERO_MOD_P_7) out[0] = ld_f29<Pm>(in).template is_zero_mod_p<7>() ? 1u : 0u;
  else if constexpr (OP == ARITH_F29_IS_ZERO_MOD_P_3) out[0] = ld_f29<Pm>(in).template is_zero_mod_p<3>() ? 1u : 0u;
  else if constexpr (OP == ARITH_F29_FROM_FP) st_f29(out, F::from_fp(ld_fp<Pm>(in)));
  else if constexpr (OP == ARITH_F29_TO_FP) st_fp(out, ld_f29<Pm>(in).to_fp());
  else if constexpr (OP == ARITH_F29_SCALED_TO_FP) st_fp(out, ld_f29<Pm>(in).scaled_to_fp());
  else if constexpr (OP == ARITH_F29X2_MUL || OP == ARITH_F29X2_SQR) {
    constexpr bool sq = OP == ARITH_F29X2_SQR;
    if (arg == 2) f29x2_case<FqParams::SUBC_2P_1>(sq, in, out);
    else if (arg == 4) f29x2_case<FqParams::SUBC_4P_1>(sq, in, out);
    else if (arg == 6) f29x2_case<FqParams::SUBC_6P_1>(sq, in, out);
    else f29x2_case<FqParams::SUBC_8P_1>(sq, in, out);
  } else if constexpr (OP == ARITH_SCRIPT_G1_29) script29<XYZZ29<FqParams>, G1Affine, false>(in, out);
  else if constexpr (OP == ARITH_SCRIPT_G1_29_DISTINCT) script29<XYZZ29<FqParams>, G1Affine, true>(in, out);
  else if constexpr (OP == ARITH_SCRIPT_G1) script_plain<G1XYZZ, G1Affine>(in, out);
  else if constexpr (OP == ARITH_SCRIPT_G2_29) script29<XYZZ29G2, G2Affine, false>(in, out);
  else if constexpr (OP == ARITH_SCRIPT_G2_29_DISTINCT) script29<XYZZ29G2, G2Affine, true>(in, out);
  else if constexpr (OP == ARITH_SCRIPT_G2) script_plain<G2XYZZ, G2Affine>(in, out);
  else if constexpr (OP == ARITH_HINT_GLV_SPLIT) glv_case(in, out);
  else if constexpr (OP == ARITH_HINT_EMUL_REDUCE) emul_case(in, out);
  else if constexpr (OP == ARITH_HINT_GRUMPKIN_MUL) grumpkin_case(in, out);
  else if constexpr (OP == ARITH_BIGS_ADD || OP == ARITH_BIGS_SUB || OP == ARITH_BIGS_ADD_SMALL_MUL) {
    Big384 a = ld_big(in);
    const Big384 b = ld_big(in + 12);
    if constexpr (OP == ARITH_BIGS_ADD) a.add(b);
    else if constexpr (OP == ARITH_BIGS_SUB) a.sub(b);
    else a.add_small_mul(b, (int)(int16_t)(uint16_t)arg);
    st_big(out, a);
  } else if constexpr (OP == ARITH_BIGS_NEGATE || OP == ARITH_BIGS_SAR64) {
    Big384 a = ld_big(in);
    if constexpr (OP == ARITH_BIGS_NEGATE) a.negate();
    else a.sar64();
    st_big(out, a);
  } else if constexpr (OP == ARITH_BIGS_LT) out[0] = ld_big(in).lt(ld_big(in + 12)) ? 1u : 0u;
  else if constexpr (OP == ARITH_BIGS_LOW64_ZERO) out[0] = ld_big(in).low64_zero() ? 1u : 0u;
  else if constexpr (OP == ARITH_BIG_MUL_ACC_4X4_12) mul_acc_case<12, 4, 4>(in, out);
  else if constexpr (OP == ARITH_BIG_MUL_ACC_2X2_12) mul_acc_case<12, 2, 2>(in, out);
  else if constexpr (OP == ARITH_BIG_MUL_ACC_8X8_8) mul_acc_case<8, 8, 8>(in, out);
}

}  // namespace spp
