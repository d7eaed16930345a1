// Lookup-inverse wires of a circuit and how their share of an MSM is summed by byte bucket (kernels_msm_lookup.hip).
//
// Builder::finalize_lookups (circuit.cpp) proves every 8-bit range check with a log-derivative argument: lookup i gets a wire
// inv_i = 1 / (X - v_i), X the challenge wire, v_i the looked-up value (hint row h0 + i of OP_COUNT8).  Such a wire is a full-size
// scalar -- 16 additions in a 16-bit table walk -- but within one proof the 6 464 of them in the audit circuit take at most 256
// distinct values INV[t] = 1 / (X - t).  For a base set S
//     sum_i inv_i * S_i  =  sum_{t < 256} INV[t] * Bkt_t,     Bkt_t = sum_{i : v_i = t} S_i
// so the bases are added ONCE each into 256 buckets per proof (first level) and the 256 buckets take a variable-base sum with
// shared doublings (second level): signed LKB_C-bit windows, per window the classic bucket accumulation and running sum, the
// window sums put together by k_msm_horner.  The digit planes of the set hold zero for these bases (MSM_ROW_ZERO), which the flat
// walk skips.  The sums are the same group elements, the proofs the same bytes.
//
// Soundness of the bucket index: the hint rows of OP_COUNT8 are the values the circuit range-checks; a row in which one of them is
// no byte is refused through its status word by the satisfaction check, whatever is summed here -- the index only has to stay
// inside the bucket array (the rule of `mag <= blk.E` in msm_flat_walk).
//
// Host and device: the scan reads circuit.hpp only; the recoding and the window sum are SPP_HD so that a host program can pin
// them against an independent sum (tests/host/msm_lookup_check.cpp).
#pragma once
#include <map>
#include "msm_classes.hpp"

namespace spp {

static constexpr uint32_t LKB_VALUES = 256;                            // buckets of the first level: the looked-up byte
static constexpr uint32_t LKB_C = 5;                                   // window bits of the second level
static constexpr uint32_t LKB_WINDOWS = (254 + LKB_C - 1) / LKB_C;     // 51 (the folded magnitude is below 2^253: no carry out of the top)
static constexpr uint32_t LKB_BUCKETS = 1u << (LKB_C - 1);             // 16: digit magnitudes 1 .. 16
static constexpr uint32_t LKB_SLICES = 8;                              // first level: lanes per proof, each with its own 256 buckets
// Default smallest batch that takes the path (SPP_LOOKUP_BUCKETS=N sets another, 0 turns the path off).  The first level runs
// LKB_SLICES * P lanes, each a chain of L / LKB_SLICES additions through memory: at 1024 proofs that is 128 waves per set, half a
// wave per CU.  Below it the chain is pure latency in front of a pipeline that is latency-bound already (the cooperative solver
// serves batches up to 1024), and the additions saved shrink with P while the launches do not.
static constexpr uint32_t LKB_MIN_BATCH = 1024;
// Fewest lookup-inverse wires for which a circuit takes the path by default (SPP_LOOKUP_BUCKETS=N takes it for any).  A wire saves
// 32 mixed additions per proof (16 in A, 16 in K) and costs 2 in the first level; the fold and the second level cost 2 x 16.5 K
// general additions per proof whatever L is, written with the plain Montgomery products of bn254.hpp -- about three times the
// instructions of the walk's 9x29 addition.  The two meet near 3 800 wires: the audit circuit has 6 464, the withdraw circuit 8.
static constexpr uint32_t LKB_MIN_LOOKUPS = 4096;
static constexpr uint32_t MSM_ROW_ZERO = 0xffffffffu;                  // rows[] entry of a base whose digits are zero (k_msm_digits)

struct LookupInverse {
  uint32_t wire;   // inv = 1 / (X - H_hint)
  uint32_t hint;   // row of H
};

// The lookup-inverse wires of a circuit, in program order.  Row k of an OP_BATCH_DIV range qualifies when
//   * its A row is one wire with coefficient 1 (the wire the division writes),
//   * its C row is the constant one,
//   * its B row is X - H_h as a linear form, X the challenge wire, h the hint row of the preceding OP_COUNT8 at the row's own
//     position in the range (finalize_lookups emits the divisions in the order of the hint rows).
// A program with an instruction this scan does not know (the solver of a decoded gnark system, an ACIR program) yields none.
inline std::vector<LookupInverse> msm_lookup_inverses(const Circuit& circ) {
  std::vector<LookupInverse> out;
  const std::vector<uint32_t>& pr = circ.program;
  const uint32_t X = circ.challenge_wire;
  if (X == 0 || X >= circ.n_wires) return out;
  std::vector<uint8_t> seen(circ.n_wires, 0);
  uint32_t h0 = 0, nh = 0;
  auto is_one = [&](uint32_t ci) { return ci < circ.coeffs.size() && circ.coeffs[ci] == Fr::one(); };
  auto qualifies = [&](uint32_t k, uint32_t h, uint32_t* wire) {
    if (k >= circ.A.rows() || k >= circ.B.rows() || k >= circ.C.rows() || h >= circ.H.rows()) return false;
    const Term* a = circ.A.terms.data() + circ.A.rowptr[k];
    const Term* c = circ.C.terms.data() + circ.C.rowptr[k];
    if (circ.A.rowptr[k + 1] - circ.A.rowptr[k] != 1 || a->wire == 0 || a->wire >= circ.n_wires || a->wire == X || !is_one(a->coeff)) return false;
    if (circ.C.rowptr[k + 1] - circ.C.rowptr[k] != 1 || c->wire != 0 || !is_one(c->coeff)) return false;
    std::map<uint32_t, Fr> form;   // B_k + H_h - X, which must vanish
    auto acc = [&](const Sparse& m, uint32_t row) {
      for (uint32_t t = m.rowptr[row]; t < m.rowptr[row + 1]; t++) {
        if (m.terms[t].coeff >= circ.coeffs.size()) return false;
        auto it = form.emplace(m.terms[t].wire, Fr::zero()).first;
        it->second = it->second + circ.coeffs[m.terms[t].coeff];
      }
      return true;
    };
    if (!acc(circ.B, k) || !acc(circ.H, h)) return false;
    if (form.count(a->wire)) return false;   // the value may not depend on the wire it defines
    auto it = form.emplace(X, Fr::zero()).first;
    it->second = it->second - Fr::one();
    for (const auto& e : form)
      if (!e.second.is_zero()) return false;
    *wire = a->wire;
    return true;
  };
  for (size_t pc = 0; pc < pr.size() && pr[pc] != OP_END;) {
    size_t len = 0;
    switch (pr[pc]) {
      case OP_SOLVE_C: case OP_SOLVE_A: case OP_MASK: len = 2; break;
      case OP_BATCH_DIV: case OP_POSEIDON2: case OP_INV_H: len = 3; break;
      case OP_COUNT8: case OP_BITS: case OP_LIMBS8: case OP_POSEIDON: len = 4; break;
      case OP_COMMIT: len = 1; break;
      case OP_GRUMPKIN: len = pc + 4 < pr.size() ? 5 + (size_t)pr[pc + 4] : 0; break;
      default: return {};
    }
    if (len == 0 || pc + len > pr.size()) return {};
    if (pr[pc] == OP_COUNT8) { h0 = pr[pc + 1]; nh = pr[pc + 2]; }
    if (pr[pc] == OP_BATCH_DIV)
      for (uint32_t i = 0; i < pr[pc + 2] && i < nh; i++) {
        uint32_t w;
        if (qualifies(pr[pc + 1] + i, h0 + i, &w) && !seen[w]) {
          seen[w] = 1;
          out.push_back({w, h0 + i});
        }
      }
    pc += len;
  }
  return out;
}

// Signed LKB_C-bit digits of a scalar, least significant first: s = sign-folded sum_j dig[j] * 2^(LKB_C * j), |dig[j]| <= LKB_BUCKETS.
// A scalar above (r - 1) / 2 is recoded as its negative with every digit negated, as k_msm_digits does.
SPP_HD void lkb_recode(const Fr& s, int8_t dig[LKB_WINDOWS]) {
  uint32_t l[8];
  s.to_canonical(l);
  const bool neg = canonical_gt_half<FrParams>(l);
  if (neg) {
    uint32_t t[8];
    canonical_negate<FrParams>(l, t);
    for (int k = 0; k < 8; k++) l[k] = t[k];
  }
  const uint32_t mask = (1u << LKB_C) - 1u;
  uint32_t carry = 0;
  for (uint32_t j = 0; j < LKB_WINDOWS; j++) {
    const uint32_t d = (l[0] & mask) + carry;
    for (int k = 0; k < 7; k++) l[k] = (l[k] >> LKB_C) | (l[k + 1] << (32 - LKB_C));
    l[7] >>= LKB_C;
    const bool over = d > LKB_BUCKETS;
    const int v = over ? (int)d - (int)(1u << LKB_C) : (int)d;
    carry = over ? 1u : 0u;
    dig[j] = (int8_t)(neg ? -v : v);
  }
}

// One window of the second level: sum_t digit(t) * point(t) over the LKB_VALUES terms.  bkt[b * stride], b < LKB_BUCKETS, is
// scratch of the caller's: term t goes into bucket |digit| - 1 with the digit's sign, then sum_b (b + 1) * bkt[b] by the running
// sum -- LKB_VALUES + 2 * LKB_BUCKETS complete additions at the most.
template <class Digit, class Point>
SPP_HD XYZZ<Fq> lkb_window_sum(XYZZ<Fq>* bkt, size_t stride, Digit digit, Point point) {
  for (uint32_t b = 0; b < LKB_BUCKETS; b++) bkt[b * stride] = XYZZ<Fq>::infinity();
  for (uint32_t t = 0; t < LKB_VALUES; t++) {
    const int d = digit(t);
    if (d == 0) continue;
    XYZZ<Fq> q = point(t);
    if (q.is_inf()) continue;
    if (d < 0) q.Y = q.Y.neg();
    const uint32_t b = (uint32_t)(d < 0 ? -d : d) - 1;
    if (b >= LKB_BUCKETS) continue;   // lkb_recode never makes one
    XYZZ<Fq> a = bkt[b * stride];
    a.add(q);
    bkt[b * stride] = a;
  }
  XYZZ<Fq> running = XYZZ<Fq>::infinity(), acc = XYZZ<Fq>::infinity();
  for (uint32_t b = LKB_BUCKETS; b-- > 0;) {
    running.add(bkt[b * stride]);
    acc.add(running);
  }
  return acc;
}

}  // namespace spp
