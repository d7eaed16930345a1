// Host-side planning of the table-walk MSM (msm_table.hpp): windows, the two padding rules, buffer sizes and the lane layout of
// a launch.  Standard library only -- any host compiler builds it (tests/host/msm_plan_check.cpp pins every function here against
// tests/golden/msm_plan.json).  Nothing here reads the environment: the tuning is an argument.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace spp {

inline uint32_t msm_windows(uint32_t c) { return (254 + c - 1) / c; }

// Proofs per slice row of the digit planes and of a launch: P rounded up to a wave, so that a wave never straddles two slices
// (batches below 64 proofs keep P: there every lane is its own (slice, proof) anyway).  The digit kernel and the walks index the
// planes with it: the one spelling of the rule.
inline uint32_t msm_padded_batch(uint32_t P) { return P >= 64 ? (P + 63) / 64 * 64 : P; }
// Rows of the table of N bases with Wt rows each, including the padding of the last 64-row block (the table layout groups rows in
// blocks of 64, msm_table.hpp).
inline size_t msm_table_rows(size_t N, uint32_t Wt) { return ((N * Wt + 63) / 64) * 64; }
// number of table elements (points) for N bases with Wt window rows each
inline size_t msm_table_elems(uint32_t N, uint32_t c, uint32_t Wt) {
  if (Wt == 0 || Wt > msm_windows(c)) Wt = msm_windows(c);
  return msm_table_rows(N, Wt) * ((size_t)1 << (c - 1));
}
// int16 digits of N scalars of P proofs: W planes of N rows of Pp
inline size_t msm_digit_elems(uint32_t N, uint32_t P, uint32_t c) { return (size_t)msm_windows(c) * N * msm_padded_batch(P); }

// Rounds of resident waves a launch of the flat walk aims at (msm_plan).  SPP_MSM_WAVES and SPP_MSM_WAVES_SMALL override the two
// figures; they are read when a circuit is loaded (Switches, spp_circuit.hpp).
struct MsmTuning {
  uint32_t rounds = 4;         // batches above 256 proofs
  uint32_t rounds_small = 2;   // batches up to 256 proofs
};
// the values of the two variables (nullptr: unset) with their clamps: 1..16, else 4; 1..64, else 2
inline MsmTuning msm_tuning_from_env(const char* waves, const char* waves_small) {
  MsmTuning t;
  const int v = waves ? atoi(waves) : 4, vs = waves_small ? atoi(waves_small) : 2;
  t.rounds = (uint32_t)(v >= 1 && v <= 16 ? v : 4);
  t.rounds_small = (uint32_t)(vs >= 1 && vs <= 64 ? vs : 2);
  return t;
}

struct MsmPlan {
  uint32_t W;        // windows per scalar
  uint32_t Wt, R;    // table rows per base, passes
  uint32_t Q, Wq;    // small batches: Q lanes share the rows of a base, Wq rows each
  uint32_t Sg;       // slices of the item range per pass
  uint32_t Pp;       // proofs per slice row: msm_padded_batch(P)
  size_t partial_elems(uint32_t P) const { return (size_t)R * Sg * P; }
  // fewer slices until the partial sums of a P-proof launch fit a buffer of `cap` elements (msm_partial_cap sizes the buffer so
  // that this does nothing at the batch sizes it was sized for)
  void fit(uint32_t P, size_t cap) {
    while (Sg > 1 && partial_elems(P) > cap) Sg--;
  }
};

// Lane layout of one launch.  Big batches: the chip holds 1024 SIMDs x `occ` waves of this kernel at a time (MsmWalk<F>::
// waves_per_simd, kernels.hpp); the waves of a launch take about the same time each, so a launch of w waves
// runs ceil(w / capacity) rounds and the last, partly filled round costs a whole one.  Sg is therefore searched around
// tuning.rounds (default 4) rounds for the value that fills its last round best (17 passes x 8 slices x 32 waves were 2.125
// rounds: the 15-bit sets ran 12 % slower per addition than the 16-bit ones until this was done).  At least 4 bases per slice.
// Small batches (a single proof is the drop-in generateProof case): when that cannot give ~64K lanes the table windows of a base
// are shared by up to 8 lanes (Q chunks of >= 4 windows) and a slice may be a single (base, chunk) item.
inline MsmPlan msm_plan(uint32_t N, uint32_t P, uint32_t c, uint32_t Wt, uint32_t occ, const MsmTuning& tuning) {
  MsmPlan pl{};
  pl.W = msm_windows(c);
  if (Wt == 0 || Wt > pl.W) Wt = pl.W;
  pl.Wt = Wt;
  pl.R = (pl.W + Wt - 1) / Wt;
  pl.Pp = msm_padded_batch(P);
  pl.Q = 1;
  const uint64_t lanes_per_slice = (uint64_t)(pl.Pp ? pl.Pp : 1) * pl.R;
  while ((uint64_t)((N + 3) / 4) * pl.Q * lanes_per_slice < 65536 && pl.Q < 8 && (Wt + 2 * pl.Q - 1) / (2 * pl.Q) >= 4) pl.Q *= 2;
  pl.Wq = (Wt + pl.Q - 1) / pl.Q;
  uint64_t S, maxS;
  if (pl.Q > 1) {
    S = (65536 + lanes_per_slice - 1) / lanes_per_slice;
    maxS = (uint64_t)N * pl.Q;
  } else {
    maxS = std::max<uint64_t>((N + 3) / 4, 1);
    const double cap = 1024.0 * (occ ? occ : 1);                       // resident waves
    const double wps = (double)lanes_per_slice / 64.0;                  // waves per slice (all passes)
    // small batches (P <= 256): TWO rounds.  Round 3's first guess was the opposite -- three times as many rounds, so that the short
    // kernels of the other batches in flight find free SIMDs sooner -- but every slice ends in a 128-byte partial sum per lane that
    // the folds read again: with the radix-8 folds and four batches in flight, 128-proof audit batches measure 25.0 ms per step
    // at 12 rounds, 24.5 at 4, 23.6 at 2, 24.1 at 1 (one box, profiles/rehearsal_probe.py)
    const uint32_t rnd = P <= 256 ? tuning.rounds_small : tuning.rounds;
    const uint64_t S0 = std::max<uint64_t>(1, (uint64_t)(rnd * cap / wps + 0.5));
    uint64_t lo = std::max<uint64_t>(1, S0 - S0 / 4), hi = S0 + S0 / 2;
    lo = std::min(lo, maxS);
    hi = std::min(hi, maxS);
    S = lo;
    double best = -1;
    for (uint64_t s = lo; s <= hi; s++) {
      const double r = s * wps / cap, eff = r / std::ceil(r - 1e-9);
      if (eff > best + 1e-6) { best = eff; S = s; }
    }
  }
  if (maxS == 0) maxS = 1;
  if (S > maxS) S = maxS;
  if (S == 0) S = 1;
  pl.Sg = (uint32_t)S;
  return pl;
}

// Elements of the partial-sum buffer of a workspace sized for batches of up to P proofs.  R * Sg(P') * P' <= lane target + R * P'
// for every P' <= P (msm_plan); small batches: up to 64K (item, pass) lanes -- the floor -- and the exact need at P and its
// halvings, the sizes most likely to be used.  A launch at another size that would need more loses slices (MsmPlan::fit).
inline size_t msm_partial_cap(uint32_t N, size_t P, uint32_t c, uint32_t Wt, uint32_t occ, const MsmTuning& tuning) {
  const uint32_t R = msm_plan(N, (uint32_t)P, c, Wt, occ, tuning).R;
  size_t cap = (size_t)256 * 4 * 8 * 64 + 65536 + (size_t)(R + 1) * (P + 64);
  for (size_t q = P; q >= 1; q /= 2) cap = std::max(cap, msm_plan(N, (uint32_t)q, c, Wt, occ, tuning).partial_elems((uint32_t)q));
  return cap;
}

}  // namespace spp
