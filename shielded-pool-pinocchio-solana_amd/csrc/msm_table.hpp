// Fixed-base multi-scalar multiplication for batched Groth16 proving on gfx950.
//
// Replaces the Pippenger MSMs of gnark's Prove: Ar / Bs1 / Krs over pk.G1.{A,B,K,Z},
// Bs over pk.G2.B, and the BSB22 Pedersen commitment + proof of knowledge. In the reference these run
// inside `sunspot prove` (client/proof.helper.ts:64) on CPU threads, one proof at a time.
//
// MI355X design: the proving key is constant across a batch and there are 288 GB of HBM, so every base
// carries a precomputed table of its multiples (affine, signed c-bit digits: 2^(c-1) entries per row; fewer for a base of the
// throughput layout whose scalar the circuit bounds to a bit or a byte, msm_ragged.hpp).  An MSM
// then needs no buckets, no sorting and no bucket reduction: each lane owns one proof of the batch and folds
// +-T[base][|digit|] into a private XYZZ accumulator with mixed additions (8M+2S).  The scalars are recoded once
// into int16 digit planes (k_msm_digits); all 64 lanes of a wave walk the SAME (base, window) sequence, so digit
// loads are one coalesced row, table gathers hit one 2^(c-1)*64 B segment, control flow is uniform, and windows in
// which every proof has a zero digit (bits, bytes, small signed noise -- most of the audit witness) are skipped for
// the whole wave.  Under the HBM budget a base keeps ONE row (16-bit windows, 2 MB per G1 base) and the 16 windows
// of a scalar become 16 passes over the same table whose sums are put together by Horner (k_msm_horner); with
// explicit small windows every window has its own row and there is a single pass.  Work is split over passes and
// slices of the base range to fill 256 CUs; the slice sums of every (pass, proof) are folded pairwise.
//
// This header holds every kernel of the walk that is a template over the coordinate field F, with its launcher.  Two translation
// units instantiate it: kernels_msm.hip for Fq (G1), built with the scheduler strategy max-ilp -- the G1 walk was 2 % faster for
// it (measured when it took 203 registers); its additions are written with product-scanning Montgomery products (F29_SCAN,
// f29.hpp), whose serial chains that scheduler interleaves: 144 registers, three waves per SIMD -- and kernels_msm_g2.hip for Fq2
// (G2) with the default scheduler: max-ilp made the G2 walk spill and 4 % slower when it ran one wave per SIMD; with the column
// products it keeps (201 registers, two waves per SIMD) a headline run with the unit under max-ilp and scanning products measured
// the same as without (profiles/README.md), so the unit's flags stay.  What differs between the two walks is MsmWalk<F>
// (kernels.hpp); the host-side planning is msm_plan.hpp.
#pragma once
#include <hip/hip_ext.h>
#include "kernels.hpp"
#include <algorithm>
#include "f29.hpp"

namespace spp {

static constexpr unsigned MSM_FOLD_COOP_MAX_BATCH = 8;   // batches up to this size fold their slice sums with 8 lanes per output
static constexpr unsigned MSM_WALK_BLOCK = 64;           // lanes per workgroup of the flat table walk (one wave: see k_msm_flat)

// ----------------------------------------------------------------------------------------------------
// table construction: one lane per (base, window) row.
// Table layout: rows are grouped in blocks of 64; entry d of row `row` lives at (off_{row/64} + d)*64 + row%64, so the
// 64 lanes of a wave that build 64 consecutive rows write 64 consecutive points (coalesced 4 KiB per step), and so do
// the XYZZ temporaries.  The MSM kernels gather single entries at random d anyway, so they lose nothing.
// Uniform layout (row-per-window tables, single-base tables; blocks = nullptr): every block holds E = 2^(c-1) entries per row,
// off_b = b*E.  Ragged layout (the flat sets, msm_ragged.hpp): block b holds E_b entries per row -- 2^(c-1) if one of its bases
// has a full-range scalar, else what the range class of its bases needs (1 for bits, 256 for bytes) -- and starts at blocks[b].off.
// A launch builds blocks of ONE length E.
// ----------------------------------------------------------------------------------------------------
template <class F>
__global__ void __launch_bounds__(64) k_build_table(const Affine<F>* __restrict__ bases, uint32_t N, uint32_t E, uint32_t Wn,
                                                    uint32_t step_bits, uint32_t row0, uint32_t nrows, Affine<F>* __restrict__ table,
                                                    XYZZ<F>* __restrict__ tmp, F* __restrict__ tmp_pre, const MsmBlock* __restrict__ blocks) {
  const uint32_t rl = blockIdx.x * blockDim.x + threadIdx.x;   // row within this launch (row0 is a multiple of 64)
  if (rl >= nrows) return;
  const uint32_t row = row0 + rl;
  const size_t off = blocks ? (size_t)blocks[row >> 6].off : (size_t)(row >> 6) * E;
  Affine<F>* out = table + off * 64 + (row & 63);                         // entry d at out[d * 64]
  XYZZ<F>* t = tmp + rl;                                                  // entry d at t[d * nrows]
  F* pre = tmp_pre + rl;
  if (row >= N * Wn) {   // padding rows of the last block
    for (uint32_t d = 0; d < E; d++) out[(size_t)d * 64] = Affine<F>::infinity();
    return;
  }
  const uint32_t i = row / Wn, j = row % Wn;
  Affine<F> base = bases[i];
  if (base.is_inf()) {
    for (uint32_t d = 0; d < E; d++) out[(size_t)d * 64] = Affine<F>::infinity();
    return;
  }
  XYZZ<F> b = XYZZ<F>::from_affine(base);
  for (uint32_t k = 0; k < step_bits * j; k++) b.dbl_inplace();
  Affine<F> bj = b.to_affine();
  XYZZ<F> acc = XYZZ<F>::from_affine(bj);
  F prod = F::one();
  for (uint32_t d = 0; d < E; d++) {
    t[(size_t)d * nrows] = acc;
    pre[(size_t)d * nrows] = prod;
    prod = prod * (acc.ZZ * acc.ZZZ);
    acc.madd(bj);
  }
  F inv = prod.inv();
  for (uint32_t d = E; d-- > 0;) {
    XYZZ<F> q = t[(size_t)d * nrows];
    F I = inv * pre[(size_t)d * nrows];
    inv = inv * (q.ZZ * q.ZZZ);
    F izz = I * q.ZZZ;
    F izzz = I * q.ZZ;
    out[(size_t)d * 64] = {q.X * izz, q.Y * izzz};
  }
}
template <class F>
void launch_build_table(hipStream_t st, const Affine<F>* bases, uint32_t N, uint32_t c, uint32_t Wt, uint32_t row0, uint32_t nrows,
                        Affine<F>* table, XYZZ<F>* tmp, F* tmp_pre, const MsmBlock* blocks, uint32_t E) {
  if (nrows == 0) return;
  const uint32_t W = msm_windows(c);
  if (Wt == 0 || Wt > W) Wt = W;
  const uint32_t R = (W + Wt - 1) / Wt;   // row m of a base holds the multiples of 2^(c*R*m) * Base (pass rho takes windows rho + R*m)
  if (!blocks) E = 1u << (c - 1);
  hipLaunchKernelGGL(k_build_table<F>, dim3((nrows + 63) / 64), dim3(64), 0, st, bases, N, E, Wt, c * R, row0, nrows, table, tmp, tmp_pre, blocks);
}

// ----------------------------------------------------------------------------------------------------
// signed-window recoding helpers (scalar in canonical limbs, magnitude < 2^253 after sign folding)
// ----------------------------------------------------------------------------------------------------
struct Recoder {
  uint32_t l[8];
  uint32_t carry;
  bool neg;
  __device__ __forceinline__ void init(const Fr& s) {
    uint32_t cl[8];
    s.to_canonical(cl);
    neg = canonical_gt_half<FrParams>(cl);
    if (neg) {
      canonical_negate<FrParams>(cl, l);
    } else {
      SPP_UNROLL for (int k = 0; k < 8; k++) l[k] = cl[k];
    }
    carry = 0;
  }
  // next window: returns magnitude (0..2^(c-1)) and sign (true = subtract)
  __device__ __forceinline__ uint32_t next(uint32_t c, bool& sgn) {
    const uint32_t mask = (1u << c) - 1u, half = 1u << (c - 1);
    uint32_t d = (l[0] & mask) + carry;
    SPP_UNROLL for (int k = 0; k < 7; k++) l[k] = (l[k] >> c) | (l[k + 1] << (32 - c));
    l[7] >>= c;
    if (d > half) {
      d = (1u << c) - d;
      carry = 1;
      sgn = !neg;
    } else {
      carry = 0;
      sgn = neg;
    }
    return d;
  }
};

// ----------------------------------------------------------------------------------------------------
// MSM accumulate over the digit planes.
//
// Window passes.  A base carries Wt table rows; row m holds the multiples (d+1) * 2^(c*R*m) * Base with R = ceil(W / Wt).
// Pass rho (0 <= rho < R) adds up  T[i][m][digit_{rho + R*m}]  over every base and row: sum_rho.  The MSM is
// sum_rho 2^(c*rho) * sum_rho, put together per proof by k_msm_horner (c doublings per pass, once per proof and set, not per
// base).  Wt = W (R = 1) is the classic layout, every window its own row -- small tables (8-bit windows) for the one-proof
// latency path, no Horner step.  Wt = 1 (R = W) is the throughput layout chosen under the HBM budget: ONE row of 2^(c-1)
// multiples per base, so for the same bytes the window is log2(W) bits wider than with a row per window -- 16-bit windows
// (16 additions per full-size scalar) where the classic layout affords 11-12 bits (22-24 additions).
//
// Lane g -> (t = g / Pp, p = g % Pp), t -> (pass rho = t / Sg, slice t % Sg); Pp = P rounded up to 64 so that a wave never
// straddles two slices (batches below 64 proofs keep Pp = P: there every lane is its own (slice, proof) anyway).  All
// lanes of a wave walk the same (base, window) sequence: digit loads are one coalesced 128 B row, a (base, window) in which
// every proof of the wave has a zero digit (bits, bytes, small signed noise -- most of the audit witness above window 0)
// is skipped for the whole wave.
// ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool words_all_zero(const Fq& v) {
  uint32_t o = 0;
  SPP_UNROLL for (int i = 0; i < 8; i++) o |= v.l[i];
  return o == 0;
}
// accumulator used by the table walk: G1 and G2 run on the unsaturated 9x29-bit form (f29.hpp)
// FORM (F29Form, f29.hpp): how the products of an addition are written -- MsmWalk<F>::product_form in the fast flat walk, the
// column form everywhere else
template <class F, int FORM = F29_COLUMNS>
struct MsmAcc;
template <int FORM>
struct MsmAcc<Fq, FORM> {
  XYZZ29<FqParams, FORM> a;
  __device__ __forceinline__ void init() { a = XYZZ29<FqParams, FORM>::infinity(); }
  __device__ __forceinline__ void madd(const Affine<Fq>& e, bool sgn) {
    if (words_all_zero(e.x) && words_all_zero(e.y)) return;   // table row of an infinity base (spp_msm_g1 callers)
    a.madd(e, sgn);
  }
  // false: the entry has the accumulator's x, nothing was added (XYZZ29::madd_distinct)
  __device__ __forceinline__ bool madd_distinct(const Affine<Fq>& e, bool sgn) {
    if (words_all_zero(e.x) && words_all_zero(e.y)) return true;
    return a.madd_distinct(e, sgn);
  }
  __device__ __forceinline__ XYZZ<Fq> result() const { return a.to_xyzz(); }
};

template <int FORM>
struct MsmAcc<Fq2, FORM> {
  XYZZ29G2F<FORM> a;
  __device__ __forceinline__ void init() { a = XYZZ29G2F<FORM>::infinity(); }
  __device__ __forceinline__ void madd(const Affine<Fq2>& e, bool sgn) {
    if (words_all_zero(e.x.c0) && words_all_zero(e.x.c1) && words_all_zero(e.y.c0) && words_all_zero(e.y.c1)) return;
    a.madd(e, sgn);
  }
  __device__ __forceinline__ bool madd_distinct(const Affine<Fq2>& e, bool sgn) {
    if (words_all_zero(e.x.c0) && words_all_zero(e.x.c1) && words_all_zero(e.y.c0) && words_all_zero(e.y.c1)) return true;
    return a.madd_distinct(e, sgn);
  }
  __device__ __forceinline__ XYZZ<Fq2> result() const { return a.to_xyzz(); }
};


// throughput layout (Wt = 1): one table row per base, slice sl takes bases sl, sl + Sg, ... (neighbouring wires have similar
// scalar sizes -- runs of bits, runs of hash states -- so a strided split gives every slice the same mix).  The digits of
// four bases are fetched ahead of their additions (2 B each, packed into one register pair).
//
// The same-x case is not in the loop.  A mixed addition whose entry has the accumulator's x is a doubling or a cancellation: the
// entry is +-(the sum so far), which a proving key produces by coincidence or with duplicate bases only.  Inline, that path
// (to_xyzz, dbl_inplace, from_xyzz) never ran and still set the register budget of the whole loop: 203 VGPRs for G1, and for G2
// 256 VGPRs + 242 AGPRs, one wave per SIMD.  The fast walk adds with madd_distinct (f29.hpp): a lane whose addition is refused
// leaves the loop and stores the redo marker in place of its slice sum; k_msm_flat_redo, launched behind every fast walk, sums the
// slices of marked lanes again with the complete addition and returns at once for every other lane.  Register counts and what
// the two walks gained: profiles/walk_redo_resources.txt, DESIGN 8.1.
//
// Redo marker: the all-zero XYZZ<F>.  No slice sum is all zero: infinity is stored as (1, 1, 0, 0) with the non-zero words of
// F::one() in X, and a finite sum has ZZ != 0 mod p, hence a non-zero word in ZZ (to_xyzz stores residues, zero words only for the
// residue 0).  The marker test reads X and ZZ.
//
// One wave per workgroup (MSM_WALK_BLOCK): a 256-lane workgroup needs FOUR free wave slots of a CU at once, and with 2 slots per SIMD
// and waves of unequal length (passes over sparse windows are shorter) a finished wave's slot waited for three more -- 1.79 resident
// waves per SIMD on average where 2 fit (measured when the G1 walk was bounded to two waves).
// The second launch bound, MsmWalk<F>::waves_per_simd, is the register budget of both kernels; the planner reads the same figure.
template <class F>
__device__ __forceinline__ void msm_store_redo_marker(XYZZ<F>* out) {
  static_assert(sizeof(XYZZ<F>) % 16 == 0, "stored as 16-byte words");
  uint4* w = reinterpret_cast<uint4*>(out);
  SPP_UNROLL for (uint32_t i = 0; i < sizeof(XYZZ<F>) / 16; i++) w[i] = make_uint4(0, 0, 0, 0);
}
template <class F>
__device__ __forceinline__ bool msm_is_redo_marker(const XYZZ<F>* v) {
  const uint32_t* x = reinterpret_cast<const uint32_t*>(&v->X);
  const uint32_t* zz = reinterpret_cast<const uint32_t*>(&v->ZZ);
  uint32_t o = 0;
  SPP_UNROLL for (uint32_t i = 0; i < sizeof(F) / 4; i++) o |= x[i] | zz[i];
  return o == 0;
}
// acc += the entries of slice sl in pass rho (dg = the digit rows of that pass for this lane's proof).  FAST: the additions are
// madd_distinct, and the walk ends with false at the first one that is refused (acc is then no sum of anything); else the complete
// madd, always true.
template <class F, bool FAST, int FORM>
__device__ __forceinline__ bool msm_flat_walk(MsmAcc<F, FORM>& acc, const Affine<F>* __restrict__ table, const MsmBlock* __restrict__ blocks,
                                              const int16_t* __restrict__ dg, uint32_t N, uint32_t Pp, uint32_t sl, uint32_t Sg) {
  for (uint32_t i0 = sl; i0 < N; i0 += 4 * Sg) {
    uint64_t pack = 0;
    SPP_UNROLL for (uint32_t k = 0; k < 4; k++) {
      const uint32_t i = i0 + k * Sg;
      const uint32_t d = i < N ? (uint32_t)(uint16_t)dg[(size_t)i * Pp] : 0u;
      pack |= (uint64_t)d << (16 * k);
    }
    if (pack == 0) continue;
#pragma unroll 1
    for (uint32_t k = 0; k < 4; k++) {
      const int d = (int)(int16_t)(uint16_t)(pack >> (16 * k));
      if (d != 0) {
        // The block of base i: where its rows start and how many entries they hold (the base index is the same for the whole
        // wave once a wave holds one slice, so this is one 16-byte line for all lanes).  A digit above the block's entry count
        // is skipped: the range class of a narrow block's wires (msm_classes.hpp) makes it impossible for a row that satisfies
        // its lookup constraints, and a row that does not is refused through its status word whatever is summed here -- the
        // compare keeps the gather inside the table.
        const uint32_t i = i0 + k * Sg;
        const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
        const MsmBlock blk = blocks[i >> 6];
        if (mag <= blk.E) {
          const Affine<F> e = table[((size_t)blk.off + (mag - 1)) * 64 + (i & 63)];
          if constexpr (FAST) {
            if (!acc.madd_distinct(e, d < 0)) return false;
          } else {
            acc.madd(e, d < 0);
          }
        }
      }
    }
  }
  return true;
}
template <class F>
__global__ void __launch_bounds__(MSM_WALK_BLOCK, MsmWalk<F>::waves_per_simd) k_msm_flat(const Affine<F>* __restrict__ table, const MsmBlock* __restrict__ blocks,
                                                  const int16_t* __restrict__ dig, XYZZ<F>* __restrict__ partial, uint32_t N, uint32_t P,
                                                  uint32_t Pp, uint32_t R, uint32_t Sg) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t p = g % Pp, t = g / Pp;
  if (t >= R * Sg || p >= P) return;
  const uint32_t rho = t / Sg, sl = t % Sg;
  MsmAcc<F, MsmWalk<F>::product_form> acc;
  acc.init();
  if (msm_flat_walk<F, true>(acc, table, blocks, dig + ((size_t)rho * N) * Pp + p, N, Pp, sl, Sg)) partial[(size_t)t * P + p] = acc.result();
  else msm_store_redo_marker(partial + (size_t)t * P + p);
}
// Behind every k_msm_flat, same grid and arguments: a lane whose slice sum is the redo marker sums its slice again with the complete
// addition; every other lane returns at once.  Bounded to the registers of the fast walk it follows (it may use scratch: it is
// cold) -- with more it would wait for a whole SIMD to drain behind the MSM waves of the other batch in flight.  When every lane is
// marked (one base repeated) this is the walk with the inline same-x path.  redo_count (optional): the number of lanes that walked
// again.
template <class F>
__global__ void __launch_bounds__(MSM_WALK_BLOCK, MsmWalk<F>::waves_per_simd) k_msm_flat_redo(const Affine<F>* __restrict__ table, const MsmBlock* __restrict__ blocks,
                                                  const int16_t* __restrict__ dig, XYZZ<F>* __restrict__ partial, uint32_t N, uint32_t P,
                                                  uint32_t Pp, uint32_t R, uint32_t Sg, uint32_t* __restrict__ redo_count) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t p = g % Pp, t = g / Pp;
  if (t >= R * Sg || p >= P) return;
  XYZZ<F>* out = partial + (size_t)t * P + p;
  if (!msm_is_redo_marker(out)) return;
  if (redo_count) atomicAdd(redo_count, 1u);
  const uint32_t rho = t / Sg, sl = t % Sg;
  MsmAcc<F> acc;
  acc.init();
  msm_flat_walk<F, false>(acc, table, blocks, dig + ((size_t)rho * N) * Pp + p, N, Pp, sl, Sg);
  *out = acc.result();
}

// general layout (Wt rows per base; Q > 1: the rows of a base are shared by Q lanes, items = (base, chunk of Wq rows) in
// chunk-major order so that the lanes of a wave share the chunk)
template <class F>
__global__ void __launch_bounds__(256) k_msm_rows(const Affine<F>* __restrict__ table, const int16_t* __restrict__ dig,
                                                  XYZZ<F>* __restrict__ partial, uint32_t N, uint32_t P, uint32_t Pp, uint32_t c,
                                                  uint32_t Wt, uint32_t R, uint32_t W, uint32_t Sg, uint32_t Q, uint32_t Wq) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t p = g % Pp, t = g / Pp;
  if (t >= R * Sg || p >= P) return;
  const uint32_t rho = t / Sg, sl = t % Sg;
  const uint32_t E = 1u << (c - 1);
  const size_t plane = (size_t)N * Pp;
  MsmAcc<F> acc;
  acc.init();
  const uint32_t items = N * Q;
  for (uint32_t it = sl; it < items; it += Sg) {
    uint32_t i = it, q = 0;
    if (Q > 1) {
      i = it % N;
      q = it / N;
    }
    const uint32_t m0 = q * Wq, m1 = m0 + Wq < Wt ? m0 + Wq : Wt;
    const int16_t* __restrict__ dg = dig + (size_t)i * Pp + p;
#pragma unroll 1
    for (uint32_t m = m0; m < m1; m++) {
      const uint32_t j = rho + R * m;
      if (j >= W) break;
      const int d = dg[(size_t)j * plane];
      if (d != 0) {
        const uint32_t row = i * Wt + m;
        const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
        acc.madd(table[((size_t)(row >> 6) * E + (mag - 1)) * 64 + (row & 63)], d < 0);
      }
    }
  }
  partial[(size_t)t * P + p] = acc.result();
}

// ev_start / ev_stop (optional): receive the dispatch's own start and stop timestamps (hipExtLaunchKernelGGL), i.e. the
// kernel's duration as a profiler reports it -- an event pair recorded around the launch would also count the time the
// launch waits for kernels of the other proving stream.
// The flat walk is two launches: the fast walk, which the event pair times, and the redo kernel behind it.  redo_count: see there.
template <class F>
void launch_msm_accumulate(hipStream_t st, const Affine<F>* table, const MsmBlock* blocks, const int16_t* dig, XYZZ<F>* partial, uint32_t N, uint32_t P,
                           uint32_t c, const MsmPlan& pl, hipEvent_t ev_start, hipEvent_t ev_stop, uint32_t* redo_count) {
  if (N == 0 || P == 0) {
    if (ev_start) hipEventRecord(ev_start, st);
    if (ev_stop) hipEventRecord(ev_stop, st);
    return;
  }
  const uint64_t lanes = (uint64_t)pl.R * pl.Sg * pl.Pp;
  if (pl.Wt == 1) {
    const dim3 grid((uint32_t)((lanes + MSM_WALK_BLOCK - 1) / MSM_WALK_BLOCK));
    hipExtLaunchKernelGGL(k_msm_flat<F>, grid, dim3(MSM_WALK_BLOCK), 0, st, ev_start, ev_stop, 0, table, blocks, dig, partial, N, P, pl.Pp, pl.R, pl.Sg);
    hipLaunchKernelGGL(k_msm_flat_redo<F>, grid, dim3(MSM_WALK_BLOCK), 0, st, table, blocks, dig, partial, N, P, pl.Pp, pl.R, pl.Sg, redo_count);
  } else
    hipExtLaunchKernelGGL(k_msm_rows<F>, dim3((uint32_t)((lanes + 255) / 256)), dim3(256), 0, st, ev_start, ev_stop, 0, table, dig, partial, N, P, pl.Pp, c,
                          pl.Wt, pl.R, pl.W, pl.Sg, pl.Q, pl.Wq);
}

// Fold the Sg slice sums of every (set, pass, proof): radix 8, one launch per level, every lane busy -- lane (s, p) with
// s < next = ceil(S_cur / 8) adds partial[s + next * m][p], m = 1 .. 7, into partial[s][p].  (Pairwise levels were 8 dependent
// launches for the 192 slices of a 128-proof batch; behind a chip full of MSM waves every launch waits for free SIMDs, the
// G2 fold with its 256 registers longest: 0.7 ms per level in the trace of pipelined 128-proof batches.)  blockIdx.y = set,
// blockIdx.z = pass; up to MSM_FOLD_SETS sets share the launches (the five G1 sums of a proof are independent).  A set with
// one pass leaves the fold in out[p]; with R > 1 passes the pass sums stay in partial[rho * Sg * P + p] for k_msm_horner.
template <class T>
__device__ __forceinline__ T msm_shfl_xor(const T& v, int mask) {
  static_assert(sizeof(T) % 4 == 0, "word-sized");
  T r;
  const uint32_t* s = reinterpret_cast<const uint32_t*>(&v);
  uint32_t* d = reinterpret_cast<uint32_t*>(&r);
  SPP_UNROLL for (uint32_t i = 0; i < sizeof(T) / 4; i++) d[i] = (uint32_t)__shfl_xor((int)s[i], mask, 64);
  return r;
}
// coop (a handful of proofs, the generateProof latency path): the 8 terms of an output sit on 8 neighbouring lanes and meet in a
// 3-step shuffle tree instead of one lane adding 7 of them in sequence -- the fold of a single proof's G2 sum is 5 levels deep:
// 35 dependent G2 additions (0.9 ms, what k_assemble waited for) become 15.
template <class F>
__global__ void __launch_bounds__(64) k_msm_fold_multi(MsmFoldSets<F> fs, uint32_t P, uint32_t coop) {
  const uint32_t set = blockIdx.y, rho = blockIdx.z;
  const uint32_t next = fs.half[set], S_cur = fs.cur[set];
  if (next == 0 || rho >= fs.R[set]) return;   // this set is already folded / has fewer passes (whole workgroups)
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  XYZZ<F>* __restrict__ partial = fs.partial[set] + (size_t)rho * fs.Sg[set] * P;
  if (coop) {
    static_assert(MSM_FOLD_RADIX == 8, "three shuffle steps");
    const uint32_t o = g >> 3, m = g & 7;
    const bool live = o < next * P;
    const uint32_t s = live ? o / P : 0, p = live ? o % P : 0, t = s + next * m;
    XYZZ<F> a = XYZZ<F>::infinity();
    if (live && t < S_cur) a = partial[(size_t)t * P + p];
    SPP_UNROLL for (int d = 4; d >= 1; d >>= 1) {               // every lane of the wave reaches the shuffles
      const XYZZ<F> b = msm_shfl_xor(a, d);
      a.add(b);
    }
    if (live && m == 0) {
      if (next == 1 && fs.R[set] == 1) fs.out[set][p] = a;
      else partial[(size_t)s * P + p] = a;
    }
    return;
  }
  if (g >= next * P) return;
  const uint32_t s = g / P, p = g % P;
  XYZZ<F> a = partial[(size_t)s * P + p];
#pragma unroll 1
  for (uint32_t t = s + next; t < S_cur; t += next) a.add(partial[(size_t)t * P + p]);
  if (next == 1 && fs.R[set] == 1) fs.out[set][p] = a;   // last level of a one-pass set: the result leaves the scratch array
  else partial[(size_t)s * P + p] = a;
}
// out[p] = sum_rho 2^(c*rho) * pass_sum[rho][p]  (Horner from the top pass down; one lane per (set, proof)).  The c doublings
// between two passes run in Jacobian coordinates (a = 0: 2M + 5S, "dbl-2009-l", against 6M + 3S for an XYZZ doubling):
// (X, Y, ZZ, ZZZ) -> (X*ZZ, Y*ZZZ, Z = ZZ) and back with ZZ' = Z^2, ZZZ' = Z^3 -- two products each way per pass.  The
// chain of c * (R - 1) = 240 doublings is what a single proof waits for here (G2: 3.7 -> 2.7 ms).
template <class F>
__global__ void __launch_bounds__(64) k_msm_horner(MsmFoldSets<F> fs, uint32_t P) {
  const uint32_t set = blockIdx.y;
  const uint32_t R = fs.R[set], c = fs.c[set];
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (R <= 1 || p >= P) return;
  const size_t stride = (size_t)fs.Sg[set] * P;
  const XYZZ<F>* __restrict__ sums = fs.partial[set];
  XYZZ<F> acc = sums[(size_t)(R - 1) * stride + p];
#pragma unroll 1
  for (uint32_t rho = R - 1; rho-- > 0;) {
    if (!acc.is_inf()) {
      F X = acc.X * acc.ZZ, Y = acc.Y * acc.ZZZ, Z = acc.ZZ;
#pragma unroll 1
      for (uint32_t k = 0; k < c; k++) {
        const F A = X.sqr(), B = Y.sqr(), C = B.sqr();
        const F t = (X + B).sqr() - A - C;
        const F D = t.dbl();
        const F E = A.dbl() + A;
        const F X3 = E.sqr() - D.dbl();
        const F C8 = C.dbl().dbl().dbl();
        const F Z3 = (Y * Z).dbl();
        Y = E * (D - X3) - C8;
        X = X3;
        Z = Z3;
      }
      const F zz = Z.sqr();
      acc.X = X;
      acc.Y = Y;
      acc.ZZ = zz;
      acc.ZZZ = zz * Z;
    }
    acc.add(sums[(size_t)rho * stride + p]);
  }
  fs.out[set][p] = acc;
}
template <class F>
__global__ void __launch_bounds__(256) k_msm_fill_inf(XYZZ<F>* __restrict__ out, uint32_t P) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < P) out[g] = XYZZ<F>::infinity();
}

// fs: partial / out / Sg / R / c filled by the caller per set (Sg = 0: empty set, out = infinity)
template <class F>
void launch_msm_reduce_multi(hipStream_t st, MsmFoldSets<F> fs, uint32_t nsets, uint32_t P) {
  if (P == 0 || nsets == 0) return;
  uint32_t cur[MSM_FOLD_SETS];
  bool done[MSM_FOLD_SETS];
  uint32_t maxR = 1;
  bool horner = false;
  for (uint32_t i = 0; i < nsets; i++) {
    cur[i] = fs.Sg[i];
    done[i] = false;
    if (fs.Sg[i] == 0) {
      hipLaunchKernelGGL(k_msm_fill_inf<F>, dim3((P + 255) / 256), dim3(256), 0, st, fs.out[i], P);
      done[i] = true;
      fs.R[i] = 1;
      continue;
    }
    if (fs.R[i] > 1) horner = true;
    if (fs.R[i] > 1 && fs.Sg[i] == 1) done[i] = true;   // nothing to fold: the pass sums are already in place
    maxR = std::max(maxR, fs.R[i]);
  }
  for (;;) {
    uint64_t lanes = 0;
    for (uint32_t i = 0; i < nsets; i++) {
      fs.half[i] = done[i] ? 0 : (cur[i] + MSM_FOLD_RADIX - 1) / MSM_FOLD_RADIX;
      fs.cur[i] = cur[i];
      lanes = std::max<uint64_t>(lanes, (uint64_t)fs.half[i] * P);
    }
    if (lanes == 0) break;
    const uint32_t coop = P <= MSM_FOLD_COOP_MAX_BATCH ? 1u : 0u;
    if (coop) lanes *= MSM_FOLD_RADIX;
    hipLaunchKernelGGL(k_msm_fold_multi<F>, dim3((uint32_t)((lanes + 63) / 64), nsets, maxR), dim3(64), 0, st, fs, P, coop);
    for (uint32_t i = 0; i < nsets; i++)
      if (!done[i]) {
        cur[i] = fs.half[i];
        if (cur[i] == 1) done[i] = true;
      }
  }
  if (horner) {
    for (uint32_t i = 0; i < nsets; i++)
      if (fs.Sg[i] == 0) fs.R[i] = 1;
    hipLaunchKernelGGL(k_msm_horner<F>, dim3((P + 63) / 64, nsets), dim3(64), 0, st, fs, P);
  }
}
template <class F>
void launch_msm_reduce(hipStream_t st, XYZZ<F>* partial, XYZZ<F>* out, uint32_t P, const MsmPlan& pl, uint32_t c, bool empty) {
  MsmFoldSets<F> fs{};
  fs.partial[0] = partial;
  fs.out[0] = out;
  fs.Sg[0] = empty ? 0 : pl.Sg;
  fs.R[0] = pl.R;
  fs.c[0] = c;
  launch_msm_reduce_multi<F>(st, fs, 1, P);
}

// ----------------------------------------------------------------------------------------------------
// setup: out[i] = scalars[i] * G using the window table of the single base G
// ----------------------------------------------------------------------------------------------------
template <class F>
__global__ void __launch_bounds__(64) k_fixed_base_mul(const Affine<F>* __restrict__ gen_table, uint32_t c, uint32_t Wn,
                                                       const Fr* __restrict__ scalars, uint32_t n, Affine<F>* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t E = 1u << (c - 1);
  Fr s = scalars[i];
  XYZZ<F> acc = XYZZ<F>::infinity();
  if (!s.is_zero()) {
    Recoder rc;
    rc.init(s);
#pragma unroll 1
    for (uint32_t j = 0; j < Wn; j++) {
      bool sgn;
      uint32_t d = rc.next(c, sgn);
      if (d != 0) {
        Affine<F> e = gen_table[((size_t)(j >> 6) * E + (d - 1)) * 64 + (j & 63)];
        if (sgn) e.y = e.y.neg();
        acc.madd(e);
      }
    }
  }
  out[i] = acc.to_affine();
}
template <class F>
void launch_fixed_base_mul(hipStream_t st, const Affine<F>* gen_table, uint32_t c, const Fr* scalars, uint32_t n, Affine<F>* out) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_fixed_base_mul<F>, dim3((n + 63) / 64), dim3(64), 0, st, gen_table, c, msm_windows(c), scalars, n, out);
}

}  // namespace spp
