// Stand-alone witness-INPUT kernels: everything the reference computes on the client before it can call the
// prover, batched on the GPU.
//
//   k_rlwe_witness        scripts/generate_audit.py:45-66,236-243,507-554 (negacyclic products, quotient witnesses)
//                         + pack_values :154-163  -- also demo-frontend/app/lib/rlwe.ts:157-247
//   k_poseidon_hash       client/merkle.ts:22-38 (poseidonHash2/4), noir_circuit/src/main.nr:1-9
//   k_merkle_path         noir_circuit/src/main.nr:11-29, client/merkle.ts:198-221
//   k_merkle_level        client/merkle.ts:165-176 (getRoot: one tree level per launch)
//   k_grumpkin_keygen     client/merkle.ts:98-113 (generateIdentityKeypair), main.nr:54-59
//   k_withdraw_rows       client/payroll-demo.ts:323-340 (keygen, wa_commitment, nullifier, getRoot, getProof -> one withdraw row)
//   k_deposit_leaves      client/payroll-demo.ts:264-292 (keygen, calculateCommitment, mt.insert)
//   k_deposit_roots       the same deposits' mt.getRoot() after each insert
//   k_deposit_rows        a deposit's row for the deposit circuit: the roots before and after its insert, one set of siblings
//   k_leaf_index_insert / k_leaf_find / k_wallet_identity / k_wallet_locate
//                         demo-frontend/app/lib/storage.ts:9-26,45-50 (leafIndex, nullifier, waCommitment, status of a DepositRecord
//                         from the secrets, the leaf list and the pool's accounts; the leaf index is leaf_index.hpp)
//   k_merkle_frontier / k_prefix_roots / k_merkle_gather_at / k_withdraw_rows_at
//                         the same getRoot / getProof / withdraw row for the tree of the first n leaves (merkle_prefix.hpp): the root
//                         a deposit pushed (instructions/deposit.rs:31-36,73), which demo-frontend/app/lib/on-chain.ts:93-125 looks for
//   k_poseidon2_sponge    ct_helper/src/main.nr:15-34 (= scripts/generate_audit.py:355-374)
//   k_audit_open          scripts/rlwe_decrypt.py:61-149 for a batch of (pw, ciphertext) records, with the binding checks it omits
//   k_partial_scale / k_partial_commit / k_rlwe_partial / k_rlwe_combine
//                         no counterpart (the reference rebuilds the key, rlwe_decrypt.py:61-91): one auditor's partial decryptions
//                         from its own share and their combination (rlwe_partial.hpp); k_audit_open<true> opens records from them
//   k_rlwe_keygen         scripts/rlwe_keygen.py:98-116 (the audit key pair), k_rlwe_key_noise: the check a key holder can make
//   k_shamir_split        scripts/rlwe_keygen.py:51-65 (shamir_share_field), the inverse of k_shamir_combine
#include "kernels.hpp"
#include "poseidon29.hpp"
#include "poseidon2.hpp"
#include "rlwe_ntt.hpp"
#include "audit_open.hpp"
#include "rlwe_partial.hpp"
#include "rlwe_keygen.hpp"
#include "leaf_index.hpp"
#include "merkle_prefix.hpp"
#include "deposit_rows.hpp"

namespace spp {

// ----------------------------------------------------------------------------------------------------
// RLWE witness generation: one wavefront per instance, exact negacyclic products through a 1024-point NTT held in LDS
// (rlwe_ntt.hpp: two prime fields q and 7*2^26+1, CRT digit = the quotient witness).  Per instance:
//   forward transform of r (twisted by psi^j) in both fields                                   -> R
//   R . NTT(a)/1024, inverse transform, untwist, CRT  -> c1[1024], k1[1024]   (generate_audit.py:517-518, 547-554)
//   R . NTT(b)/1024, inverse transform, untwist, CRT  -> c0[64],   k0[64]     (:513-514, 539-545; slots 0..63 only)
//   pack_values (:154-163) from LDS.
// Lane t owns coefficients t + 64 j: every global access of a wave is a contiguous 64-element row.  The transforms of the
// public key (k_rlwe_pk_ntt, once per call) use the same routine.
// ----------------------------------------------------------------------------------------------------
static constexpr int RL_N = 1024, RL_SLOTS = 64;
static constexpr long long RL_Q = 167772161ll, RL_DELTA = 655360ll;

template <bool REDUCE>
__device__ __forceinline__ void rn_ntt1(uint32_t lane, int32_t (&x)[16], int32_t* lds, const RnField& f, const int32_t* w, int dir) {
  rn_pass1<REDUCE>(lane, x, lds, f, w, dir);
  __syncthreads();
  rn_pass2_read(lane, x, lds);
  __syncthreads();
  rn_pass2<REDUCE>(lane, x, lds, f, w, dir);
  __syncthreads();
  rn_pass3(lane, x, lds, f, dir);
  __syncthreads();
}

// block 0: a, block 1: b.  hat[field][i] = NTT(pk psi^j)[i] / 1024 in Montgomery form, zero positions listed.
__global__ void __launch_bounds__(64) k_rlwe_pk_ntt(RnTables tb, const uint32_t* __restrict__ pk_a, const uint32_t* __restrict__ pk_b,
                                                    int32_t pk_scale0, int32_t pk_scale1, RlwePkDev* __restrict__ out) {
  __shared__ int32_t lds[RN_LDS_WORDS];
  __shared__ uint32_t nz;
  const uint32_t lane = threadIdx.x, poly = blockIdx.x;
  const uint32_t* src = poly == 0 ? pk_a : pk_b;
  if (lane == 0) nz = 0;
  __syncthreads();
  int32_t x[16];
#pragma unroll
  for (int j = 0; j < 16; j++) {
    const uint32_t i = lane + 64 * j, v = src[i];
    if (v == 0) out->zeros[poly][atomicAdd(&nz, 1u)] = (uint16_t)i;
    x[j] = rn_mul((int32_t)v, tb.psi[0][i], tb.f[0]);
  }
  rn_ntt1<true>(lane, x, lds, tb.f[0], tb.w[0][0], 0);
#pragma unroll
  for (int j = 0; j < 16; j++) out->hat[poly][0][lane + 64 * j] = rn_mul(x[j], pk_scale0, tb.f[0]);
#pragma unroll
  for (int j = 0; j < 16; j++) x[j] = rn_mul((int32_t)src[lane + 64 * j], tb.psi[1][lane + 64 * j], tb.f[1]);
  rn_ntt1<false>(lane, x, lds, tb.f[1], tb.w[1][0], 0);
#pragma unroll
  for (int j = 0; j < 16; j++) out->hat[poly][1][lane + 64 * j] = rn_mul(x[j], pk_scale1, tb.f[1]);
  __syncthreads();
  if (lane == 0) out->nzeros[poly] = nz;
}

// out[j] = (R . hat) transformed back (before the untwist) at coefficient lane + 64 j, field K
template <int K>
__device__ __forceinline__ void rn_product(uint32_t lane, const int32_t (&R)[16], const int32_t* __restrict__ hat, int32_t (&out)[16],
                                           int32_t* lds, const RnTables& tb) {
#pragma unroll
  for (int j = 0; j < 16; j++) out[j] = rn_mul(R[j], hat[lane + 64 * j], tb.f[K]);
  rn_ntt1<K == 0>(lane, out, lds, tb.f[K], tb.w[K][1], 1);
}

// coefficient `lane` (< 64) of the same product through the pruned inverse transform
template <int K>
__device__ __forceinline__ int32_t rn_product_first64(uint32_t lane, const int32_t (&R)[16], const int32_t* __restrict__ hat, int32_t* lds,
                                                      const RnTables& tb) {
  int32_t x[16];
#pragma unroll
  for (int j = 0; j < 16; j++) x[j] = rn_mul(R[j], hat[lane + 64 * j], tb.f[K]);
  rn_pass1<K == 0>(lane, x, lds, tb.f[K], tb.w[K][1], 1);
  __syncthreads();
  rn_pass2_read(lane, x, lds);
  __syncthreads();
  rn_pass2_first64<K == 0>(lane, x, lds, tb.f[K], tb.w[K][1], 1);
  __syncthreads();
  const int32_t v = rn_pass3_first64(lane, lds);
  __syncthreads();
  return v;
}

__global__ void __launch_bounds__(64, 4) k_rlwe_witness(RnTables tb, const RlwePkDev* __restrict__ pk, const int8_t* __restrict__ r_in,
                                                        const int8_t* __restrict__ e1_in, const int8_t* __restrict__ e2_in,
                                                        const uint8_t* __restrict__ msg_in, uint32_t* __restrict__ c0_out,
                                                        uint32_t* __restrict__ c1_out, int32_t* __restrict__ k0_out,
                                                        int32_t* __restrict__ k1_out, uint8_t* __restrict__ packed_be, uint32_t count) {
  __shared__ int32_t lds[RN_LDS_WORDS];       // exchange buffer of the transform in flight (one field at a time)
  __shared__ int32_t pre[RL_N + 64];          // prefix scan of r -> suffix sums at [64 + i]; then c0 | c1 for the packing epilogue
  __shared__ int8_t rbytes[RL_N];
  __shared__ int32_t tot[64], offs[64];
  const uint32_t inst = blockIdx.x, lane = threadIdx.x;
  if (inst >= count) return;
  // ---- r: one 16-byte load per lane, transposed through LDS to the lane layout i = lane + 64 j ----
  reinterpret_cast<uint4*>(rbytes)[lane] = reinterpret_cast<const uint4*>(r_in + (size_t)inst * RL_N)[lane];
  __syncthreads();
  int32_t R0[16], R1[16];
  int32_t suffix0;   // wrap correction of coefficient `lane` (needed again for the message slots)
  {
    int32_t rv[16];
#pragma unroll
    for (int j = 0; j < 16; j++) rv[j] = rbytes[lane + 64 * j];
    // forward transforms of r psi^j in both fields
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const uint32_t i = lane + 64 * j;
      R0[j] = rn_mul(rv[j], tb.psi[0][i], tb.f[0]);     // signed arithmetic: r_j in [-128, 127] goes in as it is
      R1[j] = rn_mul(rv[j], tb.psi[1][i], tb.f[1]);
    }
    // wrap correction: suffix sums of r (rlwe_ntt.hpp), left in LDS at pre[64 + i] (the slot that later receives c1[i])
    rn_scan_scatter(lane, rv, pre);
    __syncthreads();
    rn_scan_chunk(lane, pre, tot);
    __syncthreads();
    int32_t offset, total;
    rn_scan_offsets(lane, tot, offset, total);
    offs[lane] = offset;
    __syncthreads();
    int32_t suffix[16];
    rn_scan_gather(lane, total, pre, offs, suffix);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 16; j++) pre[64 + lane + 64 * j] = suffix[j];
    suffix0 = suffix[0];
  }
  rn_ntt1<true>(lane, R0, lds, tb.f[0], tb.w[0][0], 0);
  rn_ntt1<false>(lane, R1, lds, tb.f[1], tb.w[1][0], 0);
  uint32_t* cs = reinterpret_cast<uint32_t*>(pre);   // c0 at [0,64), c1 at [64, 1088)
  // ---- a: c1 / k1 ----
  {
    int32_t s0[16], y[16];
    rn_product<0>(lane, R0, pk->hat[0][0], s0, lds, tb);
#pragma unroll
    for (int j = 0; j < 16; j++) s0[j] = rn_canon(rn_mul(s0[j], tb.ipsi[0][lane + 64 * j], tb.f[0]), tb.f[0]);
    rn_product<1>(lane, R1, pk->hat[0][1], y, lds, tb);
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const uint32_t i = lane + 64 * j;
      const int32_t s1 = rn_canon(rn_mul(y[j], tb.ipsi[1][i], tb.f[1]), tb.f[1]);
      const int32_t t = rn_crt_digit(s0[j], s1, tb.f[1]);
      int32_t k;
      uint32_t rem;
      rn_quot_rem(s0[j], t, (int32_t)e2_in[(size_t)inst * RL_N + i], k, rem);
      k += pre[64 + i];                 // own slot: read the suffix sum, then overwrite it with the remainder
      c1_out[(size_t)inst * RL_N + i] = rem;
      k1_out[(size_t)inst * RL_N + i] = k;
      cs[RL_SLOTS + i] = rem;
    }
  }
  // ---- b: c0 / k0 (message slots: coefficients 0..63 = element j = 0 of every lane) ----
  {
    const int32_t y0 = rn_product_first64<0>(lane, R0, pk->hat[1][0], lds, tb);
    const int32_t y1 = rn_product_first64<1>(lane, R1, pk->hat[1][1], lds, tb);
    const uint32_t i = lane;
    const int32_t s0 = rn_canon(rn_mul(y0, tb.ipsi[0][i], tb.f[0]), tb.f[0]);
    const int32_t s1 = rn_canon(rn_mul(y1, tb.ipsi[1][i], tb.f[1]), tb.f[1]);
    const int32_t t = rn_crt_digit(s0, s1, tb.f[1]);
    int32_t k;
    uint32_t rem;
    rn_quot_rem(s0, t, (int32_t)e1_in[(size_t)inst * RL_SLOTS + i] + (int32_t)RL_DELTA * (int32_t)msg_in[(size_t)inst * RL_SLOTS + i], k, rem);
    k += suffix0;
    c0_out[(size_t)inst * RL_SLOTS + i] = rem;
    k0_out[(size_t)inst * RL_SLOTS + i] = k;
    cs[i] = rem;
  }
  // ---- rare: the public key has zero coefficients (probability 1/q each): the wrapped term is 0, not q * r_j ----
  const uint32_t nza = pk->nzeros[0], nzb = pk->nzeros[1];
  if (nza | nzb) {
    if (nza)
#pragma unroll 1
      for (uint32_t j = 0; j < 16; j++) {
        const uint32_t i = lane + 64 * j;
        k1_out[(size_t)inst * RL_N + i] -= rn_zero_correction(i, pk->zeros[0], nza, rbytes);
      }
    if (nzb) k0_out[(size_t)inst * RL_SLOTS + lane] -= rn_zero_correction(lane, pk->zeros[1], nzb, rbytes);
  }
  __syncthreads();
  // ---- pack 7 x 32-bit per field (pack_values), 32-byte big-endian: 10 + 147 fields; one 32-bit word per lane and step ----
  if (packed_be) {
    uint32_t* out = reinterpret_cast<uint32_t*>(packed_be + (size_t)inst * 157 * 32);
    for (uint32_t w = lane; w < 157 * 8; w += 64) {
      const uint32_t f = w >> 3, jw = 7 - (w & 7);      // big-endian word w & 7 of field f  <->  little-endian word jw
      uint32_t v = 0;
      if (jw < 7) {
        if (f < 10) { const uint32_t idx = 7 * f + jw; if (idx < RL_SLOTS) v = cs[idx]; }
        else { const uint32_t idx = 7 * (f - 10) + jw; if (idx < RL_N) v = cs[RL_SLOTS + idx]; }
      }
      out[w] = __builtin_bswap32(v);
    }
  }
}
void launch_rlwe_witness(hipStream_t st, const RlweDev& rd, const uint32_t* pk_a, const uint32_t* pk_b, const int8_t* r, const int8_t* e1,
                         const int8_t* e2, const uint8_t* msg, uint32_t* c0, uint32_t* c1, int32_t* k0, int32_t* k1, uint8_t* packed_be,
                         uint32_t count) {
  if (count == 0) return;
  hipLaunchKernelGGL(k_rlwe_pk_ntt, dim3(2), dim3(64), 0, st, rd.tb, pk_a, pk_b, rd.pk_scale[0], rd.pk_scale[1], rd.pk);
  hipLaunchKernelGGL(k_rlwe_witness, dim3(count), dim3(64), 0, st, rd.tb, rd.pk, r, e1, e2, msg, c0, c1, k0, k1, packed_be, count);
}

// ----------------------------------------------------------------------------------------------------
// Poseidon (t = 3, 5), permutation with the state in registers; one lane per hash
// ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ Fr load_be(const uint8_t* p) {
  uint8_t buf[32];
  for (int i = 0; i < 32; i++) buf[i] = p[i];
  return Fr::from_bytes_be(buf);
}
__device__ __forceinline__ void store_be(uint8_t* p, const Fr& v) {
  uint8_t buf[32];
  v.to_bytes_be(buf);
  for (int i = 0; i < 32; i++) p[i] = buf[i];
}
// the permutation itself lives in poseidon29.hpp (9x29-bit form, lazy MDS rows); nothing is emitted here
template <int T>
__device__ __noinline__ void poseidon_permute(Fr (&s)[T], const Fr* __restrict__ rc, const uint32_t* __restrict__ mds29, int rp) {
  poseidon_permute29<T, false>(s, rc, mds29, rp, PoseidonNoEmit{});
}
__device__ __forceinline__ Fr poseidon_hash2(const HashConsts& hc, const Fr& a, const Fr& b) {
  Fr s[3] = {Fr::zero(), a, b};
  poseidon_permute<3>(s, hc.pos3_rc, hc.pos3_mds29, 57);
  return s[0];
}

__global__ void __launch_bounds__(64) k_poseidon_hash(HashConsts hc, const uint8_t* __restrict__ in_be, uint32_t arity,
                                                      uint8_t* __restrict__ out_be, uint32_t count) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= count) return;
  const uint8_t* in = in_be + (size_t)g * arity * 32;
  Fr h;
  if (arity == 2) {
    h = poseidon_hash2(hc, load_be(in), load_be(in + 32));
  } else {
    Fr s[5] = {Fr::zero(), load_be(in), load_be(in + 32), load_be(in + 64), load_be(in + 96)};
    poseidon_permute<5>(s, hc.pos5_rc, hc.pos5_mds29, 60);
    h = s[0];
  }
  store_be(out_be + (size_t)g * 32, h);
}
void launch_poseidon_hash(hipStream_t st, HashConsts hc, const uint8_t* in_be, uint32_t arity, uint8_t* out_be, uint32_t count) {
  if (count) hipLaunchKernelGGL(k_poseidon_hash, dim3((count + 63) / 64), dim3(64), 0, st, hc, in_be, arity, out_be, count);
}

// root of one authentication path per lane (main.nr:11-29)
__global__ void __launch_bounds__(64) k_merkle_path(HashConsts hc, const uint8_t* __restrict__ leaf_be, const uint64_t* __restrict__ index,
                                                    const uint8_t* __restrict__ siblings_be, uint32_t depth, uint8_t* __restrict__ root_be,
                                                    uint32_t count) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= count) return;
  Fr cur = load_be(leaf_be + (size_t)g * 32);
  const uint64_t idx = index[g];
  for (uint32_t i = 0; i < depth; i++) {
    Fr sib = load_be(siblings_be + ((size_t)g * depth + i) * 32);
    cur = ((idx >> i) & 1) ? poseidon_hash2(hc, sib, cur) : poseidon_hash2(hc, cur, sib);
  }
  store_be(root_be + (size_t)g * 32, cur);
}
void launch_merkle_path(hipStream_t st, HashConsts hc, const uint8_t* leaf_be, const uint64_t* index, const uint8_t* siblings_be,
                        uint32_t depth, uint8_t* root_be, uint32_t count) {
  if (count) hipLaunchKernelGGL(k_merkle_path, dim3((count + 63) / 64), dim3(64), 0, st, hc, leaf_be, index, siblings_be, depth, root_be, count);
}

// one tree level: parents[j] = H(children[2j], children[2j+1]); a missing right/left child is the level's default hash
__global__ void __launch_bounds__(64) k_merkle_level(HashConsts hc, const Fr* __restrict__ children, uint32_t n_children, Fr dflt,
                                                     Fr* __restrict__ parents, uint32_t n_parents) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_parents) return;
  Fr l = 2 * g < n_children ? children[2 * g] : dflt;
  Fr r = 2 * g + 1 < n_children ? children[2 * g + 1] : dflt;
  parents[g] = poseidon_hash2(hc, l, r);
}
void launch_merkle_level(hipStream_t st, HashConsts hc, const Fr* children, uint32_t n_children, Fr dflt, Fr* parents, uint32_t n_parents) {
  if (n_parents) hipLaunchKernelGGL(k_merkle_level, dim3((n_parents + 63) / 64), dim3(64), 0, st, hc, children, n_children, dflt, parents, n_parents);
}
// ---- incremental tree (spp_merkle_tree_*): levels stay resident in HBM; an append touches O(count + depth) nodes ----
// default (empty-subtree) hashes: d_0 = 0, d_{l+1} = H(d_l, d_l)   (client/merkle.ts:150-156)
__global__ void __launch_bounds__(64) k_merkle_defaults(HashConsts hc, Fr* __restrict__ out, uint32_t depth) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  Fr d = Fr::zero();
  out[0] = d;
  for (uint32_t l = 0; l < depth; l++) {
    d = poseidon_hash2(hc, d, d);
    out[l + 1] = d;
  }
}
// parents [first, first + n) of one level, recomputed from its children; children at or beyond n_children are the level default
__global__ void __launch_bounds__(64) k_merkle_update(HashConsts hc, const Fr* __restrict__ children, uint64_t n_children,
                                                      const Fr* __restrict__ dflt_level, Fr* __restrict__ parents, uint64_t first, uint32_t n) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const uint64_t j = first + g;
  const Fr d = *dflt_level;
  const Fr l = 2 * j < n_children ? children[2 * j] : d;
  const Fr r = 2 * j + 1 < n_children ? children[2 * j + 1] : d;
  parents[j] = poseidon_hash2(hc, l, r);
}
// getProof (client/merkle.ts:198-221) without any hashing: sibling of level l = stored node or the level default
__global__ void __launch_bounds__(64) k_merkle_gather(const MerkleTreeDev* __restrict__ t, const uint64_t* __restrict__ indices, uint32_t nq,
                                                      uint8_t* __restrict__ out_be) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t depth = t->depth;
  if (g >= nq * depth) return;
  const uint32_t q = g / depth, l = g % depth;
  const uint64_t sib = (indices[q] >> l) ^ 1;
  const Fr v = sib < t->count[l] ? t->level[l][sib] : t->dflt[l];
  store_be(out_be + ((size_t)q * depth + l) * 32, v);
}
// ---- the tree as of an earlier size (merkle_prefix.hpp: default / frontier / stored; one frontier node per level) ----
__device__ __forceinline__ Fr poseidon_hash2_inline(const HashConsts& hc, const Fr& a, const Fr& b) {
  Fr s[3] = {Fr::zero(), a, b};
  poseidon_permute29<3, false>(s, hc.pos3_rc, hc.pos3_mds29, 57, PoseidonNoEmit{});
  return s[0];
}
// F[0..depth] of the prefix tree of `size` leaves: depth dependent permutations on one lane, once per as-of call, so that the
// per-note and per-sibling kernels below only select
__global__ void __launch_bounds__(64) k_merkle_frontier(HashConsts hc, const MerkleTreeDev* __restrict__ t, uint64_t size, Fr* __restrict__ F) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  prefix_walk(size, t->depth, [&](uint32_t l) { return (const Fr*)t->level[l]; }, t->dflt,
              [&](const Fr& a, const Fr& b) { return poseidon_hash2_inline(hc, a, b); }, F);
}
// R[first_size + g]: the same walk per lane, nothing kept but the root (k_deposit_roots' loop for leaf n-1, R[0] = dflt[depth])
__global__ void __launch_bounds__(64) k_prefix_roots(HashConsts hc, const MerkleTreeDev* __restrict__ t, uint64_t first_size, uint32_t count,
                                                     Fr* __restrict__ roots) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= count) return;
  roots[g] = prefix_walk(first_size + g, t->depth, [&](uint32_t l) { return (const Fr*)t->level[l]; }, t->dflt,
                         [&](const Fr& a, const Fr& b) { return poseidon_hash2_inline(hc, a, b); }, (Fr*)nullptr);
}
// k_merkle_gather against the prefix tree of `size` leaves; F from k_merkle_frontier, an earlier launch
__global__ void __launch_bounds__(64) k_merkle_gather_at(const MerkleTreeDev* __restrict__ t, uint64_t size, const Fr* __restrict__ F,
                                                         const uint64_t* __restrict__ indices, uint32_t nq, uint8_t* __restrict__ out_be) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t depth = t->depth;
  if (g >= nq * depth) return;
  const uint32_t q = g / depth, l = g % depth;
  store_be(out_be + ((size_t)q * depth + l) * 32, prefix_node(size, l, (indices[q] >> l) ^ 1, (const Fr*)t->level[l], t->dflt, F));
}
void launch_merkle_frontier(hipStream_t st, HashConsts hc, const MerkleTreeDev* t, uint64_t size, Fr* frontier) {
  hipLaunchKernelGGL(k_merkle_frontier, dim3(1), dim3(64), 0, st, hc, t, size, frontier);
}
void launch_prefix_roots(hipStream_t st, HashConsts hc, const MerkleTreeDev* t, uint64_t first_size, uint32_t count, Fr* roots) {
  if (count) hipLaunchKernelGGL(k_prefix_roots, dim3((count + 63) / 64), dim3(64), 0, st, hc, t, first_size, count, roots);
}
void launch_merkle_gather_at(hipStream_t st, const MerkleTreeDev* t, uint32_t depth, uint64_t size, const Fr* frontier, const uint64_t* indices,
                             uint32_t nq, uint8_t* out_be) {
  const uint32_t n = nq * depth;
  if (n) hipLaunchKernelGGL(k_merkle_gather_at, dim3((n + 63) / 64), dim3(64), 0, st, t, size, frontier, indices, nq, out_be);
}
void launch_merkle_defaults(hipStream_t st, HashConsts hc, Fr* out, uint32_t depth) {
  hipLaunchKernelGGL(k_merkle_defaults, dim3(1), dim3(64), 0, st, hc, out, depth);
}
void launch_merkle_update(hipStream_t st, HashConsts hc, const Fr* children, uint64_t n_children, const Fr* dflt_level, Fr* parents,
                          uint64_t first, uint32_t n) {
  if (n) hipLaunchKernelGGL(k_merkle_update, dim3((n + 63) / 64), dim3(64), 0, st, hc, children, n_children, dflt_level, parents, first, n);
}
void launch_merkle_gather(hipStream_t st, const MerkleTreeDev* t, uint32_t depth, const uint64_t* indices, uint32_t nq, uint8_t* out_be) {
  const uint32_t n = nq * depth;
  if (n) hipLaunchKernelGGL(k_merkle_gather, dim3((n + 63) / 64), dim3(64), 0, st, t, indices, nq, out_be);
}

__global__ void __launch_bounds__(256) k_fr_from_be(const uint8_t* __restrict__ in, Fr* __restrict__ out, uint32_t n) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < n) out[g] = load_be(in + (size_t)g * 32);
}
__global__ void __launch_bounds__(256) k_fr_to_be(const Fr* __restrict__ in, uint8_t* __restrict__ out, uint32_t n) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < n) store_be(out + (size_t)g * 32, in[g]);
}
void launch_fr_from_be(hipStream_t st, const uint8_t* in, Fr* out, uint32_t n) {
  if (n) hipLaunchKernelGGL(k_fr_from_be, dim3((n + 255) / 256), dim3(256), 0, st, in, out, n);
}
void launch_fr_to_be(hipStream_t st, const Fr* in, uint8_t* out, uint32_t n) {
  if (n) hipLaunchKernelGGL(k_fr_to_be, dim3((n + 255) / 256), dim3(256), 0, st, in, out, n);
}

// ----------------------------------------------------------------------------------------------------
// Grumpkin key generation: pk = sk * G with a 4-bit window table T[j][d] = (d+1) * 16^j * G (64 x 15 used)
// ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ GkAffine grumpkin_mul_g(const GkAffine* __restrict__ table, const Fr& sk) {
  uint32_t c[8];
  sk.to_canonical(c);
  GkXYZZ acc = GkXYZZ::infinity();
  uint32_t word = 0;
#pragma unroll 1
  for (uint32_t j = 0; j < 64; j++) {
    if ((j & 7) == 0) {
      const uint32_t li = j >> 3;
      word = li == 0 ? c[0] : li == 1 ? c[1] : li == 2 ? c[2] : li == 3 ? c[3] : li == 4 ? c[4] : li == 5 ? c[5] : li == 6 ? c[6] : c[7];
    }
    const uint32_t d = word & 15;
    word >>= 4;
    if (d) acc.madd(table[j * 16 + d - 1]);
  }
  return acc.to_affine();
}
__global__ void __launch_bounds__(64) k_grumpkin_keygen(const GkAffine* __restrict__ table, const uint8_t* __restrict__ sk_be,
                                                        uint8_t* __restrict__ xy_be, uint32_t count) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= count) return;
  const GkAffine p = grumpkin_mul_g(table, load_be(sk_be + (size_t)g * 32));
  store_be(xy_be + (size_t)g * 64, p.x);
  store_be(xy_be + (size_t)g * 64 + 32, p.y);
}
void launch_grumpkin_keygen(hipStream_t st, const GkAffine* table, const uint8_t* sk_be, uint8_t* xy_be, uint32_t count) {
  if (count) hipLaunchKernelGGL(k_grumpkin_keygen, dim3((count + 63) / 64), dim3(64), 0, st, table, sk_be, xy_be, count);
}

// ----------------------------------------------------------------------------------------------------
// Withdraw rows from notes against the resident tree (client/payroll-demo.ts:323-340: identity, wa_commitment, nullifier,
// mt.getRoot(), mt.getProof(index)).  One lane per note; note = recipient | amount | secret_key | randomness | index (5 x 32 B
// big-endian, main.nr:38-51), row = root | nullifier | recipient | amount | wa_commitment | secret_key | owner_x | owner_y |
// randomness | index | siblings[depth] (spp_prove_withdraw's order).  The note commitment is not part of the row: a note that is
// not the leaf at `index` yields a row whose Merkle root differs from the public one, and the solver's check refuses it.
// ----------------------------------------------------------------------------------------------------
static constexpr uint32_t NOTE_BYTES = 160;
__device__ __forceinline__ void copy32(uint8_t* __restrict__ o, const uint8_t* __restrict__ p) {
  for (int i = 0; i < 32; i++) o[i] = p[i];
}
// One body, two entries.  ASOF = false is k_withdraw_rows as it always was (size and F unused); ASOF = true takes root and siblings
// from the prefix tree of `size` leaves: the root is F[depth], a sibling one of merkle_prefix.hpp's three cases.  The frontier is
// k_merkle_frontier's, an earlier launch: no second permutation call site and no per-lane walk here (see the VGPR note below).
// The pointers carry no __restrict__ here, the entries' parameters do: with it repeated on the inlined body k_withdraw_rows comes
// out with another register allocation; as written its instructions are the former ones but for one commutative operand order.
template <bool ASOF>
__device__ __forceinline__ void withdraw_rows_body(const GkAffine* table, const HashConsts& hc, const MerkleTreeDev* t, uint64_t size, const Fr* F,
                                                   const uint8_t* notes, uint8_t* rows, uint32_t count) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= count) return;
  const uint32_t depth = t->depth;
  const uint8_t* nt = notes + (size_t)g * NOTE_BYTES;
  uint8_t* o = rows + (size_t)g * (10 + depth) * 32;
  const Fr sk = load_be(nt + 64);
  const GkAffine pk = grumpkin_mul_g(table, sk);                     // merkle.ts:98-113, main.nr:54-62
  // wa_commitment = H(owner_x, owner_y) (main.nr:64-67), then nullifier = H(secret_key, index) (:72-74): one permutation inlined
  // in a two-trip loop.  Through the out-of-line poseidon_permute the kernel had 200 VGPRs and a 224-byte stack frame per lane
  // (as every caller of poseidon_hash2 here); inlined: 154 VGPRs, 112 bytes (the permutation's state array), no spills.
#pragma unroll 1
  for (int k = 0; k < 2; k++) {
    Fr s[3] = {Fr::zero(), k ? sk : pk.x, k ? load_be(nt + 128) : pk.y};
    poseidon_permute29<3, false>(s, hc.pos3_rc, hc.pos3_mds29, 57, PoseidonNoEmit{});
    store_be(o + (k ? 1 : 4) * 32, s[0]);
  }
  copy32(o + 2 * 32, nt);                                            // recipient
  copy32(o + 3 * 32, nt + 32);                                       // amount
  copy32(o + 5 * 32, nt + 64);                                       // secret_key
  store_be(o + 6 * 32, pk.x);
  store_be(o + 7 * 32, pk.y);
  copy32(o + 8 * 32, nt + 96);                                       // randomness
  copy32(o + 9 * 32, nt + 128);                                      // index
  // the leaf index as an integer; an index >= 2^depth never touches tree memory: its siblings are the level defaults
  bool in_range = true;
  uint64_t idx = 0;
  for (int i = 0; i < 24; i++) in_range &= nt[128 + i] == 0;
  for (int i = 24; i < 32; i++) idx = (idx << 8) | nt[128 + i];
  in_range &= (idx >> depth) == 0;
  if constexpr (ASOF) {
    // the prefix tree's root and siblings (spp_merkle_tree_root_at / _proofs_at), as k_merkle_gather_at
    store_be(o, F[depth]);
    for (uint32_t l = 0; l < depth; l++)
      store_be(o + (10 + l) * 32, in_range ? prefix_node(size, l, (idx >> l) ^ 1, (const Fr*)t->level[l], t->dflt, F) : t->dflt[l]);
  } else {
    // root at call time (spp_merkle_tree_root), siblings as k_merkle_gather
    store_be(o, t->count[depth] ? t->level[depth][0] : t->dflt[depth]);
    for (uint32_t l = 0; l < depth; l++) {
      const uint64_t sib = (idx >> l) ^ 1;
      store_be(o + (10 + l) * 32, in_range && sib < t->count[l] ? t->level[l][sib] : t->dflt[l]);
    }
  }
}
__global__ void __launch_bounds__(64) k_withdraw_rows(const GkAffine* __restrict__ table, HashConsts hc, const MerkleTreeDev* __restrict__ t,
                                                      const uint8_t* __restrict__ notes, uint8_t* __restrict__ rows, uint32_t count) {
  withdraw_rows_body<false>(table, hc, t, 0, nullptr, notes, rows, count);
}
__global__ void __launch_bounds__(64) k_withdraw_rows_at(const GkAffine* __restrict__ table, HashConsts hc, const MerkleTreeDev* __restrict__ t,
                                                         uint64_t size, const Fr* __restrict__ F, const uint8_t* __restrict__ notes,
                                                         uint8_t* __restrict__ rows, uint32_t count) {
  withdraw_rows_body<true>(table, hc, t, size, F, notes, rows, count);
}
void launch_withdraw_rows(hipStream_t st, const GkAffine* table, HashConsts hc, const MerkleTreeDev* t, const uint8_t* notes, uint8_t* rows,
                          uint32_t count) {
  if (count) hipLaunchKernelGGL(k_withdraw_rows, dim3((count + 63) / 64), dim3(64), 0, st, table, hc, t, notes, rows, count);
}
void launch_withdraw_rows_at(hipStream_t st, const GkAffine* table, HashConsts hc, const MerkleTreeDev* t, uint64_t size, const Fr* frontier,
                             const uint8_t* notes, uint8_t* rows, uint32_t count) {
  if (count) hipLaunchKernelGGL(k_withdraw_rows_at, dim3((count + 63) / 64), dim3(64), 0, st, table, hc, t, size, frontier, notes, rows, count);
}

// ----------------------------------------------------------------------------------------------------
// Deposits into the resident tree (client/payroll-demo.ts:264-292, client/test-shielded-pool.ts:218-231: generateIdentityKeypair,
// calculateCommitment, mt.insert, mt.getRoot per deposit).  deposit = secret_key | amount | randomness (3 x 32 B big-endian).
// k_deposit_leaves: one lane per deposit; the commitment H4(owner_x, owner_y, amount, randomness) (merkle.ts:126-133,
// main.nr:69-70) goes straight into level 0 of the tree.  Both Poseidon permutations below are inlined (see k_withdraw_rows).
// k_deposit_roots: after the level update, the root of the prefix tree of leaves 0..i for every deposited leaf i (what getRoot
// returns after that leaf's insert).  Walking up from leaf i, a left sibling covers only leaves < i, so it is final in the
// prefix tree and is read from the tree; a right sibling covers only leaves > i, so it is empty there: the level default.
// ----------------------------------------------------------------------------------------------------
static constexpr uint32_t DEPOSIT_BYTES = 96;
__global__ void __launch_bounds__(64) k_deposit_leaves(const GkAffine* __restrict__ table, HashConsts hc, const uint8_t* __restrict__ deposits,
                                                       Fr* __restrict__ leaves, uint32_t count) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= count) return;
  const uint8_t* d = deposits + (size_t)g * DEPOSIT_BYTES;
  const GkAffine pk = grumpkin_mul_g(table, load_be(d));             // merkle.ts:98-113 (the key as given, see spp.h)
  Fr s[5] = {Fr::zero(), pk.x, pk.y, load_be(d + 32), load_be(d + 64)};
  poseidon_permute29<5, false>(s, hc.pos5_rc, hc.pos5_mds29, 60, PoseidonNoEmit{});
  leaves[g] = s[0];
}
__global__ void __launch_bounds__(64) k_deposit_roots(HashConsts hc, const MerkleTreeDev* __restrict__ t, uint64_t first, uint32_t count,
                                                      uint8_t* __restrict__ roots_be, uint8_t* __restrict__ commitments_be) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= count) return;
  const uint64_t i = first + g;
  Fr v = t->level[0][i];
  if (commitments_be) store_be(commitments_be + (size_t)g * 32, v);
  if (!roots_be) return;
  const uint32_t depth = t->depth;
#pragma unroll 1
  for (uint32_t l = 0; l < depth; l++) {
    const uint64_t p = i >> l;
    const bool odd = p & 1;
    Fr s[3] = {Fr::zero(), odd ? t->level[l][p - 1] : v, odd ? v : t->dflt[l]};
    poseidon_permute29<3, false>(s, hc.pos3_rc, hc.pos3_mds29, 57, PoseidonNoEmit{});
    v = s[0];
  }
  store_be(roots_be + (size_t)g * 32, v);
}
void launch_deposit_leaves(hipStream_t st, const GkAffine* table, HashConsts hc, const uint8_t* deposits, Fr* leaves, uint32_t count) {
  if (count) hipLaunchKernelGGL(k_deposit_leaves, dim3((count + 63) / 64), dim3(64), 0, st, table, hc, deposits, leaves, count);
}
void launch_deposit_roots(hipStream_t st, HashConsts hc, const MerkleTreeDev* t, uint64_t first, uint32_t count, uint8_t* roots_be,
                          uint8_t* commitments_be) {
  if (count) hipLaunchKernelGGL(k_deposit_roots, dim3((count + 63) / 64), dim3(64), 0, st, hc, t, first, count, roots_be, commitments_be);
}

// ----------------------------------------------------------------------------------------------------
// Deposit rows (circuit_deposit.cpp): one lane per deposit; leaf i = first + g of the tree, which must already hold it.
// row = old_root | new_root | commitment | amount | index | owner_x | owner_y | randomness | siblings[depth], 32 B big-endian each.
// The owner and the commitment are k_deposit_leaves' (the commitment computed from the record, never read from the tree); the walk
// up is deposit_rows.hpp: k_deposit_roots' walk twice over one set of siblings, from the empty leaf to the root of size i and from
// the commitment to the root of size i + 1.  It reads stored nodes to the LEFT of the path only, at positions below count[l]
// whenever i < count[0], which the callers check on the host.  An amount >= 2^64 is copied as it is: the circuit refuses the row.
// Two permutation call sites, t = 5 once and t = 3 in the rolled two-trip loop of the walk, both inlined (see k_withdraw_rows).
// ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_deposit_rows(const GkAffine* __restrict__ table, HashConsts hc, const MerkleTreeDev* __restrict__ t,
                                                     uint64_t first, const uint8_t* __restrict__ deposits, uint8_t* __restrict__ rows,
                                                     uint32_t count) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= count) return;
  const uint32_t depth = t->depth;
  const uint64_t i = first + g;
  const uint8_t* d = deposits + (size_t)g * DEPOSIT_BYTES;
  uint8_t* o = rows + (size_t)g * (DEPOSIT_ROW_FIXED + depth) * 32;
  Fr c;
  {
    const GkAffine pk = grumpkin_mul_g(table, load_be(d));           // the key as given, as k_deposit_leaves
    store_be(o + 5 * 32, pk.x);
    store_be(o + 6 * 32, pk.y);
    Fr s[5] = {Fr::zero(), pk.x, pk.y, load_be(d + 32), load_be(d + 64)};
    poseidon_permute29<5, false>(s, hc.pos5_rc, hc.pos5_mds29, 60, PoseidonNoEmit{});
    c = s[0];
  }
  store_be(o + 2 * 32, c);
  copy32(o + 3 * 32, d + 32);                                        // amount
  for (int b = 0; b < 24; b++) o[4 * 32 + b] = 0;                    // index
  for (int b = 0; b < 8; b++) o[4 * 32 + 24 + b] = (uint8_t)(i >> (8 * (7 - b)));
  copy32(o + 7 * 32, d + 64);                                        // randomness
  Fr roots[2];
  deposit_walk(i, depth, [&](uint32_t l) { return (const Fr*)t->level[l]; }, t->dflt, Fr::zero(), c,
               [&](const Fr& a, const Fr& b) {
                 Fr s[3] = {Fr::zero(), a, b};
                 poseidon_permute29<3, false>(s, hc.pos3_rc, hc.pos3_mds29, 57, PoseidonNoEmit{});
                 return s[0];
               },
               [&](uint32_t l, const Fr& sib) { store_be(o + (DEPOSIT_ROW_FIXED + l) * 32, sib); }, roots);
  store_be(o, roots[0]);
  store_be(o + 32, roots[1]);
}
void launch_deposit_rows(hipStream_t st, const GkAffine* table, HashConsts hc, const MerkleTreeDev* t, uint64_t first, const uint8_t* deposits,
                         uint8_t* rows, uint32_t count) {
  if (count) hipLaunchKernelGGL(k_deposit_rows, dim3((count + 63) / 64), dim3(64), 0, st, table, hc, t, first, deposits, rows, count);
}

// ----------------------------------------------------------------------------------------------------
// Wallet sync (demo-frontend/app/lib/storage.ts:9-26,45-50: the DepositRecord a wallet keeps per deposit, rebuilt from its three
// secrets, the tree and the pool's accounts).  What a lane does with the leaf index and why the answers do not depend on
// scheduling is in leaf_index.hpp; the pool's sets are only READ here (pool_set_contains), which pool_table.hpp allows a launch
// that inserts nothing.
//   k_leaf_index_insert   leaves [first, first + n) each claim a slot; never in one launch with a query
//   k_leaf_find           one lane per queried value: lowest index >= from, number of occurrences
//   k_wallet_identity     one lane per secret: owner = sk * G, commitment = H4(owner, amount, randomness), wa_commitment = H2(owner)
//   k_wallet_locate       one lane per secret: the occurrences of the commitment, nullifier = H2(secret_key, index) of each one
//                         examined, the pool's two sets, the note
// Two kernels, so that the Grumpkin ladder and the t = 5 permutation are not live beside the probe loop and its t = 3
// permutation.  The permutations are inlined as in k_withdraw_rows (one call site each; the loop over the occurrences is kept
// rolled for that).  record = commitment | nullifier | wa_commitment | owner_x | owner_y (5 x 32 B big-endian).
// ----------------------------------------------------------------------------------------------------
static constexpr uint32_t WALLET_RECORD_BYTES = 160;
static constexpr uint32_t WALLET_IN_TREE = 1, WALLET_SPENT = 2, WALLET_AUDITED = 4, WALLET_REPEATED = 8;   // include/spp.h, SPP_WALLET_*
__global__ void __launch_bounds__(256) k_leaf_index_insert(LeafIndex ix, const Fr* __restrict__ leaves, uint32_t first, uint32_t n) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < n) leaf_index_insert(ix, leaves, first + g);
}
__global__ void __launch_bounds__(256) k_leaf_find(LeafIndex ix, const Fr* __restrict__ leaves, const uint8_t* __restrict__ keys_be,
                                                   const uint64_t* __restrict__ from, uint64_t* __restrict__ indices,
                                                   uint32_t* __restrict__ matches, uint32_t count) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= count) return;
  uint32_t m = 0;
  const uint32_t i = leaf_index_lowest(ix, leaves, load_be(keys_be + (size_t)g * 32), from ? from[g] : 0, &m);
  indices[g] = i == LEAF_NONE ? ~(uint64_t)0 : i;
  if (matches) matches[g] = m;
}
__global__ void __launch_bounds__(64) k_wallet_identity(const GkAffine* __restrict__ table, HashConsts hc, const uint8_t* __restrict__ deposits,
                                                        uint8_t* __restrict__ records, uint32_t count) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= count) return;
  const uint8_t* d = deposits + (size_t)g * DEPOSIT_BYTES;
  uint8_t* o = records + (size_t)g * WALLET_RECORD_BYTES;
  const GkAffine pk = grumpkin_mul_g(table, load_be(d));             // merkle.ts:98-113 (the key as given, as k_deposit_leaves)
  store_be(o + 96, pk.x);
  store_be(o + 128, pk.y);
  {
    Fr s[5] = {Fr::zero(), pk.x, pk.y, load_be(d + 32), load_be(d + 64)};
    poseidon_permute29<5, false>(s, hc.pos5_rc, hc.pos5_mds29, 60, PoseidonNoEmit{});
    store_be(o, s[0]);                                               // commitment (merkle.ts:126-133, main.nr:69-70)
  }
  Fr s[3] = {Fr::zero(), pk.x, pk.y};
  poseidon_permute29<3, false>(s, hc.pos3_rc, hc.pos3_mds29, 57, PoseidonNoEmit{});
  store_be(o + 64, s[0]);                                            // wa_commitment (main.nr:64-67)
}
// the table covers every leaf of the tree at the call (the insert launch ran before).  has_pool == false: the sets are not read.
__global__ void __launch_bounds__(64) k_wallet_locate(LeafIndex ix, HashConsts hc, const MerkleTreeDev* __restrict__ t, bool has_pool,
                                                      PoolSet nullifiers, PoolSet audits, uint64_t pool_salt,
                                                      const uint8_t* __restrict__ deposits, const uint8_t* __restrict__ recipients,
                                                      uint8_t* __restrict__ records, uint64_t* __restrict__ indices,
                                                      uint32_t* __restrict__ flags, uint8_t* __restrict__ notes, uint32_t count) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= count) return;
  const uint8_t* d = deposits + (size_t)g * DEPOSIT_BYTES;
  uint8_t* o = records + (size_t)g * WALLET_RECORD_BYTES;
  const Fr* leaves = t->level[0];
  const Fr key = load_be(o), sk = load_be(d);
  uint8_t nf[32];
  for (int i = 0; i < 32; i++) nf[i] = 0;
  uint32_t f = 0, idx = LEAF_NONE, matches = 0;
  if (leaf_index_lowest(ix, leaves, key, 0, &matches) != LEAF_NONE) {
    f = WALLET_IN_TREE | (matches > 1 ? WALLET_REPEATED : 0);
    // pass 0: the lowest occurrence whose nullifier is unspent; pass 1, when every one is spent: the lowest.  Without a pool
    // pass 0 takes the lowest.  nf is left holding the nullifier of the occurrence that was taken.
    bool any = !has_pool;
#pragma unroll 1
    for (int pass = 0; pass < 2; pass++) {
      idx = leaf_index_first(ix, leaves, key, 0, [&](uint32_t i) {
        Fr s[3] = {Fr::zero(), sk, Fr::from_u64(i)};
        poseidon_permute29<3, false>(s, hc.pos3_rc, hc.pos3_mds29, 57, PoseidonNoEmit{});   // main.nr:72-74
        s[0].to_bytes_be(nf);
        return any || !pool_set_contains(nullifiers, pool_salt, nf);
      });
      if (idx != LEAF_NONE) break;
      any = true;
    }
    if (has_pool && any) f |= WALLET_SPENT;
  }
  if (has_pool && pool_set_contains(audits, pool_salt, o + 64)) f |= WALLET_AUDITED;
  for (int i = 0; i < 32; i++) o[32 + i] = nf[i];
  indices[g] = idx == LEAF_NONE ? ~(uint64_t)0 : idx;
  flags[g] = f;
  if (notes) {
    uint8_t* nt = notes + (size_t)g * NOTE_BYTES;
    copy32(nt, recipients + (size_t)g * 32);
    copy32(nt + 32, d + 32);                                         // amount
    copy32(nt + 64, d);                                              // secret_key
    copy32(nt + 96, d + 64);                                         // randomness
    // an absent note carries 2^depth: canonical and out of range, a row k_withdraw_rows builds from defaults and the circuit refuses
    const uint64_t word = idx == LEAF_NONE ? (uint64_t)1 << t->depth : idx;
    for (int i = 0; i < 24; i++) nt[128 + i] = 0;
    for (int i = 0; i < 8; i++) nt[152 + i] = (uint8_t)(word >> (8 * (7 - i)));
  }
}
void launch_leaf_index_insert(hipStream_t st, const LeafIndex& ix, const Fr* leaves, uint32_t first, uint32_t n) {
  if (n) hipLaunchKernelGGL(k_leaf_index_insert, dim3((n + 255) / 256), dim3(256), 0, st, ix, leaves, first, n);
}
void launch_leaf_find(hipStream_t st, const LeafIndex& ix, const Fr* leaves, const uint8_t* keys_be, const uint64_t* from, uint64_t* indices,
                      uint32_t* matches, uint32_t count) {
  if (count) hipLaunchKernelGGL(k_leaf_find, dim3((count + 255) / 256), dim3(256), 0, st, ix, leaves, keys_be, from, indices, matches, count);
}
void launch_wallet_sync(hipStream_t st, const GkAffine* table, HashConsts hc, const LeafIndex& ix, const MerkleTreeDev* t, const PoolSet* sets,
                        uint64_t pool_salt, const uint8_t* deposits, const uint8_t* recipients, uint8_t* records, uint64_t* indices,
                        uint32_t* flags, uint8_t* notes, uint32_t count) {
  if (count == 0) return;
  const dim3 grid((count + 63) / 64);
  hipLaunchKernelGGL(k_wallet_identity, grid, dim3(64), 0, st, table, hc, deposits, records, count);
  const PoolSet none{nullptr, nullptr, 0};
  hipLaunchKernelGGL(k_wallet_locate, grid, dim3(64), 0, st, ix, hc, t, sets != nullptr, sets ? sets[0] : none, sets ? sets[1] : none, pool_salt,
                     deposits, recipients, records, indices, flags, notes, count);
}

// ----------------------------------------------------------------------------------------------------
// Poseidon2 t=4 sponge (rate 3) over n field elements per instance; one lane per instance
// ----------------------------------------------------------------------------------------------------
// the permutation itself lives in poseidon2.hpp; nothing is emitted here
__device__ __noinline__ void poseidon2_permute(Fr (&s)[4], const Fr* __restrict__ rc, const Fr* __restrict__ mu) {
  p2_permute<false>(s, rc, mu, Poseidon2NoEmit{});
}
__global__ void __launch_bounds__(64) k_poseidon2_sponge(HashConsts hc, const uint8_t* __restrict__ in_be, uint32_t n,
                                                         uint8_t* __restrict__ out_be, uint32_t count) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= count) return;
  const uint8_t* in = in_be + (size_t)g * n * 32;
  Fr s[4] = {Fr::zero(), Fr::zero(), Fr::zero(), Fr::zero()};
  const uint32_t full = n / 3;
  for (uint32_t i = 0; i < full; i++) {
    s[0] = s[0] + load_be(in + (size_t)(3 * i) * 32);
    s[1] = s[1] + load_be(in + (size_t)(3 * i + 1) * 32);
    s[2] = s[2] + load_be(in + (size_t)(3 * i + 2) * 32);
    poseidon2_permute(s, hc.p2_rc, hc.p2_mu);
  }
  const uint32_t rem = n - 3 * full;
  if (rem >= 1) s[0] = s[0] + load_be(in + (size_t)(3 * full) * 32);
  if (rem >= 2) s[1] = s[1] + load_be(in + (size_t)(3 * full + 1) * 32);
  poseidon2_permute(s, hc.p2_rc, hc.p2_mu);
  store_be(out_be + (size_t)g * 32, s[0]);
}
// Small counts (one audit proof through generateAuditProof, the tail of a batch): one WAVE per instance, the permutation in the
// lane-parallel form the cooperative solver uses (poseidon2.hpp: three dependent products per round instead of eight) -- 53 chained
// permutations are what a single instance waits for.  A wave spends 64 lanes' worth of issue slots on one instance, so large
// counts keep one lane per instance: 2 048 instances are 32 waves there (latency-bound, hidden behind the proving streams) and
// would be 2 048 waves x 53 permutations of chip time here.
__global__ void __launch_bounds__(64) k_poseidon2_sponge_coop(HashConsts hc, const uint8_t* __restrict__ in_be, uint32_t n,
                                                              uint8_t* __restrict__ out_be, uint32_t count) {
  const uint32_t g = blockIdx.x, lane = threadIdx.x;
  if (g >= count) return;
  const uint8_t* in = in_be + (size_t)g * n * 32;
  Fr s = Fr::zero();
  const uint32_t full = n / 3, rem = n - 3 * full;
#pragma unroll 1
  for (uint32_t i = 0; i < full; i++) {
    if (lane < 3) s = s + load_be(in + (size_t)(3 * i + lane) * 32);
    s = coop_p2_permute(hc.p2_rc, hc.p2_mu, s, lane, Poseidon2NoEmit{});
  }
  if (lane < rem) s = s + load_be(in + (size_t)(3 * full + lane) * 32);
  s = coop_p2_permute(hc.p2_rc, hc.p2_mu, s, lane, Poseidon2NoEmit{});
  if (lane == 0) store_be(out_be + (size_t)g * 32, s);
}
void launch_poseidon2_sponge(hipStream_t st, HashConsts hc, const uint8_t* in_be, uint32_t n, uint8_t* out_be, uint32_t count) {
  if (count == 0) return;
  if (count <= 256) hipLaunchKernelGGL(k_poseidon2_sponge_coop, dim3(count), dim3(64), 0, st, hc, in_be, n, out_be, count);
  else hipLaunchKernelGGL(k_poseidon2_sponge, dim3((count + 63) / 64), dim3(64), 0, st, hc, in_be, n, out_be, count);
}


// ----------------------------------------------------------------------------------------------------
// Auditor side: scripts/rlwe_decrypt.py:61-132, demo-frontend/app/lib/shamir.ts:97-169
// ----------------------------------------------------------------------------------------------------
// msg[i] = round(centered((c0 + sk*c1 mod (X^n+1, q))[i]) / Delta) mod 256 for the 64 message slots; one 64-lane block per
// ciphertext, lane i owns slot i:  (sk*c1)[i] = sum_j SK2[(i - j) mod 2048] * c1[j],  SK2 = [sk, (q - sk) mod q].
// Products are 28 x 28 bits: the 64-bit accumulator is folded mod q every 128 terms (ao_decrypt_slot, audit_open.hpp).
__global__ void __launch_bounds__(64) k_rlwe_decrypt(const uint32_t* __restrict__ sk_mod_q, const uint32_t* __restrict__ c0,
                                                     const uint32_t* __restrict__ c1, uint8_t* __restrict__ msg, uint32_t count) {
  __shared__ uint32_t SK2[2 * RL_N];
  __shared__ uint32_t cs[RL_N];
  const uint32_t inst = blockIdx.x, t = threadIdx.x;
  if (inst >= count) return;
  for (int i = t; i < RL_N; i += 64) {
    ao_sk2_entry(sk_mod_q[i], SK2[i], SK2[RL_N + i]);
    cs[i] = c1[(size_t)inst * RL_N + i];
  }
  __syncthreads();
  msg[(size_t)inst * RL_SLOTS + t] = ao_decrypt_slot(SK2, cs, c0[(size_t)inst * RL_SLOTS + t], t);   // audit_open.hpp, shared with k_audit_open
}
void launch_rlwe_decrypt(hipStream_t st, const uint32_t* sk_mod_q, const uint32_t* c0, const uint32_t* c1, uint8_t* msg, uint32_t count) {
  if (count) hipLaunchKernelGGL(k_rlwe_decrypt, dim3(count), dim3(64), 0, st, sk_mod_q, c0, c1, msg, count);
}

// Shamir reconstruction at 0: out[k] = sum_i lambda_i * y[i][k] over Fr, then centred and reduced mod q (shamir.ts:97-120)
__global__ void __launch_bounds__(256) k_shamir_combine(const Fr* __restrict__ lambda, const uint8_t* __restrict__ ys_be, uint32_t t,
                                                        uint32_t n, uint8_t* __restrict__ secret_be, uint32_t* __restrict__ sk_mod_q) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  Fr acc = Fr::zero();
  for (uint32_t i = 0; i < t; i++) acc = acc + lambda[i] * load_be(ys_be + ((size_t)i * n + k) * 32);
  if (secret_be) store_be(secret_be + (size_t)k * 32, acc);
  if (sk_mod_q) {
    uint32_t c[8];
    acc.to_canonical(c);
    sk_mod_q[k] = ao_centred_mod_q(c);   // audit_open.hpp: small for a key coefficient, reduced limb-wise whatever it is
  }
}
void launch_shamir_combine(hipStream_t st, const Fr* lambda, const uint8_t* ys_be, uint32_t t, uint32_t n, uint8_t* secret_be,
                           uint32_t* sk_mod_q) {
  if (n) hipLaunchKernelGGL(k_shamir_combine, dim3((n + 255) / 256), dim3(256), 0, st, lambda, ys_be, t, n, secret_be, sk_mod_q);
}

// ----------------------------------------------------------------------------------------------------
// Auditor key generation (scripts/rlwe_keygen.py:98-182): the key pair, the check of a key, the Shamir sharing of the secret.
// One wavefront per key, lane t owns the coefficients t + 64 j, field 0 of the tables only (rlwe_keygen.hpp has the per-lane
// phases and the bound argument of the chain: twist, two forward transforms, product, inverse transform, untwist).
// ----------------------------------------------------------------------------------------------------
// A <- A * S mod (X^1024 + 1, q) at the lane's coefficients, in (-q, q); A in [0, q), S any int32 per coefficient
__device__ __forceinline__ void rk_negacyclic(uint32_t lane, int32_t (&A)[16], int32_t (&S)[16], int32_t* lds, const RnTables& tb,
                                              int32_t scale) {
  const RnField& f = tb.f[0];
  rk_twist(lane, A, tb.psi[0], f);
  rk_twist(lane, S, tb.psi[0], f);
  rn_ntt1<true>(lane, A, lds, f, tb.w[0][0], 0);
  rn_ntt1<true>(lane, S, lds, f, tb.w[0][0], 0);
  rk_pointwise(A, S, scale, f);
  rn_ntt1<true>(lane, A, lds, f, tb.w[0][1], 1);
  rk_twist(lane, A, tb.ipsi[0], f);
}
// b = e - a * sk mod (X^1024 + 1, q) in [0, q)   (rlwe_keygen.py:110-116); sk_mod_q (optional): sk mod q (:105)
__global__ void __launch_bounds__(64) k_rlwe_keygen(RnTables tb, int32_t scale, const int8_t* __restrict__ sk_in, const uint32_t* __restrict__ a_in,
                                                    const int8_t* __restrict__ e_in, uint32_t* __restrict__ b_out,
                                                    uint32_t* __restrict__ sk_mod_q, uint32_t count) {
  __shared__ int32_t lds[RN_LDS_WORDS];
  const uint32_t inst = blockIdx.x, lane = threadIdx.x;
  if (inst >= count) return;
  const size_t base = (size_t)inst * RL_N;
  int32_t A[16], S[16];
#pragma unroll
  for (int j = 0; j < 16; j++) {
    const uint32_t i = lane + 64 * j;
    A[j] = (int32_t)a_in[base + i];
    S[j] = sk_in[base + i];                  // signed, as it is
    if (sk_mod_q) sk_mod_q[base + i] = (uint32_t)rn_canon(S[j], tb.f[0]);
  }
  rk_negacyclic(lane, A, S, lds, tb, scale);
#pragma unroll
  for (int j = 0; j < 16; j++) {
    const uint32_t i = lane + 64 * j;
    b_out[base + i] = rk_public_b(A[j], e_in[base + i], tb.f[0]);
  }
}
// max_abs[2 inst] = max_i |centred(b + a * sk mod q)_i|, max_abs[2 inst + 1] = max_i |centred(sk_i)|; sk_mod_q in [0, q)
__global__ void __launch_bounds__(64) k_rlwe_key_noise(RnTables tb, int32_t scale, const uint32_t* __restrict__ a_in,
                                                       const uint32_t* __restrict__ b_in, const uint32_t* __restrict__ sk_mod_q,
                                                       uint32_t* __restrict__ max_abs, uint32_t count) {
  __shared__ int32_t lds[RN_LDS_WORDS];
  const uint32_t inst = blockIdx.x, lane = threadIdx.x;
  if (inst >= count) return;
  const size_t base = (size_t)inst * RL_N;
  int32_t A[16], S[16];
  uint32_t msk = 0, mnoise = 0;
#pragma unroll
  for (int j = 0; j < 16; j++) {
    const uint32_t i = lane + 64 * j;
    A[j] = (int32_t)a_in[base + i];
    S[j] = (int32_t)sk_mod_q[base + i];
    msk = rk_max(msk, rk_abs_centred((uint32_t)S[j], tb.f[0]));
  }
  rk_negacyclic(lane, A, S, lds, tb, scale);
#pragma unroll
  for (int j = 0; j < 16; j++) mnoise = rk_max(mnoise, rk_noise(b_in[base + lane + 64 * j], A[j], tb.f[0]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mnoise = rk_max(mnoise, (uint32_t)__shfl_xor((int)mnoise, o, 64));
    msk = rk_max(msk, (uint32_t)__shfl_xor((int)msk, o, 64));
  }
  if (lane == 0) {
    max_abs[2 * (size_t)inst] = mnoise;
    max_abs[2 * (size_t)inst + 1] = msk;
  }
}
void launch_rlwe_keygen(hipStream_t st, const RlweDev& rd, const int8_t* sk, const uint32_t* a, const int8_t* e, uint32_t* b,
                        uint32_t* sk_mod_q, uint32_t count) {
  if (count) hipLaunchKernelGGL(k_rlwe_keygen, dim3(count), dim3(64), 0, st, rd.tb, rd.pk_scale[0], sk, a, e, b, sk_mod_q, count);
}
void launch_rlwe_key_noise(hipStream_t st, const RlweDev& rd, const uint32_t* a, const uint32_t* b, const uint32_t* sk_mod_q,
                           uint32_t* max_abs, uint32_t count) {
  if (count) hipLaunchKernelGGL(k_rlwe_key_noise, dim3(count), dim3(64), 0, st, rd.tb, rd.pk_scale[0], a, b, sk_mod_q, max_abs, count);
}

// Shamir sharing (shamir_share_field, rlwe_keygen.py:51-65): y[j][i] = sum_k c_k[i] x_j^k over Fr by Horner, c_0 = secret[i],
// c_k at coeffs_be[(k - 1) n + i].  One lane per (value i, share j), i fastest: the loads of a wave are consecutive values.
// ys_be is share-major, what k_shamir_combine reads.
__global__ void __launch_bounds__(256) k_shamir_split(const Fr* __restrict__ xs, const uint8_t* __restrict__ secrets_be,
                                                      const uint8_t* __restrict__ coeffs_be, uint32_t t, uint32_t m, uint32_t n,
                                                      uint8_t* __restrict__ ys_be) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;   // m n <= 255 * 2^20
  if (g >= m * n) return;
  const uint32_t j = g / n, i = g % n;
  const Fr x = xs[j];
  Fr acc = Fr::zero();
  for (uint32_t k = t - 1; k >= 1; k--) acc = (acc + load_be(coeffs_be + ((size_t)(k - 1) * n + i) * 32)) * x;
  acc = acc + load_be(secrets_be + (size_t)i * 32);
  store_be(ys_be + ((size_t)j * n + i) * 32, acc);
}
void launch_shamir_split(hipStream_t st, const Fr* xs, const uint8_t* secrets_be, const uint8_t* coeffs_be, uint32_t t, uint32_t m,
                         uint32_t n, uint8_t* ys_be) {
  const uint32_t lanes = m * n;
  if (lanes) hipLaunchKernelGGL(k_shamir_split, dim3((lanes + 255) / 256), dim3(256), 0, st, xs, secrets_be, coeffs_be, t, m, n, ys_be);
}

// ----------------------------------------------------------------------------------------------------
// Opening audit records (scripts/rlwe_decrypt.py:61-149 plus the two checks it leaves out, see include/spp.h): one 64-lane wave
// per 64 records, in two phases that each use the lanes the way their work is shaped.
//   phase 1, the wave on one record at a time: its ciphertext (c0 64 + c1 1024 words, 4 352 B) goes into LDS with coalesced
//     16-byte loads; every coefficient is checked against q (__any over the wave); lane t decrypts message slot t with the loop
//     and rounding of k_rlwe_decrypt (audit_open.hpp) against the doubled secret key, which is built in LDS once per block and
//     serves all 64 records; the byte goes to the owner record and to a 64 x 64-byte LDS tile.
//   phase 2, one lane per record: the 157 packed fields (pack_values: 7 x 32 bits) are formed word by word from the record's
//     coefficients -- read a second time, per lane at a 4 KB stride -- and absorbed three at a time into the Poseidon2 sponge, so the packed
//     row never exists in memory; then the lane reads its record's two 256-bit integers from the tile: both < r, y^2 = x^3 - 17,
//     H(x, y) by the t = 3 Poseidon; then the two hashes against the words of the public witness, bytewise (ao_decide), or-ed
//     with the verdict of k_verify, which ran before on the same stream (proof_ok; nullptr: no verification asked for).
// Why the sponge is not the lane-parallel one of poseidon2.hpp: 53 chained permutations per record are the bulk of the work, and a
// wave that spends its 64 lanes on one record's permutation pays about 25 times the issue slots per record of a wave whose lanes
// hold 64 records (launch_poseidon2_sponge draws the same line at 256 instances).  By the figure DESIGN.md gives for the wave
// form of the sponge (2 048 instances = about 12 ms of a saturated chip) that would be about 0.2 s at 2^15 records (an estimate);
// measured in this form (profiles/audit_open_kernel_stats.csv): 22.3 ms per launch at 2^15 records, against 20.0 + 0.45 + 0.43 ms
// for k_poseidon2_sponge, k_rlwe_decrypt and k_poseidon_hash on the same records, and 207 ms for k_verify in front of it -- the
// latency of one sponge chain either way, second read of the ciphertext included.  Small batches pay for the choice: a single
// record is one wave of the chip.
// LDS per block: 8 KB key + 4.25 KB ciphertext + 4.25 KB tile = 16.6 KB; a block is one wave and 2^15 records are 512 blocks on
// 256 CUs, so neither LDS nor registers limit what is resident.
// ----------------------------------------------------------------------------------------------------
// ct_commitment of one record by one lane: the rate-3 sponge over the 157 packed fields (ct_helper/src/main.nr:15-34),
// 157 = 52 * 3 + 1, the fields formed word by word from the record's coefficients
__device__ __forceinline__ Fr ao_ct_commitment_lane(const HashConsts& hc, const uint32_t* my0, const uint32_t* my1) {
  Fr s[4] = {Fr::zero(), Fr::zero(), Fr::zero(), Fr::zero()};
#pragma unroll 1
  for (uint32_t i = 0; i < AO_FIELDS / 3; i++) {
    SPP_UNROLL for (uint32_t j = 0; j < 3; j++) s[j] = s[j] + ao_packed_field(my0, my1, 3 * i + j);
    poseidon2_permute(s, hc.p2_rc, hc.p2_mu);
  }
  static_assert(AO_FIELDS % 3 == 1, "one field left for the last absorption");
  s[0] = s[0] + ao_packed_field(my0, my1, AO_FIELDS - 1);
  poseidon2_permute(s, hc.p2_rc, hc.p2_mu);
  return s[0];
}
static constexpr uint32_t AO_TILE_STRIDE = 68;   // bytes per record in the message tile: 17 words, so the lanes of phase 2 spread over the banks
// PARTIALS: the threshold form (rlwe_partial.hpp).  No key: sk_mod_q is then the table k_rlwe_combine left, count * 64 residues
// (sk * c1)[t] mod q, read where the other form sums SK2 against c1, and bad_partials[i] != 0 adds bit 8.  All the rest is shared.
template <bool PARTIALS>
__global__ void __launch_bounds__(64) k_audit_open(HashConsts hc, const uint32_t* __restrict__ sk_mod_q, const uint32_t* __restrict__ c0,
                                                   const uint32_t* __restrict__ c1, const uint8_t* __restrict__ pws,
                                                   const int32_t* __restrict__ proof_ok, const uint32_t* __restrict__ bad_partials,
                                                   uint8_t* __restrict__ owners, uint32_t* __restrict__ flags, uint32_t count) {
  __shared__ uint32_t SK2[PARTIALS ? 1 : 2 * AO_N];
  __shared__ __attribute__((aligned(16))) uint32_t ct[AO_CT_WORDS];
  __shared__ __attribute__((aligned(4))) uint8_t tile[64 * AO_TILE_STRIDE];
  __shared__ uint8_t coeff_bad[64];
  const uint32_t lane = threadIdx.x, first = blockIdx.x * 64;
  if (first >= count) return;
  const uint32_t nrec = count - first < 64 ? count - first : 64;
  if (!PARTIALS)
    for (uint32_t i = lane; i < AO_N; i += 64) ao_sk2_entry(sk_mod_q[i], SK2[i], SK2[AO_N + i]);
  // ---- phase 1 ----
#pragma unroll 1
  for (uint32_t k = 0; k < nrec; k++) {
    const size_t inst = (size_t)first + k;
    bool bad = false;
    ct[lane] = ao_coeff(c0[inst * AO_SLOTS + lane], bad);
    const uint4* src = reinterpret_cast<const uint4*>(c1 + inst * AO_N);   // rows of 4 KB: 16-byte aligned
#pragma unroll
    for (uint32_t j = 0; j < AO_N / 4 / 64; j++) {
      const uint32_t i = lane + 64 * j;
      uint4 v = src[i];
      v.x = ao_coeff(v.x, bad); v.y = ao_coeff(v.y, bad); v.z = ao_coeff(v.z, bad); v.w = ao_coeff(v.w, bad);
      reinterpret_cast<uint4*>(ct + AO_SLOTS)[i] = v;
    }
    const bool any_bad = __any(bad ? 1 : 0) != 0;
    if (lane == 0) coeff_bad[k] = any_bad ? 1 : 0;
    __syncthreads();
    const uint8_t m = PARTIALS ? ao_round_slot(ct[lane], sk_mod_q[inst * AO_SLOTS + lane]) : ao_decrypt_slot(SK2, ct + AO_SLOTS, ct[lane], lane);
    tile[k * AO_TILE_STRIDE + lane] = m;
    owners[inst * 64 + ao_owner_byte(lane)] = m;               // always written, whatever the decisions below
    __syncthreads();                                            // ct is overwritten by the next record
  }
  if (lane >= nrec) return;
  // ---- phase 2: ct_commitment (ao_ct_commitment_lane), then the identity ----
  const size_t inst = (size_t)first + lane;
  uint8_t ct_be[32], wa_be[32];
  ao_ct_commitment_lane(hc, c0 + inst * AO_SLOTS, c1 + inst * AO_N).to_bytes_be(ct_be);
  uint32_t x[8], y[8];
  ao_owner_limbs(tile + lane * AO_TILE_STRIDE, x, y);
  Fr fx, fy;
  const bool point_ok = ao_owner_on_curve(x, y, &fx, &fy);
  if (point_ok) poseidon_hash2(hc, fx, fy).to_bytes_be(wa_be);
  uint32_t f = ao_decide(coeff_bad[lane] != 0, ct_be, point_ok, wa_be, pws + inst * 76);
  if (proof_ok && !proof_ok[inst]) f |= AO_BAD_PROOF;
  if (PARTIALS && bad_partials[inst]) f |= RP_BAD_PARTIALS;
  flags[inst] = f;
}
void launch_audit_open(hipStream_t st, HashConsts hc, const uint32_t* sk_mod_q, const uint32_t* c0, const uint32_t* c1, const uint8_t* pws,
                       const int32_t* proof_ok, uint8_t* owners, uint32_t* flags, uint32_t count) {
  if (count)
    hipLaunchKernelGGL(k_audit_open<false>, dim3((count + 63) / 64), dim3(64), 0, st, hc, sk_mod_q, c0, c1, pws, proof_ok, (const uint32_t*)nullptr,
                       owners, flags, count);
}
void launch_audit_open_partials(hipStream_t st, HashConsts hc, const uint32_t* residues, const uint32_t* bad_partials, const uint32_t* c0,
                                const uint32_t* c1, const uint8_t* pws, const int32_t* proof_ok, uint8_t* owners, uint32_t* flags, uint32_t count) {
  if (count)
    hipLaunchKernelGGL(k_audit_open<true>, dim3((count + 63) / 64), dim3(64), 0, st, hc, residues, c0, c1, pws, proof_ok, bad_partials, owners,
                       flags, count);
}

// ----------------------------------------------------------------------------------------------------
// Threshold opening (rlwe_partial.hpp): an auditor's partial decryptions from its own share, and their combination
// ----------------------------------------------------------------------------------------------------
// the scaled share, once per call: U[1024 i + j] = limb i of lambda * s[j], the limb-major table rp_dot_slot reads
__global__ void __launch_bounds__(256) k_partial_scale(Fr lambda, const uint8_t* __restrict__ share_be, uint32_t* __restrict__ U) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= AO_N) return;
  uint8_t s[32];
  for (int i = 0; i < 32; i++) s[i] = share_be[(size_t)j * 32 + i];
  uint32_t u[RP_LIMBS];
  rp_scaled_share(lambda, s, u);
  SPP_UNROLL for (uint32_t i = 0; i < RP_LIMBS; i++) U[AO_N * i + j] = u[i];
}
// One 64-lane block per record, lane k owns slot k.  The table (32 KB) and the ciphertext (4.25 KB) go into LDS with 16-byte
// loads; the wave computes the record's ct_commitment with the lane-parallel sponge (poseidon2.hpp: 53 chained permutations over
// the 157 packed fields, formed from the ciphertext in LDS) -- the value the masks are keyed by is the one of the c0 and c1 in
// hand; then each lane runs its wide dot product against the table (consecutive lanes read consecutive words of a limb row: no
// bank is read twice; c1[j] is one address for the wave), adds its blinding and writes 32 bytes.
// LDS per block 36.4 KB: four blocks per CU, one wave per SIMD -- the dot product's sixteen-term unrolled body is what keeps a
// lone wave's LDS reads in flight.
// ct_in: the commitments are there already (k_partial_commit, large batches: launch_rlwe_partial draws the line) and the wave
// does not hash; otherwise it does and leaves them in ct_out.
__global__ void __launch_bounds__(64) k_rlwe_partial(HashConsts hc, const uint32_t* __restrict__ U_dev, uint32_t t, const uint32_t* __restrict__ xs,
                                                     uint32_t self, const uint8_t* __restrict__ seeds, const uint32_t* __restrict__ c0,
                                                     const uint32_t* __restrict__ c1, const int32_t* __restrict__ e,
                                                     const unsigned long long* __restrict__ rho, uint8_t* __restrict__ partials,
                                                     const uint8_t* __restrict__ ct_in, uint8_t* __restrict__ ct_out, uint32_t count) {
  __shared__ __attribute__((aligned(16))) uint32_t U[RP_TABLE_WORDS];
  __shared__ __attribute__((aligned(16))) uint32_t ct[AO_CT_WORDS];
  __shared__ uint8_t ct_be[32];
  const uint32_t lane = threadIdx.x;
  const size_t inst = blockIdx.x;
  if (inst >= count) return;
  {
    const uint4* src = reinterpret_cast<const uint4*>(U_dev);
#pragma unroll 4
    for (uint32_t i = lane; i < RP_TABLE_WORDS / 4; i += 64) reinterpret_cast<uint4*>(U)[i] = src[i];
    ct[lane] = c0[inst * AO_SLOTS + lane];
    const uint4* s1 = reinterpret_cast<const uint4*>(c1 + inst * AO_N);      // rows of 4 KB: 16-byte aligned
#pragma unroll
    for (uint32_t j = 0; j < AO_N / 4 / 64; j++) reinterpret_cast<uint4*>(ct + AO_SLOTS)[lane + 64 * j] = s1[lane + 64 * j];
  }
  __syncthreads();
  if (ct_in) {
    if (lane < 32) ct_be[lane] = ct_in[inst * 32 + lane];
  } else {
    // ---- ct_commitment: the rate-3 sponge over the packed fields (ct_helper/src/main.nr:15-34), lanes 0..2 absorb ----
    Fr s = Fr::zero();
#pragma unroll 1
    for (uint32_t i = 0; i < AO_FIELDS / 3; i++) {
      if (lane < 3) s = s + ao_packed_field(ct, ct + AO_SLOTS, 3 * i + lane);
      s = coop_p2_permute(hc.p2_rc, hc.p2_mu, s, lane, Poseidon2NoEmit{});
    }
    static_assert(AO_FIELDS % 3 == 1, "one field left for the last absorption");
    if (lane == 0) s = s + ao_packed_field(ct, ct + AO_SLOTS, AO_FIELDS - 1);
    s = coop_p2_permute(hc.p2_rc, hc.p2_mu, s, lane, Poseidon2NoEmit{});
    if (lane == 0) {
      uint8_t buf[32];
      s.to_bytes_be(buf);
      for (int i = 0; i < 32; i++) ct_be[i] = buf[i];
      for (int i = 0; i < 32; i++) ct_out[inst * 32 + i] = buf[i];
    }
  }
  __syncthreads();
  // ---- the slot ----
  const Fr d = rp_dot_slot(U, ct + AO_SLOTS, lane);
  uint8_t key[32];
  for (int i = 0; i < 32; i++) key[i] = ct_be[i];
  const size_t slot = inst * AO_SLOTS + lane;
  const Fr b = rp_blind_slot(e ? e[slot] : 0, rho ? rho[slot] : 0ull, t, xs, self, seeds, key, lane);
  store_be(partials + slot * RP_PARTIAL_LEN, d + b);
}
// The commitments of a large batch, one LANE per record (the sponge of k_audit_open's phase 2): 53 chained permutations cost a wave
// the same whether its lanes hold one record or 64, so from RP_COOP_SPONGE_MAX records on the wave form above would be the bulk
// of the call.  Measured at 2^15 records: 246 ms per launch with the sponge inside k_rlwe_partial; in this form 20.0 ms here and
// 2.4 ms for k_rlwe_partial (profiles/partial_decrypt_kernel_stats.csv).
__global__ void __launch_bounds__(64) k_partial_commit(HashConsts hc, const uint32_t* __restrict__ c0, const uint32_t* __restrict__ c1,
                                                       uint8_t* __restrict__ ct_be, uint32_t count) {
  const size_t g = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (g >= count) return;
  store_be(ct_be + g * 32, ao_ct_commitment_lane(hc, c0 + g * AO_SLOTS, c1 + g * AO_N));
}
// One 64-lane block per record: lane k sums slot k of the t partials (auditor-major: partial i of record r at (i count + r) 64 + k),
// centres the sum and reduces it mod q (rp_combine_residue).  residues / msg / flags: each optional; msg needs c0 (below q).
__global__ void __launch_bounds__(64) k_rlwe_combine(uint32_t t, const uint8_t* __restrict__ partials, const uint32_t* __restrict__ c0,
                                                     uint32_t* __restrict__ residues, uint8_t* __restrict__ msg, uint32_t* __restrict__ flags,
                                                     uint32_t count) {
  const uint32_t lane = threadIdx.x;
  const size_t inst = blockIdx.x;
  if (inst >= count) return;
  const size_t slot = inst * AO_SLOTS + lane;
  Fr acc = Fr::zero();
  for (uint32_t i = 0; i < t; i++) acc = acc + load_be(partials + ((size_t)i * count * AO_SLOTS + slot) * RP_PARTIAL_LEN);
  uint32_t w[8];
  acc.to_canonical(w);
  bool bad = false;
  const uint32_t res = rp_combine_residue(w, bad);
  const bool any_bad = __any(bad ? 1 : 0) != 0;
  if (residues) residues[slot] = res;
  if (msg) msg[slot] = ao_round_slot(c0[slot], res);
  if (flags && lane == 0) flags[inst] = any_bad ? RP_BAD_PARTIALS : 0u;
}
void launch_partial_scale(hipStream_t st, const Fr& lambda, const uint8_t* share_be, uint32_t* U) {
  hipLaunchKernelGGL(k_partial_scale, dim3(AO_N / 256), dim3(256), 0, st, lambda, share_be, U);
}
void launch_rlwe_partial(hipStream_t st, HashConsts hc, const uint32_t* U, uint32_t t, const uint32_t* xs, uint32_t self, const uint8_t* seeds,
                         const uint32_t* c0, const uint32_t* c1, const int32_t* e, const uint64_t* rho, uint8_t* partials, uint8_t* ct_be,
                         uint32_t count) {
  if (count == 0) return;
  // one record's sponge is 53 chained permutations either way: a wave per record (inside k_rlwe_partial) while the chip has
  // room for all of them at once and a few rounds more, a lane per record beyond that (launch_poseidon2_sponge draws its line
  // the same way; four blocks per CU here: 1 024 in flight)
  const bool lanes = count > RP_COOP_SPONGE_MAX;
  if (lanes) hipLaunchKernelGGL(k_partial_commit, dim3((count + 63) / 64), dim3(64), 0, st, hc, c0, c1, ct_be, count);
  hipLaunchKernelGGL(k_rlwe_partial, dim3(count), dim3(64), 0, st, hc, U, t, xs, self, seeds, c0, c1, e, (const unsigned long long*)rho, partials,
                     lanes ? ct_be : (const uint8_t*)nullptr, lanes ? (uint8_t*)nullptr : ct_be, count);
}
void launch_rlwe_combine(hipStream_t st, uint32_t t, const uint8_t* partials, const uint32_t* c0, uint32_t* residues, uint8_t* msg, uint32_t* flags,
                         uint32_t count) {
  if (count) hipLaunchKernelGGL(k_rlwe_combine, dim3(count), dim3(64), 0, st, t, partials, c0, residues, msg, flags, count);
}

// ----------------------------------------------------------------------------------------------------
// audit input assembly: (sk, r, e1, e2) -> the 3360-field input row of the audit circuit, all on the device
// (scripts/generate_audit.py:468-641: keygen, message slots, encryption + quotients, packing, commitments, Prover.toml)
// ----------------------------------------------------------------------------------------------------
// message = little-endian bytes of owner_x then owner_y (generate_audit.py:489-496); xy_be is 64 B big-endian per key
__global__ void __launch_bounds__(256) k_audit_msg(const uint8_t* __restrict__ xy_be, uint8_t* __restrict__ msg, uint32_t count) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= count * 64) return;
  const uint32_t inst = g / 64, s = g % 64;
  msg[g] = xy_be[(size_t)inst * 64 + (s < 32 ? 31 - s : 32 + 31 - (s - 32))];
}
__device__ __forceinline__ void store_small_signed_be(uint8_t* o, int32_t v) {
  // field encoding of a small signed integer (format_field, generate_audit.py:77-82): v >= 0 -> v, v < 0 -> r - |v|
  const uint8_t RBE[32] = {0x30, 0x64, 0x4e, 0x72, 0xe1, 0x31, 0xa0, 0x29, 0xb8, 0x50, 0x45, 0xb6, 0x81, 0x81, 0x58, 0x5d,
                           0x28, 0x33, 0xe8, 0x48, 0x79, 0xb9, 0x70, 0x91, 0x43, 0xe1, 0xf5, 0x93, 0xf0, 0x00, 0x00, 0x01};
  uint32_t low;
  if (v >= 0) {
    for (int i = 0; i < 28; i++) o[i] = 0;
    low = (uint32_t)v;
  } else {
    for (int i = 0; i < 28; i++) o[i] = RBE[i];
    low = 0xf0000001u - (uint32_t)(-(int64_t)v);   // |v| <= 2^31 < 0xf0000001: no borrow into the upper limbs
  }
  o[28] = (uint8_t)(low >> 24); o[29] = (uint8_t)(low >> 16); o[30] = (uint8_t)(low >> 8); o[31] = (uint8_t)low;
}
static constexpr uint32_t AUDIT_NIN = 3360;
__global__ void __launch_bounds__(256) k_audit_assemble(const uint8_t* __restrict__ wa_be, const uint8_t* __restrict__ ct_be,
                                                        const uint8_t* __restrict__ packed_be, const uint8_t* __restrict__ sk_be,
                                                        const int8_t* __restrict__ r, const int8_t* __restrict__ e1, const int8_t* __restrict__ e2,
                                                        const int32_t* __restrict__ k0, const int32_t* __restrict__ k1,
                                                        uint8_t* __restrict__ rows, uint32_t count) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (uint64_t)count * AUDIT_NIN) return;
  const uint32_t inst = (uint32_t)(g / AUDIT_NIN), f = (uint32_t)(g % AUDIT_NIN);
  uint8_t* o = rows + g * 32;
  const uint8_t* src = nullptr;
  if (f == 0) src = wa_be + (size_t)inst * 32;
  else if (f == 1) src = ct_be + (size_t)inst * 32;
  else if (f < 2 + 157) src = packed_be + ((size_t)inst * 157 + (f - 2)) * 32;
  else if (f == 159) src = sk_be + (size_t)inst * 32;
  if (src) {
    for (int i = 0; i < 32; i++) o[i] = src[i];
    return;
  }
  uint32_t k = f - 160;
  int32_t v;
  if (k < 1024) v = r[(size_t)inst * 1024 + k];
  else if ((k -= 1024) < 64) v = e1[(size_t)inst * 64 + k];
  else if ((k -= 64) < 1024) v = e2[(size_t)inst * 1024 + k];
  else if ((k -= 1024) < 64) v = k0[(size_t)inst * 64 + k];
  else v = k1[(size_t)inst * 1024 + (k - 64)];
  store_small_signed_be(o, v);
}
void launch_audit_msg(hipStream_t st, const uint8_t* xy_be, uint8_t* msg, uint32_t count) {
  if (count) hipLaunchKernelGGL(k_audit_msg, dim3((count * 64 + 255) / 256), dim3(256), 0, st, xy_be, msg, count);
}
void launch_audit_assemble(hipStream_t st, const uint8_t* wa_be, const uint8_t* ct_be, const uint8_t* packed_be, const uint8_t* sk_be,
                           const int8_t* r, const int8_t* e1, const int8_t* e2, const int32_t* k0, const int32_t* k1, uint8_t* rows,
                           uint32_t count) {
  uint64_t lanes = (uint64_t)count * AUDIT_NIN;
  if (count) hipLaunchKernelGGL(k_audit_assemble, dim3((uint32_t)((lanes + 255) / 256)), dim3(256), 0, st, wa_be, ct_be, packed_be, sk_be, r, e1, e2, k0, k1, rows, count);
}

}  // namespace spp
