// Internals shared by the translation units of libspp's C ABI.  Not installed; include/spp.h is the ABI.
//   spp_api.cpp          error channel, contexts, the stream-concurrency probe
//   spp_circuit.hpp      (private, on top of this header) struct spp_circuit, its workspaces and what the four units below share
//   spp_plan.cpp         load-time planners: cooperative-solver items, small and long rows of the matrix evaluation
//   spp_load.cpp         proving-key container, window plan and tables, circuit loading and queries, fixed-base MSM unit calls,
//                        the experiment switches of the proving path from the environment (read_switches)
//   spp_prove.cpp        workspaces, the proving pipeline and its batch entry points, timing queries
//   spp_setup.cpp        circuit construction (host only) and the trusted setup on the GPU
//   spp_witness_api.cpp  witness-input kernels, Merkle trees, their leaf index (wallet sync) and earlier sizes (merkle_prefix.hpp), auditor side
//   spp_verify_api.cpp   verification and pairing checks
//   spp_audit_api.cpp    opening audit records: verification, ciphertext binding, decryption, identity binding in one pass
//   spp_pool_api.cpp     the pool ledger: root ring, nullifier and audit-record sets, settling submit_audit / withdraw batches
//   spp_deposit_api.cpp  deposit proofs: rows from the resident tree, the check of a log of proved deposits (spp_prove_deposits itself is in spp_prove.cpp)
//   spp_withdrawals_api.cpp  the withdrawal plan: which notes of a batch still need an audit record (spp_prove_withdrawals itself is in spp_prove.cpp)
//   spp_ceremony_api.cpp the setup ceremony: contributions to a key's delta and to its sigma, their receipts and verifiers, the scaling unit call
//   spp_vss_api.cpp      the auditors' key without a dealer: verifiable sharing, the receiver's check, the sum of sub-shares
//   spp_ptau_api.cpp     the ceremony's first phase: the powers-of-tau transcript, the derivation of a circuit's keys from it, unit calls
//   spp_micro_api.cpp    the NTT / Pippenger unit and micro-benchmark entry points, the raw-word arithmetic probe (spp_debug_arith)
#pragma once
#include "../../include/spp.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "circuit.hpp"
#include "kernels.hpp"
#include "sha256.hpp"
#include "f29.hpp"
#include "pairing.hpp"
#include "pairing_fast_host.hpp"

using namespace spp;

// -----------------------------------------------------------------------------------------------------
// errors: negative SPP_ERR_* codes + a thread-local message (spp_last_error)
// -----------------------------------------------------------------------------------------------------
extern thread_local char g_spp_err[512];
inline int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_spp_err, sizeof g_spp_err, fmt, ap);
  va_end(ap);
  return code;
}
#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) return fail(SPP_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e));     \
  } while (0)

// -----------------------------------------------------------------------------------------------------
// host helpers
// -----------------------------------------------------------------------------------------------------
inline Fr fr_pow_limbs(const Fr& base, const uint32_t e[8]) {
  Fr acc = Fr::one(), b = base;
  for (int w = 0; w < 8; w++)
    for (int i = 0; i < 32; i++) {
      if ((e[w] >> i) & 1) acc = acc * b;
      b = b.sqr();
    }
  return acc;
}
inline Fr fr_root_of_unity(uint32_t logn) {
  uint32_t e[8];
  for (int i = 0; i < 8; i++) e[i] = FrParams::MOD(i);
  e[0] -= 1;
  for (uint32_t s = 0; s < logn; s++) {
    for (int i = 0; i < 7; i++) e[i] = (e[i] >> 1) | (e[i + 1] << 31);
    e[7] >>= 1;
  }
  return fr_pow_limbs(Fr::from_u64(5), e);
}
inline uint32_t bitrev(uint32_t v, uint32_t bits) {
  uint32_t r = 0;
  for (uint32_t i = 0; i < bits; i++) r |= ((v >> i) & 1) << (bits - 1 - i);
  return r;
}
inline G1Affine g1_from_raw(const uint8_t* b) {
  bool z = true;
  for (int i = 0; i < 64; i++) z &= b[i] == 0;
  if (z) return G1Affine::infinity();
  return {Fq::from_bytes_be(b), Fq::from_bytes_be(b + 32)};
}
inline G2Affine g2_from_raw(const uint8_t* b) {
  bool z = true;
  for (int i = 0; i < 128; i++) z &= b[i] == 0;
  if (z) return G2Affine::infinity();
  G2Affine p;
  p.x.c1 = Fq::from_bytes_be(b);
  p.x.c0 = Fq::from_bytes_be(b + 32);
  p.y.c1 = Fq::from_bytes_be(b + 64);
  p.y.c0 = Fq::from_bytes_be(b + 96);
  return p;
}
inline void g1_to_raw(const G1Affine& p, uint8_t* b) {
  if (p.is_inf()) { memset(b, 0, 64); return; }
  p.x.to_bytes_be(b);
  p.y.to_bytes_be(b + 32);
}
inline void g2_to_raw(const G2Affine& p, uint8_t* b) {
  if (p.is_inf()) { memset(b, 0, 128); return; }
  p.x.c1.to_bytes_be(b);
  p.x.c0.to_bytes_be(b + 32);
  p.y.c1.to_bytes_be(b + 64);
  p.y.c0.to_bytes_be(b + 96);
}
template <class F>
inline Affine<F> host_add(const Affine<F>& a, const Affine<F>& b) {
  XYZZ<F> x = XYZZ<F>::from_affine(a);
  x.madd(b);
  return x.to_affine();
}
inline bool read_file(const char* path, std::vector<uint8_t>& out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  long sz = ftell(f);
  fseek(f, 0, SEEK_SET);
  out.resize((size_t)sz);
  bool ok = fread(out.data(), 1, out.size(), f) == out.size();
  fclose(f);
  return ok;
}

template <class T>
inline hipError_t dev_upload(T** dst, const std::vector<T>& src) {
  *dst = nullptr;
  size_t bytes = sizeof(T) * std::max<size_t>(src.size(), 1);
  hipError_t e = hipMalloc((void**)dst, bytes);
  if (e != hipSuccess) return e;
  if (!src.empty()) e = hipMemcpy(*dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice);
  return e;
}

// -----------------------------------------------------------------------------------------------------
// context / circuit objects
// -----------------------------------------------------------------------------------------------------
static constexpr int SPP_NWS = 6;   // batch workspaces / proving streams per circuit (big batches use two)
struct spp_ctx {
  int device;
  hipStream_t stream;        // setup / table construction
  hipStream_t pstream[SPP_NWS];   // proving: consecutive batches take the streams in turn, so the (latency-bound, few-wave)
                                  // witness solver of batch k+1 overlaps the MSMs of batch k; small batches use up to six
  std::mutex mu;
  // lazily created constants: hc is read by the stand-alone witness kernels and by the solver of every circuit of the context
  bool consts_ready = false;
  HashConsts hc{};
  GkAffine* gk_table = nullptr;
  bool rlwe_ready = false;
  RlweDev rlwe{};              // NTT tables of the RLWE witness kernel (rlwe_ntt.hpp)
  G1Affine* vss_table = nullptr;   // window table of the sharing's two generators (vss.hpp), built by the first spp_vss_* call
  // temporaries of spp_audit_inputs_batch(_device), kept between calls (grow only): a hipFree per call would drain every
  // stream of the device, the proving streams of the batch in flight included
  void* audit_scratch = nullptr;
  size_t audit_scratch_cap = 0;
  std::vector<void*> owned;
};
// incremental tree: ShieldedPoolMerkleTree (client/merkle.ts:146-222) with the levels kept in HBM (spp_witness_api.cpp)
struct spp_merkle_tree {
  spp_ctx* ctx = nullptr;
  uint32_t depth = 0;
  uint64_t n_leaves = 0, cap_leaves = 0;       // capacity of level 0 (level l holds cap_leaves >> l, + 1)
  MerkleTreeDev host{};                        // host mirror of the device descriptor
  MerkleTreeDev* dev = nullptr;
  Fr* d_dflt = nullptr;                        // depth + 1 default hashes
  // the leaf index (leaf_index.hpp), built lazily by spp_merkle_tree_find / spp_wallet_sync and by nothing else: it covers leaves
  // [0, indexed) in index_slots slots; the salt is drawn when it is first built
  uint32_t* d_index = nullptr;
  uint32_t index_slots = 0;
  uint64_t indexed = 0, index_salt = 0;
  bool index_salted = false;
  // the tree as of an earlier size (merkle_prefix.hpp), all lazily made by the _at calls, spp_merkle_tree_prefix_roots / _find_roots
  // and spp_pool_root_sizes and by nothing else:
  Fr* d_frontier = nullptr;                    // 33 words: F[0..depth] of the as-of call last enqueued on the context's stream
  Fr* d_roots = nullptr;                       // R[n], n < roots_done, room for roots_cap: extended, never recomputed
  uint64_t roots_cap = 0, roots_done = 0;
  uint32_t* d_root_index = nullptr;            // a second leaf index, over d_roots (same salt): entries [0, roots_indexed)
  uint32_t root_index_slots = 0;
  uint64_t roots_indexed = 0;
};
// Resolves and checks `size` of an as-of call (SPP_TREE_SIZE_NOW, or <= the tree's size: else SPP_ERR_BAD_INPUT naming both) and
// enqueues k_merkle_frontier for it on the context's stream, into t->d_frontier.  ctx->mu held, device set, constants ready
// (spp_witness_api.cpp).
int spp_tree_frontier_enqueue(spp_merkle_tree* t, uint64_t* size);
// the pool's two resident sets (SPP_POOL_NULLIFIERS, SPP_POOL_AUDIT_RECORDS) and their salt, for a launch that only reads them
// (spp_pool_api.cpp).  Returns the pool's context; sets (two entries) and salt are written when sets is not NULL, which needs that
// context locked
struct spp_pool;
spp_ctx* spp_pool_view(spp_pool* p, PoolSet* sets, uint64_t* salt);
// current_root, then roots[0..31] of the pool's ring as spp_pool_state lays them out: 33 x 32 B.  Needs the pool's context locked
void spp_pool_ring_words(spp_pool* p, uint8_t words[33 * 32]);
// The withdrawal plan as stream-ordered work on ctx->stream (spp_withdrawals_api.cpp; withdrawal_plan.hpp): key i = d_keys + i * stride,
// count in [1, 2^20], pool optional (of this context); d_scratch: spp_withdrawal_plan_scratch_bytes(count); d_audit_of, d_audit_note:
// count words, *d_n_audits one word.  ctx->mu held, device set
size_t spp_withdrawal_plan_scratch_bytes(size_t count);
int spp_withdrawal_plan_enqueue(spp_ctx* ctx, spp_pool* pool, const uint8_t* d_keys, size_t stride, size_t count, void* d_scratch,
                                uint32_t* d_audit_of, uint32_t* d_audit_note, uint32_t* d_n_audits);
template <class T>
inline int ctx_upload(spp_ctx* ctx, T** dst, const std::vector<T>& src) {
  HIP_TRY(dev_upload(dst, src));
  ctx->owned.push_back((void*)*dst);
  return 0;
}

// device buffer freed on every return path
namespace {
// RAII device buffer for the host-pointer convenience entry points
struct DevBuf {
  void* p = nullptr;
  ~DevBuf() { if (p) hipFree(p); }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
  template <class T> T* as() { return (T*)p; }
};
// the window table of the single generator g for c-bit windows, one row per window (what launch_fixed_base_mul reads), into
// `table`; waits for the stream before the temporaries of the construction are released
template <class F>
int build_generator_table(hipStream_t st, const Affine<F>& g, uint32_t c, DevBuf& table) {
  const uint32_t Wn = msm_windows(c);
  const size_t rows = msm_table_rows(1, Wn), E = (size_t)1 << (c - 1);
  DevBuf d_g, tmp, pre;
  HIP_TRY(d_g.alloc(sizeof g));
  HIP_TRY(hipMemcpy(d_g.p, &g, sizeof g, hipMemcpyHostToDevice));
  HIP_TRY(table.alloc(sizeof(Affine<F>) * msm_table_elems(1, c, Wn)));
  HIP_TRY(tmp.alloc(sizeof(XYZZ<F>) * rows * E));
  HIP_TRY(pre.alloc(sizeof(F) * rows * E));
  launch_build_table<F>(st, d_g.as<Affine<F>>(), 1, c, Wn, 0, (uint32_t)rows, table.as<Affine<F>>(), tmp.as<XYZZ<F>>(), pre.as<F>());
  HIP_TRY(hipStreamSynchronize(st));
  return 0;
}
}  // namespace
#define UP(buf, src, bytes)                                                              \
  do {                                                                                    \
    HIP_TRY(buf.alloc(bytes));                                                            \
    if (bytes) HIP_TRY(hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, st));      \
  } while (0)


// the audit input pipeline as stream-ordered work (spp_witness_api.cpp); used by spp_prove_audit_from_secrets_device
size_t spp_audit_scratch_bytes(size_t count);
int spp_audit_inputs_enqueue(spp_ctx* ctx, hipStream_t st, void* scratch, const uint32_t* d_pk_a, const uint32_t* d_pk_b, uint32_t count,
                             const uint8_t* d_sk, const int8_t* d_r, const int8_t* d_e1, const int8_t* d_e2, uint8_t* d_rows, uint32_t* d_c0_out,
                             uint32_t* d_c1_out);
// withdraw notes (spp_witness_api.cpp): SPP_ERR_BAD_INPUT unless every field of every note is canonical
int spp_check_notes(size_t count, const uint8_t* notes);
// deposit proofs (spp_deposit_api.cpp): SPP_ERR_BAD_INPUT unless every field of every record is canonical and no secret_key is 0;
// unless leaves first_index .. first_index+count-1 are in the tree (ctx->mu held)
int spp_check_deposit_records(size_t count, const uint8_t* deposits);
int spp_check_deposit_range(const spp_merkle_tree* t, uint64_t first_index, size_t count);
// threshold opening (spp_partial_api.cpp): SPP_ERR_BAD_INPUT unless t is in [1, 64] and xs (optional) holds t distinct nonzero
// indices; unless every one of the t * count * 64 partials is a canonical field element
int spp_check_share_set(uint32_t t, const uint32_t* xs);
int spp_check_partials(uint32_t t, size_t count, const uint8_t* partials);
// lazily built per-context constants (spp_witness_api.cpp), called with ctx->mu held
// Poseidon / Poseidon2 constants and the Grumpkin window table.  The ONE copy of the hash constants: a circuit's DevCircuit::hc
// points into it (load_r1cs), so the buffers are in ctx->owned and live until the context goes, whatever circuits close first.
int spp_ensure_ctx_consts(spp_ctx* ctx);
int spp_ensure_rlwe(spp_ctx* ctx);         // NTT tables of the RLWE witness kernel
// Horner over the window sums launch_pippenger_g1 left on the device, after the stream was synchronised (spp_micro_api.cpp)
G1Affine pippenger_finish(const G1XYZZ* d_windows);
// a new stream that really runs beside `ref` (spp_api.cpp)
__attribute__((visibility("hidden"))) int pick_concurrent_stream(hipStream_t ref, hipStream_t* out);
