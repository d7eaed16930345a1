// Launch wrappers of the HIP kernels (one .hip file per kernel family; the table-walk MSM is msm_table.hpp, instantiated by
// kernels_msm.hip and kernels_msm_g2.hip, with its host-side planning in msm_plan.hpp), shared by the spp_*.cpp units.
// Data layout in HBM, used by every kernel of the proving path ("batch-minor"):
//   witness   W   [rows][P]      Fr Montgomery, 32 B; row = wire (plus 3 blinding rows r, s, rs)
//   abc           [3][n][P]      constraint evaluations <A_k,w>, <B_k,w>, <C_k,w>, zero padded to n
//   MSM tables    [N][Wn][E]     affine multiples (d+1) * 2^(c*j) * Base_i,  E = 2^(c-1)
//   partials      [S][P]         XYZZ partial sums of one MSM, reduced over S by msm_reduce
// P (proofs in the batch) is the fastest index everywhere, so a wavefront whose 64 lanes hold 64 proofs
// reads/writes 2 KiB contiguous per field element and executes one uniform instruction stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bn254.hpp"
#include "coop_items.hpp"
#include "f29.hpp"
#include "msm_plan.hpp"
#include "msm_ragged.hpp"
#include "rlwe_ntt.hpp"

namespace spp {

struct DevSparse {
  const uint32_t* rowptr;
  const uint32_t* wire;
  const uint32_t* coeff;   // bit31: coefficient is +1, bit30: coefficient is -1, low bits: table index
  const uint32_t* lit;     // 0, or the coefficient itself when |c| < 2^28: magnitude, bit31 = negative (matrix evaluation
                           // accumulates those terms as wide integers instead of doing a field multiplication each)
};
// COEFF_ONE, COEFF_MINUS_ONE, COEFF_MASK: coop_items.hpp

// Poseidon / Poseidon2 constants in HBM (Montgomery form): one upload per context (spp_ensure_ctx_consts), read by the solver
// through DevCircuit::hc and by the stand-alone hash kernels
struct HashConsts {
  // the Poseidon round constants are canonical words (< p): poseidon29.hpp's value bounds rely on it
  const Fr* pos3_rc;  const Fr* pos3_mds;   // t=3: 195 rc, 9 mds (row-major)
  const Fr* pos5_rc;  const Fr* pos5_mds;   // t=5: 340 rc, 25 mds
  const Fr* p2_rc;    const Fr* p2_mu;      // 88 rc, 4 mu
  // Poseidon MDS matrices in the 9x29-bit form, scaled by 2^261 (f29.hpp): mont29(state word, entry) stays an x*2^256 word
  const uint32_t* pos3_mds29;               // 9 x 9 limbs
  const uint32_t* pos5_mds29;               // 25 x 9 limbs
};

struct DevCircuit {
  DevSparse A, B, C, H;
  const Fr* coeffs;
  const Fr* aux;            // hint constants (Grumpkin window tables)
  const uint32_t* program;
  uint32_t n_wires, n_constraints, n_public, n_inputs, challenge_wire;
  // matrix evaluation: constraints grouped into runs of consecutive rows whose B rows are identical (the four
  // constraints of a Poseidon S-box share B = the S-box input): run r covers rows run_start[r] .. run_start[r+1]-1
  const uint32_t* run_start;
  uint32_t n_runs;
  uint32_t max_row_terms;   // longest row of A, B, C (small batches of circuits with long rows take the 16-lanes-per-row evaluation)
  // solver shortcuts per constraint: bit 0 = the B row is identical to the B row of constraint k - 1, bit 1 = the A row is
  // identical to the B row (a square).  A solver lane that has just evaluated row k - 1 reuses the value instead of walking
  // the same linear form again: the rows of a power map share their B side, and compiled (ACIR) circuits have long forms.
  const uint8_t* row_flags;
  // "small rows" of the matrix evaluation (spp_plan.cpp, small_rows_plan): rows whose every term is a small integer coefficient
  // times a wire that the lookup argument bounds to a byte-sized range (the audit circuit's 1 088 quotient equations: 1 024
  // public-key coefficients < 2^28 times noise values in [-3, 3], generate_audit.py:57-66,236-243, plus ciphertext bytes).  The
  // bounded wires are extracted once per batch as int16 (k_small_extract), the rows are summed as 64-bit integers
  // (k_spmv_small_rows) and land in the a / b / c arrays before k_spmv_check runs, which then skips them (row_small bits).
  const uint32_t* sm_wires;     // wire of small slot s (slot 0 = wire 0, the constant one)
  const int32_t* sm_lo;         // lowest value the lookup argument allows for slot s (highest = lo + 255)
  uint32_t sm_nslots;
  const uint32_t* sm_rowptr;    // per small row: terms [rowptr[r], rowptr[r+1])
  const uint32_t* sm_slot;      // slot of a term
  const int32_t* sm_coef;       // its coefficient
  const uint32_t* sm_rest_ptr;  // per small row: its few OTHER terms (any wire, any coefficient) [rest_ptr[r], rest_ptr[r+1]),
  const uint32_t* sm_rest_wire; //   added with field arithmetic (the quotient k * q and the message bits of a quotient equation)
  const uint32_t* sm_rest_coeff;//   index into coeffs
  const uint32_t* sm_row_out;   // matrix (0 = A, 1 = B, 2 = C) << 30 | constraint
  uint32_t sm_nrows;
  const uint8_t* row_small;     // per constraint: bit 0 A, bit 1 B, bit 2 C is a small row (nullptr: none)
  // LONG rows (more than LONG_ROW_MIN terms and not small: the audit circuit's lookup sum has 6 720): one lane per (run, proof)
  // would leave 32 waves walking such a row alone for milliseconds after the rest of the grid has drained.  k_spmv_long_rows
  // evaluates them first, 16 lanes per (row, proof) meeting through LDS, and they carry the same "already in abc" bits.
  const uint32_t* lg_rows;      // (matrix << 30) | constraint
  uint32_t lg_n;
  const uint8_t* row_long;      // the bits of the long rows alone (what k_spmv_check reads when the small-row path is off)
  HashConsts hc;                            // the context's hash constants
  const Fr* byte_mont;                      // Montgomery forms of 0..255
};

// ---- stand-alone witness-input kernels (kernels_witness.hip) ----
// device-resident constants of the RLWE witness kernel (rlwe_ntt.hpp) + scratch for the transformed public key
struct RlwePkDev {
  int32_t hat[2][2][1024];    // [a | b][field][i]: NTT(pk psi^j)[i] / 1024, Montgomery form, in (-p, p)
  uint32_t nzeros[2];
  uint16_t zeros[2][1024];    // positions of zero coefficients (wrap correction)
};
struct RlweDev {
  RnTables tb;
  int32_t pk_scale[2];
  RlwePkDev* pk = nullptr;
};
void launch_rlwe_witness(hipStream_t st, const RlweDev& rd, const uint32_t* pk_a, const uint32_t* pk_b, const int8_t* r, const int8_t* e1,
                         const int8_t* e2, const uint8_t* msg, uint32_t* c0, uint32_t* c1, int32_t* k0, int32_t* k1, uint8_t* packed_be,
                         uint32_t count);
void launch_poseidon_hash(hipStream_t st, HashConsts hc, const uint8_t* in_be, uint32_t arity, uint8_t* out_be, uint32_t count);
void launch_merkle_path(hipStream_t st, HashConsts hc, const uint8_t* leaf_be, const uint64_t* index, const uint8_t* siblings_be,
                        uint32_t depth, uint8_t* root_be, uint32_t count);
void launch_merkle_level(hipStream_t st, HashConsts hc, const Fr* children, uint32_t n_children, Fr dflt, Fr* parents, uint32_t n_parents);
// incremental Poseidon-Merkle tree resident in HBM (spp_merkle_tree_*): level[l] holds count[l] = ceil(n_leaves / 2^l) nodes
struct MerkleTreeDev {
  Fr* level[33];
  uint64_t count[33];
  Fr dflt[33];
  uint32_t depth;
};
void launch_merkle_defaults(hipStream_t st, HashConsts hc, Fr* out, uint32_t depth);
void launch_merkle_update(hipStream_t st, HashConsts hc, const Fr* children, uint64_t n_children, const Fr* dflt_level, Fr* parents,
                          uint64_t first, uint32_t n);
void launch_merkle_gather(hipStream_t st, const MerkleTreeDev* t, uint32_t depth, const uint64_t* indices, uint32_t nq, uint8_t* out_be);
void launch_fr_from_be(hipStream_t st, const uint8_t* in, Fr* out, uint32_t n);
void launch_fr_to_be(hipStream_t st, const Fr* in, uint8_t* out, uint32_t n);
void launch_grumpkin_keygen(hipStream_t st, const GkAffine* table, const uint8_t* sk_be, uint8_t* xy_be, uint32_t count);
void launch_withdraw_rows(hipStream_t st, const GkAffine* table, HashConsts hc, const MerkleTreeDev* t, const uint8_t* notes, uint8_t* rows,
                          uint32_t count);
void launch_deposit_leaves(hipStream_t st, const GkAffine* table, HashConsts hc, const uint8_t* deposits, Fr* leaves, uint32_t count);
void launch_deposit_roots(hipStream_t st, HashConsts hc, const MerkleTreeDev* t, uint64_t first, uint32_t count, uint8_t* roots_be,
                          uint8_t* commitments_be);
// rows for the deposit circuit (deposit_rows.hpp): leaves first .. first+count-1 must be in the tree (first + count <= t->count[0], checked
// by the caller); rows = count * (8 + depth) * 32 B
void launch_deposit_rows(hipStream_t st, const GkAffine* table, HashConsts hc, const MerkleTreeDev* t, uint64_t first, const uint8_t* deposits,
                         uint8_t* rows, uint32_t count);
// The resident tree as of an earlier size (merkle_prefix.hpp has the rule).  size <= t->count[0], checked by the caller.
//   launch_merkle_frontier   one lane: frontier[0..depth] of `size`; the as-of launches below read it in a LATER launch on the stream
//   launch_merkle_gather_at / launch_withdraw_rows_at   launch_merkle_gather / launch_withdraw_rows with the three-case selection
//   launch_prefix_roots      roots[k] = root of size first_size + k, k < count, one lane each (not big-endian: Fr as the levels hold it)
void launch_merkle_frontier(hipStream_t st, HashConsts hc, const MerkleTreeDev* t, uint64_t size, Fr* frontier);
void launch_merkle_gather_at(hipStream_t st, const MerkleTreeDev* t, uint32_t depth, uint64_t size, const Fr* frontier, const uint64_t* indices,
                             uint32_t nq, uint8_t* out_be);
void launch_withdraw_rows_at(hipStream_t st, const GkAffine* table, HashConsts hc, const MerkleTreeDev* t, uint64_t size, const Fr* frontier,
                             const uint8_t* notes, uint8_t* rows, uint32_t count);
void launch_prefix_roots(hipStream_t st, HashConsts hc, const MerkleTreeDev* t, uint64_t first_size, uint32_t count, Fr* roots);
// the leaf index of a resident tree and the wallet sync over it (leaf_index.hpp has the structures and what a lane does).  An insert
// launch and a query launch never coincide: insert first, query in a later launch on the same stream.
struct LeafIndex;
struct PoolSet;
void launch_leaf_index_insert(hipStream_t st, const LeafIndex& ix, const Fr* leaves, uint32_t first, uint32_t n);
void launch_leaf_find(hipStream_t st, const LeafIndex& ix, const Fr* leaves, const uint8_t* keys_be, const uint64_t* from, uint64_t* indices,
                      uint32_t* matches, uint32_t count);
// identity + locate: records count * 160 B (always), notes optional (then recipients count * 32 B); sets: the pool's
// { nullifiers, audit records } with its salt, or nullptr
void launch_wallet_sync(hipStream_t st, const GkAffine* table, HashConsts hc, const LeafIndex& ix, const MerkleTreeDev* t, const PoolSet* sets,
                        uint64_t pool_salt, const uint8_t* deposits, const uint8_t* recipients, uint8_t* records, uint64_t* indices,
                        uint32_t* flags, uint8_t* notes, uint32_t count);
void launch_poseidon2_sponge(hipStream_t st, HashConsts hc, const uint8_t* in_be, uint32_t n, uint8_t* out_be, uint32_t count);
void launch_rlwe_decrypt(hipStream_t st, const uint32_t* sk_mod_q, const uint32_t* c0, const uint32_t* c1, uint8_t* msg, uint32_t count);
void launch_shamir_combine(hipStream_t st, const Fr* lambda, const uint8_t* ys_be, uint32_t t, uint32_t n, uint8_t* secret_be,
                           uint32_t* sk_mod_q);
// auditor key generation (rlwe_keygen.hpp): one wave per key; b, sk_mod_q (optional) count * 1024; max_abs count * 2
void launch_rlwe_keygen(hipStream_t st, const RlweDev& rd, const int8_t* sk, const uint32_t* a, const int8_t* e, uint32_t* b,
                        uint32_t* sk_mod_q, uint32_t count);
void launch_rlwe_key_noise(hipStream_t st, const RlweDev& rd, const uint32_t* a, const uint32_t* b, const uint32_t* sk_mod_q,
                           uint32_t* max_abs, uint32_t count);
// t-of-m sharing of n values: xs m share indices as Fr, coeffs_be (t - 1) * n * 32 B, ys_be m * n * 32 B share-major
void launch_shamir_split(hipStream_t st, const Fr* xs, const uint8_t* secrets_be, const uint8_t* coeffs_be, uint32_t t, uint32_t m,
                         uint32_t n, uint8_t* ys_be);
// verifiable sharing of the auditors' key (vss.hpp; kernels_vss.hip).  table: VSS_TABLE_POINTS affine points, built once from the 64
// window bases; every scalar is 32 B big-endian and canonical (the caller's check)
//   launch_vss_commit  commitments t * n * 64 B, C_k[v] at (k n + v) * 64; coeffs (t - 1) * n * 32 B as launch_shamir_split reads them
//   launch_vss_check   flags dealers * n; commitments dealers * t * n * 64 B; ys, ys_blind, zero_blinds (optional) dealers * n * 32 B
//   launch_vss_sum     out[v] = base[v] (optional) + sum over dealers of ys[d][v]
void launch_vss_table(hipStream_t st, const G1Affine* wbases, G1Affine* table);
void launch_vss_commit(hipStream_t st, const G1Affine* table, const uint8_t* secrets_be, const uint8_t* coeffs_be, const uint8_t* blinds_be,
                       const uint8_t* coeffs_blind_be, uint32_t t, uint32_t n, uint8_t* commitments);
void launch_vss_check(hipStream_t st, const G1Affine* table, uint32_t t, uint32_t x, uint32_t dealers, uint32_t n, const uint8_t* commitments,
                      const uint8_t* ys_be, const uint8_t* ys_blind_be, const uint8_t* zero_blinds_be, uint32_t* flags);
void launch_vss_sum(hipStream_t st, const uint8_t* base_be, const uint8_t* ys_be, uint32_t dealers, uint32_t n, uint8_t* out_be);
// the committee's commitments and resharing (vss.hpp, last section)
//   launch_vss_decode         points[i], flags[i] (SPP_VSS_BAD_POINT or 0) from raw[i * 64 ..], i < count
//   launch_vss_lincomb        out[i] = base[i] (optional) + sum_d w_d points[d * count + i], i < count = t n; weights dealers * 8
//                             canonical words, the same for every lane, or nullptr: plain sums
//   launch_vss_share_commit   out[(i n + v) 64 ..] = sum_k xs[i]^k committee[(k n + v) 64 ..], i < count
//   launch_vss_reshare_check  flags t_old * n: vss_check_value at (t_new, x_new) of each old member's dealing | SPP_VSS_NOT_SHARE
//   launch_vss_weighted_sum   out[v] = sum_d weights[d] ys[d][v]
void launch_vss_decode(hipStream_t st, const uint8_t* raw, size_t count, G1Affine* points, uint32_t* flags);
void launch_vss_lincomb(hipStream_t st, uint32_t dealers, const uint32_t* weights, const G1Affine* points, const G1Affine* base, uint32_t count,
                        uint8_t* out);
void launch_vss_share_commit(hipStream_t st, uint32_t t, const uint32_t* xs, uint32_t count, uint32_t n, const uint8_t* committee, uint8_t* out);
void launch_vss_reshare_check(hipStream_t st, const G1Affine* table, uint32_t t_old, const uint32_t* xs_old, uint32_t t_new, uint32_t x_new,
                              uint32_t n, const uint8_t* committee, const uint8_t* commitments, const uint8_t* ys_be, const uint8_t* ys_blind_be,
                              uint32_t* flags);
void launch_vss_weighted_sum(hipStream_t st, const Fr* weights, const uint8_t* ys_be, uint32_t dealers, uint32_t n, uint8_t* out_be);
// one wave per 64 audit records (audit_open.hpp): owners count * 64 B, flags[i] = SPP_AUDIT_* bits; proof_ok (optional): the verdicts
// of launch_verify for the same records, enqueued before on `st`
void launch_audit_open(hipStream_t st, HashConsts hc, const uint32_t* sk_mod_q, const uint32_t* c0, const uint32_t* c1, const uint8_t* pws,
                       const int32_t* proof_ok, uint8_t* owners, uint32_t* flags, uint32_t count);
// the threshold form (rlwe_partial.hpp): residues count * 64 = (sk * c1)[t] mod q from launch_rlwe_combine in the place of the key,
// bad_partials[i] != 0 adds SPP_AUDIT_BAD_PARTIALS
void launch_audit_open_partials(hipStream_t st, HashConsts hc, const uint32_t* residues, const uint32_t* bad_partials, const uint32_t* c0,
                                const uint32_t* c1, const uint8_t* pws, const int32_t* proof_ok, uint8_t* owners, uint32_t* flags, uint32_t count);
// U: 8 * 1024 words, the limb-major table of lambda * share (share_be 1024 * 32 B canonical)
void launch_partial_scale(hipStream_t st, const Fr& lambda, const uint8_t* share_be, uint32_t* U);
// one block per record: partials count * 64 * 32 B; xs[t], seeds t * 32 B or nullptr, e / rho count * 64 or nullptr; ct_be count * 32 B,
// always written: the commitments the masks are keyed by (a kernel of their own above RP_COOP_SPONGE_MAX records)
void launch_rlwe_partial(hipStream_t st, HashConsts hc, const uint32_t* U, uint32_t t, const uint32_t* xs, uint32_t self, const uint8_t* seeds,
                         const uint32_t* c0, const uint32_t* c1, const int32_t* e, const uint64_t* rho, uint8_t* partials, uint8_t* ct_be,
                         uint32_t count);
// partials t * count * 64 * 32 B auditor-major -> residues count * 64, msg count * 64 (needs c0), flags count: each optional
void launch_rlwe_combine(hipStream_t st, uint32_t t, const uint8_t* partials, const uint32_t* c0, uint32_t* residues, uint8_t* msg, uint32_t* flags,
                         uint32_t count);
void launch_audit_msg(hipStream_t st, const uint8_t* xy_be, uint8_t* msg, uint32_t count);
void launch_audit_assemble(hipStream_t st, const uint8_t* wa_be, const uint8_t* ct_be, const uint8_t* packed_be, const uint8_t* sk_be,
                           const int8_t* r, const int8_t* e1, const int8_t* e2, const int32_t* k0, const int32_t* k1, uint8_t* rows,
                           uint32_t count);

// ---- witness ----
void launch_load_inputs(hipStream_t st, const uint8_t* d_inputs_be, const uint8_t* d_rs_be, Fr* W, uint32_t n_inputs,
                        uint32_t n_wires, uint32_t P);
// runs the solver program from word `pc` until OP_COMMIT / OP_END; scratch: [SOLVE_SCRATCH_ROWS or more][P] Fr
static constexpr uint32_t SOLVE_SCRATCH_MIN_ROWS = 324;
void launch_solve(hipStream_t st, DevCircuit dc, Fr* W, Fr* scratch, uint32_t pc_begin, uint32_t pc_end, uint32_t P);
// cooperative solver for small batches (one wave per proof; kernels_solve.hip): items = (kind, a, b) triples, kinds in coop_items.hpp
struct DevCoop {
  const uint32_t* items;      // 3 words per item
  const uint32_t* par;        // COOP_PAR: (pc_begin, pc_end) pairs of independent instructions
  const uint32_t* lvl_ptr;    // COOP_LEVELS: rows lvl_rows[lvl_ptr[l] .. lvl_ptr[l+1]) form dependency level l
  const uint32_t* lvl_rows;
  const uint32_t* lvl_gen;    // three words per entry of lvl_rows: side (COOP_NONE: a plain OP_SOLVE_C row), inv, odiv of an OP_SOLVE_ROW row
  // COOP_LEVEL_STREAM (a = first chunk, b = chunks): the same levels flattened into self-contained records, in chunks of
  // COOP_CHUNK words that the wave stages through LDS one ahead.  Level: [rows n | lanes per row << 24 | some A form << 29 | some C rest << 30][words in the level][offset of row 0..n-1]
  // then per row [output wire][terms of A | bit 31: A = B][terms of B][terms of C without the output][(wire, coefficient word) ...];
  // 0xffffffff instead of n: the rest of the chunk is padding.  No level crosses a chunk boundary.  A generic row (OP_SOLVE_ROW) has
  // COOP_ROW_GENERIC | side << 29 in its B word, counts its own side without the output, and carries [inv][odiv] before its terms.
  const uint32_t* lvl_stream;
  uint32_t generic;           // the program holds the generic solver instructions: the kernel instance that knows them runs
};
void launch_solve_coop(hipStream_t st, DevCircuit dc, DevCoop co, Fr* W, Fr* scratch, CoopTracks tracks, uint32_t P);
// wide forms of the two data-parallel solver instructions (one lane per (element chunk, proof) instead of one per proof)
void launch_batch_div(hipStream_t st, DevCircuit dc, Fr* W, Fr* scratch, uint32_t k0, uint32_t n, uint32_t P);
void launch_count8(hipStream_t st, DevCircuit dc, Fr* W, uint32_t* counters, uint32_t h0, uint32_t n, uint32_t out0, uint32_t P);
// a,b,c evaluation + satisfaction check (status[p] |= 1 when some row fails)
// ---- batched verification (kernels_verify.hip); the structures live in pairing_fast.hpp ----
struct VerifyKeyDev;
void launch_verify(hipStream_t st, const VerifyKeyDev* vk, const uint8_t* proofs, const uint8_t* pws, uint32_t pw_len, uint32_t count,
                   int32_t* ok);
struct PairingCheckDev;
void launch_pairing_check(hipStream_t st, const PairingCheckDev* a, int32_t* ok);
// k_verify over a compacted list: ok[list[j]] for j < *n_list (a device word; at most max_count), the other entries of ok untouched
void launch_verify_list(hipStream_t st, const VerifyKeyDev* vk, const uint8_t* proofs, const uint8_t* pws, uint32_t pw_len, uint32_t max_count,
                        const uint32_t* list, const uint32_t* n_list, int32_t* ok);
// ---- batch verification by random linear combination (kernels_verify_rlc.hip); the structures live in verify_rlc.hpp ----
// one slice of a call: terms (one lane per proof), groups (one wave per `group` proofs), then k_verify_list over the proofs of the
// refused groups unless SPP_RLC_NO_FALLBACK.  ws: rlc_elems(nk) * count elements; live, list: count words; *n_list = 0 on entry;
// stats[1..3] are added to.  index0: the index of the slice's first proof in the call (the scalars are derived from it)
struct RlcKeyDev;
struct RlcSeed;
struct W256;
void launch_verify_rlc(hipStream_t st, const VerifyKeyDev* vk, const RlcKeyDev* rk, const uint8_t* proofs, const uint8_t* pws, uint32_t pw_len,
                       uint32_t count, const RlcSeed& seed, uint32_t index0, uint32_t group, uint32_t flags, W256* ws, uint32_t* live,
                       int32_t* ok, uint32_t* list, uint32_t* n_list, uint32_t* stats);
// the same over a compacted list (verify_rlc_list.hpp): the proofs in_list[0 .. *n_in) of a batch, *n_in a device word <= max_count
// that the host never reads; ok[in_list[j]] = 1 for the accepted ones, the other entries of ok untouched (the caller cleared them).
// Slices of at most 2^18 list positions, each: *n_list = 0, terms, groups, k_verify_list over the proofs of the refused groups
// (max_count <= 2^18: exactly these three launches).  ws: rlc_elems(nk) * min(max_count, rlc_slice_len(group)) elements; live, list
// (the fallback list): as many words; stats[0..3] are added to (groups are counted on the device).  The scalars are derived from
// the seed and the index in the batch, in_list[j], not from j.  max_count > 0
void launch_verify_rlc_list(hipStream_t st, const VerifyKeyDev* vk, const RlcKeyDev* rk, const uint8_t* proofs, const uint8_t* pws, uint32_t pw_len,
                            uint32_t max_count, const uint32_t* in_list, const uint32_t* n_in, const RlcSeed& seed, uint32_t group, W256* ws,
                            uint32_t* live, int32_t* ok, uint32_t* list, uint32_t* n_list, uint32_t* stats);
// ---- pool ledger (kernels_pool.hip); the structures and what a lane does live in pool_table.hpp ----
struct PoolSet;
struct PoolState;
void launch_pool_screen_audit(hipStream_t st, const PoolSet& audits, uint64_t salt, const uint8_t* pws, uint32_t count, int32_t* prov, uint32_t* list,
                              uint32_t* n_list);
void launch_pool_screen_withdraw(hipStream_t st, const PoolState* state, const PoolSet& audits, const PoolSet& nullifiers, uint64_t salt,
                                 const uint8_t* pws, const uint8_t* recipients, uint32_t count, int32_t* prov, uint64_t* amounts, uint32_t* list,
                                 uint32_t* n_list);
// a withdraw of a log: the ring and the audit records as of its position (PoolLogView, pool_table.hpp); count > 0
struct PoolLogView;
void launch_pool_screen_withdraw_log(hipStream_t st, const PoolLogView& view, const PoolSet& audits, const PoolSet& nullifiers, uint64_t salt,
                                     const uint8_t* pws, const uint8_t* recipients, const uint32_t* deposits_before, const uint32_t* audits_before,
                                     uint32_t count, int32_t* prov, uint64_t* amounts, uint32_t* list, uint32_t* n_list);
// result[pos[i]] = codes[i] and, unless amounts_out is nullptr, amounts_out[pos[i]] = amounts[i]; count > 0
void launch_pool_scatter(hipStream_t st, const uint32_t* pos, uint32_t count, const int32_t* codes, int32_t* result, const uint64_t* amounts,
                         uint64_t* amounts_out);
void launch_pool_screen_import(hipStream_t st, const PoolSet& set, uint64_t salt, const uint8_t* keys, uint32_t count, int32_t* prov);
void launch_pool_contains(hipStream_t st, const PoolSet& set, uint64_t salt, const uint8_t* keys, uint32_t count, uint8_t* present);
// claim + settle: slots = the resolve table (mask + 1 words, all POOL_NONE), key of instruction i = keys + i * stride;
// proof_ok == nullptr: every pending instruction is a candidate; dup = the code of an instruction that meets an earlier winner
void launch_pool_resolve(hipStream_t st, uint32_t* slots, uint32_t mask, uint64_t salt, const uint8_t* keys, uint32_t stride, uint32_t count,
                         const int32_t* prov, const int32_t* proof_ok, int32_t dup, int32_t* result);
void launch_pool_commit(hipStream_t st, const PoolSet& set, uint64_t salt, const uint8_t* keys, uint32_t stride, uint32_t count, const int32_t* result,
                        uint32_t* set_count);
// ---- withdrawal plan (kernels_withdrawals.hip); what a lane, a wave and a tile do lives in withdrawal_plan.hpp ----
// Five launches whatever the keys are: claim, winners + tile counts, scan, scatter, assign.  count in [1, 2^20]; key i = keys + i * stride;
// audits: the pool's audit-record set (read only) or nullptr; slots: mask + 1 words, all POOL_NONE; resident: count bytes; rep, pos,
// audit_of, audit_note: count words; tile_counts, tile_base: 1024 words; *n_audits: one word
void launch_withdrawal_plan(hipStream_t st, const PoolSet* audits, uint64_t salt, uint32_t* slots, uint32_t mask, const uint8_t* keys, size_t stride,
                            uint32_t count, uint8_t* resident, uint32_t* rep, uint32_t* pos, uint32_t* tile_counts, uint32_t* tile_base,
                            uint32_t* audit_of, uint32_t* audit_note, uint32_t* n_audits);
// small: [sm_nslots][P] int16 scratch of the small rows (may be nullptr when the circuit has none)
void launch_spmv_check(hipStream_t st, DevCircuit dc, const Fr* W, Fr* abc, uint32_t n, uint32_t P, uint32_t* status, int16_t* small = nullptr);

// ---- NTT / QAP ----
// in-place radix-2 passes over data [n][P]; dif: natural->bitreversed with table tw (w^-k or w^k), else DIT
// post (optional): n row factors multiplied into the output rows by the last pass (fused coset shift)
void launch_ntt(hipStream_t st, Fr* data, uint32_t logn, uint32_t P, const Fr* tw, bool dif, uint32_t nbatch, size_t batch_stride,
                const Fr* post = nullptr);
void launch_scale_rows(hipStream_t st, Fr* data, const Fr* table, uint32_t n, uint32_t P, uint32_t nbatch, size_t batch_stride);
void launch_qap_pointwise(hipStream_t st, Fr* abc, uint32_t n, uint32_t P, Fr zinv);
void launch_qap_product(hipStream_t st, Fr* abc, uint32_t n, uint32_t P);   // a <- a * b

// ---- MSM with precomputed window tables (msm_table.hpp: the kernels, templates over the coordinate field, instantiated by
// kernels_msm.hip for G1 and kernels_msm_g2.hip for G2; msm_plan.hpp: windows, padding, buffer sizes, the lane layout MsmPlan) ----
// A base carries Wt table rows of 2^(c-1) affine multiples; row m = multiples of 2^(c*R*m) * Base, R = ceil(W / Wt) window passes
// (W = ceil(254 / c) windows per scalar).  Wt = W: one row per window, no passes (the small-table latency layout).  Wt = 1: one row
// per base and W passes whose sums are combined by Horner (the throughput layout: widest window for the bytes).
// What tells the G1 walk from the G2 walk, in one place: k_msm_flat and k_msm_flat_redo take their launch bound and the fast walk
// its product form from here, and the host passes occ(Wt) to msm_plan / msm_partial_cap, so the planner counts the waves the kernel it
// plans for can have resident.  The flat walk keeps the same-x case of the mixed addition out of its loop (msm_table.hpp), which
// is what its register counts rest on; k_msm_rows adds with the inline path and keeps the occupancy it had.  product_form: how the
// fast walk writes the nine Montgomery products of an addition (F29Form, f29.hpp), chosen by tests/micro/f29_madd_chain.hip and the
// headline A/B (profiles/f29_scan_ab.json); the redo kernel, k_msm_rows and every other user of F29 keep the column form.
template <class F>
struct MsmWalk;
template <>
struct MsmWalk<Fq> {
  static constexpr uint32_t waves_per_simd = 3;         // flat walk: at most 168 VGPRs (it takes 144; the redo kernel 168 and 128 B of scratch)
  static constexpr uint32_t rows_waves_per_simd = 2;    // k_msm_rows
  static constexpr int product_form = F29_SCAN;         // F29Form of the fast flat walk's additions (the redo kernel and k_msm_rows: F29_COLUMNS)
  static constexpr uint32_t occ(uint32_t Wt) { return Wt == 1 ? waves_per_simd : rows_waves_per_simd; }
};
template <>
struct MsmWalk<Fq2> {
  static constexpr uint32_t waves_per_simd = 2;         // flat walk: at most 256 VGPRs, no AGPRs
  static constexpr uint32_t rows_waves_per_simd = 1;    // k_msm_rows: up to 512 registers
  static constexpr int product_form = F29_COLUMNS;      // G2: the scanning form did not beat the column form at two waves (profiles/f29_madd_chain.txt)
  static constexpr uint32_t occ(uint32_t Wt) { return Wt == 1 ? waves_per_simd : rows_waves_per_simd; }
};
// builds rows [row0, row0 + nrows) (row = base * Wt + m; row0 a multiple of 64) of the table of N bases, E entries each;
// tmp / tmp_pre: nrows * E elements each.  blocks = nullptr: the uniform layout, E = 2^(c-1) for every row; else the ragged layout
// of a flat set (msm_ragged.hpp), the launch covering blocks of E entries.  Layout: see msm_table.hpp.
template <class F>
void launch_build_table(hipStream_t st, const Affine<F>* bases, uint32_t N, uint32_t c, uint32_t Wt, uint32_t row0, uint32_t nrows,
                        Affine<F>* table, XYZZ<F>* tmp, F* tmp_pre, const MsmBlock* blocks = nullptr, uint32_t E = 0);
// signed c-bit digits of scalars[rows[i]][p] as int16 planes dig[j][i][p] (Pp = msm_padded_batch(P) per row; msm_digit_elems);
// rows[i] = 0xffffffff (MSM_ROW_ZERO, msm_lookup.hpp): zero digits, whatever the scalars
void launch_msm_digits(hipStream_t st, const uint32_t* rows, const Fr* scalars, int16_t* dig, uint32_t N, uint32_t P, uint32_t c);
// lane g -> (pass, slice, proof); partial[R * Sg][P].  blocks: the block table of a flat set (pl.Wt == 1), required there
template <class F>
void launch_msm_accumulate(hipStream_t st, const Affine<F>* table, const MsmBlock* blocks, const int16_t* dig, XYZZ<F>* partial, uint32_t N, uint32_t P,
                           uint32_t c, const MsmPlan& pl, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr, uint32_t* redo_count = nullptr);
// out[p] = sum over slices and passes (empty: out[p] = infinity); folds in place: `partial` is scratch afterwards
template <class F>
void launch_msm_reduce(hipStream_t st, XYZZ<F>* partial, XYZZ<F>* out, uint32_t P, const MsmPlan& pl, uint32_t c, bool empty);
// several sets folded by the same launches (one launch per level for all of them, one Horner launch)
static constexpr uint32_t MSM_FOLD_SETS = 8;
static constexpr uint32_t MSM_FOLD_RADIX = 8;   // slices summed per lane and fold level
template <class F>
struct MsmFoldSets {
  XYZZ<F>* partial[MSM_FOLD_SETS];
  XYZZ<F>* out[MSM_FOLD_SETS];
  uint32_t Sg[MSM_FOLD_SETS], R[MSM_FOLD_SETS], c[MSM_FOLD_SETS];   // per set: slices per pass (0 = empty set), passes, window bits
  uint32_t cur[MSM_FOLD_SETS], half[MSM_FOLD_SETS];                 // per level: slices before / after it (launch_msm_reduce_multi)
};
template <class F>
void launch_msm_reduce_multi(hipStream_t st, MsmFoldSets<F> fs, uint32_t nsets, uint32_t P);

// ---- the lookup-inverse wires' share of the A and K sums by byte bucket (kernels_msm_lookup.hip; the method: msm_lookup.hpp) ----
struct LkbSets {               // index 0: A, 1: K
  const Affine<Fq>* table[2];
  const MsmBlock* blocks[2];
  const uint32_t* pos[2];      // per lookup: its base's index in the set (0xffffffff: the set has no base for it)
  XYZZ<Fq>* out[2];            // the set's sum (launch_lkb_join)
};
size_t lkb_bucket_elems(size_t P);   // elements of `bkt` for a batch of P proofs
// bytes[j][p] = the value hint row hints[j] takes in proof p if it is a byte, else 0 (kernels_solve.hip)
void launch_lookup_bytes(hipStream_t st, DevCircuit dc, const Fr* W, const uint32_t* hints, uint32_t L, uint32_t P, uint8_t* bytes);
// inv[t][p] = 1 / (X_p - t), t < 256, and its digit planes dig[window][t][p]; a proof with X_p = t is refused through status
void launch_lkb_inverses(hipStream_t st, const Fr* W, uint32_t challenge_wire, uint32_t P, Fr* inv, int8_t* dig, uint32_t* status);
// both levels for both sets: win[set][window][p] = sum_t dig[window][t][p] * Bkt[set][t][p], the pass sums of a Horner with
// Sg = 1, R = LKB_WINDOWS, c = LKB_C (launch_msm_reduce_multi)
void launch_lkb_sums(hipStream_t st, const LkbSets& s, const uint8_t* bytes, const int8_t* dig, XYZZ<Fq>* bkt, XYZZ<Fq>* win, uint32_t L, uint32_t P);
void launch_lkb_join(hipStream_t st, const LkbSets& s, const XYZZ<Fq>* sum, uint32_t P);   // out[set][p] += sum[set][p]

// the H bases of a proving key in the evaluation basis on the coset (kernels_msm.hip): out[bitrev(i)] = Z'_i
void launch_g1_eval_basis(hipStream_t st, const G1Affine* pts, uint32_t n_pts, uint32_t logn, const Fr* scale, const Fr* tw_inv, G1XYZZ* work,
                          G1Affine* out);

// out[s] = sum over t in [seg[s], seg[s+1]) of coeff[t] * base[row[t]]  (work: nterms points)
void launch_g1_column_sums(hipStream_t st, const G1Affine* base, const uint32_t* row, const Fr* coeff, uint32_t nterms, const uint32_t* seg,
                           uint32_t nseg, G1XYZZ* work, G1Affine* out);

// ---- general-base Pippenger (kernels_pippenger.hip) ----
size_t pippenger_workspace_bytes(uint32_t n);
size_t pippenger_workspace_bytes_g2(uint32_t n);
void launch_pippenger_g2(hipStream_t st, const G2Affine* bases, const Fr* scalars, uint32_t n, void* workspace, G2XYZZ** out_windows,
                         hipEvent_t ev0, hipEvent_t ev1);
uint32_t pippenger_windows();
void launch_pippenger_g1(hipStream_t st, const G1Affine* bases, const Fr* scalars, uint32_t n, void* workspace, G1XYZZ** out_windows,
                         hipEvent_t ev0, hipEvent_t ev1);

// ---- raw-word probe of the arithmetic headers (kernels_arith_probe.hip, arith_probe.hpp): spp_debug_arith, test only ----
// in: n * in_words, out: n * out_words device words (arith_probe_shape); false = unknown selector or arg, nothing launched
bool launch_arith_probe(hipStream_t st, uint32_t selector, uint32_t arg, const uint32_t* in, uint32_t* out, uint32_t n);

// ---- commitment challenge, proof assembly ----
void launch_challenge(hipStream_t st, const G1XYZZ* commit, Fr* W, uint32_t challenge_wire, uint32_t P, G1Affine* commit_affine,
                      uint32_t* status);
struct AssembleArgs {
  const G1XYZZ* mA; const G1XYZZ* mB1; const G2XYZZ* mB2; const G1XYZZ* mK; const G1XYZZ* mZ; const G1XYZZ* mPok;
  const G1Affine* commit_affine;
  const Fr* W; uint32_t row_r, row_s; uint32_t n_public;
  // small batches: s*Ar and r*Bs1 arrive as two more fixed-base sums over the scaled witness (nullptr: the lanes multiply)
  const G1XYZZ* sAr; const G1XYZZ* rBs1;
  uint8_t* proofs;   // [P][388]
  uint8_t* pws;      // [P][12+32*(n_public-1)]
  uint32_t P;
};
void launch_assemble(hipStream_t st, AssembleArgs a);
void launch_spin(hipStream_t st, uint64_t ticks_100mhz, uint32_t* sink);   // one lane busy-waits (bounded); stream-concurrency probe
void launch_touch(hipStream_t st, uint32_t* sink);
// Ws[row][p] = s_p * W[row][p], Wr[row][p] = r_p * W[row][p] for rows < n_rows (r, s = rows row_r, row_s of W)
void launch_scale_witness(hipStream_t st, const Fr* W, Fr* Ws, Fr* Wr, uint32_t n_rows, uint32_t row_r, uint32_t row_s, uint32_t P);

// ---- setup helpers ----
// out[i] = scalars[i] * G for a generator table built with launch_build_table (N=1)
template <class F>
void launch_fixed_base_mul(hipStream_t st, const Affine<F>* gen_table, uint32_t c, const Fr* scalars, uint32_t n, Affine<F>* out);
// ---- setup ceremony (kernels_setup.hip; the method: setup_contrib.hpp) ----
// out[i] = k * pts[i] for ONE scalar k, given as the len digits of its non-adjacent form (sc_naf_recode), least significant first
void launch_g1_scale(hipStream_t st, const G1Affine* pts, uint32_t n, const int8_t* dig, uint32_t len, G1Affine* out);
// raw: n points of 64 B (X | Y big-endian) -> pts[i] in Montgomery form and flags[i] = SC_POINT_OK / SC_POINT_INF / SC_POINT_BAD
void launch_g1_decode_check(hipStream_t st, const uint8_t* raw, uint32_t n, G1Affine* pts, uint32_t* flags);
// ---- powers-of-tau transcript (kernels_ptau.hip; the method: ptau.hpp) ----
// out[i] = sc[i] * pts[i]: a scalar of its own per point, 8 canonical words each (least significant first), 0 < sc[i] < r
void launch_g1_mul_each(hipStream_t st, const G1Affine* pts, uint32_t n, const uint32_t* sc, G1Affine* out);
void launch_g2_mul_each(hipStream_t st, const G2Affine* pts, uint32_t n, const uint32_t* sc, G2Affine* out);
// raw: n points of 128 B -> pts[i] and flags[i] = SC_POINT_*: coordinates below q, on the twist y^2 = x^3 + twist_b; NOT the subgroup
void launch_g2_decode_check(hipStream_t st, const uint8_t* raw, uint32_t n, const Fq2& twist_b, G2Affine* pts, uint32_t* flags);
// nbatch inverse NTTs over points, each 2^logn (logn >= 1) elements laid end to end: out[b][k] = (1 / n) sum_i w^(-k i) in[b][i].
// work: 2 * (nbatch << logn) elements (the stages go from one half to the other); tw: w^-j, j < n / 2, 8 canonical words each; dig, len: the NAF digits of 1 / n (sc_naf_recode).
// ev_passes / ev_finish (optional): recorded after the last stage and after the scaling
template <class F>
void launch_ec_intt(hipStream_t st, const Affine<F>* in, XYZZ<F>* work, uint32_t logn, uint32_t nbatch, const uint32_t* tw, const int8_t* dig,
                    uint32_t len, Affine<F>* out, hipEvent_t ev_passes = nullptr, hipEvent_t ev_finish = nullptr);
// out[j] = sum of column j's terms (row, coefficient) * bases[row] for a ColPlan (ptau.hpp): terms, chunk_ptr (nchunks + 1), col_ptr
// (ncols + 1); mags / meta: the signed coefficient table (pt_signed_coeff); partial: nchunks elements
template <class F>
void launch_col_gather(hipStream_t st, const Affine<F>* bases, const uint32_t* terms, const uint32_t* chunk_ptr, uint32_t nchunks,
                       const uint32_t* col_ptr, uint32_t ncols, const uint32_t* mags, const uint32_t* meta, XYZZ<F>* partial, Affine<F>* out);
// out[i] = pts[i + n] - pts[i], i < count
void launch_g1_shifted_diff(hipStream_t st, const G1Affine* pts, uint32_t n, uint32_t count, G1Affine* out);

}  // namespace spp
