/* libspp -- C ABI of the MI355X-native Groth16 prover for the shielded-pool circuits.
 *
 * Drop-in boundary for the proving path of Ham3798/shielded-pool-pinocchio-solana. Each entry point
 * names the reference interface it replaces (paths relative to the reference tree):
 *
 *   spp_prove_withdraw        client/proof.helper.ts:28-72  generateProof(): the two child processes
 *                             `nargo execute` (:55) + `sunspot prove` (:64) and the .proof/.pw reads (:68-69)
 *   spp_prove_batch           client/payroll-demo.ts:326-352 (Promise.all over generateProof) and
 *                             audit_circuit/prove_audit.sh:74-99 / scripts/generate_audit.py:668-685
 *   spp_setup                 `sunspot setup <ccs>`   noir_circuit/prove_linux.sh:72-79, generate_audit.py:670-677
 *   spp_circuit_build         `sunspot compile <acir>` noir_circuit/prove_linux.sh:66-70, generate_audit.py:659-665
 *   spp_rlwe_witness_batch    scripts/generate_audit.py:507-584 (encrypt + quotient witnesses + packing),
 *                             demo-frontend/app/lib/rlwe.ts:157-247
 *   spp_poseidon_*            client/merkle.ts:22-38,119-140,165-221 (circomlibjs Poseidon, Merkle tree)
 *   spp_grumpkin_keygen_batch client/merkle.ts:98-113 generateIdentityKeypair
 *   spp_audit_inputs_batch    scripts/generate_audit.py:468-641 (everything before `nargo execute`)
 *   spp_prove_withdraw_notes  client/payroll-demo.ts:323-340 (getRoot / getProof / generateProof per recipient) against the
 *                             resident tree (spp_merkle_tree_*)
 *   spp_merkle_tree_deposit   client/payroll-demo.ts:264-292 (generateIdentityKeypair / calculateCommitment / insert / getRoot
 *                             per deposit) into the same tree
 *   spp_deposit_rows_from_tree / spp_prove_deposits(_device) / spp_verify_deposit_chain
 *                             no counterpart: the reference's deposit carries no proof -- the program ignores the commitment, pushes
 *                             the new_root it is sent and transfers an amount nothing binds to the note
 *                             (shielded_pool_program/src/instructions/deposit.rs:31-36,73).  A proof per deposit of the root before,
 *                             the root after, the commitment, its amount and its index, and the check of a log of them
 *   spp_verify                `sunspot verify` noir_circuit/prove_linux.sh:86-87, audit_circuit/prove_audit.sh:98-99
 *   spp_verify_batch          the same for many proofs on the GPU
 *   spp_verify_batch_rlc      the same by random linear combination: key-side pairings once per group of proofs
 *   spp_shamir_reconstruct / spp_rlwe_decrypt_batch   scripts/rlwe_decrypt.py:61-132, demo-frontend/app/lib/shamir.ts:97-169
 *   spp_rlwe_sample_key / spp_rlwe_keygen_batch / spp_rlwe_key_check / spp_shamir_split
 *                             scripts/rlwe_keygen.py:98-182 (the audit key pair and its files) and :51-65 (shamir_share_field)
 *   spp_vss_deal              scripts/rlwe_keygen.py:51-65 (shamir_share_field) by every auditor for its own part of the key, with
 *                             public commitments (no counterpart in the reference, whose :98-182 draw and share the key in one place)
 *   spp_vss_receive           the check of those commitments and the sum that is a share file of :157-171
 *   spp_vss_combine_commitments / spp_vss_share_commitments / spp_vss_reshare_receive
 *                             the committee's commitments and handing the key to a new committee (no counterpart in the reference)
 *   spp_prove_audit_records   scripts/generate_audit.py:468-691 with the ciphertext.json of :590-606: the audit RECORD
 *                             (proof, public witness, ciphertext) from the prover's raw secrets
 *   spp_audit_open_batch      scripts/rlwe_decrypt.py:61-149 for a batch of such records, after `sunspot verify`
 *                             (audit_circuit/prove_audit.sh:98-99) and with the two binding checks the script leaves out
 *   spp_audit_open_batch_rlc  the same, the proofs verified by random linear combination
 *   spp_rlwe_partial_decrypt_batch / spp_rlwe_combine_partials / spp_audit_open_batch_partials / spp_rlwe_sample_smudge
 *                             the same opening by t of m auditors who never rebuild the key (no counterpart in the reference, whose
 *                             rlwe_decrypt.py:61-91 and shamir.ts:97-169 reconstruct it)
 *   spp_pool_*                the pool program's state and decisions, shielded_pool_program/src: ShieldedPoolState and its root ring
 *                             (state.rs:6-46, instructions/initialize.rs:65-69), process_submit_audit
 *                             (instructions/submit_audit.rs:41-87) and process_withdraw (instructions/withdraw.rs:94-175) for a
 *                             batch of instructions in order -- what the relayer sends without any pre-check
 *                             (demo-frontend/app/api/relay/withdraw/route.ts:224-276)
 *   spp_pool_add_roots        state.add_root (state.rs:28-33) for the new_root of every deposit (instructions/deposit.rs:21-37)
 *   spp_pool_settle_log       a log in which the three kinds alternate, as the chain's does (one audit and one withdraw transaction per
 *                             withdrawal, route.ts:224-276, deposits in between), settled in one call: state.rs:28-46,
 *                             instructions/deposit.rs:21-37, submit_audit.rs:41-87, withdraw.rs:94-175
 *   spp_merkle_tree_find      from a leaf value back to its position(s) in the resident tree: MerkleTreeState.leaves.indexOf, the
 *                             leafIndex of a DepositRecord (demo-frontend/app/lib/storage.ts:9-26,45-50)
 *   spp_wallet_sync           the DepositRecord of every deposit of a wallet -- commitment, leafIndex, nullifier, waCommitment, status
 *                             "pending" | "withdrawn" (storage.ts:9-26), what exportData / importDeposits carry between browsers
 *                             (storage.ts:233-260) -- recomputed from the three secrets per note, the resident tree and the pool's
 *                             accounts: the nullifier PDAs and the audit records process_withdraw tests (withdraw.rs:94-147)
 *   spp_merkle_tree_root_at / _proofs_at / _prefix_roots, spp_withdraw_rows_from_tree_at, spp_prove_withdraw_notes_at(_device)
 *                             getRoot / getProof / the withdraw row and proof for the tree of the first `size` leaves: the root a
 *                             deposit computed locally and pushed (client/payroll-demo.ts:285-292), which the program takes as sent
 *                             (shielded_pool_program/src/instructions/deposit.rs:31-36, :73) -- the resident tree is usually ahead
 *   spp_merkle_tree_find_roots / spp_pool_root_sizes
 *                             from a root word back to the size it belongs to, and which size this pool accepts a proof against:
 *                             isRootValid / getRootAge / isRootNearExpiry (demo-frontend/app/lib/on-chain.ts:93-125,202-235)
 *   spp_withdrawal_audit_plan / spp_prove_withdrawals
 *                             the two transactions of a withdrawal, submit_audit then withdraw (demo-frontend/app/api/relay/withdraw/
 *                             route.ts:129-287), for a batch of notes: every withdraw proof, and one audit record per identity that has
 *                             none yet -- process_submit_audit answers Ok before the proof when it exists (submit_audit.rs:65-73)
 *   spp_msm_g1(_pippenger) / spp_ntt_fr   micro-benchmark entry points (BASELINE.json configs[4]); no reference equivalent
 *
 * Conventions: field elements cross the boundary as 32-byte big-endian canonical integers (the encoding
 * of the reference's .pw files, shielded_pool_program/src/instructions/withdraw.rs:74-90); points as
 * gnark raw uncompressed bytes (64 B G1, 128 B G2). The caller owns every buffer it passes; the library
 * owns device memory inside spp_circuit. All functions return 0 on success or a negative SPP_ERR_* code,
 * with a thread-local message available from spp_last_error(). Calls on one spp_ctx are serialised.
 * There is no CPU fallback: without a HIP device spp_init fails with SPP_ERR_NO_DEVICE.
 */
#ifndef SPP_H
#define SPP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SPP_OK 0
#define SPP_ERR_BAD_INPUT (-1)
#define SPP_ERR_NO_DEVICE (-2)
#define SPP_ERR_IO (-3)
#define SPP_ERR_UNSAT (-4)       /* the inputs do not satisfy the circuit (proof refused before the MSMs) */
#define SPP_ERR_HIP (-5)
#define SPP_ERR_NOT_IMPLEMENTED (-6)
#define SPP_ERR_FORMAT (-7)

#define SPP_CIRCUIT_WITHDRAW 1   /* noir_circuit/src/main.nr */
#define SPP_CIRCUIT_AUDIT 2      /* audit_circuit (scripts/generate_audit.py:246-465) */
/* spp_circuit_build only: the withdraw statement padded with ballast multiplications to the dimensions of the
 * reference's gnark R1CS (noir_circuit/target/shielded_pool_verifier.ccs: 12 452 constraints, domain 2^14), for
 * like-for-like throughput figures.  The container it writes is an ordinary SPP_CIRCUIT_WITHDRAW circuit. */
#define SPP_CIRCUIT_WITHDRAW_REFSHAPE 3
/* spp_circuit_build only: the withdraw statement over a depth-20 tree (20 siblings, 25 secret inputs) -- the synthetic
 * variant of SURVEY 8d Config 2 / BASELINE.json configs[1]; the reference's circuit is depth 16 (main.nr:11). */
#define SPP_CIRCUIT_WITHDRAW_DEPTH20 4

#define SPP_PROOF_LEN 388        /* withdraw.rs:13, submit_audit.rs:18 */
#define SPP_WITHDRAW_PW_LEN 172  /* withdraw.rs:14-16 */
#define SPP_AUDIT_PW_LEN 76      /* submit_audit.rs:19-21 */
#define SPP_TREE_DEPTH 16        /* noir_circuit/src/main.nr:5 */
#define SPP_NOTE_LEN 160         /* one withdraw note: recipient | amount | secret_key | randomness | index, 5 x 32 B */
#define SPP_DEPOSIT_LEN 96       /* one deposit: secret_key | amount | randomness, 3 x 32 B big-endian (main.nr:38-51) */

typedef struct spp_ctx spp_ctx;
typedef struct spp_circuit spp_circuit;

/* Inputs of the withdraw circuit, field order of ShieldedPoolInputs (client/proof.helper.ts:6-21). */
typedef struct {
  uint8_t root[32], nullifier[32], recipient[32];
  uint64_t amount;
  uint8_t wa_commitment[32];
  uint8_t secret_key[32], owner_x[32], owner_y[32], randomness[32];
  uint64_t index;
  uint8_t siblings[SPP_TREE_DEPTH][32];
} spp_withdraw_inputs;

const char* spp_last_error(void);
const char* spp_version(void);

/* ---- host-only: circuit construction (no GPU needed) ---- */
/* Writes the R1CS + solver program container ("SPPC"). aux: for SPP_CIRCUIT_AUDIT the RLWE public key as
 * 2048 uint32 (a[1024] then b[1024], demo-frontend/public/rlwe/rlwe_pk.json); NULL for withdraw.
 * Prints nothing; *n_constraints (optional) receives the constraint count (`nbConstraints=` of sunspot compile). */
int spp_circuit_build(int circuit_id, const uint32_t* aux, const char* out_path, uint32_t* n_constraints);

/* `sunspot compile <acir>` (noir_circuit/prove_linux.sh:66-70) for a program compiled by nargo: lowers the ACIR opcodes --
 * AssertZero, RANGE, the fixed-base Grumpkin MultiScalarMul and the Brillig hints of the reference's withdraw circuit
 * (noir_circuit/target/shielded_pool_verifier.json) -- to an R1CS + solver program in the same SPPC container, so the
 * reference's OWN compiled circuit is what gets set up and proved.  blob: the decoded opcode list written by
 * spp/acir.py:to_blob (bincode decoding stays on the host side).  circuit_id: id stored in the container (0 = generic;
 * SPP_CIRCUIT_WITHDRAW when the program has the withdraw circuit's ABI, so that spp_prove_withdraw accepts it). */
/* The deposit statement (csrc/circuit_deposit.cpp; no counterpart in the reference, whose program checks nothing about a deposit,
 * shielded_pool_program/src/instructions/deposit.rs:31-36,73).  aux NULL.  Depth SPP_TREE_DEPTH.
 *   public  (.pw order): old_root | new_root | commitment | amount | index
 *   private            : owner_x | owner_y | randomness | siblings[SPP_TREE_DEPTH]
 * amount is a u64; commitment == H(owner_x, owner_y, amount, randomness) (main.nr:69-70); index < 2^depth; over the bits of index and
 * ONE set of siblings the path from the empty leaf 0 (client/merkle.ts:152) ends in old_root and the path from commitment in new_root.
 * No secret key: one may deposit to an owner whose key one does not hold; an owner off the curve is an unspendable note. */
#define SPP_CIRCUIT_DEPOSIT 6
#define SPP_CIRCUIT_ACIR 5
int spp_circuit_build_acir(const uint8_t* blob, size_t blob_len, int circuit_id, const char* out_path, uint32_t* n_constraints);

/* ---- device context ---- */
int spp_init(int device, spp_ctx** out);
void spp_free_ctx(spp_ctx* ctx);

/* Deterministic trusted setup on the GPU from a 32-byte seed: writes pk ("SPPK") and vk (gnark raw layout). */
int spp_setup(spp_ctx* ctx, const char* circuit_path, const uint8_t seed[32], const char* pk_path, const char* vk_path);

/* Loads R1CS + proving key, builds the window tables in HBM. window_bits in [4,16] = the same window for every MSM set;
 * 0 = per-set windows chosen greedily within env SPP_TABLE_BUDGET_GB (default 240) and 85 % of the free HBM, single-row tables walked once per window (16 bits = 16 additions per scalar), the row of a base whose wire the circuit bounds to a bit or a byte (solver decompositions, looked-up inputs) only as long as that range (env SPP_RAGGED=0: full rows for every base, for comparison); env SPP_SERIAL=1 (profiling aid) puts both batch workspaces and the G2 MSM on one stream. */
int spp_load_circuit(spp_ctx* ctx, const char* circuit_path, const char* pk_path, int window_bits, spp_circuit** out);
/* Several circuits on ONE GPU at the same time (the reference's relayer submits an audit proof AND a withdraw proof per withdrawal,
 * demo-frontend/app/api/relay/withdraw/route.ts:238-276): plan the windows of all their MSM sets under one HBM budget, then load
 * each circuit with its share.  sizes / bits: n_circuits x 7 in the order of spp_circuit_msm_sizes; spp_pk_msm_sizes reads the
 * sizes from a proving-key file; both are host-only.  spp_load_circuit_with_windows = spp_load_circuit(window_bits = 0) with
 * the planned bits instead of a budget of its own (single-row tables; the two commitment sets keep one row per window).
 * spp_plan_windows has no circuit to read ranges from: it prices every base at a full row, so the loaded tables take at most the
 * planned bytes (spp_circuit_table_bytes tells what they took). */
int spp_pk_msm_sizes(const char* pk_path, uint32_t sizes[7]);
int spp_plan_windows(uint32_t n_circuits, const uint32_t* sizes, double budget_bytes, uint32_t* bits);
int spp_load_circuit_with_windows(spp_ctx* ctx, const char* circuit_path, const char* pk_path, const uint32_t bits[7], spp_circuit** out);
void spp_free_circuit(spp_circuit* c);
/* info[0..7] = id, n_public (without the constant), n_secret, n_wires, n_constraints, domain_log, n_inputs, window_bits */
int spp_circuit_info(const spp_circuit* c, uint32_t info[8]);
/* number of bases per MSM of one proof: G1 sets A, B1, K, Z, commitment basis, commitment basis^sigma; then the G2 set B2 */
int spp_circuit_msm_sizes(const spp_circuit* c, uint32_t sizes[7]);
/* window bits of the table of each of those sets (same order) */
int spp_circuit_msm_windows(const spp_circuit* c, uint32_t bits[7]);
/* table rows per base of each of those sets (same order): 1 = one row of up to 2^(bits-1) multiples, walked once per window
 * (the throughput layout chosen with window_bits = 0); ceil(254 / bits) = one row per window (explicit window_bits) */
int spp_circuit_msm_table_rows(const spp_circuit* c, uint32_t rows[7]);
/* out[0] = lookup-inverse wires 1 / (X - looked-up byte) on the flat A and K sets whose share of those sums is added up by byte
 * bucket instead of one table walk each (0: fewer than 4 096 of them, the sets are not flat, or env SPP_LOOKUP_BUCKETS=0 at load),
 * out[1] = the smallest batch (or 64-aligned batch body) that does so: 1024.  Env SPP_LOOKUP_BUCKETS=N at load (experiment): any
 * circuit with such a wire, batches from N >= 64 proofs.  Same proof bytes either way. */
int spp_circuit_lookup_buckets(const spp_circuit* c, uint32_t out[2]);
/* out[0] = rows of A / B / C that the matrix evaluation sums in integer arithmetic (every term a small coefficient times a wire the
 * lookup argument bounds to a byte range: the audit circuit's 1 088 quotient equations), out[1] = such wires (+1: the constant) */
int spp_circuit_small_rows(const spp_circuit* c, uint32_t out[2]);
/* What the load-time planners made of the circuit (read-only; for tests that must show which path a shape takes):
 * out[0] = runs of constraints that share a B row, out[1] = terms of the longest row of A / B / C, out[2] = rows summed in integer
 * arithmetic, out[3] = byte-ranged wires they read (+1: the constant), out[4] = long rows (16 lanes per proof);
 * out[5..8] = items of the cooperative solver of kind SEQ, PAR, LEVELS, LEVEL_STREAM, out[9] = chunks of the level stream,
 * out[10] = tracks in use (the most of any sequential stretch); out[11] = divisions of the largest wide OP_BATCH_DIV,
 * out[12] = wide steps (OP_BATCH_DIV of 64 or more divisions and OP_COUNT8), out[13] = the wide OP_BATCH_DIV among them;
 * out[14] = OP_SOLVE_ROW rows (the solver of a decoded gnark system) that the cooperative solver takes in level items, out[15] = those
 * among them whose other factor is inverted at run time; both 0 for a circuit without such rows and under SPP_NO_COOP=1 */
int spp_circuit_plan_stats(const spp_circuit* c, uint32_t out[16]);
/* exact bytes of HBM held by the window tables, as allocated (rows sized by range included) */
uint64_t spp_circuit_table_bytes(const spp_circuit* c);

/* ---- proving ---- */
/* Generic batch: inputs = count * n_inputs * 32 B (public then secret, big-endian), rs = count * 64 B blinding
 * (r || s, reduced mod r; NULL = OS randomness). Outputs: proofs count*388, pws count*(12+32*n_public),
 * status[count] (0 ok, SPP_ERR_UNSAT). Returns 0 if every proof was produced, else the first error. */
int spp_prove_batch(spp_circuit* c, size_t count, const uint8_t* inputs, const uint8_t* rs, uint8_t* proofs, uint8_t* pws,
                    int32_t* status);
/* Same with every buffer already resident in HBM (device pointers); asynchronous until spp_sync().
 * Consecutive calls rotate over several HIP streams and workspaces -- two for large batches, four for up to 768 proofs, six for
 * up to 256 -- so the latency-bound phases of a batch (witness solver, Horner combines) overlap the MSMs of the others: output
 * buffers must not be shared by calls that may be in flight together (up to six consecutive calls).
 * d_status: uint32 per proof, nonzero = unsatisfied. */
int spp_prove_batch_device(spp_circuit* c, size_t count, const void* d_inputs, const void* d_rs, void* d_proofs, void* d_pws,
                           void* d_status);
int spp_sync(spp_circuit* c);
/* The value of the circuit's commitment challenge for `count` (partial) input rows: loads the rows, commits to the committed
 * wires (BSB22 / Pedersen, the commitment basis of the proving key) and hashes the commitment to the field exactly as the prover
 * does between its two solver phases; out = count x 32 B big-endian.  For systems whose witness is completed OUTSIDE the library --
 * the reference's own gnark R1CS (noir_circuit/target/shielded_pool_verifier.ccs decoded by spp/ccs.py, every wire an input): the
 * wires after the commitment (the lookup argument's) depend on this value, gnark's solver gets it from the
 * Bsb22CommitmentComputePlaceholder hint (`sunspot prove`, client/proof.helper.ts:58-64).  Wires not known yet are passed as 0.
 * (Circuits built by spp_circuit_build* derive one committed wire, the hiding mask, from the blinding factors of the proof; this
 * call has none and takes them as zero, so for those circuits its result is not the challenge of any real proof.) */
int spp_commitment_challenge(spp_circuit* c, size_t count, const uint8_t* inputs, uint8_t* challenges);
/* per-stage device time of the last spp_prove_batch_device call, milliseconds:
 * [0] witness solve (+commitment), [1] matrix eval, [2] NTT/QAP, [3] MSM G1, [4] wait for the G2 MSM (it runs on a side
 * stream from the end of [0]), [5] assembly, [6] total;
 * [7] = average duration of one k_msm_fixed<G1> launch (the dominant kernel), [8] = number of such launches */
int spp_last_timings(spp_circuit* c, float ms[9]);
/* which = 0: the last enqueued batch, 1: the one before it (consecutive batches alternate between two streams,
 * so reading batch k-1 while batch k runs does not drain the pipeline) */
int spp_timings(spp_circuit* c, int which, float ms[9]);

/* durations (ms) of the MSM kernel launches of one batch (which: as spp_timings), from the dispatches' own timestamps, in launch
 * order: commitment, A, B1, K, Z, proof of knowledge (the six k_msm_fixed<G1> launches), then the G2 launch */
int spp_msm_kernel_ms(spp_circuit* c, int which, float ms[7]);
/* on = 1: run everything of this circuit on one stream (profiling / roofline probe: a kernel's duration is then its own, not
 * stretched by the other batch or by the G2 side stream sharing the chip); on = 0: back to the pipelined default.
 * Synchronises the device. */
int spp_set_serial(spp_circuit* c, int on);

int spp_prove_withdraw(spp_circuit* c, const spp_withdraw_inputs* in, const uint8_t rs_seed[64], uint8_t proof[SPP_PROOF_LEN],
                       uint8_t pw[SPP_WITHDRAW_PW_LEN]);

/* `sunspot verify <vk> <proof> <pw>` (noir_circuit/prove_linux.sh:86-87, audit_circuit/prove_audit.sh:98-99,
 * scripts/generate_audit.py:687-691): host-side Groth16 + BSB22 check. *ok = 1 accepted, 0 rejected; the return value
 * is an error only for malformed inputs. Needs no GPU. */
int spp_verify(const uint8_t* vk, size_t vk_len, const uint8_t* proof, size_t proof_len, const uint8_t* pw, size_t pw_len, int* ok);

/* debug / parity: full witness of proof 0 of the last batch, n_wires * 32 B big-endian */
int spp_debug_witness(spp_circuit* c, uint8_t* out, size_t n_wires);

/* debug / parity, TEST ONLY: the device compile of the arithmetic headers (csrc/bn254.hpp, csrc/f29.hpp, csrc/gnark_hints.hpp) on RAW words.  Unlike every
 * other entry point nothing is converted, reduced or moved to another domain on either side: `in` holds n cases of in_words
 * little-endian uint32 limbs each, exactly the words the header function sees, and `out` receives out_words limbs per case,
 * exactly what it returned.  One lane per case; the kernel loads, calls, stores -- all checking is the caller's
 * (tests/test_gpu_arith.py against Python integers; tests/host/arith_raw_check.cpp is the g++ twin of the same dispatch).
 * selector = field | operation: SPP_ARITH_FR or SPP_ARITH_FQ, plus one of the operation codes of csrc/arith_probe.hpp, which also
 * fixes in_words / out_words per operation (Fp 8 words, F29 9 limbs, Fq2 / F29x2 two of them, c0 first; predicates one word).
 * arg: the k of mul_small; for F29x2 mul / sqr which lifted constant negates a1 (2, 4, 6, 8 = SUBC_kP_1); for BIGS_ADD_SMALL_MUL the
 * multiplier m as a signed 16-bit value, |m| <= 64; otherwise ignored.
 * Accumulator scripts (per case: step count <= 16, 16 step words `table index | negate << 8`, a table of 8 affine points as Fp
 * words) run madd / madd_distinct from infinity and return the inf flag, to_xyzz().to_affine(), one bit per step for what
 * madd_distinct returned, and the accumulator's own limbs.
 * Solver hints (codes >= 128, SPP_ARITH_FR only; word layouts in csrc/arith_probe.hpp): HINT_GLV_SPLIT (the 28 constant words of
 * the solver's scalar-decomposition step, then the scalar -> found, s1, s2), HINT_EMUL_REDUCE (six limb values, q and q^-1 mod 2^256
 * -> quotient, remainder, the six carries as raw 384-bit words and as canonical field elements), HINT_GRUMPKIN_MUL (scalar, gy ->
 * finite, x, y), and the wide-integer primitives under them: BIGS_ADD / SUB / NEGATE / LT / SAR64 / LOW64_ZERO / ADD_SMALL_MUL on
 * 12-word two's-complement operands, BIG_MUL_ACC_4X4_12 / 2X2_12 / 8X8_8 (accumulator, a, b -> accumulator).
 * The probe does NOT check the preconditions the headers state (operands < 2p, limb bounds of the lazy forms, column sums
 * < 2^64, table entries not infinity): out-of-range operands give the header's unspecified result, never a memory fault.
 * SPP_ERR_BAD_INPUT: NULL pointers, n == 0 or n > 2^20, an unknown selector (or an Fq-only operation with SPP_ARITH_FR, an Fr-only one with SPP_ARITH_FQ), an arg
 * the operation does not know, in_words / out_words other than the operation's. */
#define SPP_ARITH_FR 0x000u
#define SPP_ARITH_FQ 0x100u
int spp_debug_arith(spp_ctx* ctx, uint32_t selector, uint32_t arg, size_t n, const uint32_t* in, size_t in_words, uint32_t* out,
                    size_t out_words);

/* ---- witness-input generation (what the reference computes on the client before proving) ---- */
/* RLWE encryption + quotient witnesses for `count` instances (scripts/generate_audit.py:507-554, rlwe.ts:157-247):
 * pk_a, pk_b: 1024 coefficients in [0,q); r, e2: count*1024 int8; e1: count*64 int8; msg: count*64 bytes.
 * Out: c0 count*64, c1 count*1024 (in [0,q)); k0 count*64, k1 count*1024 (signed quotients);
 * packed_be (optional): count * 157 fields of 32 B big-endian = pack_values(c0) ++ pack_values(c1) (:154-163). */
int spp_rlwe_witness_batch(spp_ctx* ctx, const uint32_t* pk_a, const uint32_t* pk_b, size_t count, const int8_t* r, const int8_t* e1,
                           const int8_t* e2, const uint8_t* msg, uint32_t* c0, uint32_t* c1, int32_t* k0, int32_t* k1,
                           uint8_t* packed_be);
/* same, every pointer a device pointer; asynchronous on the context stream until spp_ctx_sync() */
int spp_rlwe_witness_batch_device(spp_ctx* ctx, const void* d_pk_a, const void* d_pk_b, size_t count, const void* d_r, const void* d_e1,
                                  const void* d_e2, const void* d_msg, void* d_c0, void* d_c1, void* d_k0, void* d_k1,
                                  void* d_packed_be);
int spp_ctx_sync(spp_ctx* ctx);
/* Poseidon hash_2 / hash_4 (client/merkle.ts:22-38): in = count * arity * 32 B, out = count * 32 B */
int spp_poseidon_hash_batch(spp_ctx* ctx, size_t count, int arity, const uint8_t* in, uint8_t* out);
/* compute_merkle_root (noir_circuit/src/main.nr:11-29) for count paths: siblings = count * depth * 32 B */
int spp_merkle_root_batch(spp_ctx* ctx, size_t count, uint32_t depth, const uint8_t* leaves, const uint64_t* indices,
                          const uint8_t* siblings, uint8_t* roots);
/* ShieldedPoolMerkleTree.getRoot + getProof (client/merkle.ts:165-221): tree of n_leaves inserted leaves, missing
 * nodes = default hashes (:150-156); siblings_out = n_queries * depth * 32 B */
int spp_merkle_build(spp_ctx* ctx, size_t n_leaves, uint32_t depth, const uint8_t* leaves, size_t n_queries,
                     const uint64_t* query_indices, uint8_t* siblings_out, uint8_t* root_out);
/* The same tree kept RESIDENT in HBM and updated incrementally: insert() appends leaves and recomputes only the
 * touched paths -- O(count + depth) Poseidon hashes per call instead of the O(2^depth) recomputation of every getRoot() /
 * getProof() in client/merkle.ts:165-221; getRoot is one read, getProof `depth` reads per query.  Leaves must be canonical
 * field elements (32 B big-endian).  Calls on one tree are serialised with the other calls on its context. */
typedef struct spp_merkle_tree spp_merkle_tree;
int spp_merkle_tree_new(spp_ctx* ctx, uint32_t depth, spp_merkle_tree** out);
void spp_merkle_tree_free(spp_merkle_tree* t);
uint64_t spp_merkle_tree_size(const spp_merkle_tree* t);
/* ShieldedPoolMerkleTree.insert (client/merkle.ts:158-163) for `count` leaves; *first_index (optional) = index of the first */
int spp_merkle_tree_insert(spp_merkle_tree* t, size_t count, const uint8_t* leaves, uint64_t* first_index);
int spp_merkle_tree_root(spp_merkle_tree* t, uint8_t root[32]);
/* getProof for n leaf indices (any index below 2^depth, inserted or not): siblings_out = n * depth * 32 B */
int spp_merkle_tree_proofs(spp_merkle_tree* t, size_t n, const uint64_t* indices, uint8_t* siblings_out);
/* Deposits from secrets: generateIdentityKeypair, calculateCommitment, mt.insert and mt.getRoot for every deposit
 * (client/payroll-demo.ts:264-292, client/test-shielded-pool.ts:218-231), whose instruction then carries
 * amount u64 LE | commitment | new_root (shielded_pool_program/src/instructions/deposit.rs:21-37; the program pushes new_root
 * into its root ring, state.rs:28-46).  For deposit k of the call, leaf i = *first_index + k:
 *   owner       = secret_key * G on Grumpkin, the key used as given (generateIdentityKeypair reduces it mod 2^128 first,
 *                 client/merkle.ts:98-113; spp_withdraw_rows_from_tree does not, so a deposit and its withdrawal see one key)
 *   commitment  = H(owner_x, owner_y, amount, randomness) (client/merkle.ts:126-133, main.nr:69-70) becomes leaf i
 *   roots[k]    = the root after leaves 0..i: what spp_merkle_tree_root returns if the deposits are inserted one at a time
 * deposits = count * SPP_DEPOSIT_LEN B; commitments and roots = count * 32 B big-endian; first_index, commitments and roots are
 * optional (NULL = not wanted).  Afterwards the tree, its root, size and proofs, and the withdraw-notes path see the new leaves
 * exactly as if spp_merkle_tree_insert had appended the commitments.
 * Refused with SPP_ERR_BAD_INPUT before any device work, the tree unchanged, the offending deposit named in spp_last_error():
 * a field >= r, amount >= 2^64 (main.nr's `amount: pub u64`, deposit.rs's u64), secret_key == 0, count > 2^24, more deposits
 * than the tree has room for (2^depth - size), NULL t, NULL deposits with count > 0.  count == 0 is SPP_OK and sets
 * *first_index = size.  Synchronous; holds the context lock for its whole length, like spp_merkle_tree_insert, so concurrent
 * depositors get disjoint, contiguous index ranges. */
int spp_merkle_tree_deposit(spp_merkle_tree* t, size_t count, const uint8_t* deposits, uint64_t* first_index, uint8_t* commitments,
                            uint8_t* roots);

/* generateIdentityKeypair's sk * G on Grumpkin (client/merkle.ts:98-113; scalar = the canonical field element,
 * as noir_circuit/src/main.nr:54-59): sk count * 32 B -> (x, y) count * 64 B */
int spp_grumpkin_keygen_batch(spp_ctx* ctx, size_t count, const uint8_t* sk, uint8_t* xy);
/* ct_commitment sponge (ct_helper/src/main.nr:15-34): in = count * n * 32 B, out = count * 32 B */
int spp_poseidon2_sponge_batch(spp_ctx* ctx, size_t count, uint32_t n, const uint8_t* in, uint8_t* out);

/* Everything scripts/generate_audit.py:468-641 computes before `nargo execute`, for `count` instances, on the GPU:
 * keygen, wa_commitment, message slots, RLWE encryption + quotients, packing, ct_commitment -> rows of 3360 fields
 * (32 B big-endian, main()'s parameter order :405-417) ready for spp_prove_batch on the audit circuit. */
int spp_audit_inputs_batch(spp_ctx* ctx, const uint32_t* pk_a, const uint32_t* pk_b, size_t count, const uint8_t* sk, const int8_t* r,
                           const int8_t* e1, const int8_t* e2, uint8_t* rows);
int spp_audit_inputs_batch_device(spp_ctx* ctx, const void* d_pk_a, const void* d_pk_b, size_t count, const void* d_sk, const void* d_r,
                                  const void* d_e1, const void* d_e2, void* d_rows);

/* End to end on the device: audit proofs from the provers' raw secrets.  Replaces the whole of scripts/generate_audit.py:468-691
 * for `count` instances -- keygen, wa_commitment, RLWE encryption with the public key (pk_a, pk_b: 1024 x u32 each), quotient
 * witnesses, packing, ct_commitment (:468-641), then `nargo execute` + `sunspot prove` (:668-685, audit_circuit/prove_audit.sh:
 * 74-95) -- without a host round trip: all pointers are device memory (sk count*32 B big-endian, r / e2 count*1024 int8,
 * e1 count*64 int8, rs count*64 B), outputs as spp_prove_batch_device.  Asynchronous, pipelined like spp_prove_batch_device. */
int spp_prove_audit_from_secrets_device(spp_circuit* c, size_t count, const void* d_pk_a, const void* d_pk_b, const void* d_sk, const void* d_r,
                                        const void* d_e1, const void* d_e2, const void* d_rs, void* d_proofs, void* d_pws, void* d_status);

/* The audit record, not just the proof.  spp_prove_audit_from_secrets_device plus the ciphertext each proof commits to: d_c0 count*64 u32,
 * d_c1 count*1024 u32, coefficients in [0,q) -- the c0_sparse / c1 of ciphertext.json (generate_audit.py:590-606), the layout
 * spp_rlwe_decrypt_batch and spp_audit_open_batch read.  Without it the proofs of the call above are records nobody can decrypt.
 * The ciphertext is written by the RLWE kernel of the input pipeline, on the batch's own proving stream: complete after spp_sync(),
 * also for a row the circuit refuses (status != 0).  Same argument checks, pipelining and workspace rotation, same proof and
 * public-witness bytes as the call above; the ciphertext buffers, like the other outputs, must not be shared by calls in flight. */
int spp_prove_audit_records_device(spp_circuit* c, size_t count, const void* d_pk_a, const void* d_pk_b, const void* d_sk, const void* d_r,
                                   const void* d_e1, const void* d_e2, const void* d_rs, void* d_proofs, void* d_pws, void* d_status,
                                   void* d_c0, void* d_c1);
/* host convenience (host buffers, rs NULL = OS randomness, status optional), chunked like spp_prove_withdraw_notes: at most 2 048
 * records per chunk, two chunks in flight.  proofs, pws, status as spp_prove_batch (a refused record: status SPP_ERR_UNSAT, proof
 * bytes zero, ciphertext still written); returns SPP_ERR_UNSAT if any record was refused.  Also refused with SPP_ERR_BAD_INPUT: a
 * public-key coefficient >= q, count > 2^24. */
int spp_prove_audit_records(spp_circuit* c, const uint32_t* pk_a, const uint32_t* pk_b, size_t count, const uint8_t* sk, const int8_t* r,
                            const int8_t* e1, const int8_t* e2, const uint8_t* rs, uint8_t* proofs, uint8_t* pws, int32_t* status,
                            uint32_t* c0, uint32_t* c1);

/* Withdraw proofs from notes against the resident tree: the withdraw counterpart of the call above.  Replaces the per-recipient
 * loop of client/payroll-demo.ts:323-340 -- generateIdentityKeypair (client/merkle.ts:98-113), wa_commitment and nullifier
 * (payroll-demo.ts:264-271), mt.getRoot() / mt.getProof(index) (client/merkle.ts:165-176,198-221), generateProof -- with one
 * kernel that expands each note into a withdraw row on the device.
 *   note = recipient | amount | secret_key | randomness | index    (SPP_NOTE_LEN = 5 x 32 B big-endian, main.nr:38-51)
 *   row  = root | nullifier | recipient | amount | wa_commitment | secret_key | owner_x | owner_y | randomness | index |
 *          siblings[depth]                                        (10 + depth fields, the order spp_prove_withdraw packs)
 * owner = secret_key * G (Grumpkin), wa_commitment = H(owner_x, owner_y), nullifier = H(secret_key, index); root and siblings are
 * the tree's (default hashes for absent nodes).  The note commitment H(owner_x, owner_y, amount, randomness) is not recomputed:
 * a note that is not the leaf at `index` (another leaf, an empty slot, index >= 2^depth -- siblings are then the level defaults
 * and no tree memory is read), amount >= 2^64 or recipient == 0 gives a row the circuit refuses, in place (status != 0).
 * Refused with SPP_ERR_BAD_INPUT: a circuit that is not SPP_CIRCUIT_WITHDRAW, one whose input count is not 10 + the tree's depth,
 * a tree of another spp_ctx, NULL pointers; by the host entry points also any note field >= r.  count == 0 is SPP_OK.
 *
 * Snapshot: every proof of one call is against the root of the tree at the time of the call.  The rows are gathered on the
 * tree's stream, in stream order with spp_merkle_tree_insert, so leaves inserted after the call returns -- even while its
 * proofs are still in flight -- are not seen by it; spp_prove_withdraw_notes builds all rows before its first chunk is proved.
 */
/* rows only (host buffers): notes = count * SPP_NOTE_LEN B -> rows = count * (10 + depth) * 32 B, ready for spp_prove_batch */
int spp_withdraw_rows_from_tree(spp_merkle_tree* t, size_t count, const uint8_t* notes, uint8_t* rows);
/* end to end on the device (device pointers: notes count * SPP_NOTE_LEN B, rs count * 64 B; outputs as spp_prove_batch_device),
 * asynchronous until spp_sync(); pipelined and workspace-rotated like spp_prove_batch_device.  No field check on the notes (the
 * contract of spp_prove_batch_device). */
int spp_prove_withdraw_notes_device(spp_circuit* c, spp_merkle_tree* t, size_t count, const void* d_notes, const void* d_rs, void* d_proofs,
                                    void* d_pws, void* d_status);
/* host convenience: proofs count*388, pws count*(12+32*n_public), status[count] (optional) as spp_prove_batch, which it uses for
 * the proving (large batches in chunks); rs NULL = OS randomness.  Returns SPP_ERR_UNSAT if any note was refused. */
int spp_prove_withdraw_notes(spp_circuit* c, spp_merkle_tree* t, size_t count, const uint8_t* notes, const uint8_t* rs, uint8_t* proofs,
                             uint8_t* pws, int32_t* status);

/* ---- deposit proofs ----
 * The reference's deposit is unchecked: process_deposit reads the commitment and ignores it, pushes whatever new_root the client sent
 * and transfers `amount` lamports that nothing ties to the amount inside the commitment (shielded_pool_program/src/instructions/
 * deposit.rs:31-36,73).  Its program does NOT verify the proofs made here; they serve a pool program that does, and any indexer,
 * relayer or auditor who wants to check a deposit log without rebuilding the tree.
 *   deposit = secret_key | amount | randomness                       (SPP_DEPOSIT_LEN, as spp_merkle_tree_deposit)
 *   row     = old_root | new_root | commitment | amount | index | owner_x | owner_y | randomness | siblings[depth]
 * for leaf i = first_index + k of the tree, which must already hold it (spp_merkle_tree_deposit first): owner = secret_key * G, the
 * key as given; commitment = H(owner_x, owner_y, amount, randomness), computed from the RECORD, never read from the tree; sibling l is
 * the stored node to the left of the path when (i >> l) is odd -- a subtree of leaves below i, final -- and the level default
 * otherwise; old_root and new_root are the path from 0 and from the commitment over those siblings: the roots of sizes i and i + 1
 * (spp_merkle_tree_root_at), whatever the tree's size is now, unchanged by later inserts.
 * A record that is not the deposit at that index (other key, amount or randomness) still gives a self-consistent row and a proof
 * that verifies, of "this commitment at this index after old_root"; its new_root is then not the tree's.  What binds a proof to the
 * real tree is the chain check below, not the row builder.  amount >= 2^64 is not refused here: the row is made and the circuit
 * refuses it in place (status != 0, proof bytes zero), the rest of the batch is proved.
 * Refused with SPP_ERR_BAD_INPUT before any device work, the index named in spp_last_error(): NULL pointers, a circuit that is not
 * SPP_CIRCUIT_DEPOSIT or whose input count is not SPP_DEPOSIT_INPUTS, a tree of another spp_ctx or of a depth other than
 * SPP_TREE_DEPTH (rows only: any depth), first_index + count > the tree's size, count > 2^24; by the host entry points also a field >= r
 * and secret_key == 0.  count == 0 is SPP_OK.
 * Snapshot: the rows are gathered on the tree's stream, in stream order with inserts, as spp_prove_withdraw_notes_device does. */
#define SPP_DEPOSIT_PW_LEN 172
#define SPP_DEPOSIT_INPUTS 24     /* fields per row */
/* rows only, host buffers; leaves first_index .. first_index+count-1 must already be in the tree; rows = count * (8 + depth) * 32 B */
int spp_deposit_rows_from_tree(spp_merkle_tree* t, uint64_t first_index, size_t count, const uint8_t* deposits, uint8_t* rows);
/* end to end on the device, asynchronous until spp_sync(); contract of spp_prove_withdraw_notes_device (no field check on the records) */
int spp_prove_deposits_device(spp_circuit* c, spp_merkle_tree* t, uint64_t first_index, size_t count, const void* d_deposits,
                              const void* d_rs, void* d_proofs, void* d_pws, void* d_status);
/* host convenience, chunked like spp_prove_withdraw_notes; rs NULL = OS randomness; SPP_ERR_UNSAT if any row was refused */
int spp_prove_deposits(spp_circuit* c, spp_merkle_tree* t, uint64_t first_index, size_t count, const uint8_t* deposits,
                       const uint8_t* rs, uint8_t* proofs, uint8_t* pws, int32_t* status);

/* Checking a log of proved deposits, as a program that keeps (current_root, leaf count) would: the instructions are taken one after
 * another from (start_root, start_index); codes[i] is the FIRST failing check in the order below, words compared bytewise as the pool
 * ledger compares them.  An accepted instruction advances (current_root, count) to (its new_root, its index + 1); a rejected one
 * advances nothing, so a deposit built on a rejected one is STALE_ROOT.  end_root / end_index (optional) receive the state after the
 * last accepted instruction.  lamports (optional): the amount each instruction transfers; NULL skips the amount check.
 * The proofs are verified once for the whole batch, independent of position, by spp_verify_batch (SPP_DEPOSIT_BAD_PROOF is its
 * decision, a malformed witness header included); the chain is a sequential scan of 76 bytes per instruction on the host after one
 * download of the flags.  No spp_pool is read or changed: feed the accepted new_roots to spp_pool_add_roots.
 * SPP_ERR_FORMAT: a vk that does not parse or whose public-input count is not 5.  SPP_ERR_BAD_INPUT: NULL ctx, vk, codes or
 * start_root, NULL proofs or pws with count > 0, count > 2^24.  count == 0 is SPP_OK with the end state = the start state. */
#define SPP_DEPOSIT_OK 0
#define SPP_DEPOSIT_BAD_AMOUNT 1   /* pw amount != the instruction's lamports */
#define SPP_DEPOSIT_STALE_ROOT 2   /* pw old_root != the current root at this position */
#define SPP_DEPOSIT_BAD_INDEX 3    /* pw index != the leaf count at this position */
#define SPP_DEPOSIT_BAD_PROOF 4    /* the decision of spp_verify_batch, witness header included */
int spp_verify_deposit_chain(spp_ctx* ctx, const uint8_t* vk, size_t vk_len, size_t count, const uint8_t* proofs, const uint8_t* pws,
                             const uint64_t* lamports /* optional */, const uint8_t start_root[32], uint64_t start_index,
                             uint32_t* codes, uint8_t end_root[32], uint64_t* end_index);

/* Batched verification on the GPU (`sunspot verify` for many proofs against one key, the checks of the
 * deployed verifier withdraw.rs:63-90 / submit_audit.rs:41-54): proofs = count * 388 B, pws = count * pw_len B (host
 * buffers), ok[i] = 1 iff proof i verifies.  Same decisions as spp_verify; one lane per proof. kernel_ms (optional):
 * duration of the verification kernel. */
int spp_verify_batch(spp_ctx* ctx, const uint8_t* vk, size_t vk_len, size_t count, const uint8_t* proofs, const uint8_t* pws, size_t pw_len,
                     int32_t* ok, float* kernel_ms);

/* The same verification by random linear combination (`sunspot verify` for many proofs against one key,
 * noir_circuit/prove_linux.sh:86-87, audit_circuit/prove_audit.sh:98-99).  The proofs are cut into groups of `group`; each
 * proof keeps its format, curve and subgroup checks and one Miller loop, and the pairings against the key and the final
 * exponentiation are paid once per group, on one combined equation weighted by secret 128-bit scalars derived from seed32 and
 * the proof's index.  A group whose equation fails is settled proof by proof by the verifier of spp_verify_batch.
 *   - The decisions are those of spp_verify_batch, except with probability about 2^-127 per call.
 *   - A seed the prover knows or can influence voids that guarantee: with the scalars known, invalid proofs whose errors cancel
 *     in the combination can be built.
 *   - A caller-supplied seed must therefore be drawn AFTER the batch is fixed, and never reused for a batch the prover saw it
 *     used on.  seed32 = NULL takes 32 bytes from the operating system per call.
 * group: a multiple of 64 in [64, 4096], 0 = the default (256).  stats (optional): groups, groups refused, proofs re-verified,
 * proofs dropped (refused by the format, curve or subgroup checks).  kernel_ms (optional) covers all launches of the call.
 * Other arguments and their checks as spp_verify_batch; the key may have at most 34 public inputs. */
#define SPP_RLC_SERIAL_TAIL 1   /* one-lane rlc_final_serial instead of the cooperative tail (tests, probe) */
#define SPP_RLC_NO_FALLBACK 2   /* ok[i] of a refused group's surviving proofs = 0, nothing re-verified     */
int spp_verify_batch_rlc(spp_ctx* ctx, const uint8_t* vk, size_t vk_len, size_t count,
                         const uint8_t* proofs, const uint8_t* pws, size_t pw_len,
                         const uint8_t* seed32 /* NULL: 32 bytes from the OS */, uint32_t group /* 0: default */,
                         uint32_t flags, int32_t* ok,
                         uint32_t stats[4] /* optional: groups, groups refused, proofs re-verified, proofs dropped */,
                         float* kernel_ms);

/* prod_k e(P_k, Q_k) == 1 for 1..4 caller-supplied pairs (G1 64 B, G2 128 B, gnark raw uncompressed), computed on the GPU
 * with the device pairing code of spp_verify_batch (curve + subgroup checks included; *ok = 0 when a point is invalid).
 * No call site in the reference: it exists so that the only gnark-made curve data the reference holds -- its verifying keys
 * noir_circuit/target/shielded_pool_verifier.vk and audit_circuit/target/rlwe_audit.vk -- can be put through the device
 * pairing path (e(beta1, G2) == e(G1, beta2) etc.; tests/test_vk_pins.py).  The _host variant runs the single-proof host
 * pairing of spp_verify instead and needs no GPU. */
int spp_pairing_check(spp_ctx* ctx, uint32_t n_pairs, const uint8_t* g1s, const uint8_t* g2s, int* ok);
int spp_pairing_check_host(uint32_t n_pairs, const uint8_t* g1s, const uint8_t* g2s, int* ok);

/* ---- auditor side (scripts/rlwe_decrypt.py:61-132, demo-frontend/app/lib/shamir.ts:97-169) ---- */
/* Shamir reconstruction at 0 over BN254 Fr for n coefficients from t shares: xs[t] share indices, ys = t * n * 32 B
 * (share-major, big-endian). secret_be (optional): n * 32 B; sk_mod_q (optional): the centred value reduced mod q
 * (reconstructSk, shamir.ts:97-120). */
int spp_shamir_reconstruct(spp_ctx* ctx, uint32_t t, const uint32_t* xs, const uint8_t* ys, size_t n, uint8_t* secret_be,
                           uint32_t* sk_mod_q);
/* rlweDecrypt (shamir.ts:134-169 / rlwe_decrypt.py:106-132) for `count` ciphertexts: c0 count*64, c1 count*1024 in
 * [0,q); msg = count * 64 recovered byte slots (owner_x = slots 0..31 little-endian, owner_y = slots 32..63).
 * A sk_mod_q, c0 or c1 value >= q is refused with SPP_ERR_BAD_INPUT before any device work, the ciphertext and the coefficient
 * named in spp_last_error(), msg untouched: the kernel's sums are sized for coefficients below q.  Records that may be
 * malformed are opened in place by spp_audit_open_batch, which decrypts the residues and raises SPP_AUDIT_BAD_CIPHERTEXT. */
int spp_rlwe_decrypt_batch(spp_ctx* ctx, const uint32_t* sk_mod_q, size_t count, const uint32_t* c0, const uint32_t* c1, uint8_t* msg);

/* ---- auditor key generation (scripts/rlwe_keygen.py:98-182, shamir_share_field :51-65) ----
 * The key pair the audit circuit embeds and spp_prove_audit_records encrypts to, and the t-of-m shares spp_shamir_reconstruct
 * reads.  Polynomials have 1024 coefficients, q = 167772161; `count` keys are count * 1024 values, key after key.
 * All four calls refuse with SPP_ERR_BAD_INPUT before any device work, naming the offending index in spp_last_error(): NULL
 * pointers (checked before the context is touched), an a / pk_a / pk_b / sk_mod_q value >= q, a field element >= r, t == 0,
 * t > 64, m < t, m > 255, an x equal to 0 or repeated, count > 2^16, n > 2^20.  count == 0 and n == 0 are SPP_OK.  Synchronous and
 * serialised on the context.  Device buffers that held sk or sharing coefficients are zeroed before they are freed, host scratch
 * that held them is wiped; the caller's own buffers are the caller's to wipe. */
/* host-only, OS randomness, uniform by rejection: sk, e count*1024 in [-bound, bound] (bound in [1,127]), a count*1024 in [0,q) */
int spp_rlwe_sample_key(size_t count, uint32_t bound, int8_t* sk, uint32_t* a, int8_t* e);
/* b = e - a*sk mod (X^1024+1, q).  pk_b count*1024; sk_mod_q optional, count*1024 */
int spp_rlwe_keygen_batch(spp_ctx* ctx, size_t count, const int8_t* sk, const uint32_t* a, const int8_t* e, uint32_t* pk_b,
                          uint32_t* sk_mod_q);
/* max_abs = count*2: { max |centred(b + a*sk)|, max |centred(sk)| }; the caller compares with its bound */
int spp_rlwe_key_check(spp_ctx* ctx, size_t count, const uint32_t* pk_a, const uint32_t* pk_b, const uint32_t* sk_mod_q,
                       uint32_t* max_abs);
/* t-of-m sharing of n field elements.  xs: m distinct non-zero indices, NULL = 1..m.  secrets_be n*32 canonical.
 * coeffs_be (t-1)*n*32, coefficient of x^k of value i at ((k-1)*n + i)*32, canonical; NULL = OS randomness (rejection below r).
 * ys = m*n*32, share-major.  t == 1: every share equals the secret. */
int spp_shamir_split(spp_ctx* ctx, uint32_t t, uint32_t m, const uint32_t* xs, size_t n, const uint8_t* secrets_be,
                     const uint8_t* coeffs_be, uint8_t* ys);

/* ---- the auditors' key without a dealer: verifiable (Pedersen) sharing, the joint key, share refresh ----
 * spp_rlwe_keygen_batch + spp_shamir_split run on ONE machine, which sees the whole key.  Here each of the m auditors i draws its
 * own s_i, e_i, computes b_i = e_i - a*s_i (spp_rlwe_keygen_batch, a from spp_dkg_a_from_seed) and deals s_i mod r to the others:
 *   C_k[v] = c_k[v] G + c'_k[v] H, k < t, public, c_0 = s_i, c'_0 and every higher coefficient random below r;
 *   y_j[v] = sum_k c_k[v] x_j^k,  y'_j[v] = sum_k c'_k[v] x_j^k, for receiver j alone.
 * G = (1, 2); H = (x, the smaller y) at the first ctr = 0, 1, ... for which x = SHA-256("spp-vss-pedersen-h" | ctr, 4 B big-endian)
 * mod p has x^3 + 3 a square (ctr = 1): nobody knows log_G H, which plain Feldman commitments s G of a coefficient in [-3, 3] would
 * need nobody to look up.  Receiver j accepts value v of dealer i iff y G + y' H == sum_k x_j^k C_k[v].  The key is
 * (a, sum_i b_i mod q), auditor j's share sum_i y_{i->j} mod r: a share file of spp_shamir_split's format for a key nobody ever held.
 * The same dealing with s = 0 refreshes shares: the dealer also publishes c'_0, the receiver also checks C_0 == c'_0 H and adds the
 * sum to its old share; the key stays.  Each dealer publishes the SHA-256 of its public values before any are revealed (else the
 * last one chooses b_i as a function of the others'); that, and who talks to whom, is the caller's (spp dkg-deal / dkg-receive).
 * a: SHA-256("spp-dkg-a" | seed | ctr, 4 B big-endian), ctr = 0, 1, ..., each digest eight big-endian words masked to 28 bits and
 * kept when below q, the first 1024 kept.
 * Refusals as in the key-generation block (SPP_ERR_BAD_INPUT before any device work, the index named in spp_last_error()): NULL
 * required pointers, t == 0, t > 64, m < t, m > 255, an x equal to 0 or repeated, a field element >= r, n > 2^20, dealers == 0,
 * dealers > 255.  n == 0 is SPP_OK.  Synchronous and serialised on the context; device buffers that held secrets, blinds,
 * coefficients or sub-shares are zeroed before they are freed.  The commitments are sums of entries of a table of multiples of G
 * and H (built on the device by the first call, freed with the context) selected by the bytes of the scalars: the addresses read
 * depend on the secrets. */
#define SPP_VSS_BAD_POINT 1   /* a commitment is not 64 canonical bytes of a curve point or of infinity */
#define SPP_VSS_BAD_SHARE 2   /* y G + y' H != sum_k x^k C_k */
#define SPP_VSS_NOT_ZERO  4   /* refresh only: C_0 != s' H */
/* host-only: the two generators as X | Y big-endian; a of the joint key from the agreed seed */
int spp_vss_generators(uint8_t g[64], uint8_t h[64]);
int spp_dkg_a_from_seed(const uint8_t seed[32], uint32_t a[1024]);
/* commitments: t*n*64, C_k[v] at (k*n + v)*64 (infinity: 64 zero bytes)
 * ys, ys_blind: m*n*32 share-major, as spp_shamir_split writes ys
 * blinds_be (n*32): NULL = OS randomness
 * coeffs_be, coeffs_blind_be ((t-1)*n*32, layout of spp_shamir_split): NULL = OS randomness
 * blinds_out (optional, n*32): the constant-term blinds that were used, for a refresh dealer to publish */
int spp_vss_deal(spp_ctx* ctx, uint32_t t, uint32_t m, const uint32_t* xs, size_t n, const uint8_t* secrets_be, const uint8_t* blinds_be,
                 const uint8_t* coeffs_be, const uint8_t* coeffs_blind_be, uint8_t* ys, uint8_t* ys_blind, uint8_t* commitments,
                 uint8_t* blinds_out);
/* The same; ms (optional) receives the device times of the two evaluations together and of the commitment kernel, in milliseconds */
int spp_vss_deal_timed(spp_ctx* ctx, uint32_t t, uint32_t m, const uint32_t* xs, size_t n, const uint8_t* secrets_be,
                       const uint8_t* blinds_be, const uint8_t* coeffs_be, const uint8_t* coeffs_blind_be, uint8_t* ys, uint8_t* ys_blind,
                       uint8_t* commitments, uint8_t* blinds_out, float ms[2]);
/* The receiver at x.
 * commitments: dealers*t*n*64;  ys, ys_blind: dealers*n*32
 * zero_blinds (optional): dealers*n*32, the refresh check
 * flags: dealers*n SPP_VSS_* bits, always written; a commitment that is no point ends that value's check (SPP_VSS_BAD_POINT alone)
 * share_out (optional, n*32) = base_be (optional, else 0) + sum over dealers of ys
 *   written only when every flag is 0; *bad = number of non-zero flags */
int spp_vss_receive(spp_ctx* ctx, uint32_t t, uint32_t x, uint32_t dealers, size_t n, const uint8_t* commitments, const uint8_t* ys,
                    const uint8_t* ys_blind, const uint8_t* zero_blinds, const uint8_t* base_be, uint32_t* flags, uint8_t* share_out,
                    size_t* bad);

/* ---- the committee's commitments, and handing the key to a new committee (verifiable resharing) ----
 * The Pedersen commitments of the dealings are public, and their sums D_k[v] = sum_i C_{i,k}[v], k < t, commit to the ONE polynomial
 * whose value at 0 is the key coefficient sk[v] and whose value at x_j is auditor j's share.  A refresh round adds its dealers'
 * commitments to D: D_0[v] then commits to the same sk[v] under another blind.  E_x[v] = sum_k x^k D_k[v] is the public commitment of the share at x:
 * share_j[v] G + blind_j[v] H == E_{x_j}[v], where blind_j is the sum of every y_blind auditor j was ever dealt.  A member checks
 * its own (share, blind) against the committee with spp_vss_receive itself, called with dealers = 1, commitments = D, x = x_j: no
 * other call is needed for that.
 * Resharing from a set S of exactly t old members to a new committee (t', m'): member j of S deals secret = share_j, blinds =
 * blind_j at threshold t' with spp_vss_deal (blinds_be), not scaled by anything, so its C'_{j,0}[v] is exactly E_{x_j}[v].  The
 * new member at x' checks each sub-share against C'_j (as spp_vss_receive does), checks C'_{j,0} == E_{x_j} (SPP_VSS_NOT_SHARE), and
 * takes share' = sum_{j in S} lambda_j y_j mod r, the blind alike, lambda_j the Lagrange coefficient at 0 of x_j in S; the new
 * committee's commitments are D'_k[v] = sum_{j in S} lambda_j C'_{j,k}[v], k < t', with D'_0 == D_0: the key stays, nobody held it,
 * and old and new shares do not combine.
 * Refusals as in the block above (SPP_ERR_BAD_INPUT before any device work, the index named in spp_last_error()): NULL pointers,
 * a threshold of 0 or above 64, dealers == 0 or > 255 (> 64 with weights), count == 0 or > 255, an index equal to 0 or repeated,
 * a weight or a sub-share >= r, n > 2^20, and a base or a committee entry that is no point (they are the caller's own earlier
 * outputs).  n == 0 is SPP_OK.  Synchronous and serialised on the context; device buffers that held sub-shares, blinds, the new
 * share or the new blind are zeroed before they are freed. */
#define SPP_VSS_NOT_SHARE 8   /* reshare: an old member's C'_0 is not its public share commitment E_x */
/* out_k[v] = base_k[v] + sum_d w_d C_{d,k}[v].
 * commitments: dealers*t*n*64, dealer after dealer;  weights_be: dealers*32 canonical, or NULL (every weight 1; dealers <= 255)
 * base (optional), out: t*n*64
 * flags: dealers*t*n, SPP_VSS_BAD_POINT for every input that is no point, always written; *bad = number of non-zero flags
 * out is written only when *bad == 0 */
int spp_vss_combine_commitments(spp_ctx* ctx, uint32_t t, uint32_t dealers, size_t n, const uint8_t* commitments, const uint8_t* weights_be,
                                const uint8_t* base, uint8_t* out, uint32_t* flags, size_t* bad);
/* The same; kernel_ms (optional) receives the device time of the kernels (decoding the points, the sum), in milliseconds */
int spp_vss_combine_commitments_timed(spp_ctx* ctx, uint32_t t, uint32_t dealers, size_t n, const uint8_t* commitments,
                                      const uint8_t* weights_be, const uint8_t* base, uint8_t* out, uint32_t* flags, size_t* bad,
                                      float* kernel_ms);
/* out[(i*n + v)*64 ..] = sum_k xs[i]^k D_k[v];  committee: t*n*64;  xs: count <= 255 non-zero distinct indices */
int spp_vss_share_commitments(spp_ctx* ctx, uint32_t t, size_t n, const uint8_t* committee, uint32_t count, const uint32_t* xs,
                              uint8_t* out);
/* The new member at x_new.
 * xs_old: the set S, t_old indices;  committee: the old committee's D, t_old*n*64
 * commitments: t_old * t_new*n*64, the dealings of the members of S in xs_old order;  ys, ys_blind: t_old*n*32, in that order
 * flags: t_old*n, SPP_VSS_BAD_POINT (alone) / SPP_VSS_BAD_SHARE / SPP_VSS_NOT_SHARE, always written; *bad = number of non-zero flags
 * share_out, blind_out (n*32) and committee_out (t_new*n*64) are written only when *bad == 0 */
int spp_vss_reshare_receive(spp_ctx* ctx, uint32_t t_old, const uint32_t* xs_old, uint32_t t_new, uint32_t x_new, size_t n,
                            const uint8_t* committee, const uint8_t* commitments, const uint8_t* ys, const uint8_t* ys_blind, uint32_t* flags,
                            uint8_t* share_out, uint8_t* blind_out, uint8_t* committee_out, size_t* bad);

/* Opening audit records in one pass: what an auditor replaying submit_audit logs asks of every record (proof, public witness,
 * ciphertext) -- does the proof verify, is this the ciphertext the proof committed to, is the decrypted identity the one the
 * withdrawal is bound to.  (scripts/rlwe_decrypt.py:135-149 only compares with an expected owner the PROVER wrote.)  One upload,
 * k_verify, then one kernel over the records: range check, packing + ct_commitment sponge, decryption, identity checks, comparison with
 * the two words of the public witness; one download.  Each bit is decided on its own: a record with a bad proof still has bits 2
 * and 4 evaluated and its owner written.  The comparisons are bytewise against the canonical value computed here. */
#define SPP_AUDIT_BAD_PROOF 1       /* the proof does not verify under vk: the decision of spp_verify / spp_verify_batch */
#define SPP_AUDIT_BAD_CIPHERTEXT 2  /* a coefficient >= q, or Poseidon2 sponge(pack(c0) ++ pack(c1)) != the pw's ct_commitment */
#define SPP_AUDIT_BAD_IDENTITY 4    /* decrypted owner_x or owner_y >= r, not on Grumpkin, or H(owner_x, owner_y) != the pw's wa_commitment */
/* proofs count*388, pws count*76, c0 count*64 u32, c1 count*1024 u32 (host buffers); sk_mod_q: 1024 u32 in [0,q) from
 * spp_shamir_reconstruct.  owners: count*64 B, owner_x | owner_y as 32 B big-endian each, the decrypted bytes as they are, always
 * written (a coefficient >= q decrypts as its residue mod q).  flags[i] = 0: record i is proved, bound to this ciphertext, and
 * decrypts to the identity wa_commitment commits to.
 * vk NULL (vk_len 0): records already verified elsewhere (the chain did) -- bit 1 is never set, proofs may be NULL.
 * Refused before any device work: NULL pointers, sk_mod_q[i] >= q, count > 2^24 (SPP_ERR_BAD_INPUT); a malformed vk or one whose
 * public-input count is not 2 (SPP_ERR_FORMAT).  count == 0 is SPP_OK. */
int spp_audit_open_batch(spp_ctx* ctx, const uint8_t* vk, size_t vk_len, const uint32_t* sk_mod_q, size_t count, const uint8_t* proofs,
                         const uint8_t* pws, const uint32_t* c0, const uint32_t* c1, uint8_t* owners, uint32_t* flags);
/* The same with the random-linear-combination verifier of spp_verify_batch_rlc in front of the open kernel instead of k_verify: same
 * argument checks, outputs and vk == NULL behaviour; bit 1 of flags[i] is the decision of spp_audit_open_batch except with probability
 * about 2^-127 per call.  The seed is 32 bytes from the operating system, drawn per call; slices and workspace as in
 * spp_verify_batch_rlc.  group: a multiple of 64 in [64, 4096], 0 = 256 (else SPP_ERR_BAD_INPUT).  stats (optional): groups, groups
 * refused, proofs re-verified, proofs dropped; all zero without a key. */
int spp_audit_open_batch_rlc(spp_ctx* ctx, const uint8_t* vk, size_t vk_len, const uint32_t* sk_mod_q, size_t count, const uint8_t* proofs,
                             const uint8_t* pws, const uint32_t* c0, const uint32_t* c1, uint32_t group, uint8_t* owners, uint32_t* flags,
                             uint32_t stats[4] /* optional */);

/* ---- threshold opening: t of m auditors open records and nobody ever holds the key ----
 * spp_shamir_reconstruct puts the whole RLWE key on one machine, which can then open every record, past and future.  Here each
 * auditor i of a participating set S (|S| = t) computes a PARTIAL decryption from its own share s_i (the share files of
 * spp_shamir_split, unchanged) and a combiner who holds no share turns t partials into the message:
 *   p_i[k] = lambda_i * (s_i * c1 mod X^1024+1)[k] + blind_i[k]  over BN254 Fr, for the 64 message slots k, lambda_i the Lagrange
 *            coefficient at 0 of x_i in S;  sum_i lambda_i s_i = sk coefficient by coefficient and the product is linear, so
 *   sum_i p_i[k] = (sk * c1)[k] + sum_i blind_i[k], a small integer whose centred lift is exact: reduced mod q, added to c0[k] and
 *            rounded it is the byte spp_rlwe_decrypt_batch gives, bit for bit (with e = 0; see below).
 *   blind_i[k] = e + q * rho + sum_{j in S, j != i} sgn(x_i, x_j) * M(seed_ij, ct_commitment, k):  e (int32) and rho (uint64) are the
 *            caller's smudging noise (spp_rlwe_sample_smudge): q * rho vanishes mod q, e joins the ciphertext's noise -- the sum over S
 *            must stay well below Delta/2 = 327 680 together with the ciphertext's own (<= 18 435 when honest).  M is fr.Hash
 *            (expand_message_xmd, SHA-256, 48 bytes mod r) under the tag "spp-partial-mask" of the 64 bytes seed_ij | bytes 4..31 of the
 *            big-endian ct_commitment | k as 4 bytes big-endian; sgn = +1 when x_i < x_j, else -1: the masks of a pair cancel in
 *            the sum, and a single partial is uniformly masked.  The commitment is the Poseidon2 sponge RECOMPUTED from the c0 and c1
 *            handed in, so a mask is never used for two different c1.
 * What this does and does not protect is spelt out in INTEGRATION.md, "Threat model of the threshold opening".
 * All three device calls refuse with SPP_ERR_BAD_INPUT before any device work, naming the offending index in spp_last_error() and
 * leaving the outputs untouched: NULL required pointers, t == 0, t > 64, self >= t, an x equal to 0 or repeated, a share value or a
 * partial >= r, a c0 or c1 value >= q (the partial and the combine call; the open call flags bit 2 as spp_audit_open_batch does),
 * count > 2^24.  count == 0 is SPP_OK.  Synchronous and serialised on the context.  Device buffers that held the share, the scaled
 * share or the pair seeds are zeroed before they are freed. */
#define SPP_PARTIAL_LEN 32
#define SPP_AUDIT_BAD_PARTIALS 8   /* some slot of the combined partials is not a small integer (|.| >= 2^104; honest ones stay
                                      below 2^99): a wrong share, set or record */
/* host-only, OS randomness, uniform by rejection: e[n] in [-bound, bound] (bound <= 2^20), rho[n] uniform 64-bit */
int spp_rlwe_sample_smudge(size_t n, uint32_t bound, int32_t* e, uint64_t* rho);
/* Auditor `self` (a position in xs) of the set xs[t]: partials = count*64*32 B, record-major, 32 B big-endian canonical each.
 * share_be: 1024*32 B canonical, the auditor's own share.  c0 count*64, c1 count*1024 in [0,q).  e, rho: count*64 each, or NULL
 * (= 0).  pair_seeds: t*32 B in xs order, entry j the seed shared with auditor xs[j] (entry `self` is not read), or NULL: no masks --
 * for tests and for t == 1 only, an unmasked partial is a linear equation in the share.  ct_commitments (optional out): count*32 B,
 * the commitments the masks were keyed by; the caller compares them with the records' public witnesses.
 * With t == 1 the partial is s * c1 + blind. */
int spp_rlwe_partial_decrypt_batch(spp_ctx* ctx, uint32_t t, const uint32_t* xs, uint32_t self, const uint8_t* share_be, size_t count,
                                   const uint32_t* c0, const uint32_t* c1, const int32_t* e, const uint64_t* rho,
                                   const uint8_t* pair_seeds, uint8_t* partials, uint8_t* ct_commitments);
/* The combiner: partials = t*count*64*32 B, auditor-major (auditor i's output of the call above at i*count*64*32).  msg: count*64
 * byte slots as spp_rlwe_decrypt_batch writes them, always written; flags (optional): count, 0 or SPP_AUDIT_BAD_PARTIALS. */
int spp_rlwe_combine_partials(spp_ctx* ctx, uint32_t t, size_t count, const uint8_t* partials, const uint32_t* c0, uint8_t* msg,
                              uint32_t* flags);
/* spp_audit_open_batch with t partials per record in the place of sk_mod_q: same vk == NULL behaviour, same owners, bits 1, 2 and 4
 * decided as there on the combined decryption, bit 8 (SPP_AUDIT_BAD_PARTIALS) added. */
int spp_audit_open_batch_partials(spp_ctx* ctx, const uint8_t* vk, size_t vk_len, uint32_t t, const uint8_t* partials, size_t count,
                                  const uint8_t* proofs, const uint8_t* pws, const uint32_t* c0, const uint32_t* c1, uint8_t* owners,
                                  uint32_t* flags);

/* ---- the pool ledger: which of these proofs would the pool accept? ---- */
/* A device-resident restatement of the state the pool program decides on (shielded_pool_program/src): ShieldedPoolState's root ring
 * (state.rs:6-46; fresh = all zero, instructions/initialize.rs:65-69, so on a fresh pool an all-zero root passes check_root, as it
 * does in the program) and the two sets of accounts whose existence the program tests -- spent nullifiers, the ["nullifier", n] PDAs,
 * and audit records, the ["audit", wa_commitment] PDAs.  Keys are the 32 raw bytes of the public-witness word, compared bytewise:
 * v and v + r are different keys, as they are different PDAs.  Each set is an open-addressing table in HBM with a power-of-two slot
 * count >= 2 x capacity (capacity: keys per set, fixed at creation); the slot of a key is the low 64 bits of the key mixed with a
 * per-pool 64-bit salt, from OS randomness unless env SPP_POOL_SALT (hex) is set.  Both verifying keys are prepared once and stay
 * resident; the withdraw key must have 5 public inputs and the audit key 2 (else SPP_ERR_FORMAT).
 *
 * The two batch calls settle instructions 0..count-1 WITH THE DECISIONS THE PROGRAM MAKES PROCESSING THEM ONE AFTER ANOTHER on the
 * state as it stood at the call: each instruction reports the first check that fails, in program order, and an instruction that
 * succeeds creates its account for the ones after it -- inside the batch too.  Duplicates inside a batch are resolved in parallel
 * on the device (csrc/pool_table.hpp has the argument); the results do not depend on scheduling.  "The proof verifies" is the
 * decision of spp_verify / spp_verify_batch, the 12-byte witness header included.
 * This is a pre-screen and a replay tool; it does not replace the on-chain program.  NOT modelled: the vault balance and the lamport
 * transfers (withdraw.rs:199-228) -- `amounts` is returned so that a caller can model them -- and signer / writability / program-id
 * checks on the accounts of a transaction (withdraw.rs:21-59, submit_audit.rs:24-39).
 * All buffers are host memory, all calls synchronous and serialised with the other calls on the pool's spp_ctx.  The return value
 * is an error only for refused calls and HIP failures, never because instructions were rejected.  Refused with SPP_ERR_BAD_INPUT
 * before anything changes: NULL arguments (checked before the context is touched), count > 2^24, and a call that could overflow a
 * set (size + count > capacity).  count == 0 is SPP_OK. */
typedef struct spp_pool spp_pool;
#define SPP_POOL_STATE_LEN 1072            /* size_of::<ShieldedPoolState>(), state.rs:6-17 */
#define SPP_POOL_NULLIFIERS 0
#define SPP_POOL_AUDIT_RECORDS 1
#define SPP_POOL_OK 0                      /* the instruction succeeds; its account is created */
#define SPP_POOL_AUDIT_EXISTS 1            /* submit_audit.rs:66-73: Ok, nothing verified, nothing written */
#define SPP_POOL_NO_AUDIT_RECORD 2         /* withdraw.rs:94-125 */
#define SPP_POOL_BAD_ROOT 3                /* withdraw.rs:131 */
#define SPP_POOL_NULLIFIER_USED 4          /* withdraw.rs:137-147 */
#define SPP_POOL_BAD_RECIPIENT 5           /* withdraw.rs:150-154 */
#define SPP_POOL_BAD_PROOF 6               /* the verifier CPI fails: withdraw.rs:164-175, submit_audit.rs:82-87 */

int  spp_pool_new(spp_ctx*, const uint8_t* withdraw_vk, size_t withdraw_vk_len, const uint8_t* audit_vk, size_t audit_vk_len,
                  uint64_t capacity, spp_pool** out);
void spp_pool_free(spp_pool*);
/* Which verifier the three settling calls below run over the proofs the screen leaves (opt-in; a fresh pool is in mode EACH).
 * Mode RLC verifies the compacted list by random linear combination (spp_verify_batch_rlc above has the scheme): groups of `group`
 * list entries, one combined equation each, a refused group settled by the per-proof kernel.
 *   - The decisions -- codes, amounts, state, sets -- are those of mode EACH except with probability about 2^-127 per verifier launch.
 *   - Only how ok[i] ("the proof of instruction i verifies") is computed changes; every kernel that reads ok[i] is the same, so the
 *     ordering argument of csrc/pool_table.hpp is untouched.
 *   - The weights of a proof are derived from the launch's seed and its instruction index, not from its place in the list, which
 *     depends on scheduling.  The seed is 32 bytes from the operating system for EVERY verifier launch (spp_pool_settle_log makes
 *     two and draws two: instruction ranks overlap between the two kinds).  There is no seed argument and no environment override:
 *     a reused or known seed voids the guarantee (see spp_verify_batch_rlc).
 *   - Launches of the verifier for count <= 2^18 instructions of a kind: three (terms, groups, fallback), whatever the list holds;
 *     beyond that three per slice of 2^18 list entries.  The length of the list is never read back.
 *   - With env SPP_POOL_COMPACT=0 mode RLC runs the dense verifier of spp_verify_batch_rlc over all instructions of the kind.
 * The beta line table and -alpha1 of both keys are prepared when RLC is first selected and stay resident until spp_pool_free.
 * group: a multiple of 64 in [64, 4096], 0 = 256.  Refused with SPP_ERR_BAD_INPUT, the pool unchanged: a NULL pool, an unknown mode,
 * a bad group (in either mode). */
#define SPP_POOL_VERIFY_EACH  0     /* k_verify_list / k_verify: one lane per proof, the default */
#define SPP_POOL_VERIFY_RLC   1     /* random linear combination over the compacted list */
int  spp_pool_set_verifier(spp_pool*, int mode, uint32_t group /* multiple of 64 in [64,4096], 0 = 256 */);
/* The verifier's counters of the last settling call (submit_audit_batch, withdraw_batch, settle_log) that got as far as the device:
 * stats[0..3] for the withdraw key, stats[4..7] for the audit key, each: groups, groups refused, proofs re-verified, proofs dropped
 * (refused by the format, curve or subgroup checks).  All zero after a call in mode EACH. */
int  spp_pool_verify_stats(spp_pool*, uint32_t stats[8]);
/* state.add_root for `count` deposits in order: roots = count * 32 B, the `roots` output of spp_merkle_tree_deposit as it is */
int  spp_pool_add_roots(spp_pool*, size_t count, const uint8_t* roots);
/* the account bytes as bytemuck lays them out: "poolstat", current_root, roots[32], roots_index as u32 LE, 4 zero bytes */
int  spp_pool_state(spp_pool*, uint8_t state[SPP_POOL_STATE_LEN]);
/* counts[0] = spent nullifiers, counts[1] = audit records */
int  spp_pool_counts(spp_pool*, uint64_t counts[2]);
/* accounts known from elsewhere (bootstrapping from chain state): keys = count * 32 B into set `which`; duplicates, within the
 * call or with the set, are ignored */
int  spp_pool_import_keys(spp_pool*, int which, size_t count, const uint8_t* keys);
/* present[i] = 1 if keys[i] is in set `which`, else 0 */
int  spp_pool_contains(spp_pool*, int which, size_t count, const uint8_t* keys, uint8_t* present);
/* process_submit_audit for `count` instructions: proofs = count * 388 B, pws = count * 76 B; key = the wa_commitment word.
 * result[i]: a record with that key exists -- before the call, or made by an earlier instruction of this batch -- gives
 * SPP_POOL_AUDIT_EXISTS whatever proof i is (the program returns Ok before the CPI); otherwise a valid proof gives SPP_POOL_OK and
 * the record is created, an invalid one SPP_POOL_BAD_PROOF. */
int  spp_pool_submit_audit_batch(spp_pool*, size_t count, const uint8_t* proofs, const uint8_t* pws, int32_t* result);
/* process_withdraw for `count` instructions: proofs = count * 388 B, pws = count * 172 B (root, nullifier, recipient, amount,
 * wa_commitment), recipients = count * 32 B account addresses.  result[i] = the first of: no audit record for wa_commitment
 * (NO_AUDIT_RECORD), root neither current nor in the ring (BAD_ROOT), nullifier spent -- before the call, or by an earlier
 * instruction of this batch that succeeded -- (NULLIFIER_USED), recipient word != 00 00 | address[0..30] (BAD_RECIPIENT), proof
 * fails (BAD_PROOF); else SPP_POOL_OK and the nullifier is spent.  Neither the ring nor the audit set changes during the call
 * (spp_pool_settle_log is the call for a log in which they do).
 * amounts (optional): amounts[i] = the u64 in bytes 24..31 of the amount word (withdraw.rs:157-161), written for every instruction. */
int  spp_pool_withdraw_batch(spp_pool*, size_t count, const uint8_t* proofs, const uint8_t* pws, const uint8_t* recipients,
                             int32_t* result, uint64_t* amounts);
/* A log of `count` instructions of all three kinds, in the order the chain processed them: kinds[i] is the kind of instruction i,
 * and the k-th instruction of a kind takes row k of that kind's columns -- roots = n_deposits * 32 B as for spp_pool_add_roots
 * (the new_root a deposit pushes, instructions/deposit.rs:21-37; add_root / check_root are state.rs:28-46), audit_proofs / audit_pws as for
 * spp_pool_submit_audit_batch (submit_audit.rs:41-87), withdraw_proofs / withdraw_pws / recipients as for spp_pool_withdraw_batch
 * (withdraw.rs:94-175).  result[i] = the SPP_POOL_* code the program gives instruction i processing instructions 0..count-1 one
 * after another on the state as it stood at the call; a deposit gives SPP_POOL_OK.  A withdraw meets the audit records and the ring
 * AS OF ITS POSITION: the records that were resident or that an earlier submit_audit of the log created -- a withdraw ahead of its
 * own submit_audit gets NO_AUDIT_RECORD --, and check_root (state.rs:36-46) after exactly the deposits before it, so a root is
 * known for the 32 pushes that follow it and the zero root of a fresh pool until the 32nd push, inside the log as across calls.
 * amounts (optional): the u64 of the amount word for withdraws, 0 elsewhere.  After the call the ring, both sets, spp_pool_state and
 * spp_pool_counts are as if the instructions had gone through the three calls above one at a time.  The number of kernel launches is
 * fixed (two of the verifier), whatever the interleaving.
 * Refused with SPP_ERR_BAD_INPUT before anything changes: NULL arguments (a column may be NULL only when its count is 0), a kinds
 * byte above 2, per-kind counts that do not match kinds or do not sum to count, count > 2^24, audit records + n_audits > capacity,
 * nullifiers + n_withdraws > capacity.  count == 0 is SPP_OK. */
#define SPP_INSTR_DEPOSIT 0
#define SPP_INSTR_SUBMIT_AUDIT 1
#define SPP_INSTR_WITHDRAW 2
int  spp_pool_settle_log(spp_pool*, size_t count, const uint8_t* kinds,
                         size_t n_deposits, const uint8_t* roots,
                         size_t n_audits, const uint8_t* audit_proofs, const uint8_t* audit_pws,
                         size_t n_withdraws, const uint8_t* withdraw_proofs, const uint8_t* withdraw_pws, const uint8_t* recipients,
                         int32_t* result, uint64_t* amounts);

/* ---- wallet sync: find a wallet's notes in the resident tree and say which are spent ---- */
/* A withdraw note needs its leaf index, and an index otherwise has one source: *first_index of the spp_merkle_tree_deposit call that
 * made the leaf, in the same process.  The reference keeps the state per deposit in the browser (DepositRecord and MerkleTreeState,
 * demo-frontend/app/lib/storage.ts:9-26,45-50, carried along by exportData / importDeposits :233-260); all of it derives from the
 * three secrets of a note, the leaf list and the pool's accounts, so here it is recomputed: deposit (or insert the chain's leaves),
 * sync, prove from the returned notes, settle, sync again.
 * Both calls use a leaf index on the tree (csrc/leaf_index.hpp has the layout and the argument why the answers do not depend on
 * scheduling): an open-addressing table of 32-bit leaf indices in HBM, built lazily by these two calls only and extended by the
 * leaves that came since (one insert launch, then the query in a later launch), its slot function salted per tree from OS
 * randomness unless env SPP_TREE_INDEX_SALT (hex) is set when the index is first built.  spp_merkle_tree_insert, _deposit, _root,
 * _proofs and the notes path neither read nor change it; spp_merkle_tree_free releases it.  A value that sits at k leaves costs its
 * queries k table entries to look at, and spp_wallet_sync one nullifier hash per occurrence it examines; k is not capped.
 * Both calls are synchronous, hold the context lock for their whole length and run on the context's stream, so they are ordered with
 * inserts, deposits and the pool's commits.  Refused with SPP_ERR_BAD_INPUT before any device work, tree, index and pool unchanged,
 * the offender named in spp_last_error(): NULL t / leaves / indices / deposits / flags with count > 0 (checked before the context
 * is touched), a value >= r, count > 2^24, a tree of more than 2^30 leaves; count == 0 is SPP_OK. */
/* position of leaf values: indices[i] = the lowest leaf index >= from[i] (from NULL = 0) whose leaf equals leaves[i], UINT64_MAX if
 * none; matches[i] (optional) = how many leaves equal it in the whole tree.  leaves count*32 B canonical big-endian. */
int spp_merkle_tree_find(spp_merkle_tree* t, size_t count, const uint8_t* leaves, const uint64_t* from, uint64_t* indices, uint32_t* matches);

/* For secret i (secret_key | amount | randomness, the key used as given, as spp_merkle_tree_deposit does): owner = secret_key * G,
 * commitment = H(owner_x, owner_y, amount, randomness), wa_commitment = H(owner_x, owner_y), the occurrences of the commitment among
 * the leaves, and nullifier = H(secret_key, index) of the occurrence that is reported:
 *   - with a pool, the lowest index whose nullifier is not in the pool's nullifier set (withdraw.rs:137-147 would pass); if every
 *     occurrence is spent, the lowest index, with SPP_WALLET_SPENT.  Anyone can deposit a copy of a commitment and the owner can
 *     withdraw each copy under its own nullifier, so "first unspent" is the answer that leads to a payable proof;
 *     spp_merkle_tree_find with `from` enumerates the rest;
 *   - without a pool, the lowest index; SPENT and AUDITED are never set.
 * A commitment that is no leaf: indices[i] = UINT64_MAX, no IN_TREE, nullifier word zero; AUDITED is still evaluated.  Nullifier and
 * audit keys are compared bytewise with the canonical encoding computed here, which is what this library's prover writes into the
 * public witness.  notes[i] is the note spp_prove_withdraw_notes takes (recipient | amount | secret_key | randomness | index); for an
 * absent commitment its index word is 2^depth, canonical and out of range: a row the circuit refuses in place (status != 0).
 * Also refused (as above): notes without recipients, secret_key == 0, amount >= 2^64, a recipient word >= r, a pool of another
 * spp_ctx than the tree's. */
#define SPP_WALLET_RECORD_LEN 160   /* commitment | nullifier | wa_commitment | owner_x | owner_y, 5 x 32 B big-endian */
#define SPP_WALLET_IN_TREE  1       /* the commitment is a leaf */
#define SPP_WALLET_SPENT    2       /* H(secret_key, index) is in the pool's nullifier set      (status "withdrawn") */
#define SPP_WALLET_AUDITED  4       /* the pool holds the audit record of wa_commitment         (withdraw.rs:94-125 would pass) */
#define SPP_WALLET_REPEATED 8       /* the commitment sits at more than one leaf */
int spp_wallet_sync(spp_merkle_tree* t, spp_pool* pool /* optional */, size_t count, const uint8_t* deposits /* count * SPP_DEPOSIT_LEN */,
                    const uint8_t* recipients /* optional: count * 32 B recipient words */, uint64_t* indices, uint32_t* flags,
                    uint8_t* records /* optional */, uint8_t* notes /* optional, needs recipients: count * SPP_NOTE_LEN */);

/* ---- the resident tree as of an earlier size: roots, paths and withdraw proofs the chain still accepts ---- */
/* The pool program never checks the root a deposit pushes: instructions/deposit.rs:31-36 reads the commitment and ignores it, :73
 * calls state.add_root on the 32 bytes the client sent, and the client computes them from its own copy of the leaves
 * (client/payroll-demo.ts:285-292).  Two depositors on one base, a lagging indexer or a forged root all leave the chain's
 * current root short of the chain's leaves, and a prover service that has inserted deposits not confirmed yet is ahead of it in any
 * case; a proof against the tree as it stands is then SPP_POOL_BAD_ROOT.  The reference's wallet asks "is my root still among the 33
 * the program accepts" (demo-frontend/app/lib/on-chain.ts:93-125,202-235: isRootValid, getRootAge, isRootNearExpiry).  An append-only
 * tree holds every earlier version of itself -- one node per level differs from what is stored, csrc/merkle_prefix.hpp has the
 * argument -- so these calls answer for the tree of the first `size` leaves (what a fresh tree holds after leaves 0..size-1, default
 * hashes elsewhere, client/merkle.ts:150-156) without building it.
 *   size: any value in [0, spp_merkle_tree_size], or SPP_TREE_SIZE_NOW, with which every _at call returns exactly what the call it
 *   is named after returns.  A larger value is SPP_ERR_BAD_INPUT, both numbers in spp_last_error().
 * An as-of result does not depend on leaves inserted before or after the call, as long as size <= the tree's size at the call: it is
 * made of values that were final when leaf size-1 arrived.  Per call one single-lane launch computes the `depth` hashes of that
 * size's frontier on the tree's stream; the launch that reads it follows on the same stream.
 * The prefix roots R[0..size] are kept in a per-tree device array, extended by the sizes that came since and never recomputed, and
 * a second index of the kind spp_merkle_tree_find uses (csrc/leaf_index.hpp; same fence: insert launch first, query in a later
 * launch; same per-tree salt, env SPP_TREE_INDEX_SALT) goes from a root back to its sizes.  Both are built only by
 * spp_merkle_tree_prefix_roots (the array), spp_merkle_tree_find_roots and spp_pool_root_sizes; insert, deposit, root, proofs, the
 * notes path, find and wallet_sync neither read nor build them; spp_merkle_tree_free releases them.
 * All calls are synchronous except spp_prove_withdraw_notes_at_device, serialised on the tree's spp_ctx; NULL arguments are refused
 * before the context is touched; count == 0 (n == 0) is SPP_OK. */
#define SPP_TREE_SIZE_NOW UINT64_MAX      /* the tree's size at the call */
#define SPP_TREE_NO_SIZE  UINT64_MAX      /* in outputs: no prefix of this tree has that root */
/* getRoot (client/merkle.ts:165-176) of the first `size` leaves */
int spp_merkle_tree_root_at(spp_merkle_tree* t, uint64_t size, uint8_t root[32]);
/* getProof (client/merkle.ts:198-221) in that tree; indices and siblings_out as spp_merkle_tree_proofs (any index below 2^depth) */
int spp_merkle_tree_proofs_at(spp_merkle_tree* t, uint64_t size, size_t n, const uint64_t* indices, uint8_t* siblings_out);
/* roots = count * 32 B: the roots of sizes first_size .. first_size+count-1, the last of which must be <= the tree's size.  roots[k]
 * for first_size = 1 is what spp_merkle_tree_deposit reported for leaf k (client/payroll-demo.ts:285-292) */
int spp_merkle_tree_prefix_roots(spp_merkle_tree* t, uint64_t first_size, size_t count, uint8_t* roots);   /* sizes first_size .. first_size+count-1 */
/* sizes[i] = the lowest size in [0, tree size] whose root equals roots[i] (count * 32 B) bytewise in canonical big-endian form, or
 * SPP_TREE_NO_SIZE; matches[i] = how many sizes have that root -- more than 1 only where zero-valued leaves were appended, the default
 * leaf being 0 (client/merkle.ts:150-156).  A word >= r is not an error: the chain's roots are arbitrary bytes, it matches nothing.
 * Refused: count > 2^24, a tree of more than 2^30 leaves. */
int spp_merkle_tree_find_roots(spp_merkle_tree* t, size_t count, const uint8_t* roots, uint64_t* sizes, uint32_t* matches /* optional */);
/* spp_withdraw_rows_from_tree (client/payroll-demo.ts:323-340) against the first `size` leaves: root = that size's root, siblings the prefix tree's.  A note whose
 * index is >= size is not a leaf of it: a row the circuit refuses in place (status != 0).  Every other argument check as there */
int spp_withdraw_rows_from_tree_at(spp_merkle_tree* t, uint64_t size, size_t count, const uint8_t* notes, uint8_t* rows);
/* spp_prove_withdraw_notes_device / spp_prove_withdraw_notes with such rows, so that check_root (state.rs:36-46) finds the proof's
 * root among the 33 the program holds (what isRootValid asks, demo-frontend/app/lib/on-chain.ts:93-125): argument checks, pipelining, workspaces and the body and
 * tail split are theirs; the frontier launch and the rows launch go on the tree's stream, in order */
int spp_prove_withdraw_notes_at_device(spp_circuit* c, spp_merkle_tree* t, uint64_t size, size_t count, const void* d_notes, const void* d_rs, void* d_proofs, void* d_pws, void* d_status);
int spp_prove_withdraw_notes_at(spp_circuit* c, spp_merkle_tree* t, uint64_t size, size_t count, const uint8_t* notes, const uint8_t* rs, uint8_t* proofs, uint8_t* pws, int32_t* status);
/* Which size can I prove against so that this pool accepts it?  sizes[0] is spp_merkle_tree_find_roots' answer for current_root and
 * sizes[1+k] for roots[k] of spp_pool_state (state.rs:6-46: what check_root compares with); *best = the largest size found, or
 * SPP_TREE_NO_SIZE when none of the 33 words is a prefix root of this tree -- a fresh pool's zero words never are.  Reads the pool,
 * changes neither object's visible state.  Refused: NULL pool / t / sizes, a pool and a tree of different spp_ctx, a tree of more
 * than 2^30 leaves. */
int spp_pool_root_sizes(spp_pool* pool, spp_merkle_tree* t, uint64_t sizes[33], uint64_t* best /* optional */);

/* ---- withdrawals from notes: both proofs, one audit record per new identity ---- */
/* A withdrawal costs the relayer two transactions, submit_audit and then withdraw (demo-frontend/app/api/relay/withdraw/route.ts:129-287:
 * built at :129-218, sent at :238-287).  The audit record is keyed by wa_commitment = H(owner_x, owner_y) -- by the identity, not by
 * the note -- and process_submit_audit answers Ok before it looks at the proof when the record exists (shielded_pool_program/src/
 * instructions/submit_audit.rs:65-73; the relayer's own comment is "might be already initialized", route.ts:264-268).  A recipient
 * who holds several notes under one key needs one audit proof, an identity the pool already knows none, and an audit proof costs
 * about four withdraw proofs.  These two calls turn a batch of notes into exactly what has to be posted.
 *
 * The plan, for `count` 32-byte keys compared bytewise as the pool compares them (v and v + r are two keys) and an optional pool:
 *   - key i is RESIDENT iff a pool is given and its audit-record set holds the key (what spp_pool_contains answers);
 *   - otherwise rep(i) is the lowest j with key[j] == key[i];
 *   - audit_note[0 .. *n_audits) is the ascending list of all i with rep(i) == i: the notes that get an audit record;
 *   - audit_of[i] is the position of rep(i) in audit_note, or SPP_AUDIT_RESIDENT.
 * Computed on the device, on the context's stream -- so ordered with the pool's commits and the tree's inserts -- with a fixed number
 * of launches whatever the keys are, no workgroup waiting for another one; the result depends neither on scheduling nor on the salt
 * of the per-call table (the pool's salt with a pool, else 64 bits from the operating system per call).  csrc/withdrawal_plan.hpp
 * has the argument.  The pool is read and never written. */
#define SPP_AUDIT_RESIDENT 0xFFFFFFFFu
#define SPP_WITHDRAWALS_MAX 1048576       /* keys / notes per call: 2^20 */
/* wa = count * 32 B: the wa_commitment words, e.g. word 2 of the records spp_wallet_sync writes.  audit_of and audit_note have room
 * for count entries; only the first *n_audits of audit_note are written.  Host buffers, synchronous, serialised on the context.
 * Refused with SPP_ERR_BAD_INPUT before any device work: NULL ctx, wa, audit_of, audit_note or n_audits (checked before the context is
 * touched), count > 2^20, a pool of another spp_ctx.  count == 0 is SPP_OK with *n_audits = 0. */
int spp_withdrawal_audit_plan(spp_ctx* ctx, spp_pool* pool /* optional */, size_t count, const uint8_t* wa /* count * 32 B */,
                              uint32_t* audit_of /* count */, uint32_t* audit_note /* count */, uint32_t* n_audits);

/* Both halves of `count` withdrawals in one call: the withdraw proof of every note, and the audit record of every identity that
 * still needs one.
 *   rows     the withdraw rows of all notes are built once, by the kernels of spp_withdraw_rows_from_tree(_at) on the tree's stream,
 *            against the tree as of `size` (SPP_TREE_SIZE_NOW or an earlier size);
 *   plan     the plan above over the wa_commitment word of each row (field 4), on the same stream; the plan arrays are then read back.
 *            *n_audits > audit_cap is SPP_ERR_BAD_INPUT at this point, before any proving: *n_audits, audit_of and the first audit_cap
 *            entries of audit_note are written, both numbers are in spp_last_error();
 *   proving  the withdraw batch goes to the withdraw circuit's proving streams, the audit batch -- spp_prove_audit_records' pipeline
 *            as it is, over secret_key, r, e1, e2 and rs_audit of note audit_note[s] for record s -- to the audit circuit's; each is
 *            enqueued by a host thread of its own, so both are in flight together before either is waited for.
 * Everything that belongs to note i sits at index i of its array, noise and blinding included (only the representatives' are read).
 * r, e1, e2 all NULL: every coefficient is drawn uniformly from [-3, 3] by rejection from OS randomness (the range of
 * scripts/generate_audit.py:469-506); one or two of them NULL is SPP_ERR_BAD_INPUT.  Host scratch that held noise or secret keys is wiped.
 *   - proofs, pws, status are byte for byte what spp_prove_withdraw_notes_at(withdraw, t, size, count, notes, rs_withdraw, ...) returns:
 *     a note that is no leaf (of that size) is refused in place, status SPP_ERR_UNSAT, proof bytes zero.
 *   - record s (audit_proofs, audit_pws, audit_status, c0, c1; audit_cap entries each, audit_note too) is byte for byte what
 *     spp_prove_audit_records returns for the representatives' secrets in slot order.
 *   - A representative is chosen by identity alone: a note whose withdraw row the circuit refuses may still be the representative of
 *     its identity, and its record is valid for the other notes of that identity.  This keeps the two batches independent.
 * Returns SPP_ERR_UNSAT if any row of either side was refused.  Refused with SPP_ERR_BAD_INPUT before any proving: what the two calls
 * refuse (wrong circuit kinds or input counts, a tree of another context, a note field >= r, a public-key coefficient >= q, a size
 * past the tree), secret_key == 0, circuits, tree and pool that are not all of one spp_ctx, count > 2^20, and NULL arguments (checked
 * before the context is touched; status, audit_status, the noise and the blinding may be NULL, the audit outputs when audit_cap is 0).
 * count == 0 is SPP_OK with *n_audits = 0. */
int spp_prove_withdrawals(spp_circuit* withdraw, spp_circuit* audit, spp_merkle_tree* t, spp_pool* pool /* optional */, uint64_t size,
                          const uint32_t* pk_a, const uint32_t* pk_b, size_t count, const uint8_t* notes /* count * SPP_NOTE_LEN */,
                          const int8_t* r, const int8_t* e1, const int8_t* e2 /* per NOTE: count*1024, count*64, count*1024; all three NULL = OS randomness */,
                          const uint8_t* rs_withdraw, const uint8_t* rs_audit /* per NOTE, count*64 each; NULL = OS randomness */,
                          uint8_t* proofs, uint8_t* pws, int32_t* status /* optional */,           /* the withdraw side, per note */
                          uint32_t* audit_of, uint32_t* audit_note, uint32_t* n_audits,           /* the plan */
                          size_t audit_cap, uint8_t* audit_proofs, uint8_t* audit_pws, int32_t* audit_status /* optional */,
                          uint32_t* c0, uint32_t* c1);                                             /* per audit record, audit_cap entries */

/* ---- micro-benchmark / unit entry points ---- */
/* data: n = 2^logn elements, 32 B big-endian each, natural order in and out */
int spp_ntt_fr(spp_ctx* ctx, uint8_t* data, uint32_t logn, int inverse);
/* sum_i scalars[i] * bases[i]; bases 64 B, scalars 32 B (big-endian); out 64 B. Table-based path. */
int spp_msm_g1(spp_ctx* ctx, const uint8_t* bases, const uint8_t* scalars, size_t n, int window_bits, uint8_t out[64]);
/* the same over G2: bases 128 B (gnark raw X.A1 | X.A0 | Y.A1 | Y.A0), out 128 B -- the table walk that produces a proof's Bs */
int spp_msm_g2(spp_ctx* ctx, const uint8_t* bases, const uint8_t* scalars, size_t n, int window_bits, uint8_t out[128]);
/* The flat table walk of the proving sets (one table row per base, window passes put together by Horner) over caller-supplied bases:
 * group 1 = G1 (64 B points), 2 = G2 (128 B); scalars = P rows of n (row p at scalars + 32 * n * p); out = P points.  n, P >= 1.
 * redo_lanes (optional): lanes whose slice met an addition of a point to itself or to its negative and was summed again by the
 * redo kernel (0 when all bases are distinct, up to coincidence). */
int spp_msm_flat_unit(spp_ctx* ctx, int group, const uint8_t* bases, size_t n, const uint8_t* scalars, size_t P, int window_bits, uint8_t* out,
                      uint32_t* redo_lanes);
/* TEST ONLY: the signed-digit planes of the table walks on their own -- the recoding kernel launched as the MSM stage launches it,
 * nothing summed.  scalars: M x P values, 32 B big-endian, scalar row m of proof p at scalars + 32 * (m * P + p) (the [wire][proof]
 * order the kernel reads); rows: N indices < M (base i takes scalar row rows[i]; repeats allowed).  With W = ceil(254 / window_bits)
 * and Pp = *padded_batch (P, rounded up to a multiple of 64 from 64 proofs on), planes receives W * N * Pp int16 digits, digit j of
 * (base i, proof p) at planes[(j * N + i) * Pp + p]: for the signed representative v of the scalar (v = s for s <= (r-1)/2, else
 * s - r) the unique digits in [-2^(c-1), 2^(c-1) - 1] with sum_j d_j 2^(c j) = v.  Entries with p >= P are unspecified.
 * planes_elems: the capacity of planes in digits (W * N * (P rounded up to 64) always suffices).
 * SPP_ERR_BAD_INPUT: NULL pointers, window_bits outside [4,16], M, N or P zero, M or N > 2^20, P > 2^16, a row index >= M, a
 * buffer smaller than the planes. */
int spp_debug_msm_digits(spp_ctx* ctx, const uint8_t* scalars, size_t M, size_t P, const uint32_t* rows, size_t N, int window_bits,
                         int16_t* planes, size_t planes_elems, uint32_t* padded_batch);

/* General-base Pippenger (16-bit signed windows, bucket sort + accumulate + reduce) for large n; same conventions. */
int spp_msm_g1_pippenger(spp_ctx* ctx, const uint8_t* bases, const uint8_t* scalars, size_t n, uint8_t out[64]);
/* the same over G2 (bases and out 128 B, gnark raw X.A1 | X.A0 | Y.A1 | Y.A0): the digit / count / scatter kernels are shared,
 * the bucket kernels run on the G2 accumulator of the table walk */
int spp_msm_g2_pippenger(spp_ctx* ctx, const uint8_t* bases, const uint8_t* scalars, size_t n, uint8_t out[128]);
/* Synthetic, device-resident form of the same MSM (BASELINE.json configs[4]: n = 2^24): bases k_i*G and scalars from
 * an LCG of `seed`; scale_be (optional) multiplies every scalar (linearity checks). Mean ms over `iters` runs. */
int spp_msm_g1_pippenger_bench(spp_ctx* ctx, size_t n, uint64_t seed, const uint8_t scale_be[32], int iters, uint8_t out[64],
                               float* ms_total, float* ms_bucket_kernel);
/* Same with a "witness-like" scalar distribution: small_permille / 1000 of the scalars are byte-sized (SURVEY 8d Config 5:
 * 70 % of a gnark witness is small), the rest uniform. */
int spp_msm_g1_pippenger_bench_dist(spp_ctx* ctx, size_t n, uint64_t seed, uint32_t small_permille, const uint8_t scale_be[32], int iters,
                                    uint8_t out[64], float* ms_total, float* ms_bucket_kernel);
/* Points [first, first + count) of the same n_total-point synthetic MSM: what one of N ranks computes when the 2^24 points of
 * BASELINE.json configs[4] are cut over the GPUs of a node; the N partial sums are gathered and added by the caller
 * (spp/multi.py msm_g1_sharded).  out = this share's partial sum. */
int spp_msm_g1_pippenger_bench_shard(spp_ctx* ctx, size_t n_total, size_t first, size_t count, uint64_t seed, uint32_t small_permille,
                                     const uint8_t scale_be[32], int iters, uint8_t out[64], float* ms_total, float* ms_bucket_kernel);
/* out[i] = scalar * points[i] for ONE scalar and n G1 points (64 B each, 64 zero bytes = infinity, which maps to infinity): the
 * kernel of the setup ceremony below, one lane per point.  n = 0 is SPP_OK.  SPP_ERR_BAD_INPUT: scalar 0, a scalar >= r, a point
 * that is not on the curve or has a coordinate >= q. */
int spp_g1_scale_points(spp_ctx* ctx, const uint8_t* points /* n*64 */, size_t n, const uint8_t scalar_be[32], uint8_t* out /* n*64 */);
/* The same with timings (profiles/setup_ceremony_probe.py): *kernel_ms = the scaling kernel alone, between two events; *host_ms = one
 * host thread running scalar_mul (csrc/bn254.hpp) and to_affine over the first min(host_points, n) points, whose bytes must equal
 * the kernel's (else SPP_ERR_HIP).  kernel_ms and host_ms may be NULL. */
int spp_g1_scale_points_timed(spp_ctx* ctx, const uint8_t* points, size_t n, const uint8_t scalar_be[32], uint8_t* out, float* kernel_ms,
                              size_t host_points, float* host_ms);

/* ---- setup ceremony: contributions to the delta of a proving key (Groth16 phase 2) ----
 * spp_setup derives all toxic waste from one seed, so whoever ran it can forge proofs for its key.  A contribution multiplies delta
 * by a secret d nobody else learns: delta1' = d delta1, delta2' = d delta2, K' = K / d (the private wires' section), Z' = Z / d;
 * every other byte of the proving key (SPPK layout) and of the verifying key (gnark raw layout) is copied.  After a chain of
 * contributions nobody can forge THROUGH DELTA if ONE contributor was honest and forgot d.  That makes the key sound only when
 * nobody knows its other secrets either: a key that started in spp_setup does NOT get that, because whoever ran spp_setup still
 * knows tau, alpha, beta and gamma as field elements and forges without delta (C = 0, A = a G1, B = b G2 with
 * a b = alpha beta + gamma sum x_i k_i), and knows sigma, the trapdoor of the commitment's proof of knowledge.  The first phase, which
 * re-randomises tau, alpha and beta, is the powers-of-tau transcript below (spp_ptau_*).  The contributed key loads, proves and
 * verifies through the existing calls; the on-chain verifier is redeployed from the final vk, as after spp_setup.
 *
 * (d, k) = fr.Hash(entropy, "spp-groth16-contribute-v1", 2 elements) -- the derivation of spp_setup's toxic waste; entropy NULL:
 * 32 bytes from the operating system.  The same entropy and inputs give the same three outputs byte for byte.  d = 0 is refused.
 * receipt = delta1' (64) | T = k delta1 (64) | z = k + c d mod r (32, big-endian), a proof of knowledge of d with
 * c = fr.Hash(SHA256(pk_in bytes) | delta1 | delta1' | T, "spp-groth16-contribute-c1"), points as 64 B raw.
 * d, 1/d, k and the digits of 1/d are overwritten in host and device memory before the call returns, on every path.
 * SPP_ERR_IO: a file cannot be read or written; SPP_ERR_FORMAT: pk_in / vk_in do not parse or hold an invalid point;
 * SPP_ERR_BAD_INPUT: NULL, vk_in does not carry pk_in's delta, d = 0. */
#define SPP_CONTRIB_RECEIPT_LEN 160
int spp_setup_contribute(spp_ctx* ctx, const char* pk_in, const char* vk_in, const uint8_t entropy[32] /* NULL = OS randomness */,
                         const char* pk_out, const char* vk_out, uint8_t receipt[SPP_CONTRIB_RECEIPT_LEN]);
/* One link of a chain: is (pk_after, vk_after) a contribution to (pk_before, vk_before) with this receipt?  *ok = 1 and *reason = 0,
 * or *ok = 0 and *reason = the FIRST check that fails, in this order:
 *   SPP_CONTRIB_FORMAT              a file does not parse
 *   SPP_CONTRIB_NOT_A_DELTA_CHANGE  the proving keys differ outside delta1, delta2, the K points and the Z points (header, counts,
 *                                   wire lists and every other section are compared byte for byte)
 *   SPP_CONTRIB_POINT_INVALID       a delta1, a K or a Z point of either key is not on the curve or has a coordinate >= q (checked on
 *                                   the device before any sum touches them); delta1' is infinity; a delta2 is not a point of the
 *                                   order-r subgroup of the twist; `after` has a point at infinity where `before` has none
 *   SPP_CONTRIB_RECEIPT             the receipt's delta1' is not pk_after's, T is no point, z >= r, or z delta1 != T + c delta1'
 *   SPP_CONTRIB_DELTA_PAIR          e(delta1', G2) e(-G1, delta2') != 1 (the generators of spp_setup)
 *   SPP_CONTRIB_SCALING             with rho_i = the first 128 bits of SHA256(SHA256(pk_before) | SHA256(pk_after) | i as 8 bytes
 *                                   big-endian), P = sum rho_i (K | Z)_i of pk_before and P' the same of pk_after (device Pippenger):
 *                                   e(P', delta2') e(-P, delta2) != 1.  The rho_i are fixed only once both files are: a key in which
 *                                   some point is not (1/d) times its original passes with probability about 2^-128
 *   SPP_CONTRIB_VK                  vk_after differs from vk_before outside delta1 | delta2, or does not carry pk_after's
 * A refusal is SPP_OK with *ok = 0.  The return value is an error only for I/O (SPP_ERR_IO), NULL arguments or the device. */
#define SPP_CONTRIB_OK 0
#define SPP_CONTRIB_FORMAT 1
#define SPP_CONTRIB_NOT_A_DELTA_CHANGE 2
#define SPP_CONTRIB_POINT_INVALID 3
#define SPP_CONTRIB_RECEIPT 4
#define SPP_CONTRIB_DELTA_PAIR 5
#define SPP_CONTRIB_SCALING 6
#define SPP_CONTRIB_VK 7
int spp_setup_verify_contribution(spp_ctx* ctx, const char* pk_before, const char* vk_before, const char* pk_after, const char* vk_after,
                                  const uint8_t receipt[SPP_CONTRIB_RECEIPT_LEN], int* ok, uint32_t* reason);

/* ---- setup ceremony: contributions to sigma, the trapdoor of the commitment's proof of knowledge ----
 * CS = sigma CB (the committed wires' second section) and the vk's LAST G2 point H = -rho sigma G2 are all that depends on sigma.  A
 * contribution with secret s sets CS' = s CS (the scaling kernel of the delta contributions) and H' = s H (host) and copies every
 * other byte; after a chain nobody knows sigma if ONE contributor was honest.  Sigma links and delta links are separate files of a
 * chain: each verifier compares every section it does not own byte for byte.
 * (s, k) = fr.Hash(entropy, "spp-groth16-sigma-v1", 2 elements); receipt = CS'_0 (64) | T = k CS_0 (64) | z = k + c s (32) with
 * c = fr.Hash(SHA256(pk_in bytes) | CS_0 | CS'_0 | T, "spp-groth16-sigma-c1").  Same entropy and inputs, same bytes; s = 0 refused;
 * the secrets are cleared as in spp_setup_contribute.  A key without committed wires: SPP_ERR_BAD_INPUT (both calls). */
int spp_setup_contribute_sigma(spp_ctx* ctx, const char* pk_in, const char* vk_in, const uint8_t entropy[32] /* NULL = OS randomness */,
                               const char* pk_out, const char* vk_out, uint8_t receipt[SPP_CONTRIB_RECEIPT_LEN]);
/* One sigma link.  *ok = 1 and *reason = 0, or *ok = 0 and *reason:
 *   SPP_SIGMA_FORMAT              a file does not parse
 *   SPP_SIGMA_NOT_A_SIGMA_CHANGE  the proving keys differ outside the CS points, or the verifying keys outside their last G2 point
 *   SPP_SIGMA_POINT_INVALID       a CS point of either key is not on the curve or has a coordinate >= q (the device's check); CS_0 or
 *                                 CS'_0 is infinity; `after` has infinity where `before` has none; H or H' is not in the order-r subgroup
 *   SPP_SIGMA_RECEIPT             the receipt's CS'_0 is not pk_after's, T is no point, z >= r, or z CS_0 != T + c CS'_0
 *   SPP_SIGMA_SCALING             with rho_i as in spp_setup_verify_contribution: e(sum rho_i CS'_i, H) != e(sum rho_i CS_i, H')
 *   SPP_SIGMA_VK                  vk_after does not carry s H for the receipt's s: e(CS'_0, H) != e(CS_0, H')
 * The scaling is tested against the point the vk carries, so SPP_SIGMA_VK is decided first: a vk that kept the old point is
 * SPP_SIGMA_VK whatever the CS points are; otherwise the reason is the first failing check in the order above. */
#define SPP_SIGMA_OK 0
#define SPP_SIGMA_FORMAT 1
#define SPP_SIGMA_NOT_A_SIGMA_CHANGE 2
#define SPP_SIGMA_POINT_INVALID 3
#define SPP_SIGMA_RECEIPT 4
#define SPP_SIGMA_SCALING 5
#define SPP_SIGMA_VK 6
int spp_setup_verify_sigma_contribution(spp_ctx* ctx, const char* pk_before, const char* vk_before, const char* pk_after, const char* vk_after,
                                        const uint8_t receipt[SPP_CONTRIB_RECEIPT_LEN], int* ok, uint32_t* reason);

/* ---- setup ceremony, first phase: the powers-of-tau transcript ----
 * A transcript holds powers of a secret tau in both groups, with alpha and beta applied, and nothing circuit-specific:
 *   'SPPT' | version 1 | domain_log L (u32 little-endian each), n = 2^L |
 *   T1: tau^i G1, i < 2n - 1 (64 B raw) | T2: tau^i G2, i < n (128 B raw) | A1: alpha tau^i G1, i < n | B1: beta tau^i G1, i < n |
 *   beta2 = beta G2.  No counts are stored (they follow from L); raw points as spp_setup writes them.
 * Anyone may contribute: with secrets t, a, b point i of T1 and T2 is multiplied by t^i, of A1 by a t^i, of B1 by b t^i, beta2 by b, so
 * tau' = t tau, alpha' = a alpha, beta' = b beta.  After a chain of contributions nobody knows tau, alpha or beta if ONE
 * contributor was honest and forgot t, a and b.  Anyone may verify a link from the two files and the receipt.
 *
 * spp_ptau_new writes the transcript of tau = alpha = beta = 1 (every point a generator), host only; domain_log in [1, 20].
 *
 * spp_ptau_contribute: (t, a, b, k_t, k_a, k_b) = fr.Hash(entropy, "spp-ptau-contribute-v1", 6 elements), entropy NULL: 32 bytes
 * from the operating system; a zero among t, a, b is refused.  The same entropy and input give the same bytes.  Every input point is
 * checked before anything multiplies it: coordinates below q and the curve equation on the device (G2 included), the order-r
 * subgroup of the G2 points on the host; infinity, or powers that do not start at the generators, are refused (SPP_ERR_FORMAT).
 * The per-point scalars are built on the host and uploaded once; the products run on the device, one lane per point with that
 * lane's scalar.  receipt = three proofs of knowledge, 160 B each, for (t, T1_1), (a, A1_0), (b, B1_0):
 *   base' (64, the point of the file after) | T = k base (64) | z = k + c s mod r (32, big-endian),
 *   c = fr.Hash(SHA256(in file) | base | base' | T, "spp-ptau-contribute-c1").
 * The secrets, the scalar array and their copies are overwritten in host and device memory before the call returns, on every path. */
#define SPP_PTAU_RECEIPT_LEN 480
int spp_ptau_new(uint32_t domain_log, const char* path);
int spp_ptau_contribute(spp_ctx* ctx, const char* in_path, const uint8_t entropy[32] /* NULL = OS randomness */, const char* out_path,
                        uint8_t receipt[SPP_PTAU_RECEIPT_LEN]);
/* One link: is `after` a contribution to `before` with this receipt?  *ok = 1 and *reason = 0, or *ok = 0 and *reason = the FIRST
 * check that fails, in this order:
 *   SPP_PTAU_FORMAT         a file does not parse (magic, version, L in [1, 20], the length L gives)
 *   SPP_PTAU_SIZE           the two transcripts differ in L
 *   SPP_PTAU_POINT_INVALID  in `after`: a point off the curve or with a coordinate >= q (checked on the device before any sum
 *                           touches it); infinity anywhere; T1'_0 != G1 or T2'_0 != G2; T2'_1, beta2' or one of the two
 *                           combinations of T2' points that TAU_G2 pairs is outside the order-r subgroup of the twist
 *   SPP_PTAU_RECEIPT        a proof's base' is not the file's, T is no point, z >= r, or z base != T + c base'
 *   SPP_PTAU_TAU_G1         with rho_i = the first 128 bits of SHA256(SHA256(before) | SHA256(after) | tag | i as 8 bytes big-endian)
 *                           (tag, one byte: 1 T1, 2 T2, 3 A1, 4 B1): e(sum rho_i T1'_{i+1}, G2) e(-sum rho_i T1'_i, T2'_1) != 1, i < 2n - 2
 *   SPP_PTAU_TAU_G2         e(T1'_1, sum rho_i T2'_i) e(-G1, sum rho_i T2'_{i+1}) != 1, i < n - 1
 *   SPP_PTAU_ALPHA          the T1 test over A1', i < n - 1 (A1'_0 is tied to the receipt)
 *   SPP_PTAU_BETA           the same over B1', or e(B1'_0, G2) e(-G1, beta2') != 1
 * The sums run on the device (the resident-buffer Pippenger, G1 and G2), the Miller loops on the host.  A refusal is SPP_OK with
 * *ok = 0; the return value is an error only for I/O, NULL arguments or the device. */
#define SPP_PTAU_OK 0
#define SPP_PTAU_FORMAT 1
#define SPP_PTAU_SIZE 2
#define SPP_PTAU_POINT_INVALID 3
#define SPP_PTAU_RECEIPT 4
#define SPP_PTAU_TAU_G1 5
#define SPP_PTAU_TAU_G2 6
#define SPP_PTAU_ALPHA 7
#define SPP_PTAU_BETA 8
int spp_ptau_verify_contribution(spp_ctx* ctx, const char* before_path, const char* after_path, const uint8_t receipt[SPP_PTAU_RECEIPT_LEN],
                                 int* ok, uint32_t* reason);
/* The transcript's kernels on their own: out[i] = scalar_i * points[i], a scalar per point (scalars_be: n * 32 B big-endian), G1
 * points 64 B and G2 points 128 B raw; infinity maps to infinity; n = 0 is SPP_OK.  SPP_ERR_BAD_INPUT: a scalar 0 or >= r, a point
 * that is not on the curve or has a coordinate >= q.  G2 points are NOT tested for the subgroup. */
int spp_g1_mul_each(spp_ctx* ctx, const uint8_t* points /* n*64 */, size_t n, const uint8_t* scalars_be /* n*32 */, uint8_t* out /* n*64 */);
int spp_g2_mul_each(spp_ctx* ctx, const uint8_t* points /* n*128 */, size_t n, const uint8_t* scalars_be /* n*32 */, uint8_t* out /* n*128 */);

/* ---- setup ceremony: a circuit's keys from a transcript ----
 * Deterministic and without a secret: the SPPK container and the gnark raw vk exactly as spp_setup lays them out, for the tau,
 * alpha and beta of the transcript and gamma = delta = sigma = rho = 1 (delta1 = G1, delta2 = gamma2 = G2, CS = CB, the vk's last two
 * G2 points (G2, -G2)); the sections list the same wires by the same predicates.  Checking a published derivation is re-running it
 * and comparing the files.  The delta contributions above (spp_setup_contribute) then re-randomise delta.
 *   Lagrange points  L_k = (1 / n) sum_i w^(-k i) T_i, an inverse NTT of size n = 2^domain_log over POINTS with w the root spp_setup
 *                    takes: three times in G1 (over T1[0 .. n), A1, B1) and once in G2 (over T2), on the device
 *   column gather    A_j = sum_k A[k][j] L_k, B_j the same in G1 and in G2, K_j = sum_k A[k][j] beta L_k + B[k][j] alpha L_k + C[k][j] L_k:
 *                    the host transposes the matrices and plans, the device multiplies and sums
 *   Z_i = T1_{i+n} - T1_i (i < n - 1), alpha1 = A1_0, beta1 = B1_0, beta2 from the file
 * A transcript of a larger domain_log serves (a prefix of the powers is a transcript) and gives the same bytes; a smaller one is
 * SPP_ERR_BAD_INPUT.  Every transcript point that is used is checked first (the device's range and curve checks, the G2 subgroup on
 * the host): SPP_ERR_FORMAT.  The derived key loads through spp_load_circuit. */
int spp_setup_from_ptau(spp_ctx* ctx, const char* circuit_path, const char* ptau_path, const char* pk_path, const char* vk_path);
/* The transform alone: out[k] = (1 / n) sum_i w^(-k i) points[i] for n = 2^logn raw points (logn in [1, 20]; infinity allowed).
 * SPP_ERR_BAD_INPUT: a point that is not on the curve or has a coordinate >= q.  G2 points are NOT tested for the subgroup. */
int spp_ec_intt_g1(spp_ctx* ctx, const uint8_t* points /* n*64 */, uint32_t logn, uint8_t* out /* n*64 */);
int spp_ec_intt_g2(spp_ctx* ctx, const uint8_t* points /* n*128 */, uint32_t logn, uint8_t* out /* n*128 */);
/* The same with timings (profiles/ptau_probe.py), group 1 = G1, 2 = G2: ms[0] = the logn stages, ms[1] = the scaling by 1 / n and the
 * conversion to affine, between events; *host_ms = one host thread over the first min(host_butterflies, n / 2) butterflies of stage 0,
 * the text the lanes run.  ms and host_ms may be NULL. */
int spp_ec_intt_timed(spp_ctx* ctx, int group, const uint8_t* points, uint32_t logn, uint8_t* out, float ms[2], size_t host_butterflies,
                      float* host_ms);

#ifdef __cplusplus
}
#endif
#endif
