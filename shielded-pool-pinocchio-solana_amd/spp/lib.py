"""ctypes binding of libspp.so -- fails loudly when the HIP library is missing."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "libspp.so")
_LIB = None

SPP_OK = 0
SPP_ERR_BAD_INPUT = -1
SPP_ERR_UNSAT = -4
SPP_ERR_FORMAT = -7
SPP_CIRCUIT_WITHDRAW = 1
SPP_CIRCUIT_AUDIT = 2
SPP_CIRCUIT_WITHDRAW_DEPTH20 = 4     # build only: withdraw over a depth-20 tree (synthetic variant)
SPP_CIRCUIT_WITHDRAW_REFSHAPE = 3   # build only: withdraw padded to the reference's R1CS size (12 452 constraints)
SPP_CIRCUIT_DEPOSIT = 6             # old_root | new_root | commitment | amount | index public; owner, randomness, siblings private
PROOF_LEN = 388
NOTE_LEN = 160                      # withdraw note: recipient | amount | secret_key | randomness | index
DEPOSIT_LEN = 96                    # deposit: secret_key | amount | randomness
DEPOSIT_PW_LEN = 172                # deposit public witness: header | old_root | new_root | commitment | amount | index
DEPOSIT_INPUTS = 24                 # fields of a deposit row
SPP_DEPOSIT_OK = 0                  # spp_verify_deposit_chain (include/spp.h)
SPP_DEPOSIT_BAD_AMOUNT = 1
SPP_DEPOSIT_STALE_ROOT = 2
SPP_DEPOSIT_BAD_INDEX = 3
SPP_DEPOSIT_BAD_PROOF = 4
DEPOSIT_RESULT_NAMES = ("OK", "BAD_AMOUNT", "STALE_ROOT", "BAD_INDEX", "BAD_PROOF")
AUDIT_PW_LEN = 76                   # audit public witness: header | wa_commitment | ct_commitment
# spp_audit_open_batch: bits of flags[i] (include/spp.h)
SPP_RLC_SERIAL_TAIL = 1     # spp_verify_batch_rlc flags (include/spp.h)
SPP_RLC_NO_FALLBACK = 2
SPP_AUDIT_BAD_PROOF = 1
SPP_AUDIT_BAD_CIPHERTEXT = 2
SPP_AUDIT_BAD_IDENTITY = 4
SPP_AUDIT_BAD_PARTIALS = 8          # spp_audit_open_batch_partials, spp_rlwe_combine_partials
PARTIAL_LEN = 32
# the pool ledger, spp_pool_* (include/spp.h)
WITHDRAW_PW_LEN = 172               # withdraw public witness: header | root | nullifier | recipient | amount | wa_commitment
SPP_POOL_STATE_LEN = 1072           # size_of::<ShieldedPoolState>()
SPP_POOL_NULLIFIERS = 0
SPP_POOL_AUDIT_RECORDS = 1
SPP_POOL_OK = 0
SPP_POOL_AUDIT_EXISTS = 1
SPP_POOL_NO_AUDIT_RECORD = 2
SPP_POOL_BAD_ROOT = 3
SPP_POOL_NULLIFIER_USED = 4
SPP_POOL_BAD_RECIPIENT = 5
SPP_POOL_BAD_PROOF = 6
SPP_POOL_VERIFY_EACH = 0            # spp_pool_set_verifier: one lane per proof (the default)
SPP_POOL_VERIFY_RLC = 1             # ... by random linear combination over the compacted list
SPP_INSTR_DEPOSIT = 0               # kinds of spp_pool_settle_log
SPP_INSTR_SUBMIT_AUDIT = 1
SPP_INSTR_WITHDRAW = 2
# wallet sync, spp_wallet_sync (include/spp.h): record = commitment | nullifier | wa_commitment | owner_x | owner_y
SPP_WALLET_RECORD_LEN = 160
SPP_WALLET_IN_TREE = 1              # the commitment is a leaf
SPP_WALLET_SPENT = 2                # its nullifier is in the pool's nullifier set (status "withdrawn")
SPP_WALLET_AUDITED = 4              # the pool holds the audit record of wa_commitment
SPP_WALLET_REPEATED = 8             # the commitment sits at more than one leaf
SPP_TREE_SIZE_NOW = (1 << 64) - 1   # the _at calls: the tree's size at the call (UINT64_MAX)
SPP_TREE_NO_SIZE = (1 << 64) - 1    # spp_merkle_tree_find_roots / spp_pool_root_sizes: no prefix of this tree has that root
SPP_AUDIT_RESIDENT = 0xFFFFFFFF     # spp_withdrawal_audit_plan / spp_prove_withdrawals: the pool holds this identity's audit record
SPP_WITHDRAWALS_MAX = 1 << 20       # ... keys / notes per call
SPP_ARITH_FR = 0x000               # spp_debug_arith: field bits of the selector (operation codes: csrc/arith_probe.hpp)
SPP_ARITH_FQ = 0x100
# the setup ceremony, spp_setup_contribute / spp_setup_verify_contribution (include/spp.h)
SPP_CONTRIB_RECEIPT_LEN = 160       # delta1_after | T | z
SPP_CONTRIB_OK = 0
SPP_CONTRIB_FORMAT = 1
SPP_CONTRIB_NOT_A_DELTA_CHANGE = 2
SPP_CONTRIB_POINT_INVALID = 3
SPP_CONTRIB_RECEIPT = 4
SPP_CONTRIB_DELTA_PAIR = 5
SPP_CONTRIB_SCALING = 6
SPP_CONTRIB_VK = 7
CONTRIB_REASON_NAMES = ("OK", "FORMAT", "NOT_A_DELTA_CHANGE", "POINT_INVALID", "RECEIPT", "DELTA_PAIR", "SCALING", "VK")
# sigma contributions, spp_setup_contribute_sigma / spp_setup_verify_sigma_contribution (include/spp.h); the receipt has the delta one's length
SPP_SIGMA_OK = 0
SPP_SIGMA_FORMAT = 1
SPP_SIGMA_NOT_A_SIGMA_CHANGE = 2
SPP_SIGMA_POINT_INVALID = 3
SPP_SIGMA_RECEIPT = 4
SPP_SIGMA_SCALING = 5
SPP_SIGMA_VK = 6
SIGMA_REASON_NAMES = ("OK", "FORMAT", "NOT_A_SIGMA_CHANGE", "POINT_INVALID", "RECEIPT", "SCALING", "VK")
# the powers-of-tau transcript, spp_ptau_contribute / spp_ptau_verify_contribution (include/spp.h)
SPP_PTAU_RECEIPT_LEN = 480          # three proofs of knowledge (t, a, b): base_after | T | z each
SPP_PTAU_OK = 0
SPP_PTAU_FORMAT = 1
SPP_PTAU_SIZE = 2
SPP_PTAU_POINT_INVALID = 3
SPP_PTAU_RECEIPT = 4
SPP_PTAU_TAU_G1 = 5
SPP_PTAU_TAU_G2 = 6
SPP_PTAU_ALPHA = 7
SPP_PTAU_BETA = 8
PTAU_REASON_NAMES = ("OK", "FORMAT", "SIZE", "POINT_INVALID", "RECEIPT", "TAU_G1", "TAU_G2", "ALPHA", "BETA")
POOL_RESULT_NAMES = ("OK", "AUDIT_EXISTS", "NO_AUDIT_RECORD", "BAD_ROOT", "NULLIFIER_USED", "BAD_RECIPIENT", "BAD_PROOF")


class SppError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libspp error %d: %s" % (code, msg))
        self.code = code


class WithdrawInputs(ctypes.Structure):
    _fields_ = [("root", ctypes.c_uint8 * 32), ("nullifier", ctypes.c_uint8 * 32), ("recipient", ctypes.c_uint8 * 32),
                ("amount", ctypes.c_uint64), ("wa_commitment", ctypes.c_uint8 * 32), ("secret_key", ctypes.c_uint8 * 32),
                ("owner_x", ctypes.c_uint8 * 32), ("owner_y", ctypes.c_uint8 * 32), ("randomness", ctypes.c_uint8 * 32),
                ("index", ctypes.c_uint64), ("siblings", (ctypes.c_uint8 * 32) * 16)]


def load_library():
    """Returns the loaded libspp.so; raises if it has not been built (no fallback path exists)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError("libspp.so not found at %s -- build it with __graft_entry__.build() "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
    # libspp keeps up to six batches in flight, each on a proving stream plus a side stream for the G2 sum: with the HIP
    # runtime's default of 4 hardware queues per device unrelated streams end up sharing a queue and run one after the other
    # (128-proof batches, four in flight: 3 755 proofs/s with 4 queues, 4 554 with 8).  Read when the runtime initialises.
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    L = ctypes.CDLL(LIB_PATH)
    vp, cp, u32, sz, i32 = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_int
    L.spp_last_error.restype = cp
    L.spp_version.restype = cp
    L.spp_circuit_build.argtypes = [i32, vp, cp, ctypes.POINTER(u32)]
    L.spp_circuit_build_acir.argtypes = [cp, sz, i32, cp, ctypes.POINTER(u32)]
    L.spp_init.argtypes = [i32, ctypes.POINTER(vp)]
    L.spp_free_ctx.argtypes = [vp]
    L.spp_free_ctx.restype = None
    L.spp_setup.argtypes = [vp, cp, cp, cp, cp]
    L.spp_load_circuit.argtypes = [vp, cp, cp, i32, ctypes.POINTER(vp)]
    L.spp_free_circuit.argtypes = [vp]
    L.spp_free_circuit.restype = None
    L.spp_circuit_info.argtypes = [vp, ctypes.POINTER(u32)]
    L.spp_circuit_msm_sizes.argtypes = [vp, ctypes.POINTER(u32)]
    L.spp_circuit_msm_windows.argtypes = [vp, ctypes.POINTER(u32)]
    L.spp_circuit_msm_table_rows.argtypes = [vp, ctypes.POINTER(u32)]
    L.spp_circuit_small_rows.argtypes = [vp, ctypes.POINTER(u32)]
    L.spp_circuit_plan_stats.argtypes = [vp, ctypes.POINTER(u32)]
    L.spp_pk_msm_sizes.argtypes = [cp, ctypes.POINTER(u32)]
    L.spp_plan_windows.argtypes = [u32, ctypes.POINTER(u32), ctypes.c_double, ctypes.POINTER(u32)]
    L.spp_load_circuit_with_windows.argtypes = [vp, cp, cp, ctypes.POINTER(u32), ctypes.POINTER(vp)]
    L.spp_circuit_table_bytes.argtypes = [vp]
    L.spp_circuit_table_bytes.restype = ctypes.c_uint64
    L.spp_prove_batch.argtypes = [vp, sz, cp, cp, vp, vp, vp]
    L.spp_prove_batch_device.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    L.spp_sync.argtypes = [vp]
    L.spp_last_timings.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    L.spp_timings.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_float)]
    L.spp_msm_kernel_ms.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_float)]
    L.spp_commitment_challenge.argtypes = [vp, ctypes.c_size_t, ctypes.c_char_p, vp]
    L.spp_set_serial.argtypes = [vp, i32]
    L.spp_prove_withdraw.argtypes = [vp, ctypes.POINTER(WithdrawInputs), cp, vp, vp]
    L.spp_verify.argtypes = [cp, sz, cp, sz, cp, sz, ctypes.POINTER(i32)]
    L.spp_verify_batch.argtypes = [vp, cp, sz, sz, cp, cp, sz, vp, ctypes.POINTER(ctypes.c_float)]
    L.spp_verify_batch_rlc.argtypes = [vp, cp, sz, sz, cp, cp, sz, cp, u32, u32, vp, ctypes.POINTER(u32), ctypes.POINTER(ctypes.c_float)]
    L.spp_pairing_check.argtypes = [vp, u32, cp, cp, ctypes.POINTER(i32)]
    L.spp_pairing_check_host.argtypes = [u32, cp, cp, ctypes.POINTER(i32)]
    L.spp_debug_witness.argtypes = [vp, vp, sz]
    L.spp_debug_arith.argtypes = [vp, u32, u32, sz, vp, sz, vp, sz]
    L.spp_rlwe_witness_batch.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.spp_rlwe_witness_batch_device.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.spp_ctx_sync.argtypes = [vp]
    L.spp_poseidon_hash_batch.argtypes = [vp, sz, i32, cp, vp]
    L.spp_merkle_root_batch.argtypes = [vp, sz, u32, cp, vp, cp, vp]
    L.spp_merkle_build.argtypes = [vp, sz, u32, cp, sz, vp, vp, vp]
    L.spp_merkle_tree_new.argtypes = [vp, u32, ctypes.POINTER(vp)]
    L.spp_merkle_tree_free.argtypes = [vp]
    L.spp_merkle_tree_free.restype = None
    L.spp_merkle_tree_size.argtypes = [vp]
    L.spp_merkle_tree_size.restype = ctypes.c_uint64
    L.spp_merkle_tree_insert.argtypes = [vp, sz, cp, ctypes.POINTER(ctypes.c_uint64)]
    L.spp_merkle_tree_root.argtypes = [vp, vp]
    L.spp_merkle_tree_proofs.argtypes = [vp, sz, vp, vp]
    L.spp_merkle_tree_deposit.argtypes = [vp, sz, cp, ctypes.POINTER(ctypes.c_uint64), vp, vp]
    L.spp_merkle_tree_find.argtypes = [vp, sz, cp, vp, vp, vp]
    L.spp_wallet_sync.argtypes = [vp, vp, sz, cp, cp, vp, vp, vp, vp]
    L.spp_grumpkin_keygen_batch.argtypes = [vp, sz, cp, vp]
    L.spp_poseidon2_sponge_batch.argtypes = [vp, sz, u32, cp, vp]
    L.spp_audit_inputs_batch.argtypes = [vp, vp, vp, sz, cp, vp, vp, vp, vp]
    L.spp_audit_inputs_batch_device.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp, vp]
    L.spp_prove_audit_from_secrets_device.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.spp_prove_audit_records_device.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.spp_prove_audit_records.argtypes = [vp, vp, vp, sz, cp, vp, vp, vp, cp, vp, vp, vp, vp, vp]
    L.spp_audit_open_batch.argtypes = [vp, cp, sz, vp, sz, cp, cp, vp, vp, vp, vp]
    L.spp_audit_open_batch_rlc.argtypes = [vp, cp, sz, vp, sz, cp, cp, vp, vp, u32, vp, vp, ctypes.POINTER(u32)]
    L.spp_pool_set_verifier.argtypes = [vp, i32, u32]
    L.spp_pool_verify_stats.argtypes = [vp, ctypes.POINTER(u32)]
    L.spp_pool_new.argtypes = [vp, cp, sz, cp, sz, ctypes.c_uint64, ctypes.POINTER(vp)]
    L.spp_pool_free.argtypes = [vp]
    L.spp_pool_free.restype = None
    L.spp_pool_add_roots.argtypes = [vp, sz, cp]
    L.spp_pool_state.argtypes = [vp, vp]
    L.spp_pool_counts.argtypes = [vp, vp]
    L.spp_pool_import_keys.argtypes = [vp, i32, sz, cp]
    L.spp_pool_contains.argtypes = [vp, i32, sz, cp, vp]
    L.spp_pool_submit_audit_batch.argtypes = [vp, sz, cp, cp, vp]
    L.spp_pool_withdraw_batch.argtypes = [vp, sz, cp, cp, cp, vp, vp]
    L.spp_pool_settle_log.argtypes = [vp, sz, cp, sz, cp, sz, cp, cp, sz, cp, cp, cp, vp, vp]
    L.spp_withdraw_rows_from_tree.argtypes = [vp, sz, cp, vp]
    L.spp_prove_withdraw_notes_device.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp]
    L.spp_prove_withdraw_notes.argtypes = [vp, vp, sz, cp, cp, vp, vp, vp]
    u64 = ctypes.c_uint64               # the tree as of an earlier size (include/spp.h)
    L.spp_merkle_tree_root_at.argtypes = [vp, u64, vp]
    L.spp_merkle_tree_proofs_at.argtypes = [vp, u64, sz, vp, vp]
    L.spp_merkle_tree_prefix_roots.argtypes = [vp, u64, sz, vp]
    L.spp_merkle_tree_find_roots.argtypes = [vp, sz, cp, vp, vp]
    L.spp_withdraw_rows_from_tree_at.argtypes = [vp, u64, sz, cp, vp]
    L.spp_prove_withdraw_notes_at_device.argtypes = [vp, vp, u64, sz, vp, vp, vp, vp, vp]
    L.spp_prove_withdraw_notes_at.argtypes = [vp, vp, u64, sz, cp, cp, vp, vp, vp]
    L.spp_pool_root_sizes.argtypes = [vp, vp, vp, ctypes.POINTER(u64)]
    # deposit proofs (include/spp.h)
    L.spp_deposit_rows_from_tree.argtypes = [vp, u64, sz, cp, vp]
    L.spp_prove_deposits_device.argtypes = [vp, vp, u64, sz, vp, vp, vp, vp, vp]
    L.spp_prove_deposits.argtypes = [vp, vp, u64, sz, cp, cp, vp, vp, vp]
    L.spp_verify_deposit_chain.argtypes = [vp, cp, sz, sz, cp, cp, vp, cp, u64, vp, vp, ctypes.POINTER(u64)]
    # withdrawals from notes: the audit plan, and both proofs in one call (include/spp.h)
    L.spp_withdrawal_audit_plan.argtypes = [vp, vp, sz, cp, vp, vp, ctypes.POINTER(u32)]
    L.spp_prove_withdrawals.argtypes = [vp, vp, vp, vp, u64, vp, vp, sz, cp, vp, vp, vp, cp, cp, vp, vp, vp, vp, vp, ctypes.POINTER(u32),
                                        sz, vp, vp, vp, vp, vp]
    L.spp_shamir_reconstruct.argtypes = [vp, u32, vp, cp, sz, vp, vp]
    L.spp_rlwe_decrypt_batch.argtypes = [vp, vp, sz, vp, vp, vp]
    L.spp_rlwe_sample_key.argtypes = [sz, u32, vp, vp, vp]
    L.spp_rlwe_keygen_batch.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    L.spp_rlwe_key_check.argtypes = [vp, sz, vp, vp, vp, vp]
    L.spp_shamir_split.argtypes = [vp, u32, u32, vp, sz, cp, cp, vp]
    # the auditors' key without a dealer (include/spp.h)
    L.spp_vss_generators.argtypes = [vp, vp]
    L.spp_dkg_a_from_seed.argtypes = [cp, vp]
    L.spp_vss_deal.argtypes = [vp, u32, u32, vp, sz, cp, cp, cp, cp, vp, vp, vp, vp]
    L.spp_vss_deal_timed.argtypes = [vp, u32, u32, vp, sz, cp, cp, cp, cp, vp, vp, vp, vp, ctypes.POINTER(ctypes.c_float)]
    L.spp_vss_receive.argtypes = [vp, u32, u32, u32, sz, cp, cp, cp, cp, cp, vp, vp, ctypes.POINTER(sz)]
    # the committee's commitments and verifiable resharing (include/spp.h)
    L.spp_vss_combine_commitments.argtypes = [vp, u32, u32, sz, cp, cp, cp, vp, vp, ctypes.POINTER(sz)]
    L.spp_vss_combine_commitments_timed.argtypes = [vp, u32, u32, sz, cp, cp, cp, vp, vp, ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_float)]
    L.spp_vss_share_commitments.argtypes = [vp, u32, sz, cp, u32, vp, vp]
    L.spp_vss_reshare_receive.argtypes = [vp, u32, vp, u32, u32, sz, cp, cp, cp, cp, vp, vp, vp, vp, ctypes.POINTER(sz)]
    # threshold opening (include/spp.h)
    L.spp_rlwe_sample_smudge.argtypes = [sz, u32, vp, vp]
    L.spp_rlwe_partial_decrypt_batch.argtypes = [vp, u32, vp, u32, cp, sz, vp, vp, vp, vp, cp, vp, vp]
    L.spp_rlwe_combine_partials.argtypes = [vp, u32, sz, cp, vp, vp, vp]
    L.spp_audit_open_batch_partials.argtypes = [vp, cp, sz, u32, cp, sz, cp, cp, vp, vp, vp, vp]
    L.spp_ntt_fr.argtypes = [vp, vp, u32, i32]
    L.spp_msm_g1.argtypes = [vp, cp, cp, sz, i32, vp]
    L.spp_msm_g2.argtypes = [vp, cp, cp, sz, i32, vp]
    L.spp_msm_flat_unit.argtypes = [vp, i32, cp, sz, cp, sz, i32, vp, ctypes.POINTER(ctypes.c_uint32)]
    L.spp_debug_msm_digits.argtypes = [vp, cp, sz, sz, vp, sz, i32, vp, sz, ctypes.POINTER(u32)]
    L.spp_msm_g1_pippenger.argtypes = [vp, cp, cp, sz, vp]
    L.spp_msm_g2_pippenger.argtypes = [vp, cp, cp, sz, vp]
    L.spp_g1_scale_points.argtypes = [vp, cp, sz, cp, vp]
    L.spp_g1_scale_points_timed.argtypes = [vp, cp, sz, cp, vp, ctypes.POINTER(ctypes.c_float), sz, ctypes.POINTER(ctypes.c_float)]
    L.spp_setup_contribute.argtypes = [vp, cp, cp, cp, cp, cp, vp]
    L.spp_setup_verify_contribution.argtypes = [vp, cp, cp, cp, cp, cp, ctypes.POINTER(i32), ctypes.POINTER(u32)]
    L.spp_setup_contribute_sigma.argtypes = [vp, cp, cp, cp, cp, cp, vp]
    L.spp_setup_verify_sigma_contribution.argtypes = [vp, cp, cp, cp, cp, cp, ctypes.POINTER(i32), ctypes.POINTER(u32)]
    L.spp_ptau_new.argtypes = [u32, cp]
    L.spp_ptau_contribute.argtypes = [vp, cp, cp, cp, vp]
    L.spp_ptau_verify_contribution.argtypes = [vp, cp, cp, cp, ctypes.POINTER(i32), ctypes.POINTER(u32)]
    L.spp_g1_mul_each.argtypes = [vp, cp, sz, cp, vp]
    L.spp_g2_mul_each.argtypes = [vp, cp, sz, cp, vp]
    L.spp_setup_from_ptau.argtypes = [vp, cp, cp, cp, cp]
    L.spp_ec_intt_g1.argtypes = [vp, cp, u32, vp]
    L.spp_ec_intt_g2.argtypes = [vp, cp, u32, vp]
    L.spp_ec_intt_timed.argtypes = [vp, i32, cp, u32, vp, ctypes.POINTER(ctypes.c_float), sz, ctypes.POINTER(ctypes.c_float)]
    L.spp_msm_g1_pippenger_bench.argtypes = [vp, sz, ctypes.c_uint64, cp, i32, vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    L.spp_msm_g1_pippenger_bench_dist.argtypes = [vp, sz, ctypes.c_uint64, ctypes.c_uint32, cp, i32, vp, ctypes.POINTER(ctypes.c_float),
                                                  ctypes.POINTER(ctypes.c_float)]
    L.spp_msm_g1_pippenger_bench_shard.argtypes = [vp, sz, sz, sz, ctypes.c_uint64, ctypes.c_uint32, cp, i32, vp, ctypes.POINTER(ctypes.c_float),
                                                   ctypes.POINTER(ctypes.c_float)]
    _LIB = L
    return L


def last_error():
    return load_library().spp_last_error().decode()


def check(rc):
    if rc != 0:
        raise SppError(rc, last_error())
