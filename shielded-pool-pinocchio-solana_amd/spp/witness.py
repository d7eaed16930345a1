"""Host-side mirrors of the reference's client-side witness-input code, executed by the HIP kernels.

    rlwe_witness(...)        scripts/generate_audit.py:507-584  /  demo-frontend/app/lib/rlwe.ts:157-247
    poseidon_hash2/4(...)    client/merkle.ts:22-38
    ShieldedPoolMerkleTree   client/merkle.ts:146-222
    Pool                     shielded_pool_program/src/state.rs, instructions/submit_audit.rs, instructions/withdraw.rs: the
                             pool program's state and its decisions for a batch of instructions (spp_pool_*)
    identity_public_key(...) client/merkle.ts:98-113
    pack_withdraw_notes(...) the five values a withdrawer supplies (noir_circuit/src/main.nr:38-51), for the rows / proofs
                             from notes against the resident tree (ShieldedPoolMerkleTree.withdraw_rows)
    pack_deposits(...)       the three values a depositor supplies, for ShieldedPoolMerkleTree.deposit
    ShieldedPoolMerkleTree.find / .sync
                             demo-frontend/app/lib/storage.ts:9-26,45-50,233-260: the leafIndex, nullifier, waCommitment and
                             status a wallet keeps per deposit, recomputed from its secrets, the tree and the pool's accounts
    ShieldedPoolMerkleTree.root_at / .proofs_at / .prefix_roots / .find_roots / .withdraw_rows(size=), Pool.root_sizes
                             the tree of the first `size` leaves: the root a deposit pushed (client/payroll-demo.ts:285-292,
                             instructions/deposit.rs:31-36,73), and which size a pool still accepts (demo-frontend/app/lib/
                             on-chain.ts:93-125,202-235)
    deposit_instruction_data shielded_pool_program/src/instructions/deposit.rs:21-37
    ct_commitment(...)       ct_helper/src/main.nr:15-34
    ciphertext_json(...)     scripts/generate_audit.py:590-606 (keys/ciphertext.json, what the prover leaves for the auditor)
    load_share_json(...)     scripts/rlwe_keygen.py:157-171 (keys/rlwe_sk_shares/share_<i>.json)
    rlwe_sample_key / rlwe_keygen / rlwe_key_check / shamir_split
                             scripts/rlwe_keygen.py:98-116 (the audit key pair) and :51-65 (shamir_share_field)
    vss_generators / dkg_a_from_seed / vss_deal / vss_receive
                             scripts/rlwe_keygen.py:51-65, 98-182 by the auditors together: every auditor deals its own part of
                             the key with public commitments, nobody draws the whole (no counterpart in the reference)
    vss_combine_commitments / vss_share_commitments / vss_reshare_receive
                             the committee's commitments and handing the key to a new committee (no counterpart either)
    write_rlwe_pk_json / write_rlwe_params_json / write_share_json
                             scripts/rlwe_keygen.py:124-127, 133-142, 161-169: the files `cli compile --rlwe-pk` and
                             load_share_json read
    rlwe_sample_smudge / rlwe_partial_decrypt / rlwe_combine_partials, new_pair_seeds, partial_json / load_partial_json
                             no counterpart in the reference, which rebuilds the key (scripts/rlwe_decrypt.py:61-91): t of m
                             auditors open a ciphertext from partial decryptions of their own shares (include/spp.h)
All of them take and return Python ints / lists; field elements cross the C ABI as 32-byte big-endian.
"""
import ctypes
import numpy as np
from .lib import (check, NOTE_LEN, DEPOSIT_LEN, PROOF_LEN, AUDIT_PW_LEN, WITHDRAW_PW_LEN, SPP_POOL_STATE_LEN,
                  SPP_POOL_NULLIFIERS, SPP_POOL_AUDIT_RECORDS, SPP_INSTR_DEPOSIT, SPP_INSTR_SUBMIT_AUDIT, SPP_INSTR_WITHDRAW,
                  SPP_POOL_VERIFY_EACH, SPP_POOL_VERIFY_RLC, SPP_WALLET_RECORD_LEN, SPP_TREE_SIZE_NOW, SPP_TREE_NO_SIZE)

TREE_DEPTH = 16
FR_MODULUS = 21888242871839275222246405745257275088548364400416034343698204186575808495617
NOTE_FIELDS = ("recipient", "amount", "secret_key", "randomness", "index")
DEPOSIT_FIELDS = ("secret_key", "amount", "randomness")
WALLET_ABSENT = (1 << 64) - 1       # spp_merkle_tree_find / spp_wallet_sync: no such leaf (UINT64_MAX)
RLWE_N, MSG_SLOTS = 1024, 64


def _be(vals):
    return b"".join(int(v).to_bytes(32, "big") for v in vals)


def _unbe(buf, n):
    return [int.from_bytes(buf[32 * i:32 * i + 32], "big") for i in range(n)]


def rlwe_witness(ctx, pk_a, pk_b, r, e1, e2, msg):
    """Batch form: r, e2 arrays [count,1024]; e1, msg [count,64]. Returns dict of numpy arrays + packed fields."""
    r = np.ascontiguousarray(r, dtype=np.int8).reshape(-1, RLWE_N)
    count = r.shape[0]
    e1 = np.ascontiguousarray(e1, dtype=np.int8).reshape(count, MSG_SLOTS)
    e2 = np.ascontiguousarray(e2, dtype=np.int8).reshape(count, RLWE_N)
    msg = np.ascontiguousarray(msg, dtype=np.uint8).reshape(count, MSG_SLOTS)
    a = np.ascontiguousarray(pk_a, dtype=np.uint32)
    b = np.ascontiguousarray(pk_b, dtype=np.uint32)
    c0 = np.zeros((count, MSG_SLOTS), dtype=np.uint32)
    c1 = np.zeros((count, RLWE_N), dtype=np.uint32)
    k0 = np.zeros((count, MSG_SLOTS), dtype=np.int32)
    k1 = np.zeros((count, RLWE_N), dtype=np.int32)
    packed = np.zeros((count, 157, 32), dtype=np.uint8)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    check(ctx.L.spp_rlwe_witness_batch(ctx.h, p(a), p(b), count, p(r), p(e1), p(e2), p(msg), p(c0), p(c1), p(k0), p(k1), p(packed)))
    pk = [[int.from_bytes(packed[i, f].tobytes(), "big") for f in range(157)] for i in range(count)]
    return dict(c0=c0, c1=c1, k0=k0, k1=k1, c0_packed=[x[:10] for x in pk], c1_packed=[x[10:] for x in pk])


def poseidon_hash_batch(ctx, rows):
    """rows: list of [a, b] or [a, b, c, d] -> list of hashes."""
    if not rows:
        return []
    arity = len(rows[0])
    out = ctypes.create_string_buffer(32 * len(rows))
    check(ctx.L.spp_poseidon_hash_batch(ctx.h, len(rows), arity, _be(v for r in rows for v in r), ctypes.cast(out, ctypes.c_void_p)))
    return _unbe(out.raw, len(rows))


def poseidon_hash2(ctx, a, b):
    return poseidon_hash_batch(ctx, [[a, b]])[0]


def poseidon_hash4(ctx, a, b, c, d):
    return poseidon_hash_batch(ctx, [[a, b, c, d]])[0]


def pack_withdraw_notes(notes):
    """notes: (recipient, amount, secret_key, randomness, index) tuples -> NOTE_LEN bytes per note, 32-byte big-endian fields in
    that order (spp_withdraw_rows_from_tree / spp_prove_withdraw_notes).  Host only; raises ValueError on a tuple of another
    length or a value outside [0, r)."""
    out = bytearray()
    for k, note in enumerate(notes):
        if len(note) != len(NOTE_FIELDS):
            raise ValueError("note %d: expected %d values %s, got %d" % (k, len(NOTE_FIELDS), NOTE_FIELDS, len(note)))
        for name, v in zip(NOTE_FIELDS, note):
            v = int(v)
            if not 0 <= v < FR_MODULUS:
                raise ValueError("note %d: %s is not a canonical field element" % (k, name))
            out += v.to_bytes(32, "big")
    assert len(out) == NOTE_LEN * len(notes)
    return bytes(out)


def pack_deposits(deposits):
    """deposits: (secret_key, amount, randomness) tuples -> DEPOSIT_LEN bytes per deposit, 32-byte big-endian fields in that order
    (spp_merkle_tree_deposit).  Host only; raises ValueError on a tuple of another length or a value outside [0, 2^256).  The
    library refuses the rest (a field >= r, amount >= 2^64, secret_key == 0) and names the deposit."""
    out = bytearray()
    for k, dep in enumerate(deposits):
        if len(dep) != len(DEPOSIT_FIELDS):
            raise ValueError("deposit %d: expected %d values %s, got %d" % (k, len(DEPOSIT_FIELDS), DEPOSIT_FIELDS, len(dep)))
        for name, v in zip(DEPOSIT_FIELDS, dep):
            v = int(v)
            if not 0 <= v < 1 << 256:
                raise ValueError("deposit %d: %s does not fit 32 bytes" % (k, name))
            out += v.to_bytes(32, "big")
    assert len(out) == DEPOSIT_LEN * len(deposits)
    return bytes(out)


def deposit_instruction_data(amount, commitment, root):
    """The 72-byte body of the pool program's deposit instruction (shielded_pool_program/src/instructions/deposit.rs:21-37):
    amount u64 little-endian | commitment 32 B big-endian | new root 32 B big-endian.  The 1-byte instruction tag in front of it
    is the caller's (client/payroll-demo.ts:288-292)."""
    amount, commitment, root = int(amount), int(commitment), int(root)
    if not 0 <= amount < 1 << 64:
        raise ValueError("amount does not fit a u64")
    for name, v in (("commitment", commitment), ("root", root)):
        if not 0 <= v < FR_MODULUS:
            raise ValueError("%s is not a canonical field element" % name)
    return amount.to_bytes(8, "little") + commitment.to_bytes(32, "big") + root.to_bytes(32, "big")


def merkle_roots(ctx, leaves, indices, siblings, depth=TREE_DEPTH):
    count = len(leaves)
    idx = (ctypes.c_uint64 * count)(*[int(i) for i in indices])
    out = ctypes.create_string_buffer(32 * count)
    check(ctx.L.spp_merkle_root_batch(ctx.h, count, depth, _be(leaves), ctypes.cast(idx, ctypes.c_void_p),
                                      _be(s for row in siblings for s in row), ctypes.cast(out, ctypes.c_void_p)))
    return _unbe(out.raw, count)


class ShieldedPoolMerkleTree:
    """client/merkle.ts:146-222 with the tree RESIDENT in HBM and maintained incrementally (spp_merkle_tree_*): insert() is
    O(depth) hashes, getRoot() one read, getProof() `depth` reads -- the reference recomputes up to 2^16 hashes in every
    getRoot / getProof call (merkle.ts:165-176, 198-221)."""

    def __init__(self, ctx, depth=TREE_DEPTH):
        self.ctx, self.depth = ctx, depth
        h = ctypes.c_void_p()
        check(ctx.L.spp_merkle_tree_new(ctx.h, depth, ctypes.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.ctx.L.spp_merkle_tree_free(self.h)
            self.h = None

    # the levels live in HBM: release them when the object goes away (context manager or garbage collection), not only on close()
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:   # interpreter shutdown: the library may already be gone
            pass

    def __len__(self):
        return int(self.ctx.L.spp_merkle_tree_size(self.h))

    def insert(self, commitment):
        return self.insert_many([commitment])

    def insert_many(self, commitments):
        """appends the leaves in order; returns the index of the first one"""
        first = ctypes.c_uint64(0)
        check(self.ctx.L.spp_merkle_tree_insert(self.h, len(commitments), _be(commitments), ctypes.byref(first)))
        return int(first.value)

    def getRoot(self):
        root = ctypes.create_string_buffer(32)
        check(self.ctx.L.spp_merkle_tree_root(self.h, ctypes.cast(root, ctypes.c_void_p)))
        return int.from_bytes(root.raw, "big")

    def getProofs(self, indices, raw=False):
        nq = len(indices)
        q = (ctypes.c_uint64 * max(nq, 1))(*[int(i) for i in indices])
        sib = ctypes.create_string_buffer(32 * self.depth * max(nq, 1))
        check(self.ctx.L.spp_merkle_tree_proofs(self.h, nq, ctypes.cast(q, ctypes.c_void_p), ctypes.cast(sib, ctypes.c_void_p)))
        if raw:
            return sib.raw[:32 * self.depth * nq]
        return [_unbe(sib.raw[32 * self.depth * i:], self.depth) for i in range(nq)]

    def getProof(self, index):
        return self.getProofs([index])[0]

    def deposit(self, deposits):
        """generateIdentityKeypair, calculateCommitment, insert and getRoot for every deposit (client/payroll-demo.ts:264-292) in
        one call on the device (spp_merkle_tree_deposit).  deposits: (secret_key, amount, randomness) tuples.  Returns
        (first_index, commitments, roots): deposit k is leaf first_index + k and roots[k] is the root right after it, the new_root
        of its deposit instruction (deposit_instruction_data)."""
        n = len(deposits)
        buf = pack_deposits(deposits)
        first = ctypes.c_uint64(0)
        com = ctypes.create_string_buffer(32 * max(n, 1))
        roots = ctypes.create_string_buffer(32 * max(n, 1))
        check(self.ctx.L.spp_merkle_tree_deposit(self.h, n, buf, ctypes.byref(first), ctypes.cast(com, ctypes.c_void_p),
                                                 ctypes.cast(roots, ctypes.c_void_p)))
        return int(first.value), _unbe(com.raw, n), _unbe(roots.raw, n)

    def withdraw_rows(self, notes, size=None):
        """Withdraw input rows for notes (pack_withdraw_notes) against the tree as it stands (spp_withdraw_rows_from_tree):
        per note [root, nullifier, recipient, amount, wa_commitment, secret_key, owner_x, owner_y, randomness, index,
        *siblings] -- what client/payroll-demo.ts:323-340 assembles for generateProof, computed on the device.
        size: against the tree of the first `size` leaves instead (spp_withdraw_rows_from_tree_at)."""
        buf = pack_withdraw_notes(notes)
        n_in = 10 + self.depth
        rows = ctypes.create_string_buffer(32 * n_in * max(len(notes), 1))
        if size is None:
            check(self.ctx.L.spp_withdraw_rows_from_tree(self.h, len(notes), buf, ctypes.cast(rows, ctypes.c_void_p)))
        else:
            check(self.ctx.L.spp_withdraw_rows_from_tree_at(self.h, int(size), len(notes), buf, ctypes.cast(rows, ctypes.c_void_p)))
        return [_unbe(rows.raw[32 * n_in * i:], n_in) for i in range(len(notes))]

    # ---- deposit proofs (include/spp.h): the reference's program checks nothing about a deposit
    # (shielded_pool_program/src/instructions/deposit.rs:31-36,73) and does not verify these proofs; a program that does, an indexer or
    # an auditor can ----
    def deposit_rows(self, first_index, deposits):
        """Rows of the deposit circuit for leaves first_index .. first_index + len(deposits) - 1, which the tree must already hold
        (spp_deposit_rows_from_tree): per deposit [old_root, new_root, commitment, amount, index, owner_x, owner_y, randomness,
        *siblings], the commitment computed from the record.  A record that is not the deposit at that index still gives a
        self-consistent row; its new_root is then not the tree's (verify_deposit_chain is what binds a log to one tree)."""
        buf = pack_deposits(deposits)
        n_in = 8 + self.depth
        rows = ctypes.create_string_buffer(32 * n_in * max(len(deposits), 1))
        check(self.ctx.L.spp_deposit_rows_from_tree(self.h, int(first_index), len(deposits), buf, ctypes.cast(rows, ctypes.c_void_p)))
        return [_unbe(rows.raw[32 * n_in * i:], n_in) for i in range(len(deposits))]

    def deposit_proved(self, handle, deposits, rs=None):
        """deposit(), then the proof of every one of those deposits with the deposit circuit `handle` (CircuitHandle.prove_deposits).
        Returns (first, commitments, roots, proofs, pws, status)."""
        first, commitments, roots = self.deposit(deposits)
        proofs, pws, status = handle.prove_deposits(self, first, deposits, rs)
        return first, commitments, roots, proofs, pws, status

    # ---- the tree as of an earlier size (include/spp.h): the root a deposit pushed is the root of the leaves its client knew,
    # client/payroll-demo.ts:285-292, and the program takes it as sent, shielded_pool_program/src/instructions/deposit.rs:31-36,73.
    # size: 0 .. len(self), or SPP_TREE_SIZE_NOW ----
    def root_at(self, size):
        """getRoot of the first `size` leaves (spp_merkle_tree_root_at)"""
        root = ctypes.create_string_buffer(32)
        check(self.ctx.L.spp_merkle_tree_root_at(self.h, int(size), ctypes.cast(root, ctypes.c_void_p)))
        return int.from_bytes(root.raw, "big")

    def proofs_at(self, size, indices, raw=False):
        """getProofs in the tree of the first `size` leaves (spp_merkle_tree_proofs_at)"""
        nq = len(indices)
        q = (ctypes.c_uint64 * max(nq, 1))(*[int(i) for i in indices])
        sib = ctypes.create_string_buffer(32 * self.depth * max(nq, 1))
        check(self.ctx.L.spp_merkle_tree_proofs_at(self.h, int(size), nq, ctypes.cast(q, ctypes.c_void_p), ctypes.cast(sib, ctypes.c_void_p)))
        if raw:
            return sib.raw[:32 * self.depth * nq]
        return [_unbe(sib.raw[32 * self.depth * i:], self.depth) for i in range(nq)]

    def prefix_roots(self, first_size=0, count=None):
        """the roots of sizes first_size .. first_size + count - 1 (count None: up to the tree's size): spp_merkle_tree_prefix_roots"""
        if count is None:
            count = len(self) + 1 - int(first_size)
        out = ctypes.create_string_buffer(32 * max(count, 1))
        check(self.ctx.L.spp_merkle_tree_prefix_roots(self.h, int(first_size), count, ctypes.cast(out, ctypes.c_void_p)))
        return _unbe(out.raw, count)

    def find_roots(self, roots):
        """From root words back to sizes (spp_merkle_tree_find_roots).  roots: ints below 2^256 or 32-byte strings, any bytes -- a
        word that is no field element matches nothing.  Returns (sizes, matches): the lowest size with that root or None, and how
        many sizes have it (more than one only after zero-valued leaves)."""
        buf = _key_bytes(roots)
        n = len(buf) // 32
        sizes = (ctypes.c_uint64 * max(n, 1))()
        matches = (ctypes.c_uint32 * max(n, 1))()
        check(self.ctx.L.spp_merkle_tree_find_roots(self.h, n, buf, ctypes.cast(sizes, ctypes.c_void_p), ctypes.cast(matches, ctypes.c_void_p)))
        return [None if v == SPP_TREE_NO_SIZE else int(v) for v in sizes[:n]], [int(m) for m in matches[:n]]

    def find(self, leaves, start=None):
        """From leaf values back to positions (spp_merkle_tree_find; MerkleTreeState.leaves.indexOf, demo-frontend/app/lib/
        storage.ts:45-50).  leaves: ints; start: per value the index to search from (None = 0 for all).  Returns (indices,
        matches): the lowest leaf index >= start[i] holding leaves[i] or None, and how many leaves hold it in the whole tree.
        A value at several leaves is enumerated by calling again with start = index + 1."""
        n = len(leaves)
        if start is not None and len(start) != n:
            raise ValueError("start must name one index per leaf value")
        frm = None if start is None else (ctypes.c_uint64 * max(n, 1))(*[int(v) for v in start])
        idx = (ctypes.c_uint64 * max(n, 1))()
        matches = (ctypes.c_uint32 * max(n, 1))()
        check(self.ctx.L.spp_merkle_tree_find(self.h, n, _be(leaves), None if frm is None else ctypes.cast(frm, ctypes.c_void_p),
                                              ctypes.cast(idx, ctypes.c_void_p), ctypes.cast(matches, ctypes.c_void_p)))
        return [None if v == WALLET_ABSENT else int(v) for v in idx[:n]], [int(m) for m in matches[:n]]

    def sync(self, deposits, pool=None, recipients=None):
        """The DepositRecord of every secret (demo-frontend/app/lib/storage.ts:9-26) recomputed on the device (spp_wallet_sync).
        deposits: (secret_key, amount, randomness) tuples as for deposit(); pool: a Pool of the same Context, whose nullifier and
        audit-record sets decide SPP_WALLET_SPENT / SPP_WALLET_AUDITED; recipients: one recipient word per secret.
        Returns per secret (index or None, flags, commitment, nullifier, wa_commitment, (owner_x, owner_y)): with a pool the
        lowest occurrence whose nullifier is unspent (the lowest one, flagged SPENT, when all are), without one the lowest.
        With recipients returns (records, notes), notes being (recipient, amount, secret_key, randomness, index) tuples ready for
        CircuitHandle.prove_withdraw_notes; a secret whose commitment is no leaf gets index 2^depth, which the circuit refuses."""
        n = len(deposits)
        if recipients is not None and len(recipients) != n:
            raise ValueError("recipients must name one recipient word per secret")
        buf = pack_deposits(deposits)
        rcp = None if recipients is None else _be(recipients)
        idx = (ctypes.c_uint64 * max(n, 1))()
        flags = (ctypes.c_uint32 * max(n, 1))()
        rec = ctypes.create_string_buffer(SPP_WALLET_RECORD_LEN * max(n, 1))
        notes = None if recipients is None else ctypes.create_string_buffer(NOTE_LEN * max(n, 1))
        check(self.ctx.L.spp_wallet_sync(self.h, None if pool is None else pool.h, n, buf, rcp, ctypes.cast(idx, ctypes.c_void_p),
                                         ctypes.cast(flags, ctypes.c_void_p), ctypes.cast(rec, ctypes.c_void_p),
                                         None if notes is None else ctypes.cast(notes, ctypes.c_void_p)))
        out = []
        for i in range(n):
            com, nf, wa, ox, oy = _unbe(rec.raw[SPP_WALLET_RECORD_LEN * i:], 5)
            out.append((None if idx[i] == WALLET_ABSENT else int(idx[i]), int(flags[i]), com, nf, wa, (ox, oy)))
        if notes is None:
            return out
        return out, [tuple(_unbe(notes.raw[NOTE_LEN * i:], 5)) for i in range(n)]


def _joined(items, each, what):
    """a list of byte strings (or one bytes object) as one buffer of len(items) * each bytes"""
    buf = bytes(items) if isinstance(items, (bytes, bytearray)) else b"".join(bytes(x) for x in items)
    if len(buf) % each:
        raise ValueError("%s: %d bytes each" % (what, each))
    return buf


def _key_bytes(keys):
    return b"".join(int(k).to_bytes(32, "big") if isinstance(k, int) else bytes(k) for k in keys)


def recipient_word(address):
    """The recipient public input the pool program expects for a 32-byte account address: 00 00 | address[0..30]
    (shielded_pool_program/src/instructions/withdraw.rs:150-154), as an integer."""
    address = bytes(address)
    if len(address) != 32:
        raise ValueError("an account address is 32 bytes")
    return int.from_bytes(address[:30], "big")


class Pool:
    """The pool program's state on the device (spp_pool_*): ShieldedPoolState's root ring (state.rs:6-46) and the sets of spent
    nullifiers and audit records, with the decisions process_submit_audit / process_withdraw make for a batch of instructions
    taken in order.  A pre-screen for a relayer (which of these transactions would land?) and a replay tool for an auditor; the
    vault balance and lamport transfers are not modelled -- withdraw() returns the amounts for that.
    withdraw_vk / audit_vk: the two verifying keys (bytes); capacity: keys per set, fixed.  Keys (nullifiers, wa_commitments)
    are ints or 32-byte strings; results are SPP_POOL_* codes (spp.lib.POOL_RESULT_NAMES).
    verifier: "each" (one lane per proof, the default) or "rlc" (random linear combination over the proofs the screen leaves, in
    groups of `group`, 0 = 256; spp_pool_set_verifier): the same decisions except with probability about 2^-127 per launch."""

    _VERIFIERS = {"each": SPP_POOL_VERIFY_EACH, "rlc": SPP_POOL_VERIFY_RLC}

    def __init__(self, ctx, withdraw_vk, audit_vk, capacity, verifier="each", group=0):
        if verifier not in self._VERIFIERS:
            raise ValueError("verifier: \"each\" or \"rlc\"")
        self.ctx, self.capacity = ctx, int(capacity)
        h = ctypes.c_void_p()
        check(ctx.L.spp_pool_new(ctx.h, withdraw_vk, len(withdraw_vk), audit_vk, len(audit_vk), self.capacity, ctypes.byref(h)))
        self.h = h
        if verifier != "each" or group:
            try:
                self.set_verifier(verifier, group)
            except Exception:
                self.close()
                raise

    def set_verifier(self, verifier, group=0):
        """the verifier of the settling calls from now on: "each" or "rlc"; group: a multiple of 64 in [64, 4096], 0 = 256"""
        if verifier not in self._VERIFIERS:
            raise ValueError("verifier: \"each\" or \"rlc\"")
        check(self.ctx.L.spp_pool_set_verifier(self.h, self._VERIFIERS[verifier], int(group)))

    def verify_stats(self):
        """(withdraw4, audit4) of the last settling call: (groups, groups refused, proofs re-verified, proofs dropped) of the
        verifier under each key; all zero after a call with the "each" verifier"""
        s = (ctypes.c_uint32 * 8)()
        check(self.ctx.L.spp_pool_verify_stats(self.h, s))
        return tuple(int(v) for v in s[:4]), tuple(int(v) for v in s[4:])

    def close(self):
        if getattr(self, "h", None):
            self.ctx.L.spp_pool_free(self.h)
            self.h = None

    # the sets live in HBM: release them when the object goes away (context manager or garbage collection), not only on close()
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:   # interpreter shutdown: the library may already be gone
            pass

    def add_roots(self, roots):
        """state.add_root for every deposit in order; roots: ints (ShieldedPoolMerkleTree.deposit's third result) or bytes"""
        buf = _key_bytes(roots)
        check(self.ctx.L.spp_pool_add_roots(self.h, len(buf) // 32, buf))

    def state(self):
        """the 1072 bytes of the ShieldedPoolState account"""
        out = ctypes.create_string_buffer(SPP_POOL_STATE_LEN)
        check(self.ctx.L.spp_pool_state(self.h, ctypes.cast(out, ctypes.c_void_p)))
        return out.raw

    def root_sizes(self, tree):
        """Which size of `tree` (a ShieldedPoolMerkleTree of the same Context) can a proof be made against so that this pool accepts
        it (spp_pool_root_sizes; isRootValid / getRootAge, demo-frontend/app/lib/on-chain.ts:93-125,202-235).  Returns (sizes, best):
        sizes[0] for current_root and sizes[1 + k] for roots[k] of the state, None where the word is no prefix root of the tree;
        best = the largest, or None."""
        sizes = (ctypes.c_uint64 * 33)()
        best = ctypes.c_uint64(0)
        check(self.ctx.L.spp_pool_root_sizes(self.h, tree.h, ctypes.cast(sizes, ctypes.c_void_p), ctypes.byref(best)))
        none = lambda v: None if v == SPP_TREE_NO_SIZE else int(v)
        return [none(v) for v in sizes], none(best.value)

    def counts(self):
        """(spent nullifiers, audit records)"""
        c = (ctypes.c_uint64 * 2)()
        check(self.ctx.L.spp_pool_counts(self.h, ctypes.cast(c, ctypes.c_void_p)))
        return int(c[0]), int(c[1])

    def import_keys(self, which, keys):
        """accounts known from elsewhere; which: SPP_POOL_NULLIFIERS or SPP_POOL_AUDIT_RECORDS; duplicates are ignored"""
        buf = _key_bytes(keys)
        check(self.ctx.L.spp_pool_import_keys(self.h, int(which), len(buf) // 32, buf))

    def contains(self, which, keys):
        buf = _key_bytes(keys)
        n = len(buf) // 32
        out = ctypes.create_string_buffer(max(n, 1))
        check(self.ctx.L.spp_pool_contains(self.h, int(which), n, buf, ctypes.cast(out, ctypes.c_void_p)))
        return [bool(b) for b in out.raw[:n]]

    def submit_audit(self, proofs, pws):
        """process_submit_audit for the instructions in order: proofs / pws lists of bytes (388 / 76 each).  Returns the codes."""
        pb, wb = _joined(proofs, PROOF_LEN, "proofs"), _joined(pws, AUDIT_PW_LEN, "audit public witnesses")
        n = len(pb) // PROOF_LEN
        if len(wb) != AUDIT_PW_LEN * n:
            raise ValueError("submit_audit: %d proofs need %d public witnesses of %d bytes" % (n, n, AUDIT_PW_LEN))
        res = (ctypes.c_int32 * max(n, 1))()
        check(self.ctx.L.spp_pool_submit_audit_batch(self.h, n, pb, wb, ctypes.cast(res, ctypes.c_void_p)))
        return list(res)[:n]

    def withdraw(self, proofs, pws, recipients):
        """process_withdraw for the instructions in order: proofs / pws lists of bytes (388 / 172 each), recipients the 32-byte
        addresses of the recipient accounts.  Returns (codes, amounts)."""
        pb, wb = _joined(proofs, PROOF_LEN, "proofs"), _joined(pws, WITHDRAW_PW_LEN, "withdraw public witnesses")
        rb = _joined(recipients, 32, "recipient addresses")
        n = len(pb) // PROOF_LEN
        if len(wb) != WITHDRAW_PW_LEN * n or len(rb) != 32 * n:
            raise ValueError("withdraw: %d proofs need %d public witnesses of %d bytes and %d addresses of 32" % (n, n, WITHDRAW_PW_LEN, n))
        res = (ctypes.c_int32 * max(n, 1))()
        amounts = (ctypes.c_uint64 * max(n, 1))()
        check(self.ctx.L.spp_pool_withdraw_batch(self.h, n, pb, wb, rb, ctypes.cast(res, ctypes.c_void_p), ctypes.cast(amounts, ctypes.c_void_p)))
        return list(res)[:n], [int(a) for a in amounts][:n]

    _LOG_KINDS = {"deposit": (SPP_INSTR_DEPOSIT, 1), "submit_audit": (SPP_INSTR_SUBMIT_AUDIT, 2), "withdraw": (SPP_INSTR_WITHDRAW, 3)}

    def settle_log(self, instructions):
        """A log in which the kinds alternate, as the chain's does, in ONE call (spp_pool_settle_log): instructions is a sequence of
        ("deposit", root), ("submit_audit", proof, pw) and ("withdraw", proof, pw, address) in the order the program processed
        them; a withdraw meets the ring and the audit records as of its position.  Returns (codes, amounts) in log order; a deposit
        gives SPP_POOL_OK, amounts are 0 except for withdraws."""
        kinds, cols = bytearray(), ([], [], [], [], [], [])          # roots | audit proofs, pws | withdraw proofs, pws, addresses
        for no, ins in enumerate(instructions):
            kind, fields = self._LOG_KINDS.get(ins[0], (None, 0))
            if kind is None or len(ins) != 1 + fields:
                raise ValueError("instruction %d: (\"deposit\", root), (\"submit_audit\", proof, pw) or (\"withdraw\", proof, pw, address)" % no)
            kinds.append(kind)
            first = (0, 1, 3)[kind]
            for k, v in enumerate(ins[1:]):
                cols[first + k].append(v)
        roots = _key_bytes(cols[0])
        ap, aw = _joined(cols[1], PROOF_LEN, "proofs"), _joined(cols[2], AUDIT_PW_LEN, "audit public witnesses")
        wp, ww = _joined(cols[3], PROOF_LEN, "proofs"), _joined(cols[4], WITHDRAW_PW_LEN, "withdraw public witnesses")
        rb = _joined(cols[5], 32, "recipient addresses")
        nd, na, nw = len(cols[0]), len(cols[1]), len(cols[3])
        if len(roots) != 32 * nd or len(ap) != PROOF_LEN * na or len(aw) != AUDIT_PW_LEN * na or len(wp) != PROOF_LEN * nw or \
                len(ww) != WITHDRAW_PW_LEN * nw or len(rb) != 32 * nw:
            raise ValueError("settle_log: roots and addresses of 32 bytes, proofs of %d, public witnesses of %d (submit_audit) and %d (withdraw)"
                             % (PROOF_LEN, AUDIT_PW_LEN, WITHDRAW_PW_LEN))
        n = len(kinds)
        res = (ctypes.c_int32 * max(n, 1))()
        amounts = (ctypes.c_uint64 * max(n, 1))()
        check(self.ctx.L.spp_pool_settle_log(self.h, n, bytes(kinds), nd, roots, na, ap, aw, nw, wp, ww, rb, ctypes.cast(res, ctypes.c_void_p),
                                             ctypes.cast(amounts, ctypes.c_void_p)))
        return list(res)[:n], [int(a) for a in amounts][:n]


def verify_deposit_chain(ctx, vk, proofs, pws, start_root, start_index, lamports=None):
    """A log of proved deposits checked as a program that keeps (current_root, leaf count) would (spp_verify_deposit_chain): every
    proof through the batch verifier, then one after another -- the pw amount against lamports[i] (when given), old_root against the
    current root, index against the count, the proof.  An accepted deposit moves the state to (its new_root, index + 1), a rejected
    one moves nothing.  proofs, pws: lists of bytes (or one buffer each); start_root: int or 32 bytes.  Returns (codes, end_root int, end_index); codes
    index lib.DEPOSIT_RESULT_NAMES.  No Pool is touched: feed the accepted new_roots to Pool.add_roots."""
    from .lib import DEPOSIT_PW_LEN, PROOF_LEN
    pb = _joined(proofs, PROOF_LEN, "proof")
    wb = _joined(pws, DEPOSIT_PW_LEN, "public witness")
    n = len(pb) // PROOF_LEN
    if len(wb) != n * DEPOSIT_PW_LEN or (lamports is not None and len(lamports) != n):
        raise ValueError("proofs, pws and lamports must have one entry per instruction")
    start = start_root if isinstance(start_root, (bytes, bytearray)) else int(start_root).to_bytes(32, "big")
    if len(start) != 32:
        raise ValueError("start_root is 32 bytes")
    lam = (ctypes.c_uint64 * max(n, 1))(*[int(v) for v in lamports]) if lamports is not None else None
    codes = (ctypes.c_uint32 * max(n, 1))()
    end_root = ctypes.create_string_buffer(32)
    end_index = ctypes.c_uint64(0)
    check(ctx.L.spp_verify_deposit_chain(ctx.h, bytes(vk), len(vk), n, pb, wb, ctypes.cast(lam, ctypes.c_void_p) if lam is not None else None,
                                         bytes(start), int(start_index), ctypes.cast(codes, ctypes.c_void_p),
                                         ctypes.cast(end_root, ctypes.c_void_p), ctypes.byref(end_index)))
    return list(codes)[:n], int.from_bytes(end_root.raw, "big"), int(end_index.value)


def merkle_build(ctx, leaves, queries, depth=TREE_DEPTH):
    """One-shot form (spp_merkle_build): all levels recomputed from the leaves, like the reference's getRoot/getProof.
    Returns (root, [siblings per query])."""
    nq = len(queries)
    q = (ctypes.c_uint64 * max(nq, 1))(*[int(i) for i in queries])
    sib = ctypes.create_string_buffer(32 * depth * max(nq, 1))
    root = ctypes.create_string_buffer(32)
    check(ctx.L.spp_merkle_build(ctx.h, len(leaves), depth, _be(leaves), nq, ctypes.cast(q, ctypes.c_void_p),
                                 ctypes.cast(sib, ctypes.c_void_p), ctypes.cast(root, ctypes.c_void_p)))
    return int.from_bytes(root.raw, "big"), [_unbe(sib.raw[32 * depth * i:], depth) for i in range(nq)]


def identity_public_keys(ctx, secret_keys):
    count = len(secret_keys)
    out = ctypes.create_string_buffer(64 * count)
    check(ctx.L.spp_grumpkin_keygen_batch(ctx.h, count, _be(secret_keys), ctypes.cast(out, ctypes.c_void_p)))
    v = _unbe(out.raw, 2 * count)
    return [(v[2 * i], v[2 * i + 1]) for i in range(count)]


def ct_commitments(ctx, packed_rows):
    """packed_rows: list of lists of field elements (157 for the audit ciphertext)."""
    count, n = len(packed_rows), len(packed_rows[0])
    out = ctypes.create_string_buffer(32 * count)
    check(ctx.L.spp_poseidon2_sponge_batch(ctx.h, count, n, _be(v for r in packed_rows for v in r), ctypes.cast(out, ctypes.c_void_p)))
    return _unbe(out.raw, count)


def audit_input_rows(ctx, pk_a, pk_b, secret_keys, r, e1, e2):
    """scripts/generate_audit.py:468-641 for a batch, on the GPU: returns one 3360-element input row per instance
    (wa_commitment, ct_commitment, c0_packed, c1_packed, secret_key, r, e1_sparse, e2, k0, k1 as field elements)."""
    count = len(secret_keys)
    r = np.ascontiguousarray(r, dtype=np.int8).reshape(count, RLWE_N)
    e1 = np.ascontiguousarray(e1, dtype=np.int8).reshape(count, MSG_SLOTS)
    e2 = np.ascontiguousarray(e2, dtype=np.int8).reshape(count, RLWE_N)
    a = np.ascontiguousarray(pk_a, dtype=np.uint32)
    b = np.ascontiguousarray(pk_b, dtype=np.uint32)
    rows = np.zeros((count, 3360 * 32), dtype=np.uint8)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    check(ctx.L.spp_audit_inputs_batch(ctx.h, p(a), p(b), count, _be(secret_keys), p(r), p(e1), p(e2), p(rows)))
    return [_unbe(rows[i].tobytes(), 3360) for i in range(count)]


# ---- auditor side: demo-frontend/app/lib/shamir.ts reconstructSk / rlweDecrypt, scripts/rlwe_decrypt.py ----
def reconstruct_sk(ctx, shares):
    """shares: list of {"x": int, "y": [hex or int] * 1024} (threshold = len(shares)); returns sk mod q (list of ints)."""
    t = len(shares)
    n = len(shares[0]["y"])
    xs = (ctypes.c_uint32 * t)(*[int(s["x"]) for s in shares])
    ys = _be((int(v, 16) if isinstance(v, str) else int(v)) for s in shares for v in s["y"])
    out = (ctypes.c_uint32 * n)()
    check(ctx.L.spp_shamir_reconstruct(ctx.h, t, ctypes.cast(xs, ctypes.c_void_p), ys, n, None, ctypes.cast(out, ctypes.c_void_p)))
    return list(out)


def rlwe_decrypt(ctx, sk_mod_q, c0, c1):
    """Batch: c0 [count,64], c1 [count,1024] -> list of (owner_x, owner_y) and the raw byte slots.  Coefficients in [0, q): a
    larger one is refused (SppError); Context.audit_open opens and flags records that may be malformed."""
    c0 = np.ascontiguousarray(c0, dtype=np.uint32).reshape(-1, MSG_SLOTS)
    count = c0.shape[0]
    c1 = np.ascontiguousarray(c1, dtype=np.uint32).reshape(count, RLWE_N)
    sk = np.ascontiguousarray(sk_mod_q, dtype=np.uint32)
    msg = np.zeros((count, MSG_SLOTS), dtype=np.uint8)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    check(ctx.L.spp_rlwe_decrypt_batch(ctx.h, p(sk), count, p(c0), p(c1), p(msg)))
    owners = [(int.from_bytes(msg[i, :32].tobytes(), "little"), int.from_bytes(msg[i, 32:].tobytes(), "little")) for i in range(count)]
    return owners, msg


# ---- threshold opening: partial decryptions from single shares, nobody rebuilds the key (include/spp.h) ----
SMUDGE_BOUND = 1024
SMUDGE_BUDGET = 1 << 17     # threshold * bound may not exceed it: 196 608 of Delta/2 = 327 680 stay for the ciphertext's own noise


def rlwe_sample_smudge(L, n, bound=SMUDGE_BOUND):
    """n smudging values from the operating system's randomness (host only; L: the loaded library): e int32 in [-bound, bound]
    and rho uint64, the forms rlwe_partial_decrypt takes."""
    e = np.zeros(n, dtype=np.int32)
    rho = np.zeros(n, dtype=np.uint64)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    check(L.spp_rlwe_sample_smudge(n, int(bound), p(e), p(rho)))
    return e, rho


def rlwe_partial_decrypt(ctx, xs, me, share, c0, c1, e=None, rho=None, pair_seeds=None, want_commitments=False):
    """One auditor's partial decryptions (spp_rlwe_partial_decrypt_batch).  xs: the share indices of the participating set, `me`
    this auditor's position in it, share: its 1024 field elements (ints).  c0 [count, 64], c1 [count, 1024] in [0, q).  e, rho:
    [count, 64] smudging values (rlwe_sample_smudge) or None for 0.  pair_seeds: one 32-byte seed per member of xs, in xs order
    (the entry at `me` is ignored; bytes or None there), or None for unmasked partials.  Returns uint8 [count, 64, 32], big-endian
    field elements; with want_commitments also the ct_commitments (ints) the masks were keyed by."""
    c0 = np.ascontiguousarray(c0, dtype=np.uint32).reshape(-1, MSG_SLOTS)
    count, t = c0.shape[0], len(xs)
    c1 = np.ascontiguousarray(c1, dtype=np.uint32).reshape(count, RLWE_N)
    share = [int(v) for v in share]
    if len(share) != RLWE_N:
        raise ValueError("a share is 1024 field elements")
    cx = (ctypes.c_uint32 * max(t, 1))(*[int(x) for x in xs])
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    ce = None if e is None else np.ascontiguousarray(e, dtype=np.int32).reshape(count, MSG_SLOTS)
    cr = None if rho is None else np.ascontiguousarray(rho, dtype=np.uint64).reshape(count, MSG_SLOTS)
    seeds = None
    if pair_seeds is not None:
        if len(pair_seeds) != t or any(len(s) != 32 for j, s in enumerate(pair_seeds) if j != me):
            raise ValueError("pair_seeds: one 32-byte seed per member of the set")
        seeds = b"".join(bytes(32) if j == me else bytes(s) for j, s in enumerate(pair_seeds))
    out = np.zeros((max(count, 1), MSG_SLOTS, 32), dtype=np.uint8)
    cts = ctypes.create_string_buffer(32 * max(count, 1)) if want_commitments else None
    check(ctx.L.spp_rlwe_partial_decrypt_batch(ctx.h, t, ctypes.cast(cx, ctypes.c_void_p), int(me), _be(share), count, p(c0), p(c1),
                                               None if ce is None else p(ce), None if cr is None else p(cr), seeds, p(out),
                                               None if cts is None else ctypes.cast(cts, ctypes.c_void_p)))
    out = out[:count]
    return (out, _unbe(cts.raw, count)) if want_commitments else out


def _partials_array(partials, count):
    a = np.ascontiguousarray(partials, dtype=np.uint8)
    if a.ndim != 4 or a.shape[1:] != (count, MSG_SLOTS, 32) or a.shape[0] == 0:
        raise ValueError("partials: [t, %d, 64, 32] bytes, one rlwe_partial_decrypt result per auditor" % count)
    return a


def rlwe_combine_partials(ctx, partials, c0):
    """The combiner (spp_rlwe_combine_partials): partials = the results of rlwe_partial_decrypt of the t auditors of one set on
    the same ciphertexts, [t, count, 64, 32].  Returns (owners, msg, flags) -- owners and msg as rlwe_decrypt gives them,
    flags[i] = 0 or SPP_AUDIT_BAD_PARTIALS."""
    c0 = np.ascontiguousarray(c0, dtype=np.uint32).reshape(-1, MSG_SLOTS)
    count = c0.shape[0]
    a = _partials_array(partials, count)
    msg = np.zeros((max(count, 1), MSG_SLOTS), dtype=np.uint8)
    flags = np.zeros(max(count, 1), dtype=np.uint32)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    check(ctx.L.spp_rlwe_combine_partials(ctx.h, a.shape[0], count, a.tobytes(), p(c0), p(msg), p(flags)))
    msg = msg[:count]
    owners = [(int.from_bytes(msg[i, :32].tobytes(), "little"), int.from_bytes(msg[i, 32:].tobytes(), "little")) for i in range(count)]
    return owners, msg, [int(f) for f in flags[:count]]


def new_pair_seeds(num_shares):
    """One 32-byte seed from the operating system per pair of the auditors 1..num_shares: {i: {j: seed}} with
    seeds[i][j] == seeds[j][i].  The dealer of a key sees every share already, so dealing the seeds adds no trust; auditors
    may as well agree them pairwise over an authenticated channel."""
    import os
    m = int(num_shares)
    seeds = {i: {} for i in range(1, m + 1)}
    for i in range(1, m + 1):
        for j in range(i + 1, m + 1):
            seeds[i][j] = seeds[j][i] = os.urandom(32)
    return seeds


def write_pair_seeds_json(path, x, num_shares, seeds):
    """pair_seeds_<x>.json: {"x", "num_shares", "seeds": {"<x of the other end>": hex}}"""
    import json
    with open(path, "w") as f:
        json.dump({"x": int(x), "num_shares": int(num_shares), "seeds": {str(j): bytes(s).hex() for j, s in sorted(seeds.items())}}, f, indent=1)


def load_pair_seeds_json(path):
    """(x, {x of the other end: 32 bytes}) of a pair_seeds_<x>.json; ValueError if it is not one"""
    import json
    with open(path) as f:
        d = json.load(f)
    try:
        x, seeds = int(d["x"]), {int(j): bytes.fromhex(s) for j, s in d["seeds"].items()}
    except (KeyError, TypeError, ValueError, AttributeError) as e:
        raise ValueError("%s: not a pair-seeds file (%s)" % (path, e))
    if x <= 0 or x in seeds or any(len(s) != 32 or j <= 0 for j, s in seeds.items()):
        raise ValueError("%s: pair seeds are 32 bytes each, keyed by the other auditor's index" % path)
    return x, seeds


PARTIAL_KEYS = ("x", "with", "ct_commitment", "masked", "smudge_bound", "partial")


def partial_json(x, xs, ct_commitment, masked, smudge_bound, partial):
    """the dict of one partial_<x>.json: auditor x's partial decryption of ONE ciphertext within the set xs"""
    vals = _unbe(np.ascontiguousarray(partial, dtype=np.uint8).tobytes(), MSG_SLOTS)
    return {"x": int(x), "with": sorted(int(v) for v in xs), "ct_commitment": "0x%064x" % int(ct_commitment), "masked": bool(masked),
            "smudge_bound": int(smudge_bound), "partial": ["0x%064x" % v for v in vals]}


def load_partial_json(path):
    """Reads a partial_<x>.json into {"x", "with": sorted xs, "ct_commitment": int, "masked", "smudge_bound", "partial": uint8 [64, 32]};
    ValueError if it is not one."""
    import json
    with open(path) as f:
        d = json.load(f)
    if not isinstance(d, dict) or set(PARTIAL_KEYS) - set(d):
        raise ValueError("%s: not a partial decryption (keys %s)" % (path, ", ".join(PARTIAL_KEYS)))
    try:
        vals = [int(v, 16) for v in d["partial"]]
        out = {"x": int(d["x"]), "with": sorted(int(v) for v in d["with"]), "ct_commitment": int(d["ct_commitment"], 16),
               "masked": bool(d["masked"]), "smudge_bound": int(d["smudge_bound"])}
    except (TypeError, ValueError) as e:
        raise ValueError("%s: not a partial decryption (%s)" % (path, e))
    if len(vals) != MSG_SLOTS or not all(0 <= v < FR_MODULUS for v in vals) or out["x"] not in out["with"] or len(set(out["with"])) != len(out["with"]):
        raise ValueError("%s: a partial is 64 field elements of an auditor inside its set" % path)
    out["partial"] = np.frombuffer(_be(vals), dtype=np.uint8).reshape(MSG_SLOTS, 32).copy()
    return out


# ---- the files the prover and the key holders leave for the auditor ----
RLWE_Q = 167772161
CIPHERTEXT_KEYS = ("c0_sparse", "c1", "c0_packed", "c1_packed", "pack_width", "pack_bits", "msg_slots", "q", "delta",
                   "expected_owner_x", "expected_owner_y")


def _pack7(values):
    return [sum(int(c) << (32 * j) for j, c in enumerate(values[i:i + 7])) for i in range(0, len(values), 7)]


def ciphertext_json(c0, c1, owner=None):
    """The dict scripts/generate_audit.py:593-605 dumps as keys/ciphertext.json, for one ciphertext (c0: 64 and c1: 1024
    coefficients in [0, q), e.g. a row of CircuitHandle.prove_audit_records).  owner: (owner_x, owner_y) the prover expects, or
    None -- the two expected_owner_* keys are then null: an auditor checks the identity against wa_commitment (Context.audit_open),
    not against what the prover claims."""
    c0, c1 = [int(v) for v in c0], [int(v) for v in c1]
    if len(c0) != MSG_SLOTS or len(c1) != RLWE_N or not all(0 <= v < RLWE_Q for v in c0 + c1):
        raise ValueError("a ciphertext is 64 + 1024 coefficients in [0, q)")
    return {"c0_sparse": c0, "c1": c1, "c0_packed": [hex(v) for v in _pack7(c0)], "c1_packed": [hex(v) for v in _pack7(c1)],
            "pack_width": 7, "pack_bits": 32, "msg_slots": MSG_SLOTS, "q": RLWE_Q, "delta": RLWE_Q // 256,
            "expected_owner_x": None if owner is None else hex(int(owner[0])),
            "expected_owner_y": None if owner is None else hex(int(owner[1]))}


def load_ciphertext_json(path):
    """Reads a ciphertext.json (the reference's or ciphertext_json's): returns (c0, c1, owner) with owner = (x, y) or None.  Raises
    ValueError when the file is not one: missing keys, other parameters than the circuit's, wrong lengths, packed fields that are
    not the packing of the coefficients."""
    import json
    with open(path) as f:
        d = json.load(f)
    if not isinstance(d, dict) or set(CIPHERTEXT_KEYS) - set(d):
        raise ValueError("%s: not a ciphertext.json (keys %s)" % (path, ", ".join(CIPHERTEXT_KEYS)))
    if (d["pack_width"], d["pack_bits"], d["msg_slots"], d["q"], d["delta"]) != (7, 32, MSG_SLOTS, RLWE_Q, RLWE_Q // 256):
        raise ValueError("%s: parameters differ from the audit circuit's" % path)
    c0, c1 = [int(v) for v in d["c0_sparse"]], [int(v) for v in d["c1"]]
    if len(c0) != MSG_SLOTS or len(c1) != RLWE_N or not all(0 <= v < 1 << 32 for v in c0 + c1):
        raise ValueError("%s: a ciphertext is 64 + 1024 32-bit coefficients" % path)
    if [int(v, 16) for v in d["c0_packed"]] != _pack7(c0) or [int(v, 16) for v in d["c1_packed"]] != _pack7(c1):
        raise ValueError("%s: the packed fields are not the packing of the coefficients" % path)
    ox, oy = d["expected_owner_x"], d["expected_owner_y"]
    owner = None if ox is None or oy is None else (int(ox, 16), int(oy, 16))
    return c0, c1, owner


def load_share_json(path):
    """Reads one Shamir share file of scripts/rlwe_keygen.py:157-171 ({"share_index", "threshold", "num_shares", "coefficients":
    [{"x", "y": hex}] * 1024}) into the form reconstruct_sk takes: {"x", "y": [int] * 1024, "share_index", "threshold"}."""
    import json
    with open(path) as f:
        d = json.load(f)
    try:
        co = d["coefficients"]
        xs = {int(c["x"]) for c in co}
        ys = [int(c["y"], 16) if isinstance(c["y"], str) else int(c["y"]) for c in co]
        out = {"x": xs.pop(), "y": ys, "share_index": int(d["share_index"]), "threshold": int(d["threshold"])}
    except (KeyError, TypeError, IndexError) as e:
        raise ValueError("%s: not a share file (%s)" % (path, e))
    if xs or len(ys) != RLWE_N or not all(0 <= v < FR_MODULUS for v in ys) or out["x"] <= 0:
        raise ValueError("%s: a share is 1024 field elements at one nonzero x" % path)
    return out


# ---- auditor key generation: scripts/rlwe_keygen.py ----
NOISE_BOUND = 3


def rlwe_sample_key(L, count=1, bound=NOISE_BOUND):
    """count fresh (sk, a, e) from the operating system's randomness (host only; L: the loaded library): int8 [count,1024] in
    [-bound, bound], uint32 [count,1024] in [0, q), int8 [count,1024]."""
    sk = np.zeros((count, RLWE_N), dtype=np.int8)
    a = np.zeros((count, RLWE_N), dtype=np.uint32)
    e = np.zeros((count, RLWE_N), dtype=np.int8)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    check(L.spp_rlwe_sample_key(count, bound, p(sk), p(a), p(e)))
    return sk, a, e


def rlwe_keygen(ctx, sk, a, e):
    """Batch: sk, e signed [count,1024], a [count,1024] in [0, q).  Returns (b, sk_mod_q), uint32 [count,1024]:
    b = e - a*sk mod (X^1024 + 1, q) (rlwe_keygen.py:110-116) and sk mod q, the form rlwe_decrypt takes."""
    sk = np.ascontiguousarray(sk, dtype=np.int8).reshape(-1, RLWE_N)
    count = sk.shape[0]
    a = np.ascontiguousarray(a, dtype=np.uint32).reshape(count, RLWE_N)
    e = np.ascontiguousarray(e, dtype=np.int8).reshape(count, RLWE_N)
    b = np.zeros((count, RLWE_N), dtype=np.uint32)
    skq = np.zeros((count, RLWE_N), dtype=np.uint32)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    check(ctx.L.spp_rlwe_keygen_batch(ctx.h, count, p(sk), p(a), p(e), p(b), p(skq)))
    return b, skq


def rlwe_key_check(ctx, pk_a, pk_b, sk_mod_q):
    """Batch: for every key (max |centred(b + a*sk mod q)|, max |centred(sk)|) as a list of int pairs; a key pair made with noise
    bound B has both at most B."""
    a = np.ascontiguousarray(pk_a, dtype=np.uint32).reshape(-1, RLWE_N)
    count = a.shape[0]
    b = np.ascontiguousarray(pk_b, dtype=np.uint32).reshape(count, RLWE_N)
    sk = np.ascontiguousarray(sk_mod_q, dtype=np.uint32).reshape(count, RLWE_N)
    out = np.zeros((count, 2), dtype=np.uint32)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    check(ctx.L.spp_rlwe_key_check(ctx.h, count, p(a), p(b), p(sk), p(out)))
    return [(int(x), int(y)) for x, y in out]


def shamir_split(ctx, secrets, threshold, num_shares, xs=None, coeffs=None):
    """threshold-of-num_shares sharing of a list of field elements (shamir_share_field, rlwe_keygen.py:51-65, for all of them at
    once).  xs: the share indices (default 1..num_shares); coeffs: coeffs[k-1][i] = coefficient of x^k of value i (default: drawn
    from the operating system by the library).  Returns the shares as reconstruct_sk takes them: [{"x", "y": [int] * n}]."""
    secrets = [int(v) for v in secrets]
    n, t, m = len(secrets), int(threshold), int(num_shares)
    if xs is not None and len(xs) != m:
        raise ValueError("xs must name %d shares" % m)
    if coeffs is not None and (len(coeffs) != t - 1 or any(len(row) != n for row in coeffs)):
        raise ValueError("coeffs must be %d rows of %d field elements" % (t - 1, n))
    cx = None if xs is None else (ctypes.c_uint32 * m)(*[int(x) for x in xs])
    cc = None if coeffs is None else _be(v for row in coeffs for v in row)
    out = ctypes.create_string_buffer(max(1, m * n * 32))
    check(ctx.L.spp_shamir_split(ctx.h, t, m, None if cx is None else ctypes.cast(cx, ctypes.c_void_p), n, _be(secrets), cc,
                                 ctypes.cast(out, ctypes.c_void_p)))
    ys = _unbe(out.raw, m * n)
    return [{"x": int(xs[j]) if xs is not None else j + 1, "y": ys[j * n:(j + 1) * n]} for j in range(m)]


def write_rlwe_pk_json(path, a, b):
    """rlwe_pk.json (rlwe_keygen.py:124-127): {"a", "b"}, coefficients as "0x%08x"."""
    import json
    a, b = [int(v) for v in a], [int(v) for v in b]
    if len(a) != RLWE_N or len(b) != RLWE_N or not all(0 <= v < RLWE_Q for v in a + b):
        raise ValueError("a public key is 1024 + 1024 coefficients in [0, q)")
    with open(path, "w") as f:
        json.dump({"a": ["0x%08x" % v for v in a], "b": ["0x%08x" % v for v in b]}, f)


def write_rlwe_params_json(path, threshold, num_shares, noise_bound=NOISE_BOUND):
    """rlwe_params.json (rlwe_keygen.py:133-142)."""
    import json
    with open(path, "w") as f:
        json.dump({"N": RLWE_N, "q": RLWE_Q, "noise_bound": int(noise_bound), "plaintext_modulus": 256, "delta": RLWE_Q // 256,
                   "threshold": int(threshold), "num_shares": int(num_shares), "field": "BN254"}, f, indent=2)


def share_json(share_index, threshold, num_shares, x, ys):
    """the dict of one share_<i>.json (rlwe_keygen.py:161-169); "y" is "0x%064x", zero is "0x0" (to_hex_bn254, :91-95)"""
    ys = [int(v) for v in ys]
    if not all(0 <= v < FR_MODULUS for v in ys) or int(x) <= 0:
        raise ValueError("a share is field elements at one nonzero x")
    return {"share_index": int(share_index), "threshold": int(threshold), "num_shares": int(num_shares),
            "coefficients": [{"x": int(x), "y": "0x0" if v == 0 else "0x%064x" % v} for v in ys]}


def write_share_json(path, share_index, threshold, num_shares, x, ys):
    import json
    with open(path, "w") as f:
        json.dump(share_json(share_index, threshold, num_shares, x, ys), f)


def load_rlwe_pk_json(path):
    """(a, b) of an rlwe_pk.json, the reference's (hex strings) or the fixture's (integers); ValueError if it is not one"""
    import json
    with open(path) as f:
        d = json.load(f)
    try:
        a, b = ([int(v, 16) if isinstance(v, str) else int(v) for v in d[k]] for k in ("a", "b"))
    except (KeyError, TypeError, ValueError) as e:
        raise ValueError("%s: not an rlwe_pk.json (%s)" % (path, e))
    if len(a) != RLWE_N or len(b) != RLWE_N or not all(0 <= v < RLWE_Q for v in a + b):
        raise ValueError("%s: a public key is 1024 + 1024 coefficients in [0, q)" % path)
    return a, b


def reference_key_draws(seed, threshold=2, n=RLWE_N):
    """(sk, a, e, coeffs) as scripts/rlwe_keygen.py draws them from random.Random(seed) (:99-111, :51-55): sk, a, e, then per key
    coefficient its threshold - 1 sharing coefficients.  For reproducing fixtures only: a seeded key is no key."""
    import random
    rng = random.Random(seed)
    sk = [rng.randint(-NOISE_BOUND, NOISE_BOUND) for _ in range(n)]
    a = [rng.randint(0, RLWE_Q - 1) for _ in range(n)]
    e = [rng.randint(-NOISE_BOUND, NOISE_BOUND) for _ in range(n)]
    coeffs = [[0] * n for _ in range(threshold - 1)]
    for i in range(n):
        for k in range(threshold - 1):
            coeffs[k][i] = rng.randint(0, FR_MODULUS - 1)
    return sk, a, e, coeffs


# ---- the auditors' key without a dealer: verifiable sharing, joint key, share refresh (include/spp.h) ----
VSS_BAD_POINT, VSS_BAD_SHARE, VSS_NOT_ZERO = 1, 2, 4
VSS_FLAG_NAMES = ((VSS_BAD_POINT, "point"), (VSS_BAD_SHARE, "share"), (VSS_NOT_ZERO, "not-zero"))


def vss_generators(L):
    """(G, H) of the Pedersen commitments as (x, y) pairs of ints (host only; L: the loaded library)"""
    g, h = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    check(L.spp_vss_generators(ctypes.cast(g, ctypes.c_void_p), ctypes.cast(h, ctypes.c_void_p)))
    return tuple((int.from_bytes(b.raw[:32], "big"), int.from_bytes(b.raw[32:], "big")) for b in (g, h))


def dkg_a_from_seed(L, seed):
    """the common a of a joint key from the 32-byte seed the auditors agreed on (host only): 1024 ints in [0, q)"""
    seed = bytes(seed)
    if len(seed) != 32:
        raise ValueError("the seed of a is 32 bytes")
    out = (ctypes.c_uint32 * RLWE_N)()
    check(L.spp_dkg_a_from_seed(seed, ctypes.cast(out, ctypes.c_void_p)))
    return list(out)


def vss_deal(ctx, secrets, threshold, num_shares, xs=None, blinds=None, coeffs=None, coeffs_blind=None, times=None):
    """One dealer's verifiable sharing of a list of field elements.  xs, coeffs as in shamir_split; blinds: the constant-term blinds;
    coeffs_blind: the blinding polynomial's higher coefficients; whatever is None the library draws from the operating system.
    Returns {"commitments": bytes (C_k[v] at (k n + v) * 64), "shares": [{"x", "y", "y_blind"}] per receiver, "blinds": [int] * n}.
    times (a list, optional) receives the device milliseconds of the two evaluations and of the commitment kernel."""
    secrets = [int(v) for v in secrets]
    n, t, m = len(secrets), int(threshold), int(num_shares)
    if xs is not None and len(xs) != m:
        raise ValueError("xs must name %d shares" % m)
    for name, rows in (("coeffs", coeffs), ("coeffs_blind", coeffs_blind)):
        if rows is not None and (len(rows) != t - 1 or any(len(row) != n for row in rows)):
            raise ValueError("%s must be %d rows of %d field elements" % (name, t - 1, n))
    if blinds is not None and len(blinds) != n:
        raise ValueError("blinds must be %d field elements" % n)
    cx = None if xs is None else (ctypes.c_uint32 * m)(*[int(x) for x in xs])
    flat = lambda rows: None if rows is None else _be(v for row in rows for v in row)
    ys, yb = (ctypes.create_string_buffer(max(1, m * n * 32)) for _ in range(2))
    cm = ctypes.create_string_buffer(max(1, t * n * 64))
    bo = ctypes.create_string_buffer(max(1, n * 32))
    p = lambda b: ctypes.cast(b, ctypes.c_void_p)
    args = (ctx.h, t, m, None if cx is None else p(cx), n, _be(secrets), None if blinds is None else _be(blinds), flat(coeffs),
            flat(coeffs_blind), p(ys), p(yb), p(cm), p(bo))
    if times is None:
        check(ctx.L.spp_vss_deal(*args))
    else:
        ms = (ctypes.c_float * 2)()
        check(ctx.L.spp_vss_deal_timed(*args, ms))
        times[:] = [float(ms[0]), float(ms[1])]
    y, b = _unbe(ys.raw, m * n), _unbe(yb.raw, m * n)
    return {"commitments": cm.raw[:t * n * 64],
            "shares": [{"x": int(xs[j]) if xs is not None else j + 1, "y": y[j * n:(j + 1) * n], "y_blind": b[j * n:(j + 1) * n]}
                       for j in range(m)],
            "blinds": _unbe(bo.raw, n)}


def vss_receive(ctx, threshold, x, commitments, ys, ys_blind, zero_blinds=None, base=None, want_share=True):
    """The receiver at x checks every dealer's values: commitments [bytes] per dealer, ys / ys_blind / zero_blinds [[int] * n] per
    dealer.  Returns (flags [[int] * n] per dealer, bad, share): share = base (default 0) + the sum over dealers, None when a check
    failed (or want_share is False)."""
    dealers, n, t = len(commitments), len(ys[0]) if ys else 0, int(threshold)
    if len(ys) != dealers or len(ys_blind) != dealers or (zero_blinds is not None and len(zero_blinds) != dealers):
        raise ValueError("one commitment string, one y row and one y_blind row per dealer")
    if any(len(c) != t * n * 64 for c in commitments) or any(len(r) != n for r in list(ys) + list(ys_blind) + list(zero_blinds or [])):
        raise ValueError("a dealing of %d values at threshold %d is %d commitment bytes and %d sub-shares" % (n, t, t * n * 64, n))
    if base is not None and len(base) != n:
        raise ValueError("base must be %d field elements" % n)
    flat = lambda rows: _be(v for row in rows for v in row)
    flags = (ctypes.c_uint32 * max(1, dealers * n))()
    out = ctypes.create_string_buffer(max(1, n * 32))
    bad = ctypes.c_size_t(0)
    check(ctx.L.spp_vss_receive(ctx.h, t, int(x), dealers, n, b"".join(commitments), flat(ys), flat(ys_blind),
                                None if zero_blinds is None else flat(zero_blinds), None if base is None else _be(base),
                                ctypes.cast(flags, ctypes.c_void_p), ctypes.cast(out, ctypes.c_void_p) if want_share else None,
                                ctypes.byref(bad)))
    fl = [list(flags[d * n:(d + 1) * n]) for d in range(dealers)]
    return fl, int(bad.value), (_unbe(out.raw, n) if want_share and bad.value == 0 else None)


# ---- the committee's commitments and verifiable resharing (include/spp.h) ----
VSS_NOT_SHARE = 8
VSS_RESHARE_FLAG_NAMES = ((VSS_BAD_POINT, "point"), (VSS_BAD_SHARE, "share"), (VSS_NOT_SHARE, "not-share"))


def lagrange_at_zero(xs):
    """the Lagrange coefficients at 0 of the distinct non-zero indices xs, as ints mod r"""
    xs = [int(x) for x in xs]
    lam = []
    for j, xj in enumerate(xs):
        num = den = 1
        for i, xi in enumerate(xs):
            if i != j:
                num = num * xi % FR_MODULUS
                den = den * (xi - xj) % FR_MODULUS
        lam.append(num * pow(den, -1, FR_MODULUS) % FR_MODULUS)
    return lam


def vss_combine_commitments(ctx, threshold, commitments, weights=None, base=None, times=None):
    """base + sum_d w_d C_d over the dealers' commitment strings (bytes of threshold * n * 64 each); weights: one int per dealer
    or None (plain sums: the committee's commitments of a key, or of a refresh round on top of base).  Returns (flags [[int] *
    (threshold * n)] per dealer, bad, out bytes or None when an input is no point).  times (a list, optional) receives the device
    milliseconds of the kernels."""
    dealers, t = len(commitments), int(threshold)
    size = len(commitments[0]) if commitments else 0
    n = size // (64 * t) if t else 0
    if size != n * t * 64 or any(len(c) != size for c in commitments) or (base is not None and len(base) != size):
        raise ValueError("every dealer's commitments (and base) are threshold * n * 64 bytes")
    if weights is not None and len(weights) != dealers:
        raise ValueError("one weight per dealer")
    flags = (ctypes.c_uint32 * max(1, dealers * t * n))()
    out = ctypes.create_string_buffer(max(1, size))
    bad = ctypes.c_size_t(0)
    args = (ctx.h, t, dealers, n, b"".join(commitments), None if weights is None else _be(weights), base, ctypes.cast(out, ctypes.c_void_p),
            ctypes.cast(flags, ctypes.c_void_p), ctypes.byref(bad))
    if times is None:
        check(ctx.L.spp_vss_combine_commitments(*args))
    else:
        ms = ctypes.c_float(0)
        check(ctx.L.spp_vss_combine_commitments_timed(*args, ctypes.byref(ms)))
        times[:] = [float(ms.value)]
    fl = [list(flags[d * t * n:(d + 1) * t * n]) for d in range(dealers)]
    return fl, int(bad.value), (out.raw[:size] if bad.value == 0 else None)


def vss_share_commitments(ctx, threshold, committee, xs):
    """E_x = sum_k x^k D_k for every x in xs: a list of n * 64 bytes per x (committee: threshold * n * 64 bytes)"""
    t, xs = int(threshold), [int(x) for x in xs]
    n = len(committee) // (64 * t) if t else 0
    if len(committee) != t * n * 64:
        raise ValueError("a committee's commitments are threshold * n * 64 bytes")
    cx = (ctypes.c_uint32 * max(1, len(xs)))(*xs)
    out = ctypes.create_string_buffer(max(1, len(xs) * n * 64))
    check(ctx.L.spp_vss_share_commitments(ctx.h, t, n, committee, len(xs), ctypes.cast(cx, ctypes.c_void_p), ctypes.cast(out, ctypes.c_void_p)))
    return [out.raw[i * n * 64:(i + 1) * n * 64] for i in range(len(xs))]


def vss_reshare_receive(ctx, xs_old, threshold_new, x_new, committee, commitments, ys, ys_blind):
    """The new member at x_new takes the dealings of the old members xs_old (the set S, as many as the old threshold): committee
    the old committee's commitments, commitments [bytes] / ys / ys_blind [[int] * n] per old member in xs_old order.  Returns
    (flags [[int] * n] per old member, bad, share, blind, committee_out); the last three are None when a check failed."""
    xs_old, t_new = [int(x) for x in xs_old], int(threshold_new)
    t_old, n = len(xs_old), len(ys[0]) if ys else 0
    if len(commitments) != t_old or len(ys) != t_old or len(ys_blind) != t_old:
        raise ValueError("one commitment string, one y row and one y_blind row per old member")
    if any(len(c) != t_new * n * 64 for c in commitments) or any(len(r) != n for r in list(ys) + list(ys_blind)) or len(committee) != t_old * n * 64:
        raise ValueError("a dealing of %d values at threshold %d is %d commitment bytes; the old committee's are %d"
                         % (n, t_new, t_new * n * 64, t_old * n * 64))
    flat = lambda rows: _be(v for row in rows for v in row)
    cx = (ctypes.c_uint32 * max(1, t_old))(*xs_old)
    flags = (ctypes.c_uint32 * max(1, t_old * n))()
    share, blind = (ctypes.create_string_buffer(max(1, n * 32)) for _ in range(2))
    out = ctypes.create_string_buffer(max(1, t_new * n * 64))
    bad = ctypes.c_size_t(0)
    p = lambda b: ctypes.cast(b, ctypes.c_void_p)
    check(ctx.L.spp_vss_reshare_receive(ctx.h, t_old, p(cx), t_new, int(x_new), n, committee, b"".join(commitments), flat(ys), flat(ys_blind),
                                        p(flags), p(share), p(blind), p(out), ctypes.byref(bad)))
    fl = [list(flags[j * n:(j + 1) * n]) for j in range(t_old)]
    if bad.value:
        return fl, int(bad.value), None, None, None
    return fl, 0, _unbe(share.raw, n), _unbe(blind.raw, n), out.raw[:t_new * n * 64]
