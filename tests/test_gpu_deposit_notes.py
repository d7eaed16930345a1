"""Deposits from secrets into the device-resident Merkle tree (spp_merkle_tree_deposit): the reference's KAT, commitments
against the keygen + Poseidon batch calls and the CPU oracle, every per-deposit root against a twin tree fed one leaf at a
time through spp_merkle_tree_insert, capacity, refusals that leave the tree unchanged, interleaving with insert, deposit then
withdraw from the same tree, and concurrent depositors."""
import ctypes
import random
import threading

import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None

pytestmark = pytest.mark.gpu

DEPTH = 16
BAD_INPUT = -1


@pytest.fixture(scope="module")
def ctx():
    import spp
    c = spp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def handle(ctx, withdraw_artifacts):
    h = ctx.load_circuit(withdraw_artifacts["sppc"], withdraw_artifacts["pk"], 6)
    yield h
    h.close()


def _deposits(rng, n):
    return [(rng.randrange(1, 1 << 128), rng.randrange(1, 1 << 63), rng.randrange(1 << 253)) for _ in range(n)]


def _device_commitments(ctx, deps):
    """spp_grumpkin_keygen_batch + spp_poseidon_hash_batch (arity 4): the two-call form of the same commitments."""
    from spp import witness as W
    owners = W.identity_public_keys(ctx, [d[0] for d in deps])
    return W.poseidon_hash_batch(ctx, [[o[0], o[1], d[1], d[2]] for o, d in zip(owners, deps)])


def _oracle_commitment(dep):
    from oracle import hashes as H
    sk, amount, rnd = dep
    owner = H.fixed_base_scalar_mul(sk)
    return H.poseidon_hash4(owner[0], owner[1], amount, rnd)


def _twin_roots(twin, leaves):
    """the root of the twin tree after each single insert"""
    out = []
    for leaf in leaves:
        twin.insert(leaf)
        out.append(twin.getRoot())
    return out


def _raw_deposit(tree, count, buf, want_first=True):
    first = ctypes.c_uint64(12345)
    com, roots = ctypes.create_string_buffer(32 * max(count, 1)), ctypes.create_string_buffer(32 * max(count, 1))
    rc = tree.ctx.L.spp_merkle_tree_deposit(tree.h, count, buf, ctypes.byref(first) if want_first else None,
                                            ctypes.cast(com, ctypes.c_void_p), ctypes.cast(roots, ctypes.c_void_p))
    return rc, first.value


def test_reference_kat_deposit(ctx, withdraw_kat):
    from oracle import circuit as C, hashes as H
    from spp import witness as W
    f = lambda k: int(withdraw_kat[k], 16) if isinstance(withdraw_kat[k], str) else int(withdraw_kat[k])
    sk, amount, rnd = f("secret_key"), f("amount"), f("randomness")
    assert amount == 10_000_000
    commitment = H.poseidon_hash4(f("owner_x"), f("owner_y"), amount, rnd)
    assert hex(commitment).startswith("0x1d0a5a67")
    orc = H.MerkleTree(DEPTH)
    orc.insert(commitment)
    assert orc.root() == f("root")                        # the KAT root is the root of the one-leaf tree
    with W.ShieldedPoolMerkleTree(ctx, DEPTH) as tree:
        first, coms, roots = tree.deposit([(sk, amount, rnd)])
        assert (first, coms, roots) == (0, [commitment], [f("root")])
        assert tree.getRoot() == f("root") and len(tree) == 1
        rows = tree.withdraw_rows([(f("recipient"), amount, sk, rnd, 0)])
    assert rows == [C.withdraw_inputs(withdraw_kat)]


@pytest.mark.parametrize("m", [0, 1, 63, 1021])
def test_deposit_parity_with_a_twin_tree(ctx, m):
    """Every root of a deposit call == the twin's getRoot() after inserting that leaf; 1021 + 300 crosses the 1024-leaf
    reallocation of the level arrays."""
    from oracle import hashes as H
    from oracle.bn254 import R
    from spp import witness as W
    rng = random.Random(1000 + m)
    pre = [rng.randrange(R) for _ in range(m)]
    for n in (1, 2, 64, 65, 300):
        deps = _deposits(rng, n)
        with W.ShieldedPoolMerkleTree(ctx, DEPTH) as tree, W.ShieldedPoolMerkleTree(ctx, DEPTH) as twin:
            if m:
                assert tree.insert_many(pre) == 0 and twin.insert_many(pre) == 0
            first, coms, roots = tree.deposit(deps)
            assert first == m and len(coms) == len(roots) == n
            assert coms == _device_commitments(ctx, deps), (m, n)
            assert roots == _twin_roots(twin, coms), (m, n)
            assert len(tree) == len(twin) == m + n and tree.getRoot() == twin.getRoot() == roots[-1]
            idx = sorted({0, m + n - 1, m, rng.randrange(m + n), rng.randrange(m + n)})
            assert tree.getProofs(idx) == twin.getProofs(idx)
    # the oracle on a sample of the last call (m, 300)
    for k in sorted({0, 150, n - 1} | {rng.randrange(n) for _ in range(5)}):
        assert coms[k] == _oracle_commitment(deps[k]), k
    for k in (0, 137, n - 1):
        orc = H.MerkleTree(DEPTH)
        for leaf in (pre + coms)[:m + k + 1]:
            orc.insert(leaf)
        assert roots[k] == orc.root(), k


def test_capacity(ctx):
    from spp import witness as W
    rng = random.Random(7)
    deps = _deposits(rng, 1 << DEPTH)
    with W.ShieldedPoolMerkleTree(ctx, DEPTH) as tree, W.ShieldedPoolMerkleTree(ctx, DEPTH) as twin:
        first, coms, roots = tree.deposit(deps)
        assert first == 0 and len(tree) == 1 << DEPTH
        twin.insert_many(coms)
        assert twin.getRoot() == tree.getRoot() == roots[-1]
        assert len(set(coms)) == len(coms)
        with W.ShieldedPoolMerkleTree(ctx, DEPTH) as chunked:
            for k in sorted(rng.sample(range(1 << DEPTH), 32)):
                chunked.insert_many(coms[len(chunked):k + 1])
                assert chunked.getRoot() == roots[k], k
        rc, _ = _raw_deposit(tree, 1, W.pack_deposits(_deposits(rng, 1)))
        assert rc == BAD_INPUT and "full" in tree.ctx.L.spp_last_error().decode()
        assert len(tree) == 1 << DEPTH and tree.getRoot() == roots[-1]
    with W.ShieldedPoolMerkleTree(ctx, 4) as small:
        small.insert_many(list(range(1, 11)))
        root = small.getRoot()
        rc, _ = _raw_deposit(small, 7, W.pack_deposits(_deposits(rng, 7)))
        assert rc == BAD_INPUT and "deposit 6" in small.ctx.L.spp_last_error().decode()
        assert len(small) == 10 and small.getRoot() == root
        first, coms, roots = small.deposit(_deposits(rng, 6))
        assert first == 10 and len(small) == 16 and small.getRoot() == roots[-1]


def test_refusals_leave_the_tree_unchanged(ctx):
    import spp
    from oracle.bn254 import R
    from spp import witness as W
    rng = random.Random(11)
    with W.ShieldedPoolMerkleTree(ctx, DEPTH) as tree:
        tree.insert_many([rng.randrange(R) for _ in range(5)])
        size, root = len(tree), tree.getRoot()
        good = _deposits(rng, 4)
        cases = {
            "secret_key": (R, 5, 6),
            "amount": (3, R, 6),
            "randomness": (3, 5, R),
            "amount does not fit 64 bits": (3, 1 << 64, 6),
            "secret_key is 0": (0, 5, 6),
        }
        for what, bad in cases.items():
            batch = good[:2] + [bad] + good[2:]
            rc, first = _raw_deposit(tree, len(batch), W.pack_deposits(batch))
            msg = spp.last_error()
            assert rc == BAD_INPUT and "deposit 2" in msg and what in msg, (what, msg)
            assert first == 12345                       # *first_index is not written on a refusal
            assert len(tree) == size and tree.getRoot() == root
            with pytest.raises(spp.SppError):
                tree.deposit(batch)
            assert len(tree) == size and tree.getRoot() == root
        L = ctx.L
        buf = W.pack_deposits(good)
        assert L.spp_merkle_tree_deposit(None, 1, buf, None, None, None) == BAD_INPUT
        assert L.spp_merkle_tree_deposit(tree.h, 1, None, None, None, None) == BAD_INPUT
        assert "NULL" in spp.last_error()
        assert L.spp_merkle_tree_deposit(tree.h, (1 << 24) + 1, buf, None, None, None) == BAD_INPUT
        assert len(tree) == size and tree.getRoot() == root
        # count == 0: OK, first_index = size, nothing changes
        rc, first = _raw_deposit(tree, 0, b"")
        assert rc == 0 and first == size
        assert L.spp_merkle_tree_deposit(tree.h, 0, None, None, None, None) == 0
        assert tree.deposit([]) == (size, [], [])
        assert len(tree) == size and tree.getRoot() == root
        # every output optional: a deposit without any output still lands
        assert L.spp_merkle_tree_deposit(tree.h, len(good), buf, None, None, None) == 0
        assert len(tree) == size + len(good)
        leaves = _device_commitments(ctx, good)
        assert tree.getProofs([size ^ 1])[0][0] == leaves[0]     # the level-0 sibling of leaf size ^ 1 is leaf size


def test_interleaved_with_insert(ctx):
    from oracle.bn254 import R
    from spp import witness as W
    rng = random.Random(13)
    with W.ShieldedPoolMerkleTree(ctx, DEPTH) as tree, W.ShieldedPoolMerkleTree(ctx, DEPTH) as twin:
        expect = 0
        for kind, n in (("insert", 3), ("deposit", 5), ("insert", 2), ("deposit", 4)):
            if kind == "insert":
                leaves = [rng.randrange(R) for _ in range(n)]
                assert tree.insert_many(leaves) == expect
                _twin_roots(twin, leaves)
            else:
                first, coms, roots = tree.deposit(_deposits(rng, n))
                assert first == expect
                assert roots == _twin_roots(twin, coms)
            expect += n
            assert len(tree) == expect and tree.getRoot() == twin.getRoot()


def test_deposit_then_withdraw_from_notes(ctx, handle, withdraw_artifacts):
    """130 deposits (body + tail of 64) behind existing leaves, then withdraw proofs from the five values per note."""
    from oracle import groth16, native
    from oracle.bn254 import R
    from spp import witness as W
    rng = random.Random(17)
    deps = _deposits(rng, 130)
    with W.ShieldedPoolMerkleTree(ctx, DEPTH) as tree:
        tree.insert_many([rng.randrange(R) for _ in range(37)])
        first, coms, roots = tree.deposit(deps)
        assert first == 37
        notes = [(rng.randrange(1, 1 << 240), a, sk, rnd, first + k) for k, (sk, a, rnd) in enumerate(deps)]
        rs = [(rng.randrange(1, 1 << 250), rng.randrange(1, 1 << 250)) for _ in notes]
        proofs, pws, status = handle.prove_withdraw_notes(tree, notes, rs)
        assert status == [0] * len(notes)
        rows = tree.withdraw_rows(notes)
    p2, w2, s2 = handle.prove_batch(rows, rs)
    assert s2 == status and p2 == proofs and w2 == pws
    assert all(int.from_bytes(w[12:44], "big") == roots[-1] for w in pws)
    orc = native.Prover(withdraw_artifacts["sppc"], withdraw_artifacts["pk"])
    vk = open(withdraw_artifacts["vk"], "rb").read()
    for i in (0, 129):
        rc, proof, pw = orc.prove(rows[i], *rs[i])
        assert rc == 0 and proofs[i] == proof and pws[i] == pw, i
        assert groth16.verify(vk, proof, pw)


def test_concurrent_depositors_get_disjoint_contiguous_ranges(ctx):
    from spp import witness as W
    rng = random.Random(19)
    batches = [_deposits(rng, 200), _deposits(rng, 200)]
    out = [None, None]
    with W.ShieldedPoolMerkleTree(ctx, DEPTH) as tree:
        def run(k):
            out[k] = tree.deposit(batches[k])
        threads = [threading.Thread(target=run, args=(k,)) for k in (0, 1)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        firsts = sorted(o[0] for o in out)
        assert firsts == [0, 200] and len(tree) == 400
        root = tree.getRoot()
        idx = [o[0] + k for o in out for k in range(200)]
        leaves = [c for o in out for c in o[1]]
        sib = tree.getProofs(idx)
        assert W.merkle_roots(ctx, leaves, idx, sib) == [root] * 400
