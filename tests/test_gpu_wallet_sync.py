"""GPU: wallet sync (spp_merkle_tree_find, spp_wallet_sync) -- the reference's KAT, parity with the keygen + Poseidon batch calls and
the CPU oracle, the leaf index under a fixed salt (a chain that wraps, a repeated value, a zero leaf) against the linear model of
tests/test_wallet_sync_host.py, incremental growth, the pool's two sets, the loop deposit -> sync -> prove from notes -> settle ->
sync, and the refusals."""
import ctypes
import os
import random

import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None

from conftest import GOLDEN
from test_wallet_sync_host import R, SALT, forty_leaves, model

pytestmark = pytest.mark.gpu

DEPTH = 16
BAD_INPUT = -1
IN_TREE, SPENT, AUDITED, REPEATED = 1, 2, 4, 8
NULLIFIERS, AUDITS = 0, 1


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


@pytest.fixture(scope="module")
def reference_vks():
    return tuple(open(os.path.join(GOLDEN, n), "rb").read() for n in ("reference_withdraw.vk", "reference_audit.vk"))


def _deposits(rng, n):
    return [(rng.randrange(1, 1 << 128), rng.randrange(1, 1 << 63), rng.randrange(1 << 253)) for _ in range(n)]


def _expected_records(ctx, deps, indices):
    """(commitment, nullifier, wa_commitment, owner) per secret from the calls that existed before: keygen and three hash batches"""
    from spp import witness as W
    owners = W.identity_public_keys(ctx, [d[0] for d in deps])
    coms = W.poseidon_hash_batch(ctx, [[o[0], o[1], d[1], d[2]] for o, d in zip(owners, deps)])
    was = W.poseidon_hash_batch(ctx, [[o[0], o[1]] for o in owners])
    nfs = W.poseidon_hash_batch(ctx, [[d[0], i if i is not None else 0] for d, i in zip(deps, indices)])
    return [(c, n if i is not None else 0, w, o) for c, n, w, o, i in zip(coms, nfs, was, owners, indices)]


def _nullifiers(ctx, pairs):
    from spp import witness as W
    return W.poseidon_hash_batch(ctx, [[sk, i] for sk, i in pairs])


def test_reference_kat_sync(ctx, withdraw_kat):
    from spp import witness as W
    f = lambda k: int(withdraw_kat[k], 16) if isinstance(withdraw_kat[k], str) else int(withdraw_kat[k])
    dep = (f("secret_key"), f("amount"), f("randomness"))
    with W.ShieldedPoolMerkleTree(ctx, DEPTH) as tree:
        first, coms, roots = tree.deposit([dep])
        assert first == 0 and roots == [f("root")]
        records, notes = tree.sync([dep], recipients=[f("recipient")])
        assert records == [(0, IN_TREE, coms[0], f("nullifier"), f("wa_commitment"), (f("owner_x"), f("owner_y")))]
        assert notes == [(f("recipient"), f("amount"), f("secret_key"), f("randomness"), f("index"))]
        assert tree.find(coms) == ([0], [1])
        assert tree.sync([dep]) == records


def test_parity_with_the_batch_calls_and_the_oracle(ctx):
    from oracle import hashes as H
    from spp import witness as W
    rng = random.Random(2001)
    pre, post = [rng.randrange(R) for _ in range(37)], [rng.randrange(R) for _ in range(3)]
    deps, strangers = _deposits(rng, 130), _deposits(rng, 5)
    with W.ShieldedPoolMerkleTree(ctx, DEPTH) as tree, W.ShieldedPoolMerkleTree(ctx, DEPTH) as twin:
        for t in (tree, twin):
            assert t.insert_many(pre) == 0
            first, coms, _ = t.deposit(deps)
            assert first == 37 and t.insert_many(post) == 167
        order = list(range(130))
        rng.shuffle(order)
        secrets = [deps[k] for k in order] + strangers
        known = [37 + k for k in order] + [None] * 5
        records = tree.sync(secrets)
        assert [r[0] for r in records] == known
        assert [r[1] for r in records] == [IN_TREE] * 130 + [0] * 5
        assert [r[2:] for r in records] == _expected_records(ctx, secrets, known)
        assert [r[2] for r in records[:130]] == [coms[k] for k in order]
        assert all(r[3] == 0 for r in records[130:]) and all(r[3] != 0 for r in records[:130])
        for j in sorted(rng.sample(range(135), 8) + [134]):
            sk, amount, rnd = secrets[j]
            owner = H.fixed_base_scalar_mul(sk)
            want = (H.poseidon_hash4(owner[0], owner[1], amount, rnd), H.poseidon_hash2(sk, known[j]) if known[j] is not None else 0,
                    H.poseidon_hash2(owner[0], owner[1]), (owner[0], owner[1]))
            assert records[j][2:] == want, j
        # find over the same tree: the inserted leaves too
        idx, matches = tree.find(pre + coms + post + [records[130][2]])
        assert idx == list(range(170)) + [None] and matches == [1] * 170 + [0]
        # the tree itself has not noticed: root and proofs equal those of a twin that was never synced
        assert len(tree) == len(twin) == 170 and tree.getRoot() == twin.getRoot()
        q = [0, 36, 37, 100, 166, 167, 169, 170, 65535]
        assert tree.getProofs(q) == twin.getProofs(q)


def test_find_under_a_fixed_salt(ctx):
    """40 leaves in the 128-slot table under SPP_TREE_INDEX_SALT: four values homed at the last slot (the run wraps), one value at
    leaves 3, 17 and 31, one leaf 0, absent keys homed inside the wrapped run; against the linear model."""
    from spp import witness as W
    rng = random.Random(41)
    leaves, last, triple, absent_in_run = forty_leaves(rng)
    old = os.environ.get("SPP_TREE_INDEX_SALT")
    os.environ["SPP_TREE_INDEX_SALT"] = "%x" % SALT
    try:
        with W.ShieldedPoolMerkleTree(ctx, DEPTH) as tree:
            tree.insert_many(leaves)
            keys = leaves + absent_in_run + [rng.randrange(R) for _ in range(3)]
            idx, matches = tree.find(keys)                               # the index is built here, with the salt of the environment
            want = [model(leaves, k, 0, 1, 1) for k in keys]
            assert [-1 if i is None else i for i in idx] == [w[0] for w in want] and matches == [w[1] for w in want]
            assert idx[3] == idx[17] == idx[31] == 3 and matches[3] == 3 and idx[9] == 9 and matches[9] == 1
            assert idx[40:] == [None] * 6 and matches[40:] == [0] * 6
            assert sorted(idx[p] for p in (5, 11, 22, 38)) == [5, 11, 22, 38]
            # enumeration by from: equal to, between and past the occurrences
            starts = [0, 3, 4, 16, 17, 18, 31, 32, 39, 40, 1 << 40]
            idx, matches = tree.find([triple] * len(starts), starts)
            assert idx == [3, 3, 17, 17, 17, 31, 31, None, None, None, None] and matches == [3] * len(starts)
            found, at = [], 0
            while True:
                (i,), _ = tree.find([triple], [at])
                if i is None:
                    break
                found.append(i)
                at = i + 1
            assert found == [3, 17, 31]
            assert tree.find([0, 0], [0, 10]) == ([9, None], [1, 1])
            assert tree.find([]) == ([], [])
        # the salt is read when the index is first built: a tree made now refuses a malformed one, and works once it is mended
        import spp
        with W.ShieldedPoolMerkleTree(ctx, DEPTH) as tree:
            tree.insert_many(leaves[:5])
            os.environ["SPP_TREE_INDEX_SALT"] = "xyz"
            with pytest.raises(spp.SppError, match="SPP_TREE_INDEX_SALT"):
                tree.find(leaves[:1])
            os.environ["SPP_TREE_INDEX_SALT"] = "%x" % (SALT + 1)
            assert tree.find(leaves[:5]) == ([0, 1, 2, 3, 4], [1] * 5)
    finally:
        if old is None:
            del os.environ["SPP_TREE_INDEX_SALT"]
        else:
            os.environ["SPP_TREE_INDEX_SALT"] = old


@pytest.mark.parametrize("depth,n0,n1", [(DEPTH, 1000, 300), (4, 9, 7)])
def test_incremental_index_equals_a_fresh_one(ctx, depth, n0, n1):
    """sync, deposit more, sync again (depth 16: across the 1 024-leaf reallocation of the level arrays and a table rebuild; depth 4:
    to 16 of 16 leaves) == one sync of a fresh tree fed all the leaves at once"""
    from spp import witness as W
    rng = random.Random(3000 + depth)
    deps = _deposits(rng, n0 + n1)
    deps[n0 + 1] = deps[2]                                               # a repeat that arrives with the second batch
    secrets = deps[:]
    rng.shuffle(secrets)
    secrets += _deposits(rng, 3)
    with W.ShieldedPoolMerkleTree(ctx, depth) as tree, W.ShieldedPoolMerkleTree(ctx, depth) as fresh:
        tree.deposit(deps[:n0])
        early = tree.sync(secrets)
        assert sum(r[0] is not None for r in early) == n0 + 1 and not any(r[1] & REPEATED for r in early)
        tree.deposit(deps[n0:])
        late = tree.sync(secrets)
        _, coms, _ = fresh.deposit(deps)
        assert late == fresh.sync(secrets)
        assert sum(r[0] is not None for r in late) == n0 + n1 and [r[0] for r in late[-3:]] == [None] * 3
        assert sorted(r[0] for r in late[:-3]) == sorted([i for i in range(n0 + n1) if i != n0 + 1] + [2])
        assert sum(bool(r[1] & REPEATED) for r in late) == 2
        assert tree.find(coms) == fresh.find(coms)
        assert tree.find(coms)[0] == [2 if i == n0 + 1 else i for i in range(n0 + n1)]
        assert len(tree) == n0 + n1 and tree.getRoot() == fresh.getRoot()


def test_with_a_pool(ctx, reference_vks):
    from spp import witness as W
    rng = random.Random(4001)
    n = 60
    deps = _deposits(rng, n)
    thrice = _deposits(rng, 1)[0]
    with W.ShieldedPoolMerkleTree(ctx, DEPTH) as tree, W.Pool(ctx, reference_vks[0], reference_vks[1], 128) as pool:
        tree.insert_many([rng.randrange(R) for _ in range(5)])
        tree.deposit(deps[:20] + [thrice] + deps[20:40] + [thrice, thrice] + deps[40:])
        at3 = [25, 46, 47]
        plain = tree.sync(deps + [thrice])
        assert all(r[1] == IN_TREE for r in plain[:n]) and plain[n][:2] == (25, IN_TREE | REPEATED)
        spent = [k for k in range(n) if k % 3 == 0]
        audited = [k for k in range(n) if k % 2 == 1]
        pool.import_keys(NULLIFIERS, [plain[k][3] for k in spent])
        pool.import_keys(AUDITS, [plain[k][4] for k in audited])
        got = tree.sync(deps + [thrice], pool)
        for k in range(n):
            assert got[k][1] == IN_TREE | (SPENT if k in spent else 0) | (AUDITED if k in audited else 0), k
            assert got[k][0] == plain[k][0] and got[k][2:] == plain[k][2:]
        # AUDITED is evaluated for a commitment that is no leaf as well
        stranger = _deposits(rng, 1)[0]
        absent, = tree.sync([stranger], pool)
        pool.import_keys(AUDITS, [absent[4]])
        assert tree.sync([stranger], pool) == [(None, AUDITED, absent[2], 0, absent[4], absent[5])] and absent[:2] == (None, 0)
        # the secret deposited three times: nothing spent -> the lowest index
        nf3 = _nullifiers(ctx, [(thrice[0], i) for i in at3])
        assert got[n][:2] == (25, IN_TREE | REPEATED) and got[n][3] == nf3[0]
        assert tree.find([got[n][2]] * 3, [0, 26, 47]) == ([25, 46, 47], [3] * 3)
        pool.import_keys(NULLIFIERS, [nf3[0]])                           # occurrence 0 spent -> the second index and ITS nullifier
        r, = tree.sync([thrice], pool)
        assert r[:2] == (46, IN_TREE | REPEATED) and r[3] == nf3[1]
        pool.import_keys(NULLIFIERS, [nf3[2]])                           # the third spent as well: still the second
        r, = tree.sync([thrice], pool)
        assert r[:2] == (46, IN_TREE | REPEATED) and r[3] == nf3[1]
        pool.import_keys(NULLIFIERS, [nf3[1]])                           # all three spent -> the lowest index, SPENT
        r, = tree.sync([thrice], pool)
        assert r[:2] == (25, IN_TREE | REPEATED | SPENT) and r[3] == nf3[0]
        # without a pool neither bit is ever set, whatever the pool holds
        assert tree.sync(deps + [thrice]) == plain
        assert pool.counts() == (len(spent) + 3, len(audited) + 1)


def test_the_loop_deposit_sync_prove_settle_sync(ctx, handle, withdraw_artifacts, reference_vks):
    from oracle import groth16
    from spp import witness as W
    rng = random.Random(5001)
    deps, stranger = _deposits(rng, 8), _deposits(rng, 1)[0]
    addresses = [rng.getrandbits(256).to_bytes(32, "big") for _ in range(9)]
    words = [W.recipient_word(a) for a in addresses]
    wvk = open(withdraw_artifacts["vk"], "rb").read()
    with W.ShieldedPoolMerkleTree(ctx, DEPTH) as tree, W.Pool(ctx, wvk, reference_vks[1], 16) as pool:
        tree.insert_many([rng.randrange(R) for _ in range(3)])
        tree.deposit(deps)
        pool.add_roots([tree.getRoot()])
        records, notes = tree.sync(deps + [stranger], pool, words)
        assert [r[:2] for r in records] == [(3 + k, IN_TREE) for k in range(8)] + [(None, 0)]
        assert notes[8] == (words[8], stranger[1], stranger[0], stranger[2], 1 << DEPTH)
        assert notes[:8] == [(words[k], d[1], d[0], d[2], 3 + k) for k, d in enumerate(deps)]
        pool.import_keys(AUDITS, [r[4] for r in records[:8]])           # the audit records withdraw.rs:94-125 demands
        rs = [(rng.randrange(1, 1 << 250), rng.randrange(1, 1 << 250)) for _ in notes]
        proofs, pws, status = handle.prove_withdraw_notes(tree, notes, rs)
        assert all(s == 0 for s in status[:8]) and status[8] != 0      # the absent secret's note is refused in place
        for k in range(8):
            assert groth16.verify(wvk, proofs[k], pws[k]), k
            assert pws[k][44:76] == records[k][3].to_bytes(32, "big")
        codes, amounts = pool.withdraw(proofs[:8], pws[:8], addresses[:8])
        assert codes == [0] * 8 and amounts == [d[1] for d in deps]
        again = tree.sync(deps + [stranger], pool)
        assert [r[:2] for r in again] == [(3 + k, IN_TREE | SPENT | AUDITED) for k in range(8)] + [(None, 0)]
        assert [r[2:] for r in again] == [r[2:] for r in records]


def _raw_sync(L, tree, pool, count, deposits, recipients, want=(True, True, False, False)):
    n = max(count, 1) if count <= 64 else 1
    idx, flags = (ctypes.c_uint64 * n)(), (ctypes.c_uint32 * n)()
    rec, notes = ctypes.create_string_buffer(160 * n), ctypes.create_string_buffer(160 * n)
    outs = [ctypes.cast(b, ctypes.c_void_p) if w else None for b, w in zip((idx, flags, rec, notes), want)]
    return L.spp_wallet_sync(tree.h if tree else None, pool.h if pool else None, count, deposits, recipients, *outs)


def test_refusals_leave_everything_unchanged(ctx, reference_vks):
    import spp
    from spp import witness as W
    rng = random.Random(6001)
    good = _deposits(rng, 4)
    other_ctx = spp.Context(0)
    try:
        with W.ShieldedPoolMerkleTree(ctx, DEPTH) as tree, W.Pool(ctx, *reference_vks, 16) as pool, \
                W.Pool(other_ctx, *reference_vks, 16) as foreign:
            _, coms, _ = tree.deposit(good)
            pool.import_keys(NULLIFIERS, [7, 8])
            before = (len(tree), tree.getRoot(), tree.find(coms), pool.counts(), tree.sync(good, pool))
            assert before[2] == ([0, 1, 2, 3], [1] * 4)
            buf = W.pack_deposits(good)
            words = b"".join(rng.randrange(R).to_bytes(32, "big") for _ in good)
            unchanged = lambda: (len(tree), tree.getRoot(), tree.find(coms), pool.counts(), tree.sync(good, pool)) == before
            cases = {"secret_key": (R, 5, 6), "amount": (3, R, 6), "randomness": (3, 5, R), "amount does not fit 64 bits": (3, 1 << 64, 6),
                     "secret_key is 0": (0, 5, 6)}
            for what, bad in cases.items():
                batch = good[:2] + [bad] + good[2:]
                assert _raw_sync(ctx.L, tree, pool, 5, W.pack_deposits(batch), None) == BAD_INPUT
                msg = spp.last_error()
                assert "secret 2" in msg and what in msg, (what, msg)
                with pytest.raises(spp.SppError):
                    tree.sync(batch, pool)
                assert unchanged(), what
            bad_words = words[:32] + R.to_bytes(32, "big") + words[64:]
            assert _raw_sync(ctx.L, tree, pool, 4, buf, bad_words, (True, True, True, True)) == BAD_INPUT
            assert "secret 1" in spp.last_error() and "recipient" in spp.last_error()
            assert _raw_sync(ctx.L, tree, pool, 4, buf, bad_words) == BAD_INPUT                       # also when no notes are asked for
            assert _raw_sync(ctx.L, tree, pool, 4, buf, None, (True, True, False, True)) == BAD_INPUT   # notes without recipients
            assert "recipients" in spp.last_error()
            assert _raw_sync(ctx.L, tree, foreign, 4, buf, None) == BAD_INPUT and "another spp_ctx" in spp.last_error()
            assert _raw_sync(ctx.L, tree, pool, (1 << 24) + 1, buf, None) == BAD_INPUT and "2^24" in spp.last_error()
            for tr, dp, want in ((None, buf, (True, True, False, False)), (tree, None, (True, True, False, False)),
                                 (tree, buf, (False, True, False, False)), (tree, buf, (True, False, False, False))):
                assert _raw_sync(ctx.L, tr, pool, 4, dp, None, want) == BAD_INPUT and "NULL" in spp.last_error()
            L = ctx.L
            idx = (ctypes.c_uint64 * 4)()
            p = lambda b: ctypes.cast(b, ctypes.c_void_p)
            assert L.spp_merkle_tree_find(None, 1, bytes(32), None, p(idx), None) == BAD_INPUT
            assert L.spp_merkle_tree_find(tree.h, 1, None, None, p(idx), None) == BAD_INPUT
            assert L.spp_merkle_tree_find(tree.h, 1, bytes(32), None, None, None) == BAD_INPUT and "NULL" in spp.last_error()
            assert L.spp_merkle_tree_find(tree.h, 2, bytes(32) + R.to_bytes(32, "big"), None, p(idx), None) == BAD_INPUT
            assert "leaf value 1" in spp.last_error()
            assert L.spp_merkle_tree_find(tree.h, (1 << 24) + 1, bytes(32), None, p(idx), None) == BAD_INPUT
            assert unchanged() and foreign.counts() == (0, 0)
            # count == 0: OK with every output NULL
            assert L.spp_wallet_sync(tree.h, pool.h, 0, None, None, None, None, None, None) == 0
            assert L.spp_wallet_sync(tree.h, None, 0, None, None, None, None, None, None) == 0
            assert L.spp_merkle_tree_find(tree.h, 0, None, None, None, None) == 0
            assert tree.sync([]) == [] and tree.sync([], pool, []) == ([], [])
            # matches and from are optional
            assert L.spp_merkle_tree_find(tree.h, 4, W._be(coms), None, p(idx), None) == 0 and list(idx) == [0, 1, 2, 3]
            assert unchanged()
    finally:
        other_ctx.close()


def test_cli_wallet_sync_prints_deposit_records(ctx, reference_vks, tmp_path, capsys):
    """`spp.cli wallet-sync` over files: one JSON object per secret with DepositRecord's field names (storage.ts:9-26)"""
    import json
    from spp import cli, witness as W
    rng = random.Random(7001)
    inserted = [rng.randrange(R) for _ in range(2)]
    deps, stranger = _deposits(rng, 5), _deposits(rng, 1)[0]
    with W.ShieldedPoolMerkleTree(ctx, DEPTH) as tree:
        tree.insert_many(inserted)
        _, coms, _ = tree.deposit(deps + [deps[1]])                      # secret 1 sits at leaves 3 and 7
        records = tree.sync(deps + [stranger])
        root, proofs = tree.getRoot(), tree.getProofs([2 + k for k in range(5)])
    paths = {n: str(tmp_path / n) for n in ("secrets.json", "leaves.txt", "spent.txt", "wa.txt", "w.vk", "a.vk")}
    json.dump([{"secretKey": hex(sk), "amount": str(a), "randomness": hex(r)} for sk, a, r in deps + [stranger]], open(paths["secrets.json"], "w"))
    open(paths["leaves.txt"], "w").write("".join("0x%064x\n" % v for v in inserted + coms))
    open(paths["spent.txt"], "w").write("%064x\n" % records[0][3])
    open(paths["wa.txt"], "w").write("%064x\n%064x\n" % (records[2][4], records[5][4]))
    open(paths["w.vk"], "wb").write(reference_vks[0]); open(paths["a.vk"], "wb").write(reference_vks[1])
    assert cli.main(["wallet-sync", paths["secrets.json"], paths["leaves.txt"], "--spent", paths["spent.txt"], "--audited", paths["wa.txt"],
                     "--vk", paths["w.vk"], paths["a.vk"], "--recipient", "0x1234"]) == 0
    out = [json.loads(ln) for ln in capsys.readouterr().out.strip().split("\n")]
    hx = lambda v: "0x%064x" % v
    assert len(out) == 6
    for k, rec in enumerate(out[:5]):
        assert (rec["commitment"], rec["leafIndex"], rec["root"], rec["nullifier"], rec["waCommitment"]) == \
            (hx(coms[k]), 2 + k, hx(root), hx(records[k][3]), hx(records[k][4])), k
        assert rec["siblings"] == [hx(v) for v in proofs[k]] and rec["id"] == rec["commitment"]
        assert (rec["publicKeyX"], rec["publicKeyY"]) == tuple(hx(v) for v in records[k][5])
        assert rec["status"] == ("withdrawn" if k == 0 else "pending") and rec["audited"] == (k == 2)
        assert rec["occurrences"] == (2 if k == 1 else 1) and rec["recipient"] == hx(0x1234)
        assert (rec["secretKey"], rec["amount"], rec["randomness"]) == (hx(deps[k][0]), str(deps[k][1]), hx(deps[k][2]))
    assert (out[5]["leafIndex"], out[5]["status"], out[5]["audited"], out[5]["occurrences"], out[5]["siblings"], out[5]["nullifier"]) == \
        (None, "absent", True, 0, [], None)
    # without --vk: no pool, audited unknown
    assert cli.main(["wallet-sync", paths["secrets.json"], paths["leaves.txt"]]) == 0
    out = [json.loads(ln) for ln in capsys.readouterr().out.strip().split("\n")]
    assert [r["status"] for r in out] == ["pending"] * 5 + ["absent"] and all(r["audited"] is None and "recipient" not in r for r in out)
