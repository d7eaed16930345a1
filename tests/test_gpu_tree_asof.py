"""GPU: the resident tree as of an earlier size (spp_merkle_tree_root_at / _proofs_at / _prefix_roots / _find_roots,
spp_withdraw_rows_from_tree_at, spp_prove_withdraw_notes_at(_device), spp_pool_root_sizes, `pool-replay` with commitments).

Every expectation comes from a FRESH oracle.hashes.MerkleTree fed leaves[:n] -- the tree a client holds after n deposits
(client/merkle.ts:146-222), which knows nothing of frontiers or stored nodes.  The oracle's Poseidon and Grumpkin functions are pure;
for the length of this module they are memoised (the same node is asked for by many prefix trees), the files are untouched.
The depth-16 world is the 301 notes of tests/test_gpu_withdraw_notes.py (same seed); its 302 oracle prefix roots are computed once
and shared."""
import ctypes
import functools
import json
import random

import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None

from test_gpu_withdraw_notes import ctx, handle, _fresh_notes, _rs, _dev, _rs_bytes, DEPTH, BAD_INPUT  # noqa: F401

pytestmark = pytest.mark.gpu

NOW = (1 << 64) - 1
R_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617
OK, BAD_ROOT, NULLIFIER_USED = 0, 3, 4
AUDITS = 1
SIZES = (0, 1, 2, 3, 63, 64, 65, 128, 255, 256, 257, 300, 301)


@pytest.fixture(scope="module", autouse=True)
def memoised_oracle():
    from oracle import hashes as H
    saved = H.poseidon_hash2, H.fixed_base_scalar_mul
    H.poseidon_hash2 = functools.lru_cache(maxsize=None)(saved[0])
    H.fixed_base_scalar_mul = functools.lru_cache(maxsize=None)(saved[1])
    yield
    H.poseidon_hash2, H.fixed_base_scalar_mul = saved


def _prefix_tree(leaves, n, depth):
    """a fresh oracle tree holding the first n leaves"""
    from oracle import hashes as H
    t = H.MerkleTree(depth)
    for v in leaves[:n]:
        t.insert(v)
    return t


@pytest.fixture(scope="module")
def world(ctx):
    """the 301 notes, their leaves in a resident tree, prefix(n) = the oracle's tree of the first n leaves (kept), roots[n] for all n"""
    from spp import witness as W
    notes, leaves = _fresh_notes(random.Random(4242), 301, 0)
    kept = {}

    def prefix(n):
        if n not in kept:
            kept[n] = _prefix_tree(leaves, n, DEPTH)
        return kept[n]
    roots = [_prefix_tree(leaves, n, DEPTH).root() for n in range(len(leaves) + 1)]
    tree = W.ShieldedPoolMerkleTree(ctx, DEPTH)
    assert tree.insert_many(leaves) == 0
    yield dict(notes=notes, leaves=leaves, tree=tree, prefix=prefix, roots=roots)
    tree.close()


def _row_at(note, orc):
    """the withdraw row of `note` against the oracle tree `orc` (client/payroll-demo.ts:323-340), field by field"""
    from oracle import hashes as H
    recipient, amount, sk, rnd, index = note
    sib = orc.proof(index) if index < (1 << orc.depth) else H.default_hashes(orc.depth)[:orc.depth]
    owner = H.fixed_base_scalar_mul(sk)
    return [orc.root(), H.poseidon_hash2(sk, index), recipient, amount, H.poseidon_hash2(owner[0], owner[1]), sk, owner[0], owner[1], rnd,
            index] + sib


def _note_at(notes, index):
    """the note of leaf `index`, or note 17's secrets under an index that is no leaf of the 301"""
    return notes[index] if index < len(notes) else notes[17][:4] + (index,)


def _edge_indices(size):
    """0, the last two leaves of the prefix, per level the index whose sibling is the frontier node and the one whose sibling is the
    node just past it, two indices absent from the prefix, 2^16 and 2^40"""
    idx = {0, size, size + 40, 1 << DEPTH, 1 << 40}
    idx.update(i for i in (size - 1, size - 2) if i >= 0)
    if size:
        for l in range(DEPTH):
            p = (size - 1) >> l
            idx.add((p ^ 1) << l)
            idx.add(((p + 1) ^ 1) << l)
    return sorted(idx)


@pytest.mark.parametrize("depth", [3, 5])
def test_exhaustive_small_trees(ctx, depth):
    """a full tree of 2^depth leaves, some of them zero: every size 0..2^depth, every index"""
    from spp import witness as W
    rng = random.Random(500 + depth)
    full = 1 << depth
    leaves = [0 if rng.random() < 0.2 else rng.randrange(R_MOD) for _ in range(full)]
    leaves[full - 1] = rng.randrange(1, R_MOD)
    assert leaves.count(0) >= 1
    every = list(range(full))
    with W.ShieldedPoolMerkleTree(ctx, depth) as tree:
        assert tree.insert_many(leaves[:full // 2 + 1]) == 0
        for stored in (full // 2 + 1, full):              # the tree half full, then full: the answers for n <= stored are the same
            if stored == full:
                tree.insert_many(leaves[full // 2 + 1:])
            want_roots = []
            for n in range(stored + 1):
                orc = _prefix_tree(leaves, n, depth)
                want_roots.append(orc.root())
                assert tree.root_at(n) == orc.root(), (stored, n)
                assert tree.proofs_at(n, every) == [orc.proof(i) for i in every], (stored, n)
            assert tree.prefix_roots() == want_roots
            assert tree.prefix_roots(3, stored - 3) == want_roots[3:stored]
            assert tree.root_at(stored) == tree.getRoot() == tree.root_at(NOW)
            assert tree.proofs_at(stored, every, raw=True) == tree.getProofs(every, raw=True)


def test_depth16_roots_paths_and_rows_at_edge_sizes_and_indices(world):
    notes, tree, prefix = world["notes"], world["tree"], world["prefix"]
    assert len(tree) == 301
    assert tree.prefix_roots() == world["roots"]
    for size in SIZES + (NOW,):
        n = 301 if size == NOW else size
        orc = prefix(n)
        assert orc.root() == world["roots"][n]
        assert tree.root_at(size) == orc.root(), size
        idx = _edge_indices(n)
        inside = [i for i in idx if i < (1 << DEPTH)]
        assert tree.proofs_at(size, inside) == [orc.proof(i) for i in inside], size
        query = [_note_at(notes, i) for i in idx]
        rows = tree.withdraw_rows(query, size=size)
        for note, row in zip(query, rows):
            assert row == _row_at(note, orc), (size, note[4])


def test_size_now_and_the_trees_own_size_give_the_existing_calls_bytes(world):
    from spp import witness as W
    notes, tree = world["notes"], world["tree"]
    idx = [i for i in _edge_indices(301) if i < (1 << DEPTH)]
    query = [_note_at(notes, i) for i in _edge_indices(301)]
    rows = tree.withdraw_rows(query)
    paths = tree.getProofs(idx, raw=True)
    for size in (NOW, 301):
        assert tree.root_at(size) == tree.getRoot()
        assert tree.proofs_at(size, idx, raw=True) == paths
        assert tree.withdraw_rows(query, size=size) == rows
    # the raw bytes of the C call, not only the integers
    buf = W.pack_withdraw_notes(query)
    a, b = ctypes.create_string_buffer(26 * 32 * len(query)), ctypes.create_string_buffer(26 * 32 * len(query))
    L = tree.ctx.L
    assert L.spp_withdraw_rows_from_tree(tree.h, len(query), buf, ctypes.cast(a, ctypes.c_void_p)) == 0
    assert L.spp_withdraw_rows_from_tree_at(tree.h, 301, len(query), buf, ctypes.cast(b, ctypes.c_void_p)) == 0
    assert a.raw == b.raw


@pytest.mark.parametrize("start", [301, 900])
def test_answers_at_size_137_do_not_change_when_leaves_arrive(ctx, world, start):
    """200 more leaves: 301 -> 501 inside the first reservation, 900 -> 1100 across a growth of the level arrays (1024)"""
    from spp import witness as W
    rng = random.Random(start)
    notes, leaves = world["notes"], world["leaves"]
    more = [rng.randrange(R_MOD) for _ in range(start - 301 + 200)]
    idx = [i for i in _edge_indices(137) if i < (1 << DEPTH)]
    query = [_note_at(notes, i) for i in _edge_indices(137)]
    with W.ShieldedPoolMerkleTree(ctx, DEPTH) as tree:
        tree.insert_many(leaves + more[:start - 301])
        assert len(tree) == start
        before = (tree.root_at(137), tree.proofs_at(137, idx, raw=True), tree.withdraw_rows(query, size=137), tree.prefix_roots(130, 10))
        assert before[0] == world["roots"][137] and before[2][0] == _row_at(query[0], world["prefix"](137))
        root_then = tree.getRoot()
        assert tree.insert_many(more[start - 301:]) == start
        assert len(tree) == start + 200 and tree.getRoot() != root_then
        after = (tree.root_at(137), tree.proofs_at(137, idx, raw=True), tree.withdraw_rows(query, size=137), tree.prefix_roots(130, 10))
        assert after == before
        assert tree.root_at(start) == root_then


def test_proofs_at_size_137_equal_prove_batch_on_the_oracles_rows(world, handle, withdraw_artifacts):
    """5 notes through the host form; 70 (body of 64 and a tail) through the device form, one of them a leaf of the tree but not of
    the prefix: refused in place, its neighbours proved"""
    import spp
    from spp import witness as W
    notes, tree, orc = world["notes"], world["tree"], world["prefix"](137)
    vk = open(withdraw_artifacts["vk"], "rb").read()
    five = [notes[i] for i in (0, 64, 100, 135, 136)]
    rs5 = _rs(5, 21)
    proofs, pws, status = handle.prove_withdraw_notes(tree, five, rs5, size=137)
    assert status == [0] * 5
    p2, w2, s2 = handle.prove_batch([_row_at(n, orc) for n in five], rs5)
    assert (p2, w2, s2) == (proofs, pws, status)
    assert all(int.from_bytes(w[12:44], "big") == orc.root() for w in pws) and orc.root() != tree.getRoot()
    assert all(spp.verify(vk, p, w) for p, w in zip(proofs, pws))
    batch = [notes[i] for i in range(70)]
    batch[33] = notes[200]                                   # leaf 200 exists, the prefix of 137 does not hold it
    rs = _rs(70, 22)
    d_notes, d_rs = _dev(W.pack_withdraw_notes(batch)), _dev(_rs_bytes(rs))
    d_p = torch.zeros(388 * 70, dtype=torch.uint8, device="cuda")
    d_w = torch.zeros(handle.pw_len * 70, dtype=torch.uint8, device="cuda")
    d_s = torch.ones(70, dtype=torch.int32, device="cuda")
    handle.prove_withdraw_notes_device(tree, 70, d_notes.data_ptr(), d_rs.data_ptr(), d_p.data_ptr(), d_w.data_ptr(), d_s.data_ptr(), size=137)
    handle.sync()
    st = d_s.cpu().tolist()
    pb, wb = bytes(d_p.cpu().numpy()), bytes(d_w.cpu().numpy())
    assert [k for k, s in enumerate(st) if s != 0] == [33]
    p3, w3, s3 = handle.prove_batch([_row_at(n, orc) for n in batch], rs)
    assert [k for k, s in enumerate(s3) if s != 0] == [33]
    good = [k for k in range(70) if k != 33]
    assert [pb[388 * k:388 * (k + 1)] for k in good] == [p3[k] for k in good]
    assert [wb[handle.pw_len * k:handle.pw_len * (k + 1)] for k in good] == [w3[k] for k in good]
    assert all(tree.ctx.verify_batch(vk, [p3[k] for k in good], [w3[k] for k in good]))
    # the host form refuses the same note in place
    _, _, s4 = handle.prove_withdraw_notes(tree, batch[32:35], rs[32:35], size=137)
    assert [bool(s) for s in s4] == [False, True, False]


def test_find_roots(ctx, world):
    from spp import witness as W
    tree, roots, leaves = world["tree"], world["roots"], world["leaves"]
    assert len(set(roots)) == 302
    sizes, matches = tree.find_roots(roots)
    assert sizes == list(range(302)) and matches == [1] * 302
    assert tree.find_roots([tree.getRoot()]) == ([301], [1])
    other = _prefix_tree(leaves[1:], 40, DEPTH).root()       # the root of a different tree
    strangers = [other, 0, R_MOD, (1 << 256) - 1, roots[5] + R_MOD]     # ... an all-zero word, r, 2^256 - 1, a root plus r
    assert tree.find_roots(strangers + [roots[7]]) == ([None] * 5 + [7], [0] * 5 + [1])
    rng = random.Random(77)
    a, b, c = (rng.randrange(1, R_MOD) for _ in range(3))
    with W.ShieldedPoolMerkleTree(ctx, DEPTH) as t:
        t.insert_many([a, b, 0, 0, c])
        want = [_prefix_tree([a, b, 0, 0, c], n, DEPTH).root() for n in range(6)]
        assert want[2] == want[3] == want[4] and len(set(want)) == 4
        assert t.find_roots(want) == ([0, 1, 2, 2, 2, 5], [1, 1, 3, 3, 3, 1])
        # more leaves arrive: the index is extended (a zero leaf right after c repeats the root of size 5)
        t.insert_many([0] + [rng.randrange(1, R_MOD) for _ in range(60)])
        assert len(t) == 66
        assert t.find_roots(want) == ([0, 1, 2, 2, 2, 5], [1, 1, 3, 3, 3, 2])
        assert t.find_roots([t.getRoot()]) == ([66], [1])
    with W.ShieldedPoolMerkleTree(ctx, DEPTH) as t:
        t.insert_many([0])
        empty = _prefix_tree([], 0, DEPTH).root()
        assert t.getRoot() == empty and t.find_roots([empty]) == ([0], [2])
    # the same answers on the big tree after more leaves arrived there too (a tree of its own: `world` stays at 301)
    with W.ShieldedPoolMerkleTree(ctx, DEPTH) as t:
        t.insert_many(leaves[:150])
        assert t.find_roots(roots[:151] + roots[151:160]) == (list(range(151)) + [None] * 9, [1] * 151 + [0] * 9)
        t.insert_many(leaves[150:])
        assert t.find_roots(roots) == (list(range(302)), [1] * 302)


def test_pool_root_sizes_and_proving_at_the_size_the_pool_accepts(ctx, world, handle, withdraw_artifacts, audit_artifacts):
    from spp import witness as W
    notes, leaves, roots = world["notes"], world["leaves"], world["roots"]
    wvk, avk = open(withdraw_artifacts["vk"], "rb").read(), open(audit_artifacts["vk"], "rb").read()
    rng = random.Random(88)
    addresses = [rng.getrandbits(256).to_bytes(32, "big") for _ in range(2)]
    mine = [(W.recipient_word(addresses[k]),) + notes[i][1:] for k, i in enumerate((5, 38))]
    with W.ShieldedPoolMerkleTree(ctx, DEPTH) as tree, W.Pool(ctx, wvk, avk, 64) as pool, W.Pool(ctx, wvk, avk, 64) as fresh:
        tree.insert_many(leaves[:40])
        assert fresh.root_sizes(tree) == ([None] * 33, None)
        pool.add_roots(roots[1:41])                          # 40 deposits, each pushing the root after it: the ring wraps
        sizes, best = pool.root_sizes(tree)
        assert best == 40 and sizes[0] == 40
        assert sizes[1:] == list(range(33, 41)) + list(range(9, 33))
        state = pool.state()
        by_root = {r.to_bytes(32, "big"): n for n, r in enumerate(roots)}
        assert sizes == [by_root[state[8 + 32 * k:40 + 32 * k]] for k in range(33)]
        # the service runs ahead of the chain: five leaves that nobody pushed a root for
        tree.insert_many(leaves[40:45])
        assert pool.root_sizes(tree) == (sizes, 40) and pool.state() == state and len(tree) == 45
        rs = _rs(2, 23)
        proofs, pws, status = handle.prove_withdraw_notes(tree, mine, rs, size=best)
        assert status == [0, 0]
        pool.import_keys(AUDITS, [w[140:172] for w in pws])
        late = handle.prove_withdraw_notes(tree, mine, rs, size=NOW)
        assert late[2] == [0, 0] and late[:2] == handle.prove_withdraw_notes(tree, mine, rs)[:2]
        assert pool.withdraw(late[0], late[1], addresses)[0] == [BAD_ROOT, BAD_ROOT]
        assert pool.withdraw(proofs, pws, addresses)[0] == [OK, OK]
        assert pool.withdraw(proofs, pws, addresses)[0] == [NULLIFIER_USED, NULLIFIER_USED]
        # a depositor who never saw leaf 40 pushes the root of leaves 0..39 plus leaf 41
        stale = _prefix_tree(leaves[:40] + [leaves[41]], 41, DEPTH).root()
        pool.add_roots([stale])
        sizes2, best2 = pool.root_sizes(tree)
        assert best2 == 40 and sizes2[0] is None
        assert sizes2[1:] == list(range(33, 41)) + [None] + list(range(10, 33))
        assert fresh.root_sizes(tree) == ([None] * 33, None)


@pytest.fixture(scope="module")
def audit_handle(ctx, audit_artifacts):
    h = ctx.load_circuit(audit_artifacts["sppc"], audit_artifacts["pk"], 6)
    yield h
    h.close()


def test_refusals_leave_tree_and_pool_unchanged(ctx, world, handle, audit_handle, withdraw_artifacts, audit_artifacts):
    import spp
    from spp import witness as W
    notes, tree = world["notes"], world["tree"]
    L = ctx.L
    wvk, avk = open(withdraw_artifacts["vk"], "rb").read(), open(audit_artifacts["vk"], "rb").read()
    root, size = tree.getRoot(), len(tree)
    note = W.pack_withdraw_notes([notes[0]])
    out = ctypes.create_string_buffer(1 << 16)
    vp = ctypes.cast(out, ctypes.c_void_p)
    st = (ctypes.c_int32 * 1)()
    d_note, d_rs = _dev(note), _dev(bytes(64))
    d_out = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    dev_at = lambda h, t, sz, count=1: L.spp_prove_withdraw_notes_at_device(h, t, sz, count, d_note.data_ptr(), d_rs.data_ptr(), d_out.data_ptr(),
                                                                            d_out.data_ptr() + 512, d_out.data_ptr() + 768)
    host_at = lambda h, t, sz, count=1: L.spp_prove_withdraw_notes_at(h, t, sz, count, note, bytes(64), vp, vp, st)
    q = (ctypes.c_uint64 * 1)(0)
    too_large = (lambda: L.spp_merkle_tree_root_at(tree.h, 302, vp),
                 lambda: L.spp_merkle_tree_proofs_at(tree.h, 302, 1, q, vp),
                 lambda: L.spp_merkle_tree_proofs_at(tree.h, 1 << 40, 0, None, None),
                 lambda: L.spp_withdraw_rows_from_tree_at(tree.h, 302, 1, note, vp),
                 lambda: L.spp_withdraw_rows_from_tree_at(tree.h, NOW - 1, 0, note, vp),
                 lambda: dev_at(handle.h, tree.h, 302), lambda: dev_at(handle.h, tree.h, 302, 0),
                 lambda: host_at(handle.h, tree.h, 302), lambda: host_at(handle.h, tree.h, 5000, 0))
    for k, call in enumerate(too_large):
        assert call() == BAD_INPUT, k
        msg = spp.last_error()
        assert "301" in msg and ("302" in msg or "5000" in msg or str(1 << 40) in msg or str(NOW - 1) in msg), (k, msg)
    for first, count in ((302, 1), (301, 2), (0, 303), (NOW, 2), (302, 0)):
        assert L.spp_merkle_tree_prefix_roots(tree.h, first, count, vp) == BAD_INPUT, (first, count)
        assert "301" in spp.last_error()
    assert L.spp_merkle_tree_prefix_roots(tree.h, 301, 1, vp) == 0 and L.spp_merkle_tree_prefix_roots(tree.h, 301, 0, None) == 0
    assert L.spp_merkle_tree_proofs_at(tree.h, 7, 1, (ctypes.c_uint64 * 1)(1 << DEPTH), vp) == BAD_INPUT       # as spp_merkle_tree_proofs
    bad = bytearray(note)
    bad[64:96] = R_MOD.to_bytes(32, "big")
    assert L.spp_withdraw_rows_from_tree_at(tree.h, 7, 1, bytes(bad), vp) == BAD_INPUT and "canonical" in spp.last_error()
    assert host_at(audit_handle.h, tree.h, 7) == BAD_INPUT and dev_at(audit_handle.h, tree.h, 7) == BAD_INPUT    # not a withdraw circuit
    assert "withdraw circuit" in spp.last_error()
    other = spp.Context(0)
    try:
        with W.ShieldedPoolMerkleTree(other, DEPTH) as foreign, W.Pool(ctx, wvk, avk, 8) as pool:
            foreign.insert_many(world["leaves"][:3])
            assert host_at(handle.h, foreign.h, 2) == BAD_INPUT and dev_at(handle.h, foreign.h, 2) == BAD_INPUT
            assert "another context" in spp.last_error()
            pool.add_roots([world["roots"][3]])
            state = pool.state()
            sizes = (ctypes.c_uint64 * 33)()
            assert L.spp_pool_root_sizes(pool.h, foreign.h, sizes, None) == BAD_INPUT and "another spp_ctx" in spp.last_error()
            assert L.spp_pool_root_sizes(pool.h, tree.h, None, None) == BAD_INPUT
            assert pool.state() == state and pool.counts() == (0, 0)
            assert foreign.getRoot() == world["roots"][3] and len(foreign) == 3
            assert pool.root_sizes(tree) == ([3] + [3] + [None] * 31, 3)     # ... and the same objects still answer
    finally:
        other.close()
    # count == 0 with a good size, and nothing changed
    assert dev_at(handle.h, tree.h, 7, 0) == 0 and host_at(handle.h, tree.h, 7, 0) == 0
    assert L.spp_withdraw_rows_from_tree_at(tree.h, 7, 0, note, vp) == 0 and L.spp_merkle_tree_proofs_at(tree.h, 7, 0, None, None) == 0
    assert L.spp_merkle_tree_find_roots(tree.h, 0, None, None, None) == 0
    assert tree.getRoot() == root and len(tree) == size and tree.root_at(301) == root


def test_cli_pool_replay_names_the_stale_deposit_and_the_withdraw_against_it(ctx, handle, audit_handle, withdraw_artifacts, audit_artifacts, rlwe_pk,
                                                                             tmp_path, capsys):
    """Two depositors build on the same two leaves: the second one's root omits the first one's leaf.  12 instructions, the stale root
    pushed by line 6 and the withdraw proved against it on line 8."""
    from spp import cli, witness as W, workload
    rng = random.Random(99)
    sks, r8, e18, e28 = workload.audit_noise(900, 3)
    sks = list(sks) + [rng.randrange(1, 1 << 128) for _ in range(2)]
    amounts = [rng.randrange(1, 1 << 63) for _ in range(5)]
    rnds = [rng.randrange(1 << 253) for _ in range(5)]
    addresses = [rng.getrandbits(256).to_bytes(32, "big") for _ in range(3)]
    note = lambda i, index: (W.recipient_word(addresses[i]), amounts[i], sks[i], rnds[i], index)
    with W.ShieldedPoolMerkleTree(ctx, DEPTH) as chain, W.ShieldedPoolMerkleTree(ctx, DEPTH) as second:
        _, com, honest = chain.deposit([(sks[i], amounts[i], rnds[i]) for i in range(5)])
        second.insert_many([com[0], com[1], com[3]])         # the view of the depositor of leaf 3, who never saw leaf 2
        stale = second.getRoot()
        assert stale not in honest
        w0 = handle.prove_withdraw_notes(chain, [note(0, 0)], [(3, 5)], size=2)
        w1 = handle.prove_withdraw_notes(second, [note(1, 1)], [(7, 9)])
        w2 = handle.prove_withdraw_notes(chain, [note(2, 2)], [(11, 13)], size=3)
        assert w0[2] == w1[2] == w2[2] == [0]
    ap, aw, st, _, _ = audit_handle.prove_audit_records(rlwe_pk["a"], rlwe_pk["b"], sks[:3], r8, e18, e28, [(17 * i + 7, 19 * i + 9) for i in range(3)])
    assert st == [0] * 3
    be = lambda v: "%064x" % v
    dep = lambda k, root: {"deposit": {"root": be(root), "commitment": "0x" + be(com[k])}}
    aud = lambda i: {"submit_audit": {"proof": ap[i].hex(), "pw": aw[i].hex()}}
    wd = lambda w, i: {"withdraw": {"proof": w[0][0].hex(), "pw": w[1][0].hex(), "recipient": addresses[i].hex()}}
    log = [dep(0, honest[0]), dep(1, honest[1]), aud(0), wd(w0, 0), dep(2, honest[2]), dep(3, stale), aud(1), wd(w1, 1), aud(2), wd(w2, 2),
           wd(w0, 0), dep(4, honest[4])]
    assert len(log) == 12
    path = str(tmp_path / "log.jsonl")
    open(path, "w").write("".join(json.dumps(x) + "\n" for x in log))
    assert cli.main(["pool-replay", withdraw_artifacts["vk"], audit_artifacts["vk"], path]) == 0
    lines = capsys.readouterr().out.split("\n")
    assert lines[:12] == ["OK root-of-leaves", "OK root-of-leaves", "OK", "OK size 2", "OK root-of-leaves", "OK NOT-root-of-leaves", "OK",
                          "OK foreign", "OK", "OK size 3", "NULLIFIER_USED", "OK root-of-leaves"]
    assert lines[12].startswith("roots: 5 deposits, 1 pushed a root that is not the root of the leaves; 3 withdraws accepted, 1 against")
    assert lines[13:] == [""]
    # the same log without the commitments: the lines of before
    for x in log:
        x.get("deposit", {}).pop("commitment", None)
    open(path, "w").write("".join(json.dumps(x) + "\n" for x in log))
    assert cli.main(["pool-replay", withdraw_artifacts["vk"], audit_artifacts["vk"], path]) == 0
    assert capsys.readouterr().out.split("\n") == ["OK", "OK", "OK", "OK", "OK", "OK", "OK", "OK", "OK", "OK", "NULLIFIER_USED", "OK", ""]
