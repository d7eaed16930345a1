"""Withdraw proofs from notes against the device-resident Merkle tree (spp_withdraw_rows_from_tree,
spp_prove_withdraw_notes(_device)): the rows against the CPU oracle and the reference's own KAT, the proofs against
spp_prove_batch on the same rows and against the oracle's prover, refusal in place, the root snapshot under concurrent
inserts, argument checks, and a second container with the withdraw ABI (the circuit compiled from the reference's ACIR)."""
import ctypes
import os
import random
import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEPTH = 16
BAD_INPUT = -1
UNSAT = -4


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


def _fresh_notes(rng, count, first_index):
    """count notes with random secrets at indices first_index...: (recipient, amount, secret_key, randomness, index) and their
    commitments H4(owner_x, owner_y, amount, randomness) computed by the oracle (client/merkle.ts:126-133)."""
    from oracle import hashes as H
    notes, leaves = [], []
    for i in range(count):
        sk = rng.randrange(1, 1 << 128)
        owner = H.fixed_base_scalar_mul(sk)
        amount, rnd = rng.randrange(1, 1 << 63), rng.randrange(1 << 253)
        notes.append((rng.randrange(1, 1 << 240), amount, sk, rnd, first_index + i))
        leaves.append(H.poseidon_hash4(owner[0], owner[1], amount, rnd))
    return notes, leaves


@pytest.fixture(scope="module")
def pool(ctx):
    """~300 notes in the oracle's MerkleTree and in a resident tree, with the same leaves."""
    from oracle import hashes as H
    from spp import witness as W
    notes, leaves = _fresh_notes(random.Random(4242), 301, 0)
    orc = H.MerkleTree(DEPTH)
    for leaf in leaves:
        orc.insert(leaf)
    tree = W.ShieldedPoolMerkleTree(ctx, DEPTH)
    assert tree.insert_many(leaves) == 0
    yield dict(notes=notes, oracle=orc, tree=tree)
    tree.close()


def _oracle_row(note, orc):
    from oracle import hashes as H
    recipient, amount, sk, rnd, index = note
    sib = orc.proof(index) if index < (1 << DEPTH) else H.default_hashes(DEPTH)[:DEPTH]
    v = H.withdraw_public_values(sk, amount, rnd, index, sib)
    return [orc.root(), v["nullifier"], recipient, amount, v["wa_commitment"], sk, v["owner_x"], v["owner_y"], rnd, index] + sib


def _rs(count, seed):
    rng = random.Random(seed)
    return [(rng.randrange(1, 1 << 250), rng.randrange(1, 1 << 250)) for _ in range(count)]


def _dev(raw):
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(torch.device("cuda", 0))


def _rs_bytes(rs):
    return b"".join(int(r).to_bytes(32, "big") + int(s).to_bytes(32, "big") for r, s in rs)


def test_rows_of_the_kat_note_equal_the_reference_prover_params(ctx, withdraw_kat):
    """The KAT (client/prover-params.toml) is a one-leaf tree at index 0: its note's row is the KAT, all 26 fields."""
    from oracle import circuit as C, hashes as H
    from spp import witness as W
    f = lambda k: int(withdraw_kat[k], 16) if isinstance(withdraw_kat[k], str) else int(withdraw_kat[k])
    leaf = H.poseidon_hash4(f("owner_x"), f("owner_y"), f("amount"), f("randomness"))
    with W.ShieldedPoolMerkleTree(ctx, DEPTH) as tree:
        assert tree.insert(leaf) == 0
        note = (f("recipient"), f("amount"), f("secret_key"), f("randomness"), f("index"))
        assert f("index") == 0
        rows = tree.withdraw_rows([note])
    assert rows == [C.withdraw_inputs(withdraw_kat)]


def test_rows_equal_the_oracle_at_edge_indices(pool):
    from oracle import hashes as H
    notes, orc, tree = pool["notes"], pool["oracle"], pool["tree"]
    n = len(notes)
    assert len(tree) == n and n % 2 == 1
    query = [notes[i] for i in (0, n - 1, 1, 2, 137, 138)]
    donor = notes[17]
    for index in (n, n + 1, n + 40, 1 << DEPTH, (1 << DEPTH) + 1, (1 << DEPTH) + 2 * n, 1 << 40, (1 << 64) + 3):
        query.append(donor[:4] + (index,))
    rows = tree.withdraw_rows(query)
    for note, row in zip(query, rows):
        assert row == _oracle_row(note, orc), note[4]
        if note[4] >= (1 << DEPTH):
            assert row[10:] == H.default_hashes(DEPTH)[:DEPTH]


def test_proofs_from_notes_equal_prove_batch_and_the_oracle(pool, handle, withdraw_artifacts):
    import spp
    from oracle import native
    notes = pool["notes"][100:170]
    rs = _rs(len(notes), 5)
    proofs, pws, status = handle.prove_withdraw_notes(pool["tree"], notes, rs)
    assert status == [0] * len(notes)
    rows = pool["tree"].withdraw_rows(notes)
    p2, w2, s2 = handle.prove_batch(rows, rs)
    assert s2 == status and p2 == proofs and w2 == pws
    orc = native.Prover(withdraw_artifacts["sppc"], withdraw_artifacts["pk"])
    for i in (0, 23, 64, len(notes) - 1):
        rc, proof, pw = orc.prove(rows[i], *rs[i])
        assert rc == 0 and proofs[i] == proof and pws[i] == pw, i
    vk = open(withdraw_artifacts["vk"], "rb").read()
    assert all(spp.verify(vk, p, w) for p, w in zip(proofs, pws))


def test_device_path_pipelined_equals_the_host_path(pool, handle):
    """Six small calls in flight together (six workspaces), then two 1 100-note calls (large-batch path, body + tail)."""
    notes = pool["notes"]
    sizes = (64, 1, 100, 256, 37, 70)
    calls, off = [], 0
    for k, m in enumerate(sizes):
        calls.append(([notes[(off + i) % len(notes)] for i in range(m)], _rs(m, 100 + k)))
        off += m
    big = [notes[(7 * i) % len(notes)] for i in range(1100)]
    calls += [(big, _rs(1100, 200)), (big, _rs(1100, 201))]

    def run(batch):
        from spp import witness as W
        bufs = []
        for ns, rs in batch:
            m = len(ns)
            d_notes, d_rs = _dev(W.pack_withdraw_notes(ns)), _dev(_rs_bytes(rs))
            outs = (torch.zeros(388 * m, dtype=torch.uint8, device="cuda"), torch.zeros(handle.pw_len * m, dtype=torch.uint8, device="cuda"),
                    torch.ones(m, dtype=torch.int32, device="cuda"))
            handle.prove_withdraw_notes_device(pool["tree"], m, d_notes.data_ptr(), d_rs.data_ptr(), *(o.data_ptr() for o in outs))
            bufs.append((d_notes, d_rs) + outs)
        handle.sync()
        return [(bytes(b[2].cpu().numpy()), bytes(b[3].cpu().numpy()), b[4].cpu().tolist()) for b in bufs]

    for batch in (calls[:6], calls[6:]):
        for (ns, rs), (pb, wb, st) in zip(batch, run(batch)):
            proofs, pws, status = handle.prove_withdraw_notes(pool["tree"], ns, rs)
            assert st == [0] * len(ns) and status == st
            assert pb == b"".join(proofs) and wb == b"".join(pws), len(ns)


def test_bad_notes_are_refused_in_place(pool, handle, withdraw_artifacts, tmp_path):
    import shutil
    import spp
    from spp import witness as W
    notes, tree = pool["notes"], pool["tree"]
    n = len(notes)
    good = [notes[i] for i in (3, 4, 5, 6, 7, 8)]
    bad = {
        1: notes[10][:4] + (11,),                # index of another leaf
        3: notes[12][:4] + (n + 3,),             # past the tree size
        4: notes[13][:4] + (1 << DEPTH,),        # outside the tree
        6: notes[14][:1] + (1 << 64,) + notes[14][2:],   # amount = 2^64
        7: (0,) + notes[15][1:],                 # recipient = 0
    }
    batch, it = [], iter(good)
    for k in range(len(good) + len(bad)):
        batch.append(bad[k] if k in bad else next(it))
    rs = _rs(len(batch), 9)
    proofs, pws, status = handle.prove_withdraw_notes(tree, batch, rs)
    assert [k for k, s in enumerate(status) if s != 0] == sorted(bad)
    gp, gw, gs = handle.prove_withdraw_notes(tree, good, [rs[k] for k in range(len(batch)) if k not in bad])
    assert gs == [0] * len(good)
    assert [proofs[k] for k in range(len(batch)) if k not in bad] == gp
    assert [pws[k] for k in range(len(batch)) if k not in bad] == gw
    vk = open(withdraw_artifacts["vk"], "rb").read()
    assert all(spp.verify(vk, p, w) for p, w in zip(gp, gw))
    # the C entry point reports the refusal
    L = handle.L
    out_p, out_w = ctypes.create_string_buffer(388 * len(batch)), ctypes.create_string_buffer(handle.pw_len * len(batch))
    st = (ctypes.c_int32 * len(batch))()
    rc = L.spp_prove_withdraw_notes(handle.h, tree.h, len(batch), W.pack_withdraw_notes(batch), _rs_bytes(rs),
                                    ctypes.cast(out_p, ctypes.c_void_p), ctypes.cast(out_w, ctypes.c_void_p), ctypes.cast(st, ctypes.c_void_p))
    assert rc == UNSAT and [k for k in range(len(batch)) if st[k]] == sorted(bad)
    # generateProofsFromTree raises naming the first refused note
    wdir = tmp_path / "noir_circuit"
    os.makedirs(wdir / "target")
    shutil.copy(withdraw_artifacts["sppc"], wdir / "target" / "shielded_pool_verifier.sppc")
    shutil.copy(withdraw_artifacts["pk"], wdir / "target" / "shielded_pool_verifier.pk")
    cfg = spp.CircuitConfig(str(wdir), "shielded_pool_verifier")
    with W.ShieldedPoolMerkleTree(spp.proof_helper.helper_context(cfg), DEPTH) as htree:
        htree.insert_many([pool["oracle"].leaves[i] for i in range(n)])
        out = spp.generateProofsFromTree(cfg, htree, good, [rs[k] for k in range(len(batch)) if k not in bad])
        assert [o["proof"] for o in out] == gp and [o["publicWitness"] for o in out] == gw
        with pytest.raises(spp.SppError) as e:
            spp.generateProofsFromTree(cfg, htree, batch, rs)
        assert "note 1 " in str(e.value)
        assert spp.generateProofsFromTree(cfg, htree, []) == []


def test_proofs_carry_the_root_at_call_time_across_inserts(ctx, handle, withdraw_artifacts):
    """An asynchronous call, then 2 000 more leaves at once (the level arrays are reallocated): every proof of the call is
    against the root the tree had when the call was made."""
    from spp import witness as W
    rng = random.Random(31)
    notes, leaves = _fresh_notes(rng, 128, 0)
    from oracle.bn254 import R
    leaves += [rng.randrange(R) for _ in range(1000 - len(leaves))]
    with W.ShieldedPoolMerkleTree(ctx, DEPTH) as tree:
        tree.insert_many(leaves)
        root = tree.getRoot()
        m = len(notes)
        d_notes, d_rs = _dev(W.pack_withdraw_notes(notes)), _dev(_rs_bytes(_rs(m, 77)))
        d_p = torch.zeros(388 * m, dtype=torch.uint8, device="cuda")
        d_w = torch.zeros(handle.pw_len * m, dtype=torch.uint8, device="cuda")
        d_s = torch.ones(m, dtype=torch.int32, device="cuda")
        handle.prove_withdraw_notes_device(tree, m, d_notes.data_ptr(), d_rs.data_ptr(), d_p.data_ptr(), d_w.data_ptr(), d_s.data_ptr())
        assert tree.insert_many([rng.randrange(R) for _ in range(2000)]) == 1000
        handle.sync()
        assert tree.getRoot() != root and len(tree) == 3000
        status = d_s.cpu().tolist()
        pb, wb = bytes(d_p.cpu().numpy()), bytes(d_w.cpu().numpy())
    assert status == [0] * m
    proofs = [pb[388 * i:388 * (i + 1)] for i in range(m)]
    pws = [wb[handle.pw_len * i:handle.pw_len * (i + 1)] for i in range(m)]
    assert all(int.from_bytes(w[12:44], "big") == root for w in pws)
    assert all(ctx.verify_batch(open(withdraw_artifacts["vk"], "rb").read(), proofs, pws))


def test_argument_errors(ctx, handle, pool, audit_artifacts):
    import spp
    from spp import witness as W
    from oracle.bn254 import R
    L = ctx.L
    tree = pool["tree"]
    note = W.pack_withdraw_notes([pool["notes"][0]])
    rsb = bytes(64)
    d_note, d_rs = _dev(note), _dev(rsb)
    d_p, d_w = torch.zeros(388, dtype=torch.uint8, device="cuda"), torch.zeros(handle.pw_len, dtype=torch.uint8, device="cuda")
    d_s = torch.zeros(1, dtype=torch.int32, device="cuda")
    pp, pw, ps = ctypes.create_string_buffer(388), ctypes.create_string_buffer(handle.pw_len), (ctypes.c_int32 * 1)()
    vp = lambda b: ctypes.cast(b, ctypes.c_void_p)

    def dev_call(h, t, count=1, notes_ptr=d_note.data_ptr()):
        return L.spp_prove_withdraw_notes_device(h, t, count, notes_ptr, d_rs.data_ptr(), d_p.data_ptr(), d_w.data_ptr(), d_s.data_ptr())

    def host_call(h, t, count=1, notes=note):
        return L.spp_prove_withdraw_notes(h, t, count, notes, rsb, vp(pp), vp(pw), vp(ps))

    audit = ctx.load_circuit(audit_artifacts["sppc"], audit_artifacts["pk"], 6)
    other = spp.Context(0)
    try:
        assert dev_call(audit.h, tree.h) == BAD_INPUT and host_call(audit.h, tree.h) == BAD_INPUT
        with W.ShieldedPoolMerkleTree(ctx, 20) as t20:
            assert dev_call(handle.h, t20.h) == BAD_INPUT and host_call(handle.h, t20.h) == BAD_INPUT
        with W.ShieldedPoolMerkleTree(other, DEPTH) as foreign:
            assert dev_call(handle.h, foreign.h) == BAD_INPUT and host_call(handle.h, foreign.h) == BAD_INPUT
    finally:
        audit.close()
        other.close()
    assert dev_call(handle.h, None) == BAD_INPUT and dev_call(None, tree.h) == BAD_INPUT
    assert dev_call(handle.h, tree.h, notes_ptr=None) == BAD_INPUT
    assert host_call(handle.h, tree.h, notes=None) == BAD_INPUT
    rows = ctypes.create_string_buffer(26 * 32)
    assert L.spp_withdraw_rows_from_tree(tree.h, 1, note, None) == BAD_INPUT
    # a non-canonical secret_key: refused by the host entry points
    bad = bytearray(note)
    bad[64:96] = R.to_bytes(32, "big")
    assert host_call(handle.h, tree.h, notes=bytes(bad)) == BAD_INPUT
    assert L.spp_withdraw_rows_from_tree(tree.h, 1, bytes(bad), vp(rows)) == BAD_INPUT
    assert "canonical" in spp.last_error()
    # count == 0
    assert dev_call(handle.h, tree.h, count=0) == 0 and host_call(handle.h, tree.h, count=0) == 0
    assert L.spp_withdraw_rows_from_tree(tree.h, 0, note, vp(rows)) == 0
    assert handle.prove_withdraw_notes(tree, []) == ([], [], [])
    # and the same handle still proves
    _, _, status = handle.prove_withdraw_notes(tree, [pool["notes"][0]], [(1, 2)])
    assert status == [0]


def test_acir_compiled_circuit_proves_the_same_notes(ctx, pool, tmp_path):
    """Any container with the withdraw ABI: the circuit compiled from the reference's ACIR (tests/golden/reference_withdraw_acir.json)."""
    from spp import acir
    from oracle import native
    prog = acir.load_program(os.path.join(GOLDEN, "reference_withdraw_acir.json"))
    sppc, pk, vk = (str(tmp_path / ("shielded_pool_verifier." + e)) for e in ("sppc", "pk", "vk"))
    acir.compile_to_sppc(prog, sppc)
    native.setup(sppc, b"\x0b" * 32, pk, vk)
    h = ctx.load_circuit(sppc, pk, 6)
    try:
        assert h.n_inputs == 10 + DEPTH
        notes = pool["notes"][200:240]
        rs = _rs(len(notes), 12)
        proofs, pws, status = h.prove_withdraw_notes(pool["tree"], notes, rs)
        assert status == [0] * len(notes)
        p2, w2, s2 = h.prove_batch(pool["tree"].withdraw_rows(notes), rs)
        assert s2 == status and p2 == proofs and w2 == pws
    finally:
        h.close()
