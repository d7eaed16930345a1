"""GPU: withdrawals from notes (spp_prove_withdrawals) -- the withdraw proof of every note and one audit record per identity the
pool does not hold yet -- against the calls it is made of (prove_withdraw_notes, prove_audit_records: byte for byte), the plan model
of tests/test_withdrawal_plan_host.py, the pool ledger and the oracle's verifier.  12 deposits over 5 secret keys in the pattern
0,1,0,2,1,3,0,4,2,0,1,3, then 4 further ones (three known identities, one new); noise from workload.audit_noise, one row per NOTE.
6-bit tables, as tests/test_gpu_pool.py."""
import ctypes
import json
import os
import random

import numpy as np
import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None

from conftest import GOLDEN
from test_withdrawal_plan_host import plan_model, RESIDENT

pytestmark = pytest.mark.gpu

PATTERN = [0, 1, 0, 2, 1, 3, 0, 4, 2, 0, 1, 3]
MORE = [2, 5, 0, 4]                     # the second call: identities 2, 0, 4 are known by then, 5 is new
N, M = len(PATTERN), len(MORE)
FIRST = 900
OK, BAD_PROOF = 0, 6
UNSAT = -4
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
Q = 167772161


@pytest.fixture(scope="module")
def ctx():
    import spp
    c = spp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def handles(ctx, withdraw_artifacts, audit_artifacts):
    hw = ctx.load_circuit(withdraw_artifacts["sppc"], withdraw_artifacts["pk"], 6)
    ha = ctx.load_circuit(audit_artifacts["sppc"], audit_artifacts["pk"], 6)
    yield hw, ha
    hw.close()
    ha.close()


@pytest.fixture(scope="module")
def world(ctx, withdraw_artifacts, audit_artifacts, rlwe_pk):
    """16 notes (12 + 4) with their addresses, per-note noise and blinding, the tree they go into (empty) and the two keys"""
    from spp import witness as W_, workload
    rng = random.Random(4242)
    ids, r8, e18, e28 = workload.audit_noise(FIRST, N + M)
    sks = [ids[p] for p in PATTERN + MORE]
    amounts = [rng.randrange(1, 1 << 63) for _ in sks]
    rnds = [rng.randrange(1 << 253) for _ in sks]
    addresses = [rng.getrandbits(256).to_bytes(32, "big") for _ in sks]
    notes = [(W_.recipient_word(addresses[i]), amounts[i], sks[i], rnds[i], i) for i in range(N + M)]
    tree = W_.ShieldedPoolMerkleTree(ctx, 16)
    w = dict(sks=sks, deposits=[(sks[i], amounts[i], rnds[i]) for i in range(N + M)], notes=notes, addresses=addresses, r=r8, e1=e18, e2=e28,
             rs_w=[(11 * i + 3, 13 * i + 5) for i in range(N + M)], rs_a=[(17 * i + 7, 19 * i + 9) for i in range(N + M)], tree=tree,
             pk=(rlwe_pk["a"], rlwe_pk["b"]), wvk=open(withdraw_artifacts["vk"], "rb").read(), avk=open(audit_artifacts["vk"], "rb").read())
    yield w
    tree.close()


def _prove(handles, world, idx, pool=None, size=None, notes=None, noise=True, **kw):
    """prove_withdrawals over the notes idx of the world, everything per note taken at those indices"""
    import spp
    hw, ha = handles
    sel = lambda a: None if not noise else np.ascontiguousarray(a[idx])
    return spp.prove_withdrawals(hw, ha, world["tree"], notes or [world["notes"][i] for i in idx], world["pk"][0], world["pk"][1],
                                 sel(world["r"]), sel(world["e1"]), sel(world["e2"]), pool=pool, size=size,
                                 rs_withdraw=[world["rs_w"][i] for i in idx], rs_audit=[world["rs_a"][i] for i in idx], **kw)


def _composed(handles, world, idx, reps, size=None, notes=None):
    """the same from the two calls it is made of: the withdraw proofs of the notes, the audit records of the representatives"""
    hw, ha = handles
    wp = hw.prove_withdraw_notes(world["tree"], notes or [world["notes"][i] for i in idx], [world["rs_w"][i] for i in idx], size=size)
    ap = ha.prove_audit_records(world["pk"][0], world["pk"][1], [world["sks"][i] for i in reps], world["r"][reps], world["e1"][reps],
                                world["e2"][reps], [world["rs_a"][i] for i in reps])
    return wp, ap


def _same_as_composed(bundle, wp, ap):
    assert (bundle.proofs, bundle.pws, bundle.status) == wp
    assert (bundle.audit_proofs, bundle.audit_pws, bundle.audit_status) == ap[:3]
    assert np.array_equal(bundle.c0, ap[3]) and np.array_equal(bundle.c1, ap[4])


@pytest.fixture(scope="module")
def scenario(ctx, handles, world):
    """cases 1 and 2 on one pool: 12 deposits, the bundle of their notes, its log settled; 4 further deposits, their bundle, settled"""
    from spp import witness as W_
    tree, out = world["tree"], {}
    first, commitments, roots = tree.deposit(world["deposits"][:N])
    assert first == 0
    pool = W_.Pool(ctx, world["wvk"], world["avk"], 64)
    try:
        pool.add_roots(roots)
        idx = list(range(N))
        out["b1"] = _prove(handles, world, idx, pool)
        out["composed1"] = _composed(handles, world, idx, out["b1"].audit_note)
        out["log1"] = out["b1"].log(world["addresses"][:N])
        out["settled1"] = pool.settle_log(out["log1"])
        out["counts1"] = pool.counts()
        _, more_commitments, roots2 = tree.deposit(world["deposits"][N:])
        pool.add_roots(roots2)
        idx2 = list(range(N, N + M))
        out["b2"] = _prove(handles, world, idx2, pool)
        out["log2"] = out["b2"].log(world["addresses"][N:])
        out["settled2"] = pool.settle_log(out["log2"])
        out["counts2"] = pool.counts()
    finally:
        pool.close()
    out["leaves"] = commitments + more_commitments
    out["root16"] = roots2[-1]
    return out


def test_fresh_pool_one_record_per_identity_bytes_of_the_two_calls_and_the_log_settles(scenario, world):
    from oracle import groth16
    b = scenario["b1"]
    first = [PATTERN.index(k) for k in range(5)]
    assert b.n_audits == 5 and b.audit_note == first == [0, 1, 3, 5, 7]
    assert (b.audit_of, b.audit_note) == plan_model([w[140:172] for w in b.pws])
    assert b.audit_of == PATTERN                                          # identity k first occurs in order of k
    assert b.status == [0] * N and b.audit_status == [0] * 5
    _same_as_composed(b, *scenario["composed1"])
    for s, i in enumerate(b.audit_note):                                   # the record's identity is the note's
        assert b.audit_pws[s][12:44] == b.pws[i][140:172]
    log = scenario["log1"]
    assert len(log) == 17 and [ins[0] for ins in log[:4]] == ["submit_audit", "withdraw", "submit_audit", "withdraw"]
    assert [k for k, ins in enumerate(log) if ins[0] == "submit_audit"] == [i + s for s, i in enumerate(first)]
    codes, amounts = scenario["settled1"]
    assert codes == [OK] * 17 and scenario["counts1"] == (12, 5)
    assert [a for a, ins in zip(amounts, log) if ins[0] == "withdraw"] == [n[1] for n in world["notes"][:N]]
    for k in (0, 11):
        assert groth16.verify(world["wvk"], b.proofs[k], b.pws[k])
    for s in (0, 4):
        assert groth16.verify(world["avk"], b.audit_proofs[s], b.audit_pws[s])


def test_second_call_on_that_pool_proves_only_the_new_identity(scenario):
    b = scenario["b2"]
    assert b.n_audits == 1 and b.audit_note == [1] and b.audit_of == [RESIDENT, 0, RESIDENT, RESIDENT]
    assert b.status == [0] * M and b.audit_status == [0]
    log = scenario["log2"]
    assert [ins[0] for ins in log] == ["withdraw", "submit_audit", "withdraw", "withdraw", "withdraw"]
    assert scenario["settled2"][0] == [OK] * 5 and scenario["counts2"] == (16, 6)


def test_without_a_pool_the_plan_is_the_in_batch_plan(scenario, handles, world):
    idx = [0, 1, 2, 3, 4, 5]                                               # identities 0,1,0,2,1,3 -- all resident in the scenario's pool
    b = _prove(handles, world, idx)
    assert (b.audit_of, b.audit_note) == ([0, 1, 0, 2, 1, 3], [0, 1, 3, 5]) == plan_model([w[140:172] for w in b.pws])
    assert b.status == [0] * 6 and b.audit_status == [0] * 4
    _same_as_composed(b, *_composed(handles, world, idx, b.audit_note))


def test_a_refused_note_is_still_the_representative_of_its_identity(scenario, ctx, handles, world):
    from spp import witness as W_
    idx = [3, 8, 1]                                                        # identities 2, 2, 1
    wrong = world["notes"][3][:4] + (6,)                                   # leaf 6 is another note
    notes = [wrong, world["notes"][8], world["notes"][1]]
    b = _prove(handles, world, idx, notes=notes)
    assert b.status == [UNSAT, 0, 0] and b.proofs[0] == bytes(388) and b.proofs[1] != bytes(388)
    assert (b.audit_of, b.audit_note) == ([0, 0, 1], [0, 2]) and b.audit_status == [0, 0]
    _same_as_composed(b, *_composed(handles, world, idx, [3, 1], notes=notes))
    assert b.audit_pws[0][12:44] == b.pws[1][140:172]                      # the record of the refused note serves note 8
    with W_.Pool(ctx, world["wvk"], world["avk"], 8) as pool:
        pool.add_roots([scenario["root16"]])
        log = b.log([world["addresses"][i] for i in idx])
        assert [ins[0] for ins in log] == ["submit_audit", "withdraw", "withdraw", "submit_audit", "withdraw"]
        assert pool.settle_log(log)[0] == [OK, BAD_PROOF, OK, OK, OK] and pool.counts() == (2, 2)


def test_as_of_the_size_four_deposits_earlier(scenario, handles, world):
    tree = world["tree"]
    assert len(tree) == N + M
    idx = [10, 12, 11, 15]                                                 # notes 12 and 15 are past that size
    b = _prove(handles, world, idx, size=N)
    root = tree.root_at(N).to_bytes(32, "big")
    assert root != scenario["root16"].to_bytes(32, "big")
    assert [w[12:44] for w in b.pws] == [root] * 4
    assert b.status == [0, UNSAT, 0, UNSAT] and b.proofs[1] == b.proofs[3] == bytes(388)
    assert (b.audit_of, b.audit_note) == ([0, 1, 2, 3], [0, 1, 2, 3])      # identities 1, 2, 3, 4
    _same_as_composed(b, *_composed(handles, world, idx, idx, size=N))
    assert _prove(handles, world, idx, size=ctypes.c_uint64(-1).value).status == [0] * 4     # SPP_TREE_SIZE_NOW: all are leaves


def test_null_noise_is_drawn_by_the_library(scenario, ctx, handles, world, tmp_path, capsys):
    from spp import cli, witness as W_
    from oracle import hashes as H
    idx = [0, 2, 1]
    one, two = _prove(handles, world, idx, noise=False), _prove(handles, world, idx, noise=False)
    for b in (one, two):
        assert b.audit_note == [0, 2] and b.audit_status == [0, 0] and b.status == [0] * 3
        assert int(b.c0.max()) < Q and int(b.c1.max()) < Q
    assert not np.array_equal(one.c1, two.c1) and not np.array_equal(one.c0, two.c0)
    assert one.audit_pws[0][12:44] == two.audit_pws[0][12:44] and one.audit_pws[0][44:] != two.audit_pws[0][44:]
    # audit-open on a record returns the note's owner
    fixture = json.load(open(os.path.join(GOLDEN, "rlwe_decrypt.json")))
    shares = []
    for s in fixture["shares"]:
        path = str(tmp_path / ("share_%d.json" % s["share_index"]))
        json.dump({"share_index": s["share_index"], "threshold": s["threshold"], "num_shares": 3,
                   "coefficients": [{"x": s["x"], "y": y} for y in s["y"]]}, open(path, "w"))
        shares.append(path)
    vk, proof, pw, ctj = (str(tmp_path / n) for n in ("a.vk", "a.proof", "a.pw", "ciphertext.json"))
    open(vk, "wb").write(world["avk"]); open(proof, "wb").write(one.audit_proofs[1]); open(pw, "wb").write(one.audit_pws[1])
    json.dump(W_.ciphertext_json(one.c0[1], one.c1[1]), open(ctj, "w"))
    assert cli.main(["audit-open", vk, proof, pw, ctj, "--shares"] + shares) == 0
    owner = H.fixed_base_scalar_mul(world["sks"][1])
    out = capsys.readouterr().out
    assert "owner_x = 0x%064x" % owner[0] in out and "owner_y = 0x%064x" % owner[1] in out and "proof: verified" in out


class Raw:
    """spp_prove_withdrawals through ctypes, the outputs filled with a pattern first"""
    FILL = 0xA5

    def __init__(self, handles, world, idx, cap, notes=None, pool=None, size=(1 << 64) - 1):
        self.L = handles[0].L
        self.count = len(idx)
        self.notes = notes if notes is not None else b"".join(b"".join(int(v).to_bytes(32, "big") for v in world["notes"][i]) for i in idx)
        self.r, self.e1, self.e2 = (np.ascontiguousarray(world[k][idx]) for k in ("r", "e1", "e2"))
        self.a, self.b = (np.ascontiguousarray(v, dtype=np.uint32) for v in world["pk"])
        buf = lambda n: ctypes.create_string_buffer(bytes([self.FILL]) * max(n, 1), max(n, 1))
        self.proofs, self.pws, self.status, self.audit_of = buf(388 * self.count), buf(172 * self.count), buf(4 * self.count), buf(4 * self.count)
        self.audit_note, self.aproofs, self.apws, self.astatus = buf(4 * cap), buf(388 * cap), buf(76 * cap), buf(4 * cap)
        self.c0, self.c1 = buf(4 * 64 * cap), buf(4 * 1024 * cap)
        self.n = ctypes.c_uint32(0xA5A5A5A5)
        self.cap, self.size, self.handles, self.tree, self.pool = cap, size, handles, world["tree"], pool

    def call(self, **over):
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        vp = lambda x: ctypes.cast(x, ctypes.c_void_p)
        a = dict(withdraw=self.handles[0].h, audit=self.handles[1].h, tree=self.tree.h, pool=None if self.pool is None else self.pool.h,
                 size=self.size, pk_a=p(self.a), pk_b=p(self.b), count=self.count, notes=self.notes, r=p(self.r), e1=p(self.e1), e2=p(self.e2),
                 rs_w=None, rs_a=None, proofs=vp(self.proofs), pws=vp(self.pws), status=vp(self.status), audit_of=vp(self.audit_of),
                 audit_note=vp(self.audit_note), n=ctypes.byref(self.n), cap=self.cap, aproofs=vp(self.aproofs), apws=vp(self.apws),
                 astatus=vp(self.astatus), c0=vp(self.c0), c1=vp(self.c1))
        a.update(over)
        return self.L.spp_prove_withdrawals(*a.values())

    def untouched(self, *names):
        return all(getattr(self, k).raw == bytes([self.FILL]) * len(getattr(self, k).raw) for k in names)

    def words(self, name, n):
        return list(np.frombuffer(getattr(self, name).raw, dtype=np.uint32)[:n])


def test_more_identities_than_audit_cap_is_refused_after_the_plan_and_before_any_proving(scenario, handles, world):
    import spp
    raw = Raw(handles, world, list(range(N)), 2)
    assert raw.call() == -1
    msg = spp.last_error()
    assert "5" in msg and "2" in msg and "audit_cap" in msg
    assert raw.n.value == 5 and raw.words("audit_of", N) == PATTERN and raw.words("audit_note", 2) == [0, 1]
    assert raw.untouched("proofs", "pws", "status", "aproofs", "apws", "astatus", "c0", "c1")


def test_refusals(scenario, ctx, handles, world, audit_artifacts):
    import spp
    from spp import witness as W_
    hw, ha = handles
    idx = [0, 1]
    outs = ("proofs", "pws", "status", "audit_of", "audit_note", "aproofs", "apws", "astatus", "c0", "c1")

    def refused(what, note_bytes=None, size=(1 << 64) - 1, idx=idx, **over):
        raw = Raw(handles, world, idx, len(idx), notes=note_bytes, size=size)
        assert raw.call(**over) == -1, what
        assert raw.untouched(*outs) and raw.n.value in (0, 0xA5A5A5A5), what
        return spp.last_error()

    assert "withdraw circuit" in refused("swapped circuits", withdraw=ha.h, audit=hw.h)
    assert "audit circuit" in refused("two withdraw circuits", audit=hw.h)
    other = spp.Context(0)
    try:
        with W_.ShieldedPoolMerkleTree(other, 16) as t2, W_.Pool(other, world["wvk"], world["avk"], 8) as p2:
            assert "another context" in refused("a tree of another context", tree=t2.h)
            assert "another spp_ctx" in refused("a pool of another context", pool=p2.h)
        ha2 = other.load_circuit(audit_artifacts["sppc"], audit_artifacts["pk"], 6)
        try:
            assert "audit circuit belongs to another spp_ctx" in refused("an audit circuit of another context", audit=ha2.h)
        finally:
            ha2.close()
    finally:
        other.close()
    with W_.ShieldedPoolMerkleTree(ctx, 20) as deep:
        assert "inputs" in refused("a tree of another depth", tree=deep.h)
    good = b"".join(int(v).to_bytes(32, "big") for v in world["notes"][0])
    for f in range(5):
        bad = good[:32 * f] + R.to_bytes(32, "big") + good[32 * f + 32:]
        assert "note 1" in refused("a note field >= r", note_bytes=good + bad)
    assert "secret_key is 0" in refused("secret_key == 0", note_bytes=good + good[:64] + bytes(32) + good[96:])
    for k in ("pk_a", "pk_b"):
        pk = np.ascontiguousarray(world["pk"][0 if k == "pk_a" else 1], dtype=np.uint32).copy()
        pk[1023] = Q
        assert "[0, q)" in refused("a public-key coefficient >= q", **{k: pk.ctypes.data_as(ctypes.c_void_p)})
    msg = refused("a size past the tree", size=N + M + 1)
    assert str(N + M + 1) in msg and str(N + M) in msg
    assert "2^20" in refused("count > 2^20", count=(1 << 20) + 1)
    for k in ("withdraw", "audit", "tree", "pk_a", "pk_b", "notes", "proofs", "pws", "audit_of", "audit_note", "n", "aproofs", "apws", "c0", "c1"):
        assert "NULL" in refused("NULL " + k, **{k: None})
    for k in ("r", "e1", "e2"):
        assert "all three" in refused("noise without " + k, **{k: None})
    # the empty batch; and status / audit_status are optional
    raw = Raw(handles, world, [], 0)
    empty = dict(notes=None, r=None, e1=None, e2=None, proofs=None, pws=None, audit_of=None, audit_note=None)
    assert raw.call(**empty) == 0 and raw.n.value == 0
    assert raw.call(size=N + M + 1, **empty) == -1
    raw = Raw(handles, world, [0], 1)
    assert raw.call(status=None, astatus=None) == 0 and raw.n.value == 1 and not raw.untouched("proofs") and raw.untouched("status", "astatus")


def test_cli_withdraw_bundle_end_to_end(scenario, world, withdraw_artifacts, audit_artifacts, tmp_path, capsys):
    """wallet-sync prints the notes, withdraw-bundle proves them, pool-replay settles the log it wrote"""
    from spp import cli
    secrets, leaves, pkj, wa = (str(tmp_path / n) for n in ("secrets.json", "leaves.txt", "rlwe_pk.json", "wa.txt"))
    json.dump([{"secretKey": hex(s), "amount": str(a), "randomness": hex(r)} for s, a, r in world["deposits"][:N]], open(secrets, "w"))
    open(leaves, "w").write("".join("%064x\n" % v for v in scenario["leaves"]))
    json.dump({"a": list(world["pk"][0]), "b": list(world["pk"][1])}, open(pkj, "w"))
    recipient = int.from_bytes(world["addresses"][0][:30], "big")
    assert cli.main(["wallet-sync", secrets, leaves, "--recipient", hex(recipient)]) == 0
    notes = str(tmp_path / "notes.jsonl")
    open(notes, "w").write(capsys.readouterr().out)
    out = str(tmp_path / "bundle")
    args = [notes, withdraw_artifacts["sppc"], withdraw_artifacts["pk"], audit_artifacts["sppc"], audit_artifacts["pk"], pkj, leaves,
            "--out", out, "--window", "6", "--with-deposits"]
    assert cli.main(["withdraw-bundle"] + args) == 0
    assert "12 notes, 5 audit records (0 identities already audited), 0 rows refused" in capsys.readouterr().out
    assert sorted(os.listdir(out)) == sorted(["log.jsonl"] + ["%s_%d.%s" % (a, s, b) for s in range(5) for a, b in
                                                              (("record", "proof"), ("record", "pw"), ("ciphertext", "json"))])
    from spp import witness as W_
    assert len(W_.load_ciphertext_json(os.path.join(out, "ciphertext_4.json"))[1]) == 1024
    assert cli.main(["pool-replay", withdraw_artifacts["vk"], audit_artifacts["vk"], os.path.join(out, "log.jsonl")]) == 0
    lines = capsys.readouterr().out.strip().split("\n")
    want = ["OK root-of-leaves"] * (N + M)
    for i in range(N):
        want += (["OK"] if i in (0, 1, 3, 5, 7) else []) + ["OK size %d" % (N + M)]
    assert lines[:-1] == want and lines[-1].startswith("roots: 16 deposits, 0 pushed")
    # with the identities of the first two records known to the pool, three records are left
    open(wa, "w").write("".join(open(os.path.join(out, "record_%d.pw" % s), "rb").read()[12:44].hex() + "\n" for s in (0, 1)))
    out2 = str(tmp_path / "bundle2")
    args2 = args[:7] + ["--out", out2, "--window", "6", "--audited", wa, "--vk", withdraw_artifacts["vk"], audit_artifacts["vk"]]
    assert cli.main(["withdraw-bundle"] + args2) == 0
    assert "12 notes, 3 audit records (2 identities already audited), 0 rows refused" in capsys.readouterr().out
    kinds = [list(json.loads(ln))[0] for ln in open(os.path.join(out2, "log.jsonl"))]
    assert kinds.count("submit_audit") == 3 and kinds.count("withdraw") == 12 and kinds[:4] == ["withdraw", "withdraw", "withdraw", "submit_audit"]
