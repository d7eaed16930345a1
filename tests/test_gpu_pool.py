"""GPU: the pool ledger (spp_pool_*) against the sequential model of the pool program in tests/test_pool_host.py (PoolModel: dicts,
a 33-entry ring, one instruction at a time, proof validity from the oracle's verifier, memoised by bytes; it calls no spp_pool_*
function).  12 deposits through the resident tree, 12 withdraw proofs from notes and 12 audit records from the SAME secret keys
(so the wa_commitments match), then batches made by repeating and tampering these 24 proofs: a flipped proof byte, a swapped
recipient, another instruction's public witness.

Capacity: spp_pool_* refuses a call with size + count > capacity before anything changes, so the pools that settle batches of 70
have capacity 128; the pools of the table tests have capacity 32 (64 slots), where the refusal itself is tested."""
import os
import random

import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None

from test_pool_host import (PoolModel, TableModel, keys_homed_at, slots_for, OK, AUDIT_EXISTS, NO_AUDIT_RECORD, BAD_ROOT, NULLIFIER_USED,
                            BAD_RECIPIENT, BAD_PROOF)

pytestmark = pytest.mark.gpu

N = 12
FIRST = 700
SALT = 0x0123456789ABCDEF
NULLIFIERS, AUDITS = 0, 1
BIG, SMALL = 128, 32


@pytest.fixture(scope="module", autouse=True)
def fixed_salt():
    old = os.environ.get("SPP_POOL_SALT")
    os.environ["SPP_POOL_SALT"] = "%x" % SALT
    yield
    if old is None:
        del os.environ["SPP_POOL_SALT"]
    else:
        os.environ["SPP_POOL_SALT"] = old


@pytest.fixture(scope="module")
def ctx():
    import spp
    c = spp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def world(ctx, withdraw_artifacts, audit_artifacts, rlwe_pk):
    """deposits, withdraw instructions W[i] = (proof, pw, address) and audit instructions A[i] = (proof, pw), i < 12"""
    from spp import witness as W_, workload
    rng = random.Random(31337)
    sks, r8, e18, e28 = workload.audit_noise(FIRST, N)
    amounts = [rng.randrange(1, 1 << 63) for _ in range(N)]
    rnds = [rng.randrange(1 << 253) for _ in range(N)]
    addresses = [rng.getrandbits(256).to_bytes(32, "big") for _ in range(N)]
    with W_.ShieldedPoolMerkleTree(ctx, 16) as tree:
        first, _, roots = tree.deposit([(sks[i], amounts[i], rnds[i]) for i in range(N)])
        assert first == 0 and len(set(roots)) == N
        h = ctx.load_circuit(withdraw_artifacts["sppc"], withdraw_artifacts["pk"], 6)
        try:
            notes = [(W_.recipient_word(addresses[i]), amounts[i], sks[i], rnds[i], i) for i in range(N)]
            wp, ww, st = h.prove_withdraw_notes(tree, notes, [(11 * i + 3, 13 * i + 5) for i in range(N)])
        finally:
            h.close()
        assert st == [0] * N
    h = ctx.load_circuit(audit_artifacts["sppc"], audit_artifacts["pk"], 6)
    try:
        ap, aw, st, _, _ = h.prove_audit_records(rlwe_pk["a"], rlwe_pk["b"], sks, r8, e18, e28, [(17 * i + 7, 19 * i + 9) for i in range(N)])
    finally:
        h.close()
    assert st == [0] * N
    roots = [int(r).to_bytes(32, "big") for r in roots]
    W = [(wp[i], ww[i], addresses[i]) for i in range(N)]
    A = [(ap[i], aw[i]) for i in range(N)]
    for i in range(N):                                                   # the same identities on both sides, every proof against the last root
        assert ww[i][140:172] == aw[i][12:44] and ww[i][12:44] == roots[-1]
    wvk, avk = open(withdraw_artifacts["vk"], "rb").read(), open(audit_artifacts["vk"], "rb").read()
    memo = {}
    def verifier(vk):
        from oracle import groth16
        def f(proof, pw):
            k = (vk[:8], proof, pw)
            if k not in memo:
                memo[k] = bool(groth16.verify(vk, proof, pw))
            return memo[k]
        return f
    return dict(W=W, A=A, roots=roots, amounts=amounts, wvk=wvk, avk=avk, model=lambda: PoolModel(verifier(wvk), verifier(avk)),
                nullifiers=[w[1][44:76] for w in W], was=[a[1][12:44] for a in A])


def _flip(proof):
    return proof[:100] + bytes([proof[100] ^ 1]) + proof[101:]


def _with_root(pw, root):
    return pw[:12] + root + pw[44:]


def _interleave(rng, *seqs):
    """one list holding the sequences in a random interleaving that keeps each sequence's own order"""
    seqs = [list(s) for s in seqs if s]
    out = []
    while seqs:
        s = rng.choice(seqs)
        out.append(s.pop(0))
        if not s:
            seqs.remove(s)
    return out


def _audit_batches(world):
    A, rng = world["A"], random.Random(70)
    bad = lambda i: (_flip(A[i][0]), A[i][1], ("bad", i))
    good = lambda i: (A[i][0], A[i][1], ("good", i))
    seqs = [[bad(0), good(0), good(0)],                                   # BAD_PROOF, OK, AUDIT_EXISTS
            [good(1), bad(1)],                                            # OK, AUDIT_EXISTS: the copy after the valid one is not verified
            [bad(2), bad(2), bad(2)],                                     # no copy is valid: no record
            [(A[3][0], A[4][1], ("pw4", 3)), good(4), good(3)],           # proof 3 under the pw of 4: BAD_PROOF for key 4, then both valid
            [good(5)], [bad(6), good(6)]]
    for i in range(7, 10):
        seqs.append([good(i) if rng.random() < 0.6 else bad(i) for _ in range(rng.randrange(7, 11))])
    first = _interleave(rng, *seqs)
    assert len(first) < 70
    while len(first) < 70:
        first.append(rng.choice((good, bad))(rng.randrange(7, 10)))
    second = [good(0), bad(2), good(2), bad(10), good(4), bad(1)]        # resubmissions in a second call; keys 10 and 11 never get a record
    return first, second


def _withdraw_batches(world):
    W, rng = world["W"], random.Random(71)
    good = lambda i: (W[i][0], W[i][1], W[i][2], ("good", i))
    bad = lambda i: (_flip(W[i][0]), W[i][1], W[i][2], ("bad", i))
    other = lambda i: (W[i][0], W[i][1], W[(i + 1) % N][2], ("recipient", i))      # another account's address
    unknown_root = rng.getrandbits(250).to_bytes(32, "big")
    seqs = [[bad(0), good(0), good(0)],                                   # BAD_PROOF, OK, NULLIFIER_USED
            [good(1), other(1)],                                          # wrong recipient + spent nullifier: NULLIFIER_USED comes first
            [other(2), good(2), other(2)],                                # BAD_RECIPIENT spends nothing; then OK; then NULLIFIER_USED
            [(W[3][0], W[4][1], W[4][2], ("pw4", 3)), good(4)],           # proof 3 under the pw of 4: BAD_PROOF, nullifier 4 still free
            [good(10)],                                                   # no audit record
            [(W[11][0], _with_root(W[11][1], unknown_root), W[11][2], ("noaudit+root", 11))],   # ... and an unknown root: NO_AUDIT_RECORD first
            [(W[5][0], _with_root(W[5][1], unknown_root), W[5][2], ("root", 5)), good(5)],      # BAD_ROOT, then OK
            [good(6)]]
    for i in range(7, 10):
        seqs.append([rng.choice((good, good, bad, other))(i) for _ in range(rng.randrange(9, 13))])
    first = _interleave(rng, *seqs)
    assert len(first) < 70
    while len(first) < 70:
        first.append(rng.choice((good, bad, other))(rng.randrange(7, 10)))
    second = [good(0), other(3), good(3), bad(4), good(10), good(6)]     # replays in a second call
    return first, second


def _positions(batch, tag):
    return [k for k, ins in enumerate(batch) if ins[-1] == tag]


def _same_state(pool, model, world):
    assert pool.state() == model.state()
    assert pool.counts() == (len(model.nullifiers), len(model.audits))
    extra = [bytes(32), b"\xff" * 32]
    assert pool.contains(NULLIFIERS, world["nullifiers"] + extra) == [k in model.nullifiers for k in world["nullifiers"] + extra]
    assert pool.contains(AUDITS, world["was"] + extra) == [k in model.audits for k in world["was"] + extra]


def _run_scenario(ctx, world, model=None):
    """the two audit batches, the deposits' roots, the two withdraw batches on a fresh pool (and on the model, when given);
    returns everything observed, step by step"""
    from spp import witness as W_
    a1, a2 = _audit_batches(world)
    w1, w2 = _withdraw_batches(world)
    seen, want = [], []
    with W_.Pool(ctx, world["wvk"], world["avk"], BIG) as pool:
        def snap():
            seen.append((pool.state(), pool.counts(), pool.contains(NULLIFIERS, world["nullifiers"]), pool.contains(AUDITS, world["was"])))
            if model is not None:
                _same_state(pool, model, world)
        snap()
        for batch in (a1, a2):
            seen.append(pool.submit_audit([b[0] for b in batch], [b[1] for b in batch]))
            if model is not None:
                want.append([model.submit_audit(b[0], b[1]) for b in batch])
            snap()
        pool.add_roots(world["roots"])
        if model is not None:
            for r in world["roots"]:
                model.add_root(r)
        snap()
        for batch in (w1, w2):
            seen.append(pool.withdraw([b[0] for b in batch], [b[1] for b in batch], [b[2] for b in batch]))
            if model is not None:
                res = [model.withdraw(b[0], b[1], b[2]) for b in batch]
                want.append(([c for c, _ in res], [a for _, a in res]))
            snap()
    return dict(seen=seen, want=want, batches=(a1, a2, w1, w2))


@pytest.fixture(scope="module")
def settled(ctx, world):
    return _run_scenario(ctx, world, world["model"]())


def test_audit_batches_settle_as_the_program_would_in_order(settled):
    a1, a2 = settled["batches"][:2]
    got1, got2 = settled["seen"][1], settled["seen"][3]
    print("audit batch 1:", got1, "\naudit batch 2:", got2)
    assert len(a1) == 70 and got1 == settled["want"][0] and got2 == settled["want"][1]
    p = _positions(a1, ("bad", 0)) + _positions(a1, ("good", 0))
    assert [got1[k] for k in p] == [BAD_PROOF, OK, AUDIT_EXISTS]
    assert [got1[k] for k in _positions(a1, ("good", 1)) + _positions(a1, ("bad", 1))] == [OK, AUDIT_EXISTS]
    assert [got1[k] for k in _positions(a1, ("bad", 2))] == [BAD_PROOF] * 3
    assert got1[_positions(a1, ("pw4", 3))[0]] == BAD_PROOF and got1[_positions(a1, ("good", 4))[0]] == OK
    assert got2 == [AUDIT_EXISTS, BAD_PROOF, OK, BAD_PROOF, AUDIT_EXISTS, AUDIT_EXISTS]
    # a record per OK, none otherwise; keys 0, 1, 3..6 for certain after batch 1, key 2 in batch 2
    assert settled["seen"][2][1] == (0, got1.count(OK)) and settled["seen"][4][1] == (0, got1.count(OK) + 1) and 6 <= got1.count(OK) <= 9


def test_withdraw_batches_settle_as_the_program_would_in_order(settled, world):
    w1, w2 = settled["batches"][2:]
    (got1, amounts1), (got2, amounts2) = settled["seen"][6], settled["seen"][8]
    print("withdraw batch 1:", got1, "\nwithdraw batch 2:", got2)
    assert len(w1) == 70 and (got1, amounts1) == settled["want"][2] and (got2, amounts2) == settled["want"][3]
    assert [got1[k] for k in _positions(w1, ("bad", 0)) + _positions(w1, ("good", 0))] == [BAD_PROOF, OK, NULLIFIER_USED]
    assert [got1[k] for k in _positions(w1, ("good", 1)) + _positions(w1, ("recipient", 1))] == [OK, NULLIFIER_USED]
    r2, g2 = _positions(w1, ("recipient", 2)), _positions(w1, ("good", 2))
    assert [got1[k] for k in (r2[0], g2[0], r2[1])] == [BAD_RECIPIENT, OK, NULLIFIER_USED]
    assert got1[_positions(w1, ("pw4", 3))[0]] == BAD_PROOF and got1[_positions(w1, ("good", 4))[0]] == OK
    assert got1[_positions(w1, ("good", 10))[0]] == NO_AUDIT_RECORD == got1[_positions(w1, ("noaudit+root", 11))[0]]
    assert got1[_positions(w1, ("root", 5))[0]] == BAD_ROOT and got1[_positions(w1, ("good", 5))[0]] == OK
    assert got2 == [NULLIFIER_USED, BAD_RECIPIENT, OK, NULLIFIER_USED, NO_AUDIT_RECORD, NULLIFIER_USED]
    # amounts: the notes' amounts, for every instruction whatever became of it (the pw of 4 carries the amount of 4)
    who = lambda ins: 4 if ins[-1][0] == "pw4" else ins[-1][1]
    assert amounts1 == [world["amounts"][who(ins)] for ins in w1] and amounts2 == [world["amounts"][who(ins)] for ins in w2]
    assert settled["seen"][9][1][0] == (got1 + got2).count(OK) >= 7        # a spent nullifier per OK: 0..6 for certain


def test_same_batches_on_a_second_fresh_pool_give_the_same_results_and_state(ctx, world, settled):
    again = _run_scenario(ctx, world)
    assert again["seen"] == settled["seen"]


def _one_withdraw_pool(ctx, world, i):
    """a fresh pool (and model) that knows the audit record of identity i"""
    from spp import witness as W_
    pool, model = W_.Pool(ctx, world["wvk"], world["avk"], SMALL), world["model"]()
    pool.import_keys(AUDITS, [world["was"][i]])
    model.audits[world["was"][i]] = True
    return pool, model


@pytest.mark.parametrize("later,want", [(31, OK), (32, BAD_ROOT)])
def test_a_root_leaves_the_ring_after_exactly_32_later_roots(ctx, world, later, want):
    """the proofs are against roots[11], pushed as the 12th root: 31 later roots leave it in slot 11, the 32nd overwrites it (and is
    the new current root)"""
    rng = random.Random(later)
    more = [rng.getrandbits(250).to_bytes(32, "big") for _ in range(later)]
    pool, model = _one_withdraw_pool(ctx, world, 7)
    with pool:
        pool.add_roots(world["roots"])
        pool.add_roots(more)
        for r in world["roots"] + more:
            model.add_root(r)
        p, w, a = world["W"][7]
        got = pool.withdraw([p], [w], [a])
        assert got == ([want], [world["amounts"][7]]) and got[0] == [model.withdraw(p, w, a)[0]]
        _same_state(pool, model, world)
        assert pool.counts() == (1 if want == OK else 0, 1)


def test_the_zero_root_passes_on_a_fresh_pool_as_it_does_in_the_program(ctx, world):
    p, w, a = world["W"][8]
    w0 = _with_root(w, bytes(32))
    pool, model = _one_withdraw_pool(ctx, world, 8)
    with pool:
        got, _ = pool.withdraw([p, p], [w0, w], [a, a])
        assert got == [model.withdraw(p, w0, a)[0], model.withdraw(p, w, a)[0]] == [BAD_PROOF, BAD_ROOT]    # not BAD_ROOT for the zero root
        rng = random.Random(9)
        more = [rng.getrandbits(250).to_bytes(32, "big") for _ in range(32)]
        pool.add_roots(more[:31])
        assert pool.withdraw([p], [w0], [a])[0] == [BAD_PROOF]           # slot 31 is still zero
        pool.add_roots(more[31:])
        assert pool.withdraw([p], [w0], [a])[0] == [BAD_ROOT]
        for r in more:
            model.add_root(r)
        _same_state(pool, model, world)


def test_table_chains_across_the_end_and_capacity_is_enforced(ctx, world):
    import spp
    from spp import witness as W_
    slots = slots_for(SMALL)
    rng = random.Random(64)
    last, before = keys_homed_at(slots - 1, SALT, slots, 4, rng), keys_homed_at(slots - 2, SALT, slots, 3, rng)
    twin = bytes([last[0][0] ^ 0x80]) + last[0][1:]                       # the low 64 bits of last[0], another key
    others = [rng.getrandbits(256).to_bytes(32, "big") for _ in range(6)]
    call1 = before[:2] + last[:3] + [last[0], twin] + others[:3] + [before[0]]        # duplicates inside the call
    call2 = [last[1], last[3], before[2]] + others[3:] + [others[0], others[3]]       # ... and with the set
    absent = keys_homed_at(slots - 1, SALT, slots, 2, rng) + [bytes(32), rng.getrandbits(256).to_bytes(32, "big")]
    t = TableModel(SMALL, SALT)
    with W_.Pool(ctx, world["wvk"], world["avk"], SMALL) as pool:
        for which, call in ((NULLIFIERS, call1), (NULLIFIERS, call2)):
            pool.import_keys(which, call)
            for k in call:
                t.insert(k)
            n = sum(c is not None for c in t.cell)
            assert pool.counts() == (n, 0)
        assert n == 14 and t.cell[slots - 1] is not None and all(t.cell[s] is not None for s in range(4))    # the chain wraps
        present = list(dict.fromkeys(call1 + call2))
        assert pool.contains(NULLIFIERS, present + absent) == [True] * 14 + [False] * 4
        assert pool.contains(AUDITS, present) == [False] * 14             # the other set is untouched
        # 14 keys of 32: a call with 19 more could overflow the set -- refused whatever the keys are, nothing changes
        state = pool.state()
        with pytest.raises(spp.SppError) as e:
            pool.import_keys(NULLIFIERS, present + absent + [absent[0]])
        assert e.value.code == -1 and "overflow" in str(e.value)
        a, w = world["A"][0], world["W"][0]
        with pytest.raises(spp.SppError) as e:
            pool.submit_audit([a[0]] * 33, [a[1]] * 33)
        assert e.value.code == -1
        with pytest.raises(spp.SppError) as e:
            pool.withdraw([w[0]] * 19, [w[1]] * 19, [w[2]] * 19)
        assert e.value.code == -1
        assert pool.state() == state and pool.counts() == (14, 0) and pool.contains(NULLIFIERS, absent) == [False] * 4
        pool.import_keys(NULLIFIERS, absent + absent[:1] + present[:13])  # exactly 18 more still go in
        assert pool.counts() == (18, 0) and pool.contains(NULLIFIERS, absent) == [True] * 4
        assert pool.submit_audit([], []) == [] and pool.withdraw([], [], []) == ([], [])


def test_swapped_or_malformed_keys_are_refused(ctx, world):
    import spp
    from spp import witness as W_
    for wvk, avk in ((world["avk"], world["wvk"]), (world["wvk"], world["wvk"]), (world["avk"], world["avk"]),
                     (world["wvk"][:-1], world["avk"])):
        with pytest.raises(spp.SppError) as e:
            W_.Pool(ctx, wvk, avk, SMALL)
        assert e.value.code == -7
    with pytest.raises(spp.SppError) as e:
        W_.Pool(ctx, world["wvk"], world["avk"], 0)
    assert e.value.code == -1


def test_cli_pool_replay(tmp_path, world, capsys):
    import json
    from spp import cli
    wvk, avk, log = (str(tmp_path / n) for n in ("w.vk", "a.vk", "log.jsonl"))
    open(wvk, "wb").write(world["wvk"]); open(avk, "wb").write(world["avk"])
    A, W = world["A"], world["W"]
    ins = [{"withdraw": {"proof": W[0][0].hex(), "pw": W[0][1].hex(), "recipient": W[0][2].hex()}}]
    ins += [{"deposit": {"root": r.hex()}} for r in world["roots"]]
    ins += [{"submit_audit": {"proof": A[0][0].hex(), "pw": "0x" + A[0][1].hex()}}] * 2
    ins += [{"withdraw": {"proof": W[0][0].hex(), "pw": W[0][1].hex(), "recipient": W[0][2].hex()}}] * 2
    open(log, "w").write("".join(json.dumps(i) + "\n" for i in ins))
    assert cli.main(["pool-replay", wvk, avk, log]) == 0
    assert capsys.readouterr().out.split() == ["NO_AUDIT_RECORD"] + ["OK"] * 12 + ["OK", "AUDIT_EXISTS", "OK", "NULLIFIER_USED"]
