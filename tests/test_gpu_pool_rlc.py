"""GPU: the pool ledger and the audit opening on the random-linear-combination verifier -- spp_pool_set_verifier(SPP_POOL_VERIFY_RLC)
in front of spp_pool_withdraw_batch / spp_pool_submit_audit_batch / spp_pool_settle_log (k_verify_rlc_terms_list,
k_verify_rlc_group_list over the compacted list, k_verify_list over the refused groups) and spp_audit_open_batch_rlc.  Everything
runs with group 64, the smallest shape: lists of 0, 1, 64, 65, 130 and 150 entries are 0, 1, 1, 2, 3 and 3 groups.

The expected decisions are those of the sequential PoolModel (tests/test_pool_host.py) whose verifier callbacks LOOK THE VERDICT UP
by (proof, public witness) in a table filled from the tags the instructions carry by construction -- a simulated proof
(tests/verify_vectors.py) verifies, a forgery bent from one does not, a real proof verifies under its own public witness only -- so
no pairing is computed on the host; a pair the table does not hold is a KeyError, not a guess.  The decisions do not depend on the
weights, so no test needs a seed (the library takes one from the operating system per launch and offers no way to supply one).
The order of the list is the order of the screen kernel's atomicAdd: the statistics are asserted as far as they hold for EVERY order."""
import os
import random

import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None

import verify_vectors as V
from test_pool_host import PoolModel, OK, AUDIT_EXISTS, NULLIFIER_USED, BAD_PROOF
from test_gpu_pool import ctx, world, fixed_salt, _same_state, _flip, NULLIFIERS, AUDITS, BIG  # noqa: F401
from test_gpu_pool_log import _settle, _model_log, _interleaved_log, _observed, NAMES
from test_gpu_verify_forged import keys, _pool_instructions, _bent, SEEDS  # noqa: F401
from test_gpu_audit_records import records, sk_mod_q, decrypt_fixture, _split, B_  # noqa: F401

pytestmark = pytest.mark.gpu

GROUP = 64
CAPACITY = 256
ZERO4 = (0, 0, 0, 0)
VALID_TAGS = (V.ACCEPT, "a_good", "w_good", "w_other")                    # w_other: another ADDRESS, the proof and its witness intact


class Verdicts:
    """the verifier of the model: the verdict an instruction has by construction, looked up by bytes"""

    def __init__(self):
        self.table = {}

    def add(self, proof, pw, good):
        assert self.table.setdefault((proof, pw), bool(good)) == bool(good), "one pair, two verdicts"

    def __call__(self, proof, pw):
        return self.table[(proof, pw)]

    def model(self):
        return PoolModel(self, self)


def _rlc_pool(ctx, world, capacity=CAPACITY, verifier="rlc"):
    from spp import witness as W_
    return W_.Pool(ctx, world["wvk"], world["avk"], capacity, verifier=verifier, group=GROUP)


# ------------------------------------------------------------------------------------------------- 1. the scene of simulated forgeries
@pytest.fixture(scope="module")
def scene(world):
    """the 70 instructions of tests/test_gpu_verify_forged.py (5 spent in front, 65 that reach the verifier, 26 of them forged) and
    what the sequential model answers from the tags"""
    s = _pool_instructions(world["wvk"])
    verdicts = Verdicts()
    for p, w, _, tag in s["ins"]:
        if tag != "spent":
            verdicts.add(p, w, tag == V.ACCEPT)
    s["verdicts"] = verdicts
    model = _scene_model(s, True)
    res = [model.withdraw(p, w, a) for p, w, a, _ in s["ins"]]
    s["want"] = ([c for c, _ in res], [a for _, a in res])
    assert s["want"][0] == [NULLIFIER_USED if t == "spent" else OK if t == V.ACCEPT else BAD_PROOF for *_, t in s["ins"]]
    s["dropped"] = sum(t in (V.FORMAT, V.SUBGROUP) for *_, t in s["ins"])
    assert s["dropped"] == 13
    return s


def _scene_model(scene, with_roots):
    model = scene["verdicts"].model()
    for k in scene["was"]:
        model.audits[k] = True
    for k in scene["spent"]:
        model.nullifiers[k] = True
    if with_roots:
        for r in scene["roots"]:
            model.add_root(r)
    return model


def _scene_pool(ctx, world, scene, with_roots, **kw):
    pool = _rlc_pool(ctx, world, **kw)
    pool.import_keys(AUDITS, scene["was"])
    pool.import_keys(NULLIFIERS, scene["spent"])
    if with_roots:
        pool.add_roots(scene["roots"])
    return pool


def _check_scene_stats(pool, scene):
    """a list of 65: two groups.  The first holds 64 entries, at least 12 of them live forgeries, so it is refused and its live
    members are re-verified; the second holds one entry and is refused only if that one is a live forgery"""
    w, a = pool.verify_stats()
    print("verify_stats:", w, a)
    groups, refused, reverified, dropped = w
    assert a == ZERO4 and groups == 2 and dropped == scene["dropped"]
    assert 1 <= refused <= 2
    assert 64 - dropped <= reverified <= 65 - dropped
    if refused == 2:
        assert reverified == 65 - dropped


def test_scene_of_forgeries_through_withdraw(ctx, world, scene):
    ins = scene["ins"]
    with _scene_pool(ctx, world, scene, True) as pool:
        got = pool.withdraw([i[0] for i in ins], [i[1] for i in ins], [i[2] for i in ins])
        wrong = ["%d %s: %d, want %d" % (k, i[3], g, w) for k, (i, g, w) in enumerate(zip(ins, got[0], scene["want"][0])) if g != w]
        assert not wrong, "\n".join(wrong)
        assert got == scene["want"]
        _check_scene_stats(pool, scene)
        model = _scene_model(scene, True)
        for p, w, a, _ in ins:
            model.withdraw(p, w, a)
        _same_state(pool, model, world)
        assert pool.counts() == (5 + got[0].count(OK), 3) and got[0].count(OK) == 39
        assert pool.contains(NULLIFIERS, [i[1][44:76] for i in ins]) == [t in ("spent", V.ACCEPT) for *_, t in ins]


def test_scene_of_forgeries_through_settle_log(ctx, world, scene):
    log = [(("deposit", r), ("deposit", None)) for r in scene["roots"]] + [(("withdraw", p, w, a), (t, k)) for k, (p, w, a, t) in enumerate(scene["ins"])]
    with _scene_pool(ctx, world, scene, False) as pool:
        model = _scene_model(scene, False)
        got = _settle(pool, log)
        assert got == _model_log(model, log)
        assert (got[0][2:], got[1][2:]) == scene["want"] and got[0][:2] == [OK, OK]
        _check_scene_stats(pool, scene)
        _same_state(pool, model, world)
        assert pool.contains(NULLIFIERS, [i[1][44:76] for i in scene["ins"]]) == [t in ("spent", V.ACCEPT) for *_, t in scene["ins"]]


def test_scene_of_forgeries_on_the_dense_verifier(ctx, world, scene):
    """SPP_POOL_COMPACT=0: mode RLC runs the dense kernels over all 70 instructions, the 5 settled ones (whose proofs are another
    instruction's: live, invalid) included"""
    ins = scene["ins"]
    old = os.environ.get("SPP_POOL_COMPACT")
    os.environ["SPP_POOL_COMPACT"] = "0"
    try:
        pool = _scene_pool(ctx, world, scene, True)
    finally:
        if old is None:
            del os.environ["SPP_POOL_COMPACT"]
        else:
            os.environ["SPP_POOL_COMPACT"] = old
    with pool:
        assert pool.withdraw([i[0] for i in ins], [i[1] for i in ins], [i[2] for i in ins]) == scene["want"]
        w, a = pool.verify_stats()
        print("verify_stats:", w, a)
        assert a == ZERO4 and w[0] == 2 and w[3] == scene["dropped"] and 1 <= w[1] <= 2 and 64 - 13 <= w[2] <= 70 - 13


# ------------------------------------------------------------------------------------------------- 2. real proofs of both kinds
def _log_verdicts(log):
    verdicts = Verdicts()
    for ins, (tag, _) in log:
        if ins[0] != "deposit":
            verdicts.add(ins[1], ins[2], tag in VALID_TAGS)
    return verdicts


def test_interleaved_log_of_real_proofs(ctx, world):
    """both lists are shorter than one group; equal to the sequential model and to mode EACH on an identical fresh pool"""
    log = _interleaved_log(world)
    model = _log_verdicts(log).model()
    want = _model_log(model, log)
    with _rlc_pool(ctx, world, BIG) as pool, _rlc_pool(ctx, world, BIG, verifier="each") as each:
        got, ref = _settle(pool, log), _settle(each, log)
        print("codes:", [NAMES[c] for c in got[0]])
        assert got == want and got == ref
        assert _observed(pool, world) == _observed(each, world)
        _same_state(pool, model, world)
        w, a = pool.verify_stats()
        print("verify_stats:", w, a)
        assert w[0] == 1 and a[0] == 1 and w[1] == 1 and a[1] == 1       # one group per kind; both hold proofs that do not verify
        assert 0 < w[2] + w[3] < GROUP and 0 < a[2] + a[3] < GROUP
        assert each.verify_stats() == (ZERO4, ZERO4)


# ------------------------------------------------------------------------------------------------- 3, 4, 5. simulated valid proofs
N_W, N_AGAIN, N_A, N_RESIDENT = 130, 20, 70, 6
FORGED = 77


@pytest.fixture(scope="module")
def valid(keys):
    """130 simulated withdraws with distinct nullifiers (20 of them submitted a second time: list of 150), one STAGE4 and one FORMAT
    forgery of instruction 77, and 70 simulated submit_audits of which the first 6 find their record resident (list of 64)"""
    from oracle import bn254 as B
    from spp import witness as W_
    rng = random.Random(1764)
    wvk, avk = V._vk(keys["withdraw"]), V._vk(keys["audit"])
    wtd, atd = V.trapdoor(SEEDS["withdraw"]), V.trapdoor(SEEDS["audit"])
    V.check_trapdoor(wvk, wtd)
    V.check_trapdoor(avk, atd)
    roots = [rng.getrandbits(250).to_bytes(32, "big") for _ in range(2)]
    was = [rng.randrange(B.R).to_bytes(32, "big") for _ in range(3)]
    verdicts = Verdicts()
    W, forged = [], {}
    for k in range(N_W):
        address = rng.getrandbits(256).to_bytes(32, "big")
        pub = [int.from_bytes(roots[k % 2], "big"), rng.randrange(B.R), W_.recipient_word(address), rng.randrange(1, 1 << 64),
               int.from_bytes(was[k % 3], "big")]
        pw = V.groth16.public_witness_bytes(pub)
        pts = V.simulate_points(wvk, wtd, pub, V._big(rng), V._big(rng), V._big(rng))
        W.append((V.proof_bytes(*pts), pw, address))
        verdicts.add(W[-1][0], pw, True)
        if k == FORGED:
            for kind in (V.STAGE4, V.FORMAT):
                proof, fpw = _bent(kind, 0, pts, pw, None)
                assert fpw == pw and proof != W[-1][0]
                forged[kind] = (proof, pw, address)
                verdicts.add(proof, pw, False)
    assert len({w[1][44:76] for w in W}) == N_W
    again = [W[k] for k in rng.sample(range(N_W), N_AGAIN)]
    A = []
    for k in range(N_A):
        pub = [rng.randrange(B.R), rng.randrange(B.R)]
        pw = V.groth16.public_witness_bytes(pub)
        if k < N_RESIDENT:                                                # never verified: the record exists
            A.append((A[0][0] if A else V.simulate(avk, atd, pub, 3, 5, 7)[0], pw))
            continue
        A.append(V.simulate(avk, atd, pub, V._big(rng), V._big(rng), V._big(rng)))
        verdicts.add(A[-1][0], A[-1][1], True)
    assert len({a[1][12:44] for a in A}) == N_A
    return dict(W=W, again=again, A=A, forged=forged, roots=roots, was=was, verdicts=verdicts)


def _valid_pool(ctx, world, valid, spent=(), verifier="rlc"):
    pool, model = _rlc_pool(ctx, world, verifier=verifier), valid["verdicts"].model()
    pool.import_keys(AUDITS, valid["was"] + [a[1][12:44] for a in valid["A"][:N_RESIDENT]])
    pool.add_roots(valid["roots"])
    pool.import_keys(NULLIFIERS, list(spent))
    for k in valid["was"] + [a[1][12:44] for a in valid["A"][:N_RESIDENT]]:
        model.audits[k] = True
    for r in valid["roots"]:
        model.add_root(r)
    for k in spent:
        model.nullifiers[k] = True
    return pool, model


def _withdraw(pool, model, batch):
    """(what the pool answers, what the model answers)"""
    got = pool.withdraw([b[0] for b in batch], [b[1] for b in batch], [b[2] for b in batch])
    res = [model.withdraw(*b) for b in batch]
    return got, ([c for c, _ in res], [a for _, a in res])


def test_all_valid_refuses_no_group(ctx, world, valid):
    """on valid proofs no group may be refused: the fallback cannot hide a tail that refuses wrongly"""
    rng = random.Random(5)
    batch = list(valid["W"])
    for b in valid["again"]:                                              # each resubmission somewhere behind its original
        batch.insert(rng.randrange(batch.index(b) + 1, len(batch) + 1), b)
    pool, model = _valid_pool(ctx, world, valid)
    with pool:
        got, want = _withdraw(pool, model, batch)
        assert got == want and got[0].count(OK) == N_W and got[0].count(NULLIFIER_USED) == N_AGAIN
        assert pool.verify_stats() == ((3, 0, 0, 0), ZERO4)               # 150 candidates: in-batch duplicates are verified too
        got = pool.submit_audit([a[0] for a in valid["A"]], [a[1] for a in valid["A"]])
        assert got == [model.submit_audit(*a) for a in valid["A"]] == [AUDIT_EXISTS] * N_RESIDENT + [OK] * (N_A - N_RESIDENT)
        assert pool.verify_stats() == (ZERO4, (1, 0, 0, 0))               # exactly one full group
        assert pool.counts() == (N_W, 3 + N_A)
        assert pool.contains(NULLIFIERS, [w[1][44:76] for w in valid["W"]]) == [True] * N_W


@pytest.mark.parametrize("kind", [V.STAGE4, V.FORMAT])
def test_one_forgery_among_valid_withdraws(ctx, world, valid, kind):
    batch = list(valid["W"])
    batch[FORGED] = valid["forged"][kind]
    pool, model = _valid_pool(ctx, world, valid)
    with pool:
        got, want = _withdraw(pool, model, batch)
        assert got == want
        assert got[0] == [BAD_PROOF if k == FORGED else OK for k in range(N_W)]
        assert pool.contains(NULLIFIERS, [w[1][44:76] for w in batch]) == [k != FORGED for k in range(N_W)]
        w, a = pool.verify_stats()
        print("verify_stats:", w, a)
        assert a == ZERO4 and w[0] == 3
        if kind == V.STAGE4:                                              # live and invalid: its group is refused, 64 + 64 + 2
            assert w[1] == 1 and w[2] in (64, 2) and w[3] == 0
        else:                                                             # dropped by the format check: no group sees it
            assert w[1:] == (0, 0, 1)


def test_degenerate_lists(ctx, world, valid):
    W = valid["W"]
    pool, model = _valid_pool(ctx, world, valid, spent=[w[1][44:76] for w in W[:10]])
    with pool:
        before = _observed(pool, world), pool.counts()
        got, want = _withdraw(pool, model, W[:10])                        # every nullifier spent: nothing reaches the verifier
        assert got == want and got[0] == [NULLIFIER_USED] * 10
        assert pool.verify_stats() == (ZERO4, ZERO4)
        assert (_observed(pool, world), pool.counts()) == before
        got, want = _withdraw(pool, model, W[10:11])                      # a batch of one
        assert got == want and got[0] == [OK] and pool.verify_stats() == ((1, 0, 0, 0), ZERO4)
        got, want = _withdraw(pool, model, [valid["forged"][V.STAGE4]])   # ... and a refused group of one
        assert got == want and got[0] == [BAD_PROOF] and pool.verify_stats() == ((1, 1, 1, 0), ZERO4)
        assert pool.withdraw([], [], []) == ([], []) and pool.submit_audit([], []) == [] and pool.settle_log([]) == ([], [])
        assert pool.counts() == (11, 3 + N_RESIDENT)


# ------------------------------------------------------------------------------------------------- 6. switching
def test_switching_the_verifier_and_refused_arguments(ctx, world, scene):
    import spp
    ins = scene["ins"]
    parts = (ins[:30], ins[30:50], ins[50:])
    L = ctx.L
    with _scene_pool(ctx, world, scene, True, verifier="each") as pool, _scene_pool(ctx, world, scene, True, verifier="each") as each:
        model = _scene_model(scene, True)
        for mode, part in zip(("each", "rlc", "each"), parts):
            pool.set_verifier(mode, GROUP)
            got, want = _withdraw(pool, model, [i[:3] for i in part])
            assert got == want and got == each.withdraw([i[0] for i in part], [i[1] for i in part], [i[2] for i in part]), mode
            w, a = pool.verify_stats()
            assert a == ZERO4 and ((w == ZERO4) if mode == "each" else (w[0] == 1 and w[1] == 1 and w[2] + w[3] == len(part)))
            assert each.verify_stats() == (ZERO4, ZERO4)
        assert _observed(pool, world) == _observed(each, world)
        _same_state(pool, model, world)
        # refused, the pool unchanged: still in mode RLC with group 64 afterwards
        pool.set_verifier("rlc", GROUP)
        before = _observed(pool, world), pool.counts()
        for mode, group in ((2, 0), (-1, GROUP), (1, 63), (1, 96), (1, 8192), (0, 32)):
            assert L.spp_pool_set_verifier(pool.h, mode, group) == -1, (mode, group)
            assert ("group" if mode in (0, 1) else "mode") in spp.last_error()
        assert L.spp_pool_set_verifier(None, 1, GROUP) == -1 and "NULL" in spp.last_error()
        with pytest.raises(spp.SppError):
            pool.set_verifier("rlc", 100)
        with pytest.raises(ValueError):
            pool.set_verifier("both")
        assert (_observed(pool, world), pool.counts()) == before
        part = [i[:3] for i in ins[5:70]]                                 # all spent or refused by now: 65 candidates at most
        got, want = _withdraw(pool, model, part)
        assert got == want and OK not in got[0]
        w, _ = pool.verify_stats()
        n_list = got[0].count(BAD_PROOF)
        assert n_list == 26 and w[0] == 1 and w[2] + w[3] == n_list       # one group of 64: the refusals left mode and group alone


# ------------------------------------------------------------------------------------------------- 7. audit opening
def test_audit_open_rlc_equals_audit_open(ctx, records, sk_mod_q):
    a = records["device"][0]
    vk = records["vk"]
    proofs, pws = _split(a["proofs"], 388), _split(a["pws"], 76)
    want = ctx.audit_open(vk, sk_mod_q, proofs, pws, a["c0"], a["c1"])
    owners, flags, stats = ctx.audit_open(vk, sk_mod_q, proofs, pws, a["c0"], a["c1"], rlc=True, group=GROUP, want_stats=True)
    assert (owners, flags) == want and flags == [0] * B_
    assert stats == (2, 0, 0, 0)                                          # 70 valid records: no group refused
    # a proof that is off its curve (dropped), a public witness of another record (live, refused), a tampered ciphertext
    proofs[30] = _flip(proofs[30])
    pws[40] = pws[40][:12] + pws[41][12:44] + pws[40][44:]
    c0 = a["c0"].copy()
    c0[3, 5] = (int(c0[3, 5]) + 167772161 // 256) % 167772161
    want = ctx.audit_open(vk, sk_mod_q, proofs, pws, c0, a["c1"])
    owners, flags, stats = ctx.audit_open(vk, sk_mod_q, proofs, pws, c0, a["c1"], rlc=True, group=GROUP, want_stats=True)
    print("flags:", flags, "stats:", stats)
    assert (owners, flags) == want
    assert [i for i in range(B_) if flags[i] & 1] == [30, 40] and flags[3] == 2 | 4
    assert stats == (2, 1, 63, 1)                                         # records 0..63: 30 dropped, 40 refuses the group, 63 re-verified
    # no key: nothing is verified, bit 1 is never set
    want = ctx.audit_open(None, sk_mod_q, None, pws, c0, a["c1"])
    got = ctx.audit_open(None, sk_mod_q, None, pws, c0, a["c1"], rlc=True, group=GROUP, want_stats=True)
    assert got == want + (ZERO4,) and not any(f & 1 for f in got[1])
    assert ctx.audit_open(vk, sk_mod_q, [], [], c0[:0], a["c1"][:0], rlc=True) == ([], [])


# ------------------------------------------------------------------------------------------------- 8. command line
def test_cli_pool_replay_with_the_rlc_verifier(tmp_path, world, capsys):
    import json
    from spp import cli
    wvk, avk, log = (str(tmp_path / n) for n in ("w.vk", "a.vk", "log.jsonl"))
    open(wvk, "wb").write(world["wvk"]); open(avk, "wb").write(world["avk"])
    A, W = world["A"], world["W"]
    wd = lambda i, p=None: {"withdraw": {"proof": (p or W[i][0]).hex(), "pw": W[i][1].hex(), "recipient": W[i][2].hex()}}
    au = lambda i, p=None: {"submit_audit": {"proof": (p or A[i][0]).hex(), "pw": "0x" + A[i][1].hex()}}
    ins = [wd(0)] + [{"deposit": {"root": r.hex()}} for r in world["roots"]]
    ins += [au(0), au(0), au(1, _flip(A[1][0])), au(2), wd(0), wd(0), wd(1), wd(2, _flip(W[2][0])), wd(2)]
    open(log, "w").write("".join(json.dumps(i) + "\n" for i in ins))
    assert cli.main(["pool-replay", wvk, avk, log]) == 0
    plain = capsys.readouterr().out.split()
    assert cli.main(["pool-replay", wvk, avk, log, "--verifier", "rlc", "--group", str(GROUP)]) == 0
    assert capsys.readouterr().out.split() == plain
    assert plain == ["NO_AUDIT_RECORD"] + ["OK"] * 12 + ["OK", "AUDIT_EXISTS", "BAD_PROOF", "OK", "OK", "NULLIFIER_USED", "NO_AUDIT_RECORD",
                                                          "BAD_PROOF", "OK"]
    assert cli.main(["pool-replay", wvk, avk, log, "--verifier", "rlc", "--group", "100"]) == 2
    assert "group" in capsys.readouterr().err
