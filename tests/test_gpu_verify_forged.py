"""GPU: the batched verifier (k_verify behind spp_verify_batch, k_verify_list behind the pool ledger) on the proofs of
tests/verify_vectors.py: simulated proofs with points at infinity, key points and zero public words, malleated proofs, and forgeries
whose points are all on their curves and canonically encoded, so that they are refused by the pairing (or the subgroup test) that is
there to refuse them and not by the on-curve test a flipped byte ends at.  The expectations are the verdicts the cases have BY
CONSTRUCTION; tests/test_verify_vectors_host.py shows that the oracle and the two host verifiers give the same ones.  In a batch the
lanes of a wave leave verify_one at five different places; no verdict may depend on the lane or on the neighbours.

The pool tests feed the ledger simulated withdraw instructions (the simulator signs ANY public words, so roots, nullifiers,
recipients and audit keys are free to choose) and compare with the sequential PoolModel, whose verifier is the Python oracle, memoised
by bytes, as in tests/test_gpu_pool.py; the model runs once, in a module fixture (about a second per proof that reaches a pairing)."""
import random

import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None

import verify_vectors as V
from test_pool_host import OK, NULLIFIER_USED, BAD_PROOF
from test_gpu_pool import ctx, world, fixed_salt, _same_state, NULLIFIERS, AUDITS, BIG  # noqa: F401
from test_gpu_pool_log import _settle, _model_log
from test_gpu_parity import withdraw_handle, _withdraw_variants  # noqa: F401

pytestmark = pytest.mark.gpu

SEEDS = {"withdraw": b"\x07" * 32, "audit": b"\x09" * 32}               # conftest.py: withdraw_artifacts / audit_artifacts
NPUB = {"withdraw": 5, "audit": 2}


@pytest.fixture(scope="module")
def keys(withdraw_artifacts, audit_artifacts):
    return {"withdraw": open(withdraw_artifacts["vk"], "rb").read(), "audit": open(audit_artifacts["vk"], "rb").read()}


@pytest.fixture(scope="module")
def case_lists(keys):
    return {k: V.cases(keys[k], V.trapdoor(SEEDS[k]), NPUB[k], random.Random(4048 + NPUB[k])) for k in keys}


def _report(cs, got):
    return ["%s (%s): expected %s, got %s" % (c[0], c[4], c[3], g) for c, g in zip(cs, got) if g != c[3]]


@pytest.mark.parametrize("key", ["withdraw", "audit"])
def test_every_case_gets_its_verdict_in_one_batch(ctx, keys, case_lists, key):
    cs = case_lists[key]
    assert len(cs) == V.N_CASES
    got = ctx.verify_batch(keys[key], [c[1] for c in cs], [c[2] for c in cs])
    assert len(got) == len(cs) and not _report(cs, got), "\n".join(_report(cs, got))
    assert got.count(True) == 24


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_verdicts_do_not_depend_on_lane_or_neighbours(ctx, keys, case_lists, n):
    """a seeded shuffle of the case list, cycled up to n proofs: neighbouring lanes leave verify_one at different stages (format,
    subgroup, stage 2, stage 4 refused, stage 4 accepted); the same batch reversed puts every proof on another lane, beside
    other neighbours and, at 65 and 130, in another wave"""
    cs = case_lists["withdraw"]
    order = list(range(len(cs)))
    random.Random(900 + n).shuffle(order)
    batch = [cs[order[k % len(order)]] for k in range(n)]
    if n >= 63:                                                          # the first wave holds all five exits, and most neighbours differ
        assert {c[4] for c in batch[:64]} == set(V.STAGES)
        assert 2 * sum(x[4] != y[4] for x, y in zip(batch, batch[1:])) > n
    for b in (batch, batch[::-1]):
        got = ctx.verify_batch(keys["withdraw"], [c[1] for c in b], [c[2] for c in b])
        assert len(got) == n and not _report(b, got), "\n".join(_report(b, got))


def test_malleated_real_proofs(ctx, keys, withdraw_handle, withdraw_kat):
    """proofs from the GPU prover, not from the simulator: negated, rescaled and re-randomised they stay valid (a verifier that
    refuses them locks funds); with the Krs of another real proof they are not"""
    rows = _withdraw_variants(withdraw_kat, 2)
    proofs, pws, status = withdraw_handle.prove_batch(rows, [(901, 1901), (902, 1904)])
    assert status == [0, 0] and proofs[0][192:256] != proofs[1][192:256]
    vk = keys["withdraw"]
    mal = V.malleations(vk, proofs[0], random.Random(6))
    assert len(mal) == 3 and len({m for _, m in mal} | {proofs[0]}) == 4
    good = [proofs[0]] + [m for _, m in mal]
    bad = [m[:192] + proofs[1][192:256] + m[256:] for m in good]
    got = ctx.verify_batch(vk, good + bad + [proofs[1]], [pws[0]] * 8 + [pws[1]])
    assert got == [True] * 4 + [False] * 4 + [True], got
    from oracle import groth16
    assert groth16.verify(vk, mal[2][1], pws[0])                         # the re-randomised one: Ar, Bs + t delta2, Krs + t Ar


# ---------------------------------------------------------------------------------------------------------------- the pool path
def _bent(kind, k, pts, pw, T):
    """instruction k's valid points bent into a forgery of the given reject class (variants by k)"""
    from oracle import bn254 as B
    Ar, Bs, Krs, Cm, PoK = pts
    if kind == V.STAGE2:
        return V.proof_bytes(Ar, Bs, Krs, Cm, (B.g1_neg(PoK), Cm, None)[k % 3]), pw
    if kind == V.STAGE4:
        return ((V.proof_bytes(Ar, Bs, B.g1_neg(Krs), Cm, PoK), V.proof_bytes(Ar, Bs, B.g1_add(Krs, V.G1), Cm, PoK),
                 V.proof_bytes(B.g1_add(Ar, Ar), Bs, Krs, Cm, PoK), V.proof_bytes(Ar, B.g2_neg(Bs), Krs, Cm, PoK))[k % 4]), pw
    if kind == V.SUBGROUP:
        return V.proof_bytes(Ar, (T, B.g2_add(T, Bs))[k % 2], Krs, Cm, PoK), pw
    good = V.proof_bytes(*pts)
    assert kind == V.FORMAT
    return ((V._put(good, 256, (2).to_bytes(4, "big")), pw), (V._put(good, 0, B.fe_be(B.P)), pw), (V._put(good, 32, bytes(32)), pw),
            (good, V._put(pw, 4, (1).to_bytes(4, "big"))))[k % 4]


def _pool_instructions(wvk):
    """70 withdraw instructions with distinct nullifiers: 5 whose nullifiers are already spent, in front, then 65 that reach the
    verifier, of which two in five are forgeries -- the reject classes in rotation.  [(proof, pw, address, tag)]"""
    from oracle import bn254 as B
    from spp import witness as W_
    rng = random.Random(75)
    td = V.trapdoor(SEEDS["withdraw"])
    vk = V._vk(wvk)
    V.check_trapdoor(vk, td)
    T = V.twist_point_outside_the_subgroup()
    roots = [rng.getrandbits(250).to_bytes(32, "big") for _ in range(2)]
    was = [rng.randrange(B.R).to_bytes(32, "big") for _ in range(3)]
    rejects = (V.FORMAT, V.STAGE2, V.SUBGROUP, V.STAGE4)
    ins, spent = [], []
    n_front, n_body, n_rej = 5, 65, 0
    for k in range(n_front + n_body):
        address = rng.getrandbits(256).to_bytes(32, "big")
        nullifier = rng.randrange(B.R)
        pub = [int.from_bytes(roots[k % 2], "big"), nullifier, W_.recipient_word(address), rng.randrange(1, 1 << 64),
               int.from_bytes(was[k % 3], "big")]
        pw = V.groth16.public_witness_bytes(pub)
        if k < n_front:                                                  # never verified: the nullifier check comes first
            spent.append(nullifier.to_bytes(32, "big"))
            ins.append((ins[0][0] if ins else V.simulate(vk, td, pub, 3, 5, 7)[0], pw, address, "spent"))
            continue
        j = k - n_front
        # points at infinity among the valid ones: Ar (j = 10), Cm and PoK (j = 20), Bs (j = 32)
        a, b, c = (0 if j == 10 else V._big(rng)), (0 if j == 32 else V._big(rng)), (0 if j == 20 else V._big(rng))
        pts = V.simulate_points(vk, td, pub, a, b, c)
        if j % 5 in (1, 3):                                              # 26 forgeries, spread so that no wave of the list is uniform
            kind = rejects[n_rej % 4]
            proof, pw = _bent(kind, n_rej // 4, pts, pw, T)
            n_rej += 1
            ins.append((proof, pw, address, kind))
        else:
            ins.append((V.proof_bytes(*pts), pw, address, V.ACCEPT))
    assert len(ins) == 70 and n_rej == 26 and len({i[1][44:76] for i in ins}) == 70
    return dict(ins=ins, roots=roots, was=was, spent=spent)


def _fresh(world, pool, scene, with_roots):
    model = world["model"]()
    pool.import_keys(AUDITS, scene["was"])
    pool.import_keys(NULLIFIERS, scene["spent"])
    for k in scene["was"]:
        model.audits[k] = True
    for k in scene["spent"]:
        model.nullifiers[k] = True
    if with_roots:
        pool.add_roots(scene["roots"])
        for r in scene["roots"]:
            model.add_root(r)
    return model


@pytest.fixture(scope="module")
def scene(world):
    """the instructions and what the sequential model answers (this is where the oracle's pairings are paid, once)"""
    s = _pool_instructions(world["wvk"])
    model = world["model"]()
    for k in s["was"]:
        model.audits[k] = True
    for k in s["spent"]:
        model.nullifiers[k] = True
    for r in s["roots"]:
        model.add_root(r)
    res = [model.withdraw(p, w, a) for p, w, a, _ in s["ins"]]
    s["want"] = ([c for c, _ in res], [a for _, a in res])
    # the model's verdicts are the ones the instructions have by construction
    assert s["want"][0] == [NULLIFIER_USED if t == "spent" else OK if t == V.ACCEPT else BAD_PROOF for *_, t in s["ins"]]
    return s


def test_pool_withdraw_batch_of_simulated_and_forged_instructions(ctx, world, scene):
    """k_verify_list: 70 instructions, the first 5 settled by the screen, so the list holds 65 proofs (one wave and one lane) and
    lane j verifies instruction j + 5"""
    from spp import witness as W_
    ins = scene["ins"]
    with W_.Pool(ctx, world["wvk"], world["avk"], BIG) as pool:
        model = _fresh(world, pool, scene, True)
        got = pool.withdraw([i[0] for i in ins], [i[1] for i in ins], [i[2] for i in ins])
        wrong = ["%d %s: %d, want %d" % (k, i[3], g, w) for k, (i, g, w) in enumerate(zip(ins, got[0], scene["want"][0])) if g != w]
        assert not wrong, "\n".join(wrong)
        assert got == scene["want"]
        assert [model.withdraw(p, w, a) for p, w, a, _ in ins] == list(zip(*scene["want"]))     # memoised: no pairing is redone
        _same_state(pool, model, world)
        assert pool.counts() == (5 + got[0].count(OK), 3) and got[0].count(OK) == 39
        assert pool.contains(NULLIFIERS, [i[1][44:76] for i in ins]) == [t in ("spent", V.ACCEPT) for *_, t in ins]


def test_pool_log_of_the_same_instructions(ctx, world, scene):
    """the same instructions behind their two deposits, through spp_pool_settle_log"""
    from spp import witness as W_
    log = [(("deposit", r), ("deposit", None)) for r in scene["roots"]] + [(("withdraw", p, w, a), (t, k)) for k, (p, w, a, t) in enumerate(scene["ins"])]
    with W_.Pool(ctx, world["wvk"], world["avk"], BIG) as pool:
        model = _fresh(world, pool, scene, False)
        got = _settle(pool, log)
        assert got == _model_log(model, log)
        assert (got[0][2:], got[1][2:]) == scene["want"] and got[0][:2] == [OK, OK]
        _same_state(pool, model, world)
