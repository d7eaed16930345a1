"""GPU: the random-linear-combination batch verifier (k_verify_rlc_terms, k_verify_rlc_group and, for refused groups, k_verify_list
behind spp_verify_batch_rlc) on the proofs of tests/verify_vectors.py.  The expectations are the verdicts the cases have BY
CONSTRUCTION, and the verdicts of spp_verify_batch on the same batch.  The stats (groups, groups refused, proofs re-verified, proofs
dropped) are asserted wherever they are known: on valid proofs no group may be refused, so the fallback cannot hide a cooperative
tail that wrongly refuses.  tests/test_verify_rlc_host.py runs the same scheme as a g++ build."""
import random

import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None

import verify_vectors as V
import verify_rlc_vectors as RV
from test_gpu_verify_forged import ctx, keys, case_lists, SEEDS, NPUB, _report  # noqa: F401
from test_gpu_parity import withdraw_handle, _withdraw_variants  # noqa: F401

pytestmark = pytest.mark.gpu

SERIAL_TAIL, NO_FALLBACK = 1, 2
RLC_SEEDS = (bytes(range(32)), b"\xa5" * 32)


def _rlc(ctx, vk, batch, **kw):
    return ctx.verify_batch_rlc(vk, [c[1] for c in batch], [c[2] for c in batch], **kw)


@pytest.fixture(scope="module")
def per_proof(ctx, keys, case_lists):
    """spp_verify_batch on the 55 cases of each key, once"""
    return {k: ctx.verify_batch(keys[k], [c[1] for c in case_lists[k]], [c[2] for c in case_lists[k]]) for k in keys}


@pytest.mark.parametrize("flags", [0, SERIAL_TAIL])
@pytest.mark.parametrize("group", [64, 0])
@pytest.mark.parametrize("key", ["withdraw", "audit"])
def test_every_case_gets_its_verdict_in_one_batch(ctx, keys, case_lists, per_proof, key, group, flags):
    cs = case_lists[key]
    assert len(cs) == V.N_CASES
    got, stats = _rlc(ctx, keys[key], cs, seed=RLC_SEEDS[0], group=group, flags=flags, want_stats=True)
    assert len(got) == len(cs) and not _report(cs, got), "\n".join(_report(cs, got))
    assert got == per_proof[key] and got.count(True) == 24
    assert stats == (1, 1, 39, 16)                                       # 12 format + 4 subgroup dropped, the other 39 settled one by one


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_verdicts_do_not_depend_on_lane_or_neighbours(ctx, keys, case_lists, n):
    """the seeded shuffle of tests/test_gpu_verify_forged.py and its reverse; 130 proofs are three groups, the last with two live lanes"""
    cs = case_lists["withdraw"]
    order = list(range(len(cs)))
    random.Random(900 + n).shuffle(order)
    batch = [cs[order[k % len(order)]] for k in range(n)]
    for b in (batch, batch[::-1]):
        got, stats = _rlc(ctx, keys["withdraw"], b, seed=RLC_SEEDS[1], group=64, want_stats=True)
        assert len(got) == n and not _report(b, got), "\n".join(_report(b, got))
        assert stats[0] == (n + 63) // 64 and stats[3] == sum(c[4] in (V.FORMAT, V.SUBGROUP) for c in b)


@pytest.mark.parametrize("group, stats", [(64, (4, 0, 0, 0)), (256, (1, 0, 0, 0))])
def test_all_valid_batch_re_verifies_nothing(ctx, keys, case_lists, group, stats):
    """200 accepts: full groups, a partial group and more than one group at 64; one partial group at 256"""
    batch = RV.cycled(RV.accepts(case_lists["withdraw"]), 200)
    for seed in RLC_SEEDS:
        got, st = _rlc(ctx, keys["withdraw"], batch, seed=seed, group=group, want_stats=True)
        assert got == [True] * 200 and st == stats, (seed, st)


@pytest.mark.parametrize("stage", [V.STAGE2, V.STAGE4, V.FORMAT, V.SUBGROUP])
def test_one_forgery_in_192_valid_proofs(ctx, keys, case_lists, stage):
    cs = case_lists["withdraw"]
    batch = RV.cycled(RV.accepts(cs), 192)
    at = 64 + 29
    batch[at] = next(c for c in cs if c[4] == stage)
    got, stats = _rlc(ctx, keys["withdraw"], batch, seed=RLC_SEEDS[0], group=64, want_stats=True)
    assert got == [k != at for k in range(192)], [k for k in range(192) if got[k] != (k != at)]
    assert stats == ((3, 1, 64, 0) if stage in (V.STAGE2, V.STAGE4) else (3, 0, 0, 1))


@pytest.mark.parametrize("kind", RV.KINDS)
def test_cancelling_pairs_inside_a_valid_group(ctx, keys, case_lists, kind):
    """two proofs whose errors cancel when both are weighted alike (tests/verify_rlc_vectors.py; the host test asserts that their
    unweighted product is one), adjacent in an otherwise valid group of 64"""
    vk = keys["withdraw"]
    pairs = RV.cancelling_pairs(vk, V.trapdoor(SEEDS["withdraw"]), NPUB["withdraw"], random.Random(77))
    valid = RV.cycled(RV.accepts(case_lists["withdraw"]), 62)
    pair = [(kind, p, w) for p, w in pairs[kind]]
    batch = valid[:31] + pair + valid[31:]
    got, stats = _rlc(ctx, vk, batch, seed=RLC_SEEDS[1], group=64, want_stats=True)
    assert got == [k not in (31, 32) for k in range(64)] and stats == (1, 1, 64, 0)
    got, stats = _rlc(ctx, vk, batch, seed=RLC_SEEDS[1], group=64, flags=NO_FALLBACK, want_stats=True)
    assert got == [False] * 64 and stats == (1, 1, 0, 0)                 # without the fallback the whole group reads 0
    got = _rlc(ctx, vk, pair, seed=RLC_SEEDS[0], group=64, flags=NO_FALLBACK | SERIAL_TAIL)
    assert got == [False, False]


def test_seeds_do_not_change_the_verdicts(ctx, keys, case_lists, per_proof):
    cs = case_lists["audit"]
    for seed in (None,) + RLC_SEEDS:
        assert _rlc(ctx, keys["audit"], cs, seed=seed) == per_proof["audit"], seed


def test_malleated_real_proofs(ctx, keys, withdraw_handle, withdraw_kat):
    """proofs from the GPU prover, as tests/test_gpu_verify_forged.py::test_malleated_real_proofs builds them"""
    rows = _withdraw_variants(withdraw_kat, 2)
    proofs, pws, status = withdraw_handle.prove_batch(rows, [(901, 1901), (902, 1904)])
    assert status == [0, 0] and proofs[0][192:256] != proofs[1][192:256]
    vk = keys["withdraw"]
    mal = V.malleations(vk, proofs[0], random.Random(6))
    good = [proofs[0]] + [m for _, m in mal]
    bad = [m[:192] + proofs[1][192:256] + m[256:] for m in good]
    got = ctx.verify_batch_rlc(vk, good + bad + [proofs[1]], [pws[0]] * 8 + [pws[1]])
    assert got == [True] * 4 + [False] * 4 + [True], got
    got, stats = ctx.verify_batch_rlc(vk, good + [proofs[1]], [pws[0]] * 4 + [pws[1]], want_stats=True)
    assert got == [True] * 5 and stats == (1, 0, 0, 0)


def test_cli_verify_batch(keys, case_lists, tmp_path, capsys):
    """python -m spp.cli verify-batch <vk> <proof> <pw> ...: one verdict per pair, exit 0 iff all verify"""
    from spp import cli
    cs = case_lists["audit"]
    picks = [RV.accepts(cs)[0], next(c for c in cs if c[4] == V.STAGE4), RV.accepts(cs)[1]]
    vk = tmp_path / "a.vk"
    vk.write_bytes(keys["audit"])
    files = []
    for k, c in enumerate(picks):
        (tmp_path / ("%d.proof" % k)).write_bytes(c[1])
        (tmp_path / ("%d.pw" % k)).write_bytes(c[2])
        files += [str(tmp_path / ("%d.proof" % k)), str(tmp_path / ("%d.pw" % k))]
    assert cli.main(["verify-batch", str(vk)] + files) == 1
    out = capsys.readouterr().out.strip().splitlines()
    assert [l.rsplit(" ", 1)[1] for l in out] == ["succeeded", "FAILED", "succeeded"] and out[1].startswith(files[2])
    assert cli.main(["verify-batch", str(vk)] + files[:2] + files[4:]) == 0
