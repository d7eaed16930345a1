"""GPU: spp_pool_settle_log -- a log in which deposits, submit_audits and withdraws alternate, settled in one call -- against the
sequential model of the pool program (PoolModel of tests/test_pool_host.py, fed the log ONE instruction at a time; it calls no
spp_pool_* function) and against the three calls that take one kind each.  The deposits, proofs and helpers are those of
tests/test_gpu_pool.py: 12 deposits, 12 withdraw proofs and 12 audit records from the same keys, every withdraw proof against the
last of the 12 roots; tampered variants as there (a flipped proof byte, another account's address, another instruction's public
witness, another root).  The oracle verifier behind the model is memoised by bytes; the module gives it about 50 distinct pairs."""
import random

import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None

from test_pool_host import OK, AUDIT_EXISTS, NO_AUDIT_RECORD, BAD_ROOT, NULLIFIER_USED, BAD_RECIPIENT, BAD_PROOF
from test_gpu_pool import (ctx, world, fixed_salt, _flip, _with_root, _interleave, _same_state, _one_withdraw_pool,  # noqa: F401
                           N, NULLIFIERS, AUDITS, BIG, SMALL)

pytestmark = pytest.mark.gpu

NAMES = ("OK", "AUDIT_EXISTS", "NO_AUDIT_RECORD", "BAD_ROOT", "NULLIFIER_USED", "BAD_RECIPIENT", "BAD_PROOF")


def _variants(world):
    """instruction makers, each returning (instruction, tag)"""
    A, W = world["A"], world["W"]
    unknown_root = random.Random(72).getrandbits(250).to_bytes(32, "big")
    return dict(
        a_good=lambda i: (("submit_audit", A[i][0], A[i][1]), ("a_good", i)),
        a_bad=lambda i: (("submit_audit", _flip(A[i][0]), A[i][1]), ("a_bad", i)),
        a_pw4=lambda i: (("submit_audit", A[i][0], A[4][1]), ("a_pw4", i)),                     # proof i under the public witness of 4
        w_good=lambda i: (("withdraw", W[i][0], W[i][1], W[i][2]), ("w_good", i)),
        w_bad=lambda i: (("withdraw", _flip(W[i][0]), W[i][1], W[i][2]), ("w_bad", i)),
        w_other=lambda i: (("withdraw", W[i][0], W[i][1], W[(i + 1) % N][2]), ("w_other", i)),  # another account's address
        w_pw4=lambda i: (("withdraw", W[i][0], W[4][1], W[4][2]), ("w_pw4", i)),
        w_root=lambda i: (("withdraw", W[i][0], _with_root(W[i][1], unknown_root), W[i][2]), ("w_root", i)),
        deposit=lambda r: (("deposit", r), ("deposit", None)))


def _interleaved_log(world):
    """the 12 deposits, then per identity a sequence of audit and withdraw variants in an order of its own, the sequences interleaved
    at random: [(instruction, tag)].  The comments give what the program answers, whatever the interleaving."""
    v, rng = _variants(world), random.Random(73)
    seqs = [[v["a_bad"](0), v["a_good"](0), v["w_bad"](0), v["w_good"](0), v["w_good"](0), v["a_good"](0)],
            # BAD_PROOF, OK, BAD_PROOF, OK, NULLIFIER_USED, AUDIT_EXISTS
            [v["w_good"](1), v["a_good"](1), v["w_good"](1), v["w_other"](1)],
            # the withdraw ahead of its audit: NO_AUDIT_RECORD, OK, OK, NULLIFIER_USED (before the recipient check)
            [v["w_other"](2), v["a_bad"](2), v["w_good"](2), v["a_good"](2), v["w_other"](2), v["w_good"](2), v["w_other"](2)],
            # ahead of any audit, then after an invalid one only: NO_AUDIT_RECORD, BAD_PROOF, NO_AUDIT_RECORD, OK, BAD_RECIPIENT, OK, NULLIFIER_USED
            [v["a_pw4"](3), v["a_good"](4), v["a_good"](3), v["w_pw4"](3), v["w_good"](4), v["w_good"](3)],
            # BAD_PROOF (key 4 stays free), OK, OK, BAD_PROOF (nullifier 4 stays free), OK, OK
            [v["a_good"](5), v["w_root"](5), v["w_good"](5)],            # OK, BAD_ROOT, OK
            [v["a_bad"](6), v["w_good"](6)],                             # BAD_PROOF, NO_AUDIT_RECORD
            [v["w_good"](10)],                                           # no audit at all: NO_AUDIT_RECORD
            [v["w_root"](11)]]                                           # ... and an unknown root: NO_AUDIT_RECORD comes first
    picks = ("a_good", "a_bad", "w_good", "w_good", "w_bad", "w_other")
    for i in range(7, 10):
        seqs.append([v[rng.choice(picks)](i) for _ in range(rng.randrange(6, 9))])
    body = _interleave(rng, *seqs)
    while len(body) < 58:
        body.append(v[rng.choice(picks)](rng.randrange(7, 10)))
    return [v["deposit"](r) for r in world["roots"]] + body


def _settle(pool, log):
    return pool.settle_log([ins for ins, _ in log])


def _model_log(model, log):
    codes, amounts = [], []
    for ins, _ in log:                                                   # one at a time
        if ins[0] == "deposit":
            model.add_root(ins[1])
            codes.append(OK); amounts.append(0)
        elif ins[0] == "submit_audit":
            codes.append(model.submit_audit(ins[1], ins[2])); amounts.append(0)
        else:
            c, a = model.withdraw(ins[1], ins[2], ins[3])
            codes.append(c); amounts.append(a)
    return codes, amounts


def _cut_into_runs(pool, log):
    """the log through the three calls that take one kind each, a call per run of one kind"""
    codes, amounts, i = [], [], 0
    while i < len(log):
        j = i
        while j < len(log) and log[j][0][0] == log[i][0][0]:
            j += 1
        cols = list(zip(*(ins[1:] for ins, _ in log[i:j])))
        if log[i][0][0] == "deposit":
            pool.add_roots(cols[0])
            c, a = [OK] * (j - i), [0] * (j - i)
        elif log[i][0][0] == "submit_audit":
            c, a = pool.submit_audit(cols[0], cols[1]), [0] * (j - i)
        else:
            c, a = pool.withdraw(cols[0], cols[1], cols[2])
        codes += c; amounts += a
        i = j
    return codes, amounts


def _observed(pool, world):
    return (pool.state(), pool.counts(), pool.contains(NULLIFIERS, world["nullifiers"]), pool.contains(AUDITS, world["was"]))


def _at(log, got, *tags):
    return [got[k] for t in tags for k, (_, tag) in enumerate(log) if tag == t]


@pytest.fixture(scope="module")
def settled(ctx, world):
    from spp import witness as W_
    log, model = _interleaved_log(world), world["model"]()
    want = _model_log(model, log)
    with W_.Pool(ctx, world["wvk"], world["avk"], BIG) as pool:
        got = _settle(pool, log)
        _same_state(pool, model, world)
        seen = _observed(pool, world)
    return dict(log=log, got=got, want=want, seen=seen)


def test_interleaved_log_settles_as_the_program_would_in_order(settled, world):
    log, (got, amounts) = settled["log"], settled["got"]
    print("log:", " ".join("%s%s" % (t[0], "" if t[1] is None else t[1]) for _, t in log), "\ncodes:", [NAMES[c] for c in got])
    assert 65 <= len(log) <= 75 and (got, amounts) == settled["want"]
    assert set(got) == {OK, AUDIT_EXISTS, NO_AUDIT_RECORD, BAD_ROOT, NULLIFIER_USED, BAD_RECIPIENT, BAD_PROOF}
    assert got[:N] == [OK] * N and amounts[:N] == [0] * N
    assert _at(log, got, ("a_bad", 0), ("a_good", 0)) == [BAD_PROOF, OK, AUDIT_EXISTS]
    assert _at(log, got, ("w_bad", 0), ("w_good", 0)) == [BAD_PROOF, OK, NULLIFIER_USED]
    # identities 1 and 2: the withdraw is ahead of the submit_audit that creates its record
    assert _at(log, got, ("w_good", 1), ("a_good", 1), ("w_other", 1)) == [NO_AUDIT_RECORD, OK, OK, NULLIFIER_USED]
    assert _at(log, got, ("w_other", 2)) == [NO_AUDIT_RECORD, BAD_RECIPIENT, NULLIFIER_USED]
    assert _at(log, got, ("a_bad", 2), ("w_good", 2), ("a_good", 2)) == [BAD_PROOF, NO_AUDIT_RECORD, OK, OK]
    assert _at(log, got, ("a_pw4", 3), ("a_good", 4), ("a_good", 3), ("w_pw4", 3), ("w_good", 4), ("w_good", 3)) == [BAD_PROOF, OK, OK, BAD_PROOF, OK, OK]
    assert _at(log, got, ("a_good", 5), ("w_root", 5), ("w_good", 5)) == [OK, BAD_ROOT, OK]
    assert _at(log, got, ("a_bad", 6), ("w_good", 6), ("w_good", 10), ("w_root", 11)) == [BAD_PROOF] + [NO_AUDIT_RECORD] * 3
    # amounts: the notes' amounts for every withdraw whatever became of it (the pw of 4 carries the amount of 4), 0 elsewhere
    for (ins, tag), a in zip(log, amounts):
        assert a == (0 if ins[0] != "withdraw" else world["amounts"][4 if tag[0] == "w_pw4" else tag[1]]), tag
    assert settled["seen"][1] == (sum(c == OK for (i, _), c in zip(log, got) if i[0] == "withdraw"),
                                  sum(c == OK for (i, _), c in zip(log, got) if i[0] == "submit_audit"))


def test_one_call_equals_cutting_the_log_into_runs(ctx, world):
    from spp import witness as W_
    v, rng = _variants(world), random.Random(74)
    more = [rng.getrandbits(250).to_bytes(32, "big") for _ in range(3)]
    runs = [[v["deposit"](r) for r in world["roots"]],
            [v["a_good"](0), v["a_good"](1), v["a_bad"](2)],
            [v["w_good"](0), v["w_good"](2), v["w_good"](1), v["w_good"](5)],
            [v["deposit"](more[0]), v["deposit"](more[1])],
            [v["a_good"](2), v["a_good"](0)],
            [v["w_good"](2), v["w_good"](0), v["w_other"](1)],
            [v["a_good"](5)],
            [v["w_other"](5), v["w_good"](5)],
            [v["deposit"](more[2])],
            [v["a_bad"](6), v["a_good"](5)],
            [v["w_good"](6), v["w_good"](5)]]
    log = [x for run in runs for x in run]
    assert len(runs) <= 12
    with W_.Pool(ctx, world["wvk"], world["avk"], BIG) as one, W_.Pool(ctx, world["wvk"], world["avk"], BIG) as cut:
        got, by_runs = _settle(one, log), _cut_into_runs(cut, log)
        print("one call:", [NAMES[c] for c in got[0]])
        assert got == by_runs
        assert _observed(one, world) == _observed(cut, world)
        model = world["model"]()
        assert got == _model_log(model, log)
        _same_state(one, model, world)
    assert got[0][N:] == [OK, OK, BAD_PROOF, OK, NO_AUDIT_RECORD, OK, NO_AUDIT_RECORD, OK, OK, OK, AUDIT_EXISTS, OK, NULLIFIER_USED, NULLIFIER_USED,
                          OK, BAD_RECIPIENT, OK, OK, BAD_PROOF, AUDIT_EXISTS, NO_AUDIT_RECORD, NULLIFIER_USED]


def _split_points(log):
    tags = [t for _, t in log]
    inside_the_deposits = 5                                              # 5 roots resident, 7 pushed by the second call
    after_the_audit = tags.index(("a_good", 5)) + 1                      # identity 5: its record resident, its withdraws in the second call
    between = tags.index(("a_good", 2)) + 1                              # identity 2: withdraws on both sides of its record
    return inside_the_deposits, after_the_audit, between


@pytest.mark.parametrize("which", [0, 1, 2])
def test_a_log_settled_in_two_calls_equals_the_single_call(ctx, world, settled, which):
    from spp import witness as W_
    log = settled["log"]
    k = _split_points(log)[which]
    assert 0 < k < len(log) and (which or log[k][0][0] == "deposit" == log[k - 1][0][0])
    with W_.Pool(ctx, world["wvk"], world["avk"], BIG) as pool:
        first, second = _settle(pool, log[:k]), _settle(pool, log[k:])
        assert (first[0] + second[0], first[1] + second[1]) == settled["got"]
        assert _observed(pool, world) == settled["seen"]


@pytest.mark.parametrize("before", [0, 5, 40])
def test_a_root_leaves_the_ring_after_exactly_32_later_roots_inside_a_log(ctx, world, before):
    """the proofs are against roots[11]: 31 roots pushed after it by the same log leave it in the ring, the 32nd overwrites it --
    on a fresh ring, and where the log's pushes continue a ring that 5 or 40 earlier pushes have filled"""
    from spp import witness as W_
    v, rng = _variants(world), random.Random(75 + before)
    earlier = [rng.getrandbits(250).to_bytes(32, "big") for _ in range(before)]
    later = [rng.getrandbits(250).to_bytes(32, "big") for _ in range(32)]
    log = [v["deposit"](r) for r in world["roots"]] + [v["a_good"](7), v["a_good"](8)] + [v["deposit"](r) for r in later[:31]]
    log += [v["w_good"](7), v["deposit"](later[31]), v["w_good"](8)]
    model = world["model"]()
    with W_.Pool(ctx, world["wvk"], world["avk"], SMALL) as pool:
        pool.add_roots(earlier)
        for r in earlier:
            model.add_root(r)
        got, amounts = _settle(pool, log)
        assert (got, amounts) == _model_log(model, log)
        assert _at(log, got, ("w_good", 7), ("w_good", 8)) == [OK, BAD_ROOT] and got.count(OK) == len(log) - 1
        assert _at(log, amounts, ("w_good", 7), ("w_good", 8)) == [world["amounts"][7], world["amounts"][8]]
        _same_state(pool, model, world)
        assert pool.counts() == (1, 2)


def test_the_zero_root_passes_until_the_32nd_root_of_the_log(ctx, world):
    """a fresh pool's empty slots hold the zero root (initialize.rs:65-69): after 31 deposits of the log slot 31 is still zero and
    the zero-root withdraw gets as far as its proof, after the 32nd it is a bad root"""
    v, rng = _variants(world), random.Random(76)
    p, w, a = world["W"][8]
    zero = (("withdraw", p, _with_root(w, bytes(32)), a), ("w_zero", 8))
    more = [rng.getrandbits(250).to_bytes(32, "big") for _ in range(32)]
    log = [zero] + [v["deposit"](r) for r in more[:31]] + [zero, v["deposit"](more[31]), zero]
    pool, model = _one_withdraw_pool(ctx, world, 8)
    with pool:
        got, _ = _settle(pool, log)
        assert got == _model_log(model, log)[0]
        assert _at(log, got, ("w_zero", 8)) == [BAD_PROOF, BAD_PROOF, BAD_ROOT]
        _same_state(pool, model, world)


def test_degenerate_logs(ctx, world):
    from spp import witness as W_
    v = _variants(world)
    model = world["model"]()
    with W_.Pool(ctx, world["wvk"], world["avk"], SMALL) as pool:
        before = _observed(pool, world)
        assert pool.settle_log([]) == ([], []) and _observed(pool, world) == before
        logs = ([v["deposit"](r) for r in world["roots"]],                                   # deposits only
                [v["a_good"](0), v["a_bad"](1), v["a_good"](0)],                             # audits only
                [v["w_good"](0), v["w_good"](3), v["w_good"](1), v["w_good"](0)])            # withdraws only, on resident records
        pool.import_keys(AUDITS, [world["was"][3]])
        model.audits[world["was"][3]] = True
        want = ([OK] * N, [OK, BAD_PROOF, AUDIT_EXISTS], [OK, OK, NO_AUDIT_RECORD, NULLIFIER_USED])
        for log, codes in zip(logs, want):
            got = _settle(pool, log)
            assert got == _model_log(model, log) and got[0] == codes
            _same_state(pool, model, world)
        assert pool.counts() == (2, 2)


def test_refused_logs_change_nothing(ctx, world):
    import ctypes
    import spp
    from spp import witness as W_
    v = _variants(world)
    A, W = world["A"], world["W"]
    with W_.Pool(ctx, world["wvk"], world["avk"], SMALL) as pool:
        assert _settle(pool, [v["deposit"](r) for r in world["roots"][-3:]] + [v["a_good"](0), v["w_good"](0)])[0] == [OK] * 5
        before = _observed(pool, world)
        res, amt = (ctypes.c_int32 * 4)(), (ctypes.c_uint64 * 4)()
        rp, ap = ctypes.cast(res, ctypes.c_void_p), ctypes.cast(amt, ctypes.c_void_p)
        raw = lambda kinds, nd, na, nw: ctx.L.spp_pool_settle_log(pool.h, len(kinds), bytes(kinds), nd, world["roots"][3] * nd, na, A[1][0] * na,
                                                                  A[1][1] * na, nw, W[1][0] * nw, W[1][1] * nw, W[1][2] * nw, rp, ap)
        assert raw([0, 1, 3], 1, 1, 1) == -1 and "kinds" in spp.last_error()       # a kind byte above 2
        assert raw([0, 1, 2], 2, 1, 0) == -1                                        # counts that do not match kinds
        assert raw([0, 1, 2], 1, 1, 2) == -1                                        # ... or do not sum to count
        assert raw([0, 0, 2], 1, 1, 1) == -1
        assert _observed(pool, world) == before
        # one nullifier of 32: a log with 32 more withdraws could overflow the set -- refused whatever the instructions are
        for log in ([v["deposit"](world["roots"][3])] + [v["w_good"](1)] * 32, [v["a_good"](1)] * 32 + [v["deposit"](world["roots"][3])]):
            with pytest.raises(spp.SppError) as e:
                _settle(pool, log)
            assert e.value.code == -1 and "overflow" in str(e.value)
        assert _observed(pool, world) == before and pool.counts() == (1, 1)
        assert _settle(pool, [v["deposit"](world["roots"][3])] + [v["w_good"](1)] * 31)[0] == [OK] + [NO_AUDIT_RECORD] * 31    # 31 more still go


def test_cli_pool_replay_of_an_alternating_log(tmp_path, world, capsys):
    import json
    from spp import cli
    v = _variants(world)
    wvk, avk, path = (str(tmp_path / n) for n in ("w.vk", "a.vk", "log.jsonl"))
    open(wvk, "wb").write(world["wvk"]); open(avk, "wb").write(world["avk"])
    log = []
    for i in range(10):                                                  # deposit, submit_audit, withdraw, ... : the proofs' root first
        audit = v["a_bad"](3) if i == 3 else v["a_good"](5) if i == 6 else v["a_good"](i)
        withdraw = v["w_other"](4) if i == 4 else v["w_good"](2) if i == 7 else v["w_good"](i)
        log += [v["deposit"](world["roots"][N - 1 - i]), audit, withdraw]
    lines = []
    for ins, _ in log:
        body = dict(zip({"deposit": ("root",), "submit_audit": ("proof", "pw"), "withdraw": ("proof", "pw", "recipient")}[ins[0]],
                        (x.hex() for x in ins[1:])))
        lines.append(json.dumps({ins[0]: body}))
    open(path, "w").write("\n".join(lines) + "\n")
    assert len(lines) == 30 and cli.main(["pool-replay", wvk, avk, path]) == 0
    want = [NAMES[c] for c in _model_log(world["model"](), log)[0]]
    assert capsys.readouterr().out.split() == want
    assert want[9:12] == ["OK", "BAD_PROOF", "NO_AUDIT_RECORD"] and want[12:15] == ["OK", "OK", "BAD_RECIPIENT"]
    assert want[18:24] == ["OK", "AUDIT_EXISTS", "NO_AUDIT_RECORD", "OK", "OK", "NULLIFIER_USED"]
