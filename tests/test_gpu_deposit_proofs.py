"""Deposit proofs on the GPU (spp_deposit_rows_from_tree, spp_prove_deposits(_device), spp_verify_deposit_chain): k_deposit_rows against
the Python model (tests/deposit_model.py) and, independently, against the tree's own as-of answers; the proofs against the oracle's
prover and the batch verifier; refusal in place; a record that is not the deposit at its index; the chain check against the model's
rule on a log with one failure at a time; the command-line round trip."""
import json
import os
import random

import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None
from conftest import GOLDEN
import deposit_model as M

pytestmark = pytest.mark.gpu

R = M.R
DEPTH = 16
BAD_INPUT, FORMAT = -1, -7
N_GROWN = 130          # 65 + 65: every (first, count) below fits
BATCHES = ((0, 1), (1, 62), (63, 1), (64, 1), (65, 62), (127, 3))            # (first_index, count) of the tree.deposit calls
ASKS = [(f, c) for f in (0, 1, 63, 64, 65) for c in (1, 64, 65)] + [(127, 1), (127, 3)]


@pytest.fixture(scope="module")
def ctx():
    import spp
    c = spp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def keys(ctx, workdir):
    """the deposit circuit set up on the GPU under a fixed seed, and loaded"""
    import spp
    sppc, pk, vk = (os.path.join(workdir, "gpu_deposit." + e) for e in ("sppc", "pk", "vk"))
    spp.build_circuit(6, sppc)
    ctx.setup(sppc, b"\x0d" * 32, pk, vk)
    h = ctx.load_circuit(sppc, pk, 6)
    yield dict(sppc=sppc, pk=pk, vk=open(vk, "rb").read(), vk_path=vk, handle=h)
    h.close()


@pytest.fixture(scope="module")
def records():
    rng = random.Random(0xDE9)
    return [(rng.randrange(1, R), rng.randrange(1 << 64), rng.randrange(R)) for _ in range(N_GROWN)]


@pytest.fixture(scope="module")
def model(records):
    """the model's rows of all N_GROWN deposits, computed once"""
    return M.rows_for_deposits(records)[1]


@pytest.fixture(scope="module")
def grown(ctx, records):
    """one depth-16 tree filled by tree.deposit in BATCHES; the rows asked for when it held N_GROWN leaves, then ten more leaves"""
    from spp import witness as W
    tree = W.ShieldedPoolMerkleTree(ctx, DEPTH)
    for first, count in BATCHES:
        assert tree.deposit(records[first:first + count])[0] == first
    assert len(tree) == N_GROWN
    then = {(f, c): tree.deposit_rows(f, records[f:f + c]) for f, c in ASKS}
    rng = random.Random(5)
    tree.deposit([(rng.randrange(1, R), rng.randrange(1 << 64), rng.randrange(R)) for _ in range(10)])
    yield dict(tree=tree, then=then)
    tree.close()


def _rs(count, seed):
    rng = random.Random(seed)
    return [(rng.randrange(1, 1 << 250), rng.randrange(1, 1 << 250)) for _ in range(count)]


def _pw(words):
    return (5).to_bytes(4, "big") + bytes(4) + (5).to_bytes(4, "big") + b"".join(M.word(v) for v in words)


def test_rows_equal_the_model_at_the_wave_boundaries(grown, model):
    for (f, c), rows in grown["then"].items():
        assert len(rows) == c
        for k, row in enumerate(rows):
            assert row == model[f + k], (f, c, k, [j for j in range(M.ROW_FIELDS) if row[j] != model[f + k][j]])


def test_rows_equal_the_trees_own_paths_and_roots(grown):
    tree = grown["tree"]
    roots = tree.prefix_roots(0, N_GROWN + 1)
    seen = {}
    for (f, c), rows in grown["then"].items():
        for k, row in enumerate(rows):
            seen[f + k] = row
    assert sorted(seen) == list(range(N_GROWN))
    for i, row in seen.items():
        assert row[0] == roots[i] and row[1] == roots[i + 1] and row[4] == i, i
        assert row[8:] == tree.proofs_at(i, [i])[0], i
    for i in (0, 63, 64, 129):
        assert seen[i][0] == tree.root_at(i) and seen[i][1] == tree.root_at(i + 1)


def test_rows_of_old_indices_do_not_change_when_leaves_arrive(grown, records):
    tree = grown["tree"]
    assert len(tree) == N_GROWN + 10
    for f, c in ((0, 65), (63, 65), (65, 65), (127, 3), (64, 1)):
        assert tree.deposit_rows(f, records[f:f + c]) == grown["then"][(f, c)], (f, c)


def test_last_slots_of_a_full_tree_and_the_range_refusal(ctx):
    import spp
    from spp import witness as W
    rng = random.Random(0xF011)
    with W.ShieldedPoolMerkleTree(ctx, DEPTH) as tree:
        tree.insert_many([rng.randrange(R) for _ in range((1 << DEPTH) - 2)])
        recs = [(rng.randrange(1, R), rng.randrange(1 << 64), rng.randrange(R)) for _ in range(2)]
        first, commitments, roots = tree.deposit(recs)
        assert first == (1 << DEPTH) - 2 and len(tree) == 1 << DEPTH
        rows = tree.deposit_rows(first, recs)
        for k, (rec, row) in enumerate(zip(recs, rows)):
            i = first + k
            sibs = tree.proofs_at(i, [i])[0]
            owner, c = M.commitment_of(rec)
            assert c == commitments[k]
            assert row == M.row_from_parts(owner, rec[1], rec[2], i, sibs, c), i
            assert row[0] == tree.root_at(i) and row[1] == tree.root_at(i + 1) == roots[k]
        assert rows[1][8:8 + 1] == [commitments[0]] and rows[1][1] == tree.getRoot()
        assert tree.deposit_rows(first + 1, recs[1:]) == rows[1:]
        assert tree.deposit_rows(first, []) == [] and tree.deposit_rows(1 << DEPTH, []) == []
    with W.ShieldedPoolMerkleTree(ctx, DEPTH) as tree:
        tree.deposit(recs)
        root = tree.getRoot()
        for f, part in ((1, recs), (2, recs[:1]), (3, []), ((1 << 64) - 1, recs)):
            with pytest.raises(spp.lib.SppError) as e:
                tree.deposit_rows(f, part)
            assert e.value.code == BAD_INPUT and "2 leaves" in str(e.value), f
        with pytest.raises(spp.lib.SppError) as e:
            tree.deposit_rows(0, [recs[0], (0, 1, 2)])
        assert e.value.code == BAD_INPUT and "deposit 1: secret_key is 0" in str(e.value)
        with pytest.raises(spp.lib.SppError) as e:
            tree.deposit_rows(0, [(R, 1, 2)])
        assert e.value.code == BAD_INPUT and "deposit 0" in str(e.value)
        assert len(tree) == 2 and tree.getRoot() == root


@pytest.fixture(scope="module")
def proved(ctx, keys, records):
    """a second tree with the same first 128 leaves: 63 by tree.deposit, then 65 deposited and proved with fixed rs"""
    from spp import witness as W
    tree = W.ShieldedPoolMerkleTree(ctx, DEPTH)
    tree.deposit(records[:63])
    rs = _rs(65, 99)
    first, commitments, roots, proofs, pws, status = tree.deposit_proved(keys["handle"], records[63:128], rs)
    assert first == 63 and len(tree) == 128
    yield dict(tree=tree, rs=rs, first=first, commitments=commitments, roots=roots, proofs=proofs, pws=pws, status=status)
    tree.close()


def test_proofs_equal_the_oracle_and_verify(ctx, keys, proved, model):
    from oracle import native
    assert proved["status"] == [0] * 65
    orc = native.Prover(keys["sppc"], keys["pk"])
    for k in (0, 63, 64):                                                    # first, the wave boundary, last (the tail workspace)
        rc, proof, pw = orc.prove(model[63 + k], *proved["rs"][k])
        assert rc == 0 and proved["proofs"][k] == proof and proved["pws"][k] == pw, k
    assert ctx.verify_batch(keys["vk"], proved["proofs"], proved["pws"]) == [True] * 65
    for k in range(65):
        assert proved["pws"][k] == _pw(model[63 + k][:5]), k
        assert proved["commitments"][k] == model[63 + k][2] and proved["roots"][k] == model[63 + k][1]


def test_device_entry_point_gives_the_same_bytes(keys, proved, records):
    from spp import witness as W
    h, tree = keys["handle"], proved["tree"]
    dev = lambda raw: torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(torch.device("cuda", 0))
    d_dep = dev(W.pack_deposits(records[63:128]))
    d_rs = dev(b"".join(int(r).to_bytes(32, "big") + int(s).to_bytes(32, "big") for r, s in proved["rs"]))
    d_proofs = torch.zeros(65 * 388, dtype=torch.uint8, device="cuda:0")
    d_pws = torch.zeros(65 * 172, dtype=torch.uint8, device="cuda:0")
    d_status = torch.full((65,), 7, dtype=torch.int32, device="cuda:0")
    h.prove_deposits_device(tree, 63, 65, d_dep.data_ptr(), d_rs.data_ptr(), d_proofs.data_ptr(), d_pws.data_ptr(), d_status.data_ptr())
    h.sync()
    assert d_status.cpu().tolist() == [0] * 65
    assert bytes(d_proofs.cpu().numpy()) == b"".join(proved["proofs"]) and bytes(d_pws.cpu().numpy()) == b"".join(proved["pws"])


def test_argument_refusals(ctx, keys, proved, records, withdraw_artifacts):
    import spp
    from spp import witness as W
    h, tree = keys["handle"], proved["tree"]
    for first, part in ((64, records[63:128]), (128, records[:1]), (1 << 63, records[:1])):
        with pytest.raises(spp.lib.SppError) as e:
            h.prove_deposits(tree, first, part)
        assert e.value.code == BAD_INPUT and "128 leaves" in str(e.value)
    assert h.prove_deposits(tree, 128, []) == ([], [], [])
    with W.ShieldedPoolMerkleTree(ctx, 8) as shallow:
        shallow.deposit(records[:1])
        with pytest.raises(spp.lib.SppError) as e:
            h.prove_deposits(shallow, 0, records[:1])
        assert e.value.code == BAD_INPUT and "depth" in str(e.value)
    hw = ctx.load_circuit(withdraw_artifacts["sppc"], withdraw_artifacts["pk"], 6)
    try:
        with pytest.raises(spp.lib.SppError) as e:
            hw.prove_deposits(tree, 0, records[:1])
        assert e.value.code == BAD_INPUT and "not a deposit circuit" in str(e.value)
    finally:
        hw.close()
    with pytest.raises(spp.lib.SppError) as e:
        h.prove_deposits(tree, 0, [(0, 1, 2)])
    assert e.value.code == BAD_INPUT and "secret_key is 0" in str(e.value)
    assert len(tree) == 128


def test_amount_two_to_the_64_is_refused_in_place(ctx, keys, proved, records):
    h, tree = keys["handle"], proved["tree"]
    recs = list(records[10:13])
    recs[1] = (recs[1][0], 1 << 64, recs[1][2])
    proofs, pws, status = h.prove_deposits(tree, 10, recs, _rs(3, 5))
    assert status[0] == 0 and status[2] == 0 and status[1] != 0
    assert proofs[1] == bytes(388)
    assert ctx.verify_batch(keys["vk"], [proofs[0], proofs[2]], [pws[0], pws[2]]) == [True, True]
    rows = tree.deposit_rows(10, recs)
    assert rows[1][3] == 1 << 64 and pws[0] == _pw(rows[0][:5]) and pws[2] == _pw(rows[2][:5])


def test_a_record_that_is_not_the_deposit_proves_another_root(ctx, keys, proved, records):
    from spp import witness as W
    h, tree = keys["handle"], proved["tree"]
    i = 70
    other = (records[i][0], records[i][1], (records[i][2] + 1) % R)
    proofs, pws, status = h.prove_deposits(tree, i, [other], _rs(1, 6))
    assert status == [0] and ctx.verify_batch(keys["vk"], proofs, pws) == [True]
    new_root = int.from_bytes(pws[0][12 + 32:12 + 64], "big")
    assert int.from_bytes(pws[0][12:44], "big") == tree.root_at(i) and new_root != tree.root_at(i + 1)
    k = i + 1 - 63
    codes, end_root, end_index = W.verify_deposit_chain(ctx, keys["vk"], [proofs[0], proved["proofs"][k]], [pws[0], proved["pws"][k]],
                                                        tree.root_at(i), i)
    assert codes == [M.OK, M.STALE_ROOT] and end_root == new_root and end_index == i + 1


def _chain(ctx, keys, proofs, pws, start_root, start_index, lamports):
    """the library's answer and the model's, the model fed with the batch verifier's own flags"""
    from spp import witness as W
    got = W.verify_deposit_chain(ctx, keys["vk"], proofs, pws, start_root, start_index, lamports=lamports)
    ok = ctx.verify_batch(keys["vk"], proofs, pws)
    codes, root, index = M.check_chain(pws, ok, M.word(start_root), start_index, lamports)
    assert got == (codes, int.from_bytes(root, "big"), index)
    return got


def test_chain_of_the_proved_log_and_one_failure_at_a_time(ctx, keys, proved, records):
    import spp
    from spp import witness as W
    tree, proofs, pws = proved["tree"], proved["proofs"], proved["pws"]
    start = tree.root_at(63)
    amounts = [r[1] for r in records[63:128]]
    codes, end_root, end_index = _chain(ctx, keys, proofs, pws, start, 63, amounts)
    assert codes == [M.OK] * 65 and end_root == tree.getRoot() and end_index == 128
    assert _chain(ctx, keys, proofs, pws, start, 63, None)[0] == [M.OK] * 65
    # a lamports mismatch at position 3: it and everything built on it
    lam = list(amounts); lam[3] += 1
    codes, end_root, end_index = _chain(ctx, keys, proofs, pws, start, 63, lam)
    assert codes == [M.OK] * 3 + [M.BAD_AMOUNT] + [M.STALE_ROOT] * 61 and end_root == proved["roots"][2] and end_index == 66
    # a proof byte flipped at 10
    bad = list(proofs); bad[10] = bad[10][:40] + bytes([bad[10][40] ^ 1]) + bad[10][41:]
    codes, end_root, end_index = _chain(ctx, keys, bad, pws, start, 63, amounts)
    assert codes == [M.OK] * 10 + [M.BAD_PROOF] + [M.STALE_ROOT] * 54 and end_root == proved["roots"][9] and end_index == 73
    # position 20 dropped
    drop = lambda x: x[:20] + x[21:]
    codes, end_root, end_index = _chain(ctx, keys, drop(proofs), drop(pws), start, 63, drop(amounts))
    assert codes == [M.OK] * 20 + [M.STALE_ROOT] * 44 and end_index == 83
    # position 30 duplicated: the copy is stale, the log goes on behind it
    dup = lambda x: x[:31] + x[30:]
    codes, end_root, end_index = _chain(ctx, keys, dup(proofs), dup(pws), start, 63, dup(amounts))
    assert codes == [M.OK] * 31 + [M.STALE_ROOT] + [M.OK] * 34 and end_root == tree.getRoot() and end_index == 128
    # a wrong start: index first, then root
    assert _chain(ctx, keys, proofs[:2], pws[:2], start, 62, None)[0] == [M.BAD_INDEX, M.STALE_ROOT]
    assert _chain(ctx, keys, proofs[:2], pws[:2], tree.root_at(62), 63, None)[0] == [M.STALE_ROOT, M.STALE_ROOT]
    assert W.verify_deposit_chain(ctx, keys["vk"], [], [], start, 63) == ([], start, 63)
    # a withdraw key is a key with five public inputs: accepted as a format, and no proof verifies under it -- the first instruction
    # is BAD_PROOF, and so is every one taken from its own state; behind a rejected one the order of the checks makes the rest STALE_ROOT
    wvk = open(os.path.join(GOLDEN, "reference_withdraw.vk"), "rb").read()
    codes, end_root, end_index = W.verify_deposit_chain(ctx, wvk, proofs[:4], pws[:4], start, 63, lamports=amounts[:4])
    assert codes == [M.BAD_PROOF] + [M.STALE_ROOT] * 3 and (end_root, end_index) == (start, 63)
    for k in (1, 64):
        assert W.verify_deposit_chain(ctx, wvk, proofs[k:k + 1], pws[k:k + 1], tree.root_at(63 + k), 63 + k)[0] == [M.BAD_PROOF]
    avk = open(os.path.join(GOLDEN, "reference_audit.vk"), "rb").read()
    for n in (0, 2):
        with pytest.raises(spp.lib.SppError) as e:
            W.verify_deposit_chain(ctx, avk, proofs[:n], pws[:n], start, 63)
        assert e.value.code == FORMAT and "5" in str(e.value)
    with pytest.raises(spp.lib.SppError) as e:
        W.verify_deposit_chain(ctx, keys["vk"][:-1], proofs[:1], pws[:1], start, 63)
    assert e.value.code == FORMAT


def test_cli_round_trip(keys, tmp_path, capsys):
    from spp import cli
    rng = random.Random(31)
    deps, leaves, out = (str(tmp_path / n) for n in ("deposits.jsonl", "leaves.txt", "out"))
    with open(deps, "w") as f:
        for _ in range(5):
            f.write(json.dumps({"secretKey": "0x%x" % rng.randrange(1, R), "amount": rng.randrange(1 << 40), "randomness": str(rng.randrange(R))}) + "\n")
    open(leaves, "w").write("".join("%064x\n" % rng.randrange(R) for _ in range(3)))
    assert cli.main(["deposit-prove", deps, keys["sppc"], keys["pk"], leaves, "--out", out, "--window", "6"]) == 0
    capsys.readouterr()
    log = os.path.join(out, "log.jsonl")
    lines = open(log).read().splitlines()
    assert len(lines) == 5 and sorted(os.listdir(out)) == sorted(["log.jsonl"] + ["deposit_%d.%s" % (i, e) for i in range(3, 8) for e in ("proof", "pw")])
    assert bytes.fromhex(json.loads(lines[4])["deposit"]["pw"]) == open(os.path.join(out, "deposit_7.pw"), "rb").read()
    # from the empty tree the log does not connect: three leaves came before it
    assert cli.main(["deposit-verify", keys["vk_path"], log]) == 1
    assert capsys.readouterr().out.split() == ["STALE_ROOT"] * 5
    start_root = json.loads(lines[0])["deposit"]["pw"][24:88]
    assert cli.main(["deposit-verify", keys["vk_path"], log, "--start-root", start_root, "--start-index", "3"]) == 0
    assert capsys.readouterr().out.split() == ["OK"] * 5
    d = json.loads(lines[2]); d["deposit"]["amount"] += 1
    open(log, "w").write("\n".join(lines[:2] + [json.dumps(d)] + lines[3:]) + "\n")
    assert cli.main(["deposit-verify", keys["vk_path"], log, "--start-root", start_root, "--start-index", "3"]) == 1
    res = capsys.readouterr()
    assert res.out.split() == ["OK", "OK", "BAD_AMOUNT", "STALE_ROOT", "STALE_ROOT"] and "line 3: BAD_AMOUNT" in res.err
    # pool-replay's parsers read such a log as deposits with commitments, as before
    assert [k for k, _ in cli.parse_pool_log(lines)] == ["deposit"] * 5 and len(cli.parse_pool_commitments(lines)) == 5
