"""Wallet sync, host side (no GPU): the C declarations of spp_merkle_tree_find / spp_wallet_sync, the Python mirror of the
constants, the NULL refusals, the CLI's argument errors, and csrc/leaf_index.hpp compiled for the host
(tests/host/leaf_index_check.cpp, plain and with -fsanitize=address,undefined) against the model below.

The model is a list of leaves scanned linearly: it knows nothing of slots, salts or probing."""
import json
import os
import random
import re
import subprocess

import pytest

from conftest import ROOT
from test_pool_host import home_slot, keys_homed_at, slots_for

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
SALT = 0x5EED5EED5EED5EED
CSRC = os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd", "csrc")
ORDERS = {"ascending": 0, "descending": 1, "shuffled": 2}


def be(v):
    return v.to_bytes(32, "big")


def model(leaves, key, start, pmod, prem):
    """(lowest index >= start holding key, occurrences in the whole list, lowest such index with i % pmod != prem); -1 = none"""
    occ = [i for i, v in enumerate(leaves) if v == key]
    lo = [i for i in occ if i >= start]
    fi = [i for i in lo if i % pmod != prem]
    return (lo[0] if lo else -1, len(occ), fi[0] if fi else -1)


def field_keys_homed_at(slot, slots, count, rng):
    """like keys_homed_at, canonical field elements only"""
    out = []
    while len(out) < count:
        k = keys_homed_at(slot, SALT, slots, 1, rng)[0]
        if int.from_bytes(k, "big") < R and k not in out:
            out.append(k)
    return [int.from_bytes(k, "big") for k in out]


def test_header_declares_the_calls_and_constants():
    hdr = open(os.path.join(ROOT, "include", "spp.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    for decl in (
            "int spp_merkle_tree_find(spp_merkle_tree* t, size_t count, const uint8_t* leaves, const uint64_t* from, uint64_t* indices, "
            "uint32_t* matches);",
            "int spp_wallet_sync(spp_merkle_tree* t, spp_pool* pool /* optional */, size_t count, const uint8_t* deposits "
            "/* count * SPP_DEPOSIT_LEN */, const uint8_t* recipients /* optional: count * 32 B recipient words */, uint64_t* indices, "
            "uint32_t* flags, uint8_t* records /* optional */, uint8_t* notes /* optional, needs recipients: count * SPP_NOTE_LEN */);"):
        assert decl in flat, decl
    names = dict(re.findall(r"#define (SPP_WALLET_\w+)\s+(\d+)", hdr))
    assert names == {"SPP_WALLET_RECORD_LEN": "160", "SPP_WALLET_IN_TREE": "1", "SPP_WALLET_SPENT": "2", "SPP_WALLET_AUDITED": "4",
                     "SPP_WALLET_REPEATED": "8"}
    index = hdr[:hdr.index("#ifndef SPP_H")]
    assert "spp_merkle_tree_find" in index and "spp_wallet_sync" in index
    for ref in ("storage.ts:9-26", "45-50", "storage.ts:233-260", "withdraw.rs:94-147"):
        assert ref in index, ref
    assert "SPP_TREE_INDEX_SALT" in hdr and "withdraw.rs:94-125" in hdr


def test_library_exports_the_calls_and_python_mirrors_the_constants():
    import spp
    from spp import lib, witness
    L = spp.load_library()
    assert hasattr(L, "spp_merkle_tree_find") and hasattr(L, "spp_wallet_sync")
    hdr = open(os.path.join(ROOT, "include", "spp.h")).read()
    names = re.findall(r"#define (SPP_WALLET_\w+)\s+(\d+)", hdr)
    assert len(names) == 5
    for name, val in names:
        assert getattr(lib, name) == int(val), name
    assert witness.WALLET_ABSENT == (1 << 64) - 1
    for m in ("find", "sync"):
        assert callable(getattr(witness.ShieldedPoolMerkleTree, m)), m


def test_both_calls_refuse_null_without_a_device():
    import spp
    L = spp.load_library()
    calls = (lambda: L.spp_merkle_tree_find(None, 1, bytes(32), None, None, None),
             lambda: L.spp_merkle_tree_find(None, 0, None, None, None, None),
             lambda: L.spp_wallet_sync(None, None, 1, bytes(96), None, None, None, None, None),
             lambda: L.spp_wallet_sync(None, None, 0, None, None, None, None, None, None))
    for k, call in enumerate(calls):
        L.spp_verify(None, 0, None, 0, None, 0, None)     # leaves another message behind
        assert call() == -1 and "NULL" in spp.last_error(), k


def test_cli_wallet_sync_argument_errors_touch_no_device(tmp_path, monkeypatch, capsys):
    from spp import cli, prover
    def no_device(*a, **k):
        raise AssertionError("a device context was opened")
    monkeypatch.setattr(cli, "Context", no_device)
    monkeypatch.setattr(prover.Context, "__init__", no_device)
    secrets, leaves, keys, wvk, avk = (str(tmp_path / n) for n in ("secrets.json", "leaves.txt", "keys.txt", "w.vk", "a.vk"))
    good = [{"secretKey": "0x1234", "amount": "1000", "randomness": hex(R - 1)}, {"secretKey": 7, "amount": 5, "randomness": 0}]
    assert cli.parse_wallet_secrets(json.dumps(good)) == [(0x1234, 1000, R - 1), (7, 5, 0)]
    open(leaves, "w").write("0x%064x\n\n%064x\n" % (5, 6))
    open(keys, "w").write("%064x\n" % 9)
    open(wvk, "wb").write(b"x"); open(avk, "wb").write(b"y")
    bad_secrets = ({"secretKey": "0x0", "amount": "1", "randomness": "0x1"}, {"secretKey": hex(R), "amount": "1", "randomness": "0x1"},
                   {"secretKey": "0x1", "amount": str(1 << 64), "randomness": "0x1"}, {"secretKey": "0x1", "amount": "1", "randomness": hex(R)},
                   {"secretKey": "0x1", "amount": "1"}, 3)
    for bad in bad_secrets:
        open(secrets, "w").write(json.dumps([good[0], bad]))
        assert cli.main(["wallet-sync", secrets, leaves]) == 2
        err = capsys.readouterr().err
        assert "wallet-sync" in err and ("secret 1" in err or "not a list" in err), err
    open(secrets, "w").write("{")
    assert cli.main(["wallet-sync", secrets, leaves]) == 2
    open(secrets, "w").write(json.dumps(good))
    assert cli.main(["wallet-sync", secrets, str(tmp_path / "none.txt")]) == 2
    for text, what in (("zz\n", "line 1"), ("%064x\n%066x\n" % (5, 1 << 257), "line 2"), ("%064x\n" % R, "leaf 0")):
        bad_leaves = str(tmp_path / "bad_leaves.txt")
        open(bad_leaves, "w").write(text)
        assert cli.main(["wallet-sync", secrets, bad_leaves]) == 2
        assert what in capsys.readouterr().err
    three = str(tmp_path / "three.txt")
    open(three, "w").write("05\n06\n07\n")
    assert cli.main(["wallet-sync", secrets, three, "--depth", "1"]) == 2                  # three leaves, room for two
    assert cli.main(["wallet-sync", secrets, leaves, "--depth", "0"]) == 2
    capsys.readouterr()
    assert cli.main(["wallet-sync", secrets, leaves, "--spent", keys]) == 2
    assert "--vk" in capsys.readouterr().err
    assert cli.main(["wallet-sync", secrets, leaves, "--audited", keys]) == 2
    assert cli.main(["wallet-sync", secrets, leaves, "--spent", keys, "--vk", wvk, str(tmp_path / "none.vk")]) == 2
    assert cli.main(["wallet-sync", secrets, leaves, "--spent", str(tmp_path / "none.txt"), "--vk", wvk, avk]) == 2
    assert cli.main(["wallet-sync", secrets, leaves, "--recipient", hex(R)]) == 2
    assert cli.main(["wallet-sync", secrets, leaves, "--recipient", "xyz"]) == 2


@pytest.fixture(scope="module")
def check_exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("leaf_index")
    src = os.path.join(ROOT, "tests", "host", "leaf_index_check.cpp")
    exes = []
    for name, extra in (("plain", []), ("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = str(d / ("leaf_index_check_" + name))
        subprocess.run(["g++", "-O2", "-std=c++17", "-I", CSRC, src, "-o", exe] + extra, check=True)
        exes.append(exe)
    return exes


def run_check(exes, leaves, queries, stages, order):
    """runs both builds; returns per stage (slots, rebuilt, table, homes, answers), identical for the two builds"""
    text = "%x %d %d %d %d %s\n" % (SALT, len(leaves), len(queries), ORDERS[order], len(stages), " ".join(map(str, stages)))
    text += "".join(be(v).hex() + "\n" for v in leaves)
    text += "".join("%s %d %d %d\n" % (be(k).hex(), s, pm, pr) for k, s, pm, pr in queries)
    outs = []
    for exe in exes:
        out = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert out.returncode == 0, (exe, out.returncode, out.stdout[-300:], out.stderr[-2000:])
        assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
        outs.append(out.stdout)
    assert outs[0] == outs[1]
    lines = outs[0].strip().split("\n")
    result, at = [], 0
    for stage in stages:
        m = re.fullmatch(r"slots (\d+) rebuilt ([01])", lines[at])
        table = [int(x) for x in lines[at + 1].split()[1:]]
        homes = [int(x) for x in lines[at + 2:at + 2 + stage]]
        answers = [tuple(int(x) for x in ln.split()) for ln in lines[at + 2 + stage:at + 2 + stage + len(queries)]]
        result.append((int(m.group(1)), int(m.group(2)), table, homes, answers))
        at += 2 + stage + len(queries)
    assert at == len(lines)
    return result


def check_table(leaves, slots, table, homes):
    """every leaf holds exactly one slot, and no slot between its home and its slot is empty: the invariant the queries rest on"""
    assert len(table) == slots and sorted(i for i in table if i >= 0) == list(range(len(leaves)))
    for s, i in enumerate(table):
        if i < 0:
            continue
        assert homes[i] == home_slot(be(leaves[i]), SALT, slots)
        k = homes[i]
        while k != s:
            assert table[k] >= 0, (i, s, k)
            k = (k + 1) % slots
    assert sum(1 for i in table if i >= 0) <= slots // 2


def forty_leaves(rng):
    """40 leaves for a 128-slot table: four values homed at the last slot (their run wraps to slots 0..2), one value at leaves 3, 17
    and 31, a leaf of value 0, slots 0..2's own homes left alone so that the wrapped run is exactly the chain"""
    slots = slots_for(40)
    assert slots == 128
    last = field_keys_homed_at(slots - 1, slots, 4, rng)
    triple = rng.randrange(1, R)
    leaves = []
    while len(leaves) < 40:
        v = rng.randrange(1, R)
        if home_slot(be(v), SALT, slots) in (slots - 2, slots - 1, 0, 1, 2, 3):
            continue
        leaves.append(v)
    for pos, v in zip((5, 11, 22, 38), last):
        leaves[pos] = v
    for pos in (3, 17, 31):
        leaves[pos] = triple
    leaves[9] = 0
    absent_in_run = field_keys_homed_at(slots - 1, slots, 2, rng) + field_keys_homed_at(1, slots, 1, rng)
    return leaves, last, triple, absent_in_run


def queries_for(leaves, last, triple, absent_in_run, rng):
    q = [(v, 0, 1, 1) for v in leaves]                                     # every leaf, from 0, predicate always true
    q += [(triple, s, 1, 1) for s in (0, 3, 4, 10, 17, 18, 31, 32, 40, 1 << 40)]   # from equal to, between and past the occurrences
    q += [(triple, 0, 2, 1), (triple, 0, 17, 3), (triple, 4, 17, 0), (triple, 0, 1, 0)]   # predicates that refuse some / all occurrences
    q += [(v, s, 1, 1) for v in last for s in (0, 39)]
    q += [(0, 0, 1, 1), (0, 10, 1, 1)]                                      # the leaf of value 0
    q += [(v, 0, 1, 1) for v in absent_in_run]                              # absent, home inside a full run
    q += [(rng.randrange(R), 0, 1, 1) for _ in range(5)]
    return q


def test_wrapping_chain_repeats_zero_and_absent_keys_against_the_linear_model(check_exes):
    rng = random.Random(41)
    leaves, last, triple, absent_in_run = forty_leaves(rng)
    queries = queries_for(leaves, last, triple, absent_in_run, rng)
    want = [model(leaves, *q) for q in queries]
    assert want[len(leaves)][:2] == (3, 3) and want[len(leaves) + 9][0] == -1
    answers = {}
    for order in ORDERS:
        (slots, rebuilt, table, homes, got), = run_check(check_exes, leaves, queries, [40], order)
        assert (slots, rebuilt) == (128, 1)
        check_table(leaves, slots, table, homes)
        assert got == want, order
        answers[order] = got
        # the chain homed at the last slot runs over the end of the table
        assert {table[127], table[0], table[1], table[2]} == {5, 11, 22, 38}
        assert table[3] == -1
    # the scheduling argument: slots differ between insertion orders, answers do not
    assert answers["ascending"] == answers["descending"] == answers["shuffled"]
    asc = run_check(check_exes, leaves, [], [40], "ascending")[0][2]
    desc = run_check(check_exes, leaves, [], [40], "descending")[0][2]
    assert asc != desc and (asc[127], desc[127]) == (5, 38)
    for v in absent_in_run[:2]:
        assert home_slot(be(v), SALT, 128) == 127
    assert home_slot(be(absent_in_run[2]), SALT, 128) == 1


@pytest.mark.parametrize("order", sorted(ORDERS))
def test_growth_across_a_rebuild(check_exes, order):
    """30 leaves (64 slots), then 70 (256 slots: allocated again, every leaf reinserted), answers after each stage"""
    rng = random.Random(43)
    leaves = [rng.randrange(R) for _ in range(70)]
    leaves[50] = leaves[10]                                                # a repeat that only the second stage sees
    leaves[69] = leaves[29] = leaves[2]
    queries = [(v, 0, 1, 1) for v in leaves] + [(leaves[2], s, 1, 1) for s in (3, 29, 30, 69, 70)] + [(leaves[2], 0, 27, 2)]
    stages = run_check(check_exes, leaves, queries, [30, 32, 33, 70], order)
    assert [(s[0], s[1]) for s in stages] == [(64, 1), (64, 0), (128, 1), (256, 1)]
    for n, (slots, _, table, homes, got) in zip((30, 32, 33, 70), stages):
        assert slots == slots_for(max(n, 32))
        check_table(leaves[:n], slots, table, homes)
        assert got == [model(leaves[:n], *q) for q in queries], n
    assert stages[0][4][2][:2] == (2, 2) and stages[3][4][2][:2] == (2, 3) and stages[3][4][-1][2] == 69
