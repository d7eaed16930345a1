"""The resident tree as of an earlier size, host side (no GPU): csrc/merkle_prefix.hpp compiled for the host with a toy hash
(tests/host/merkle_prefix_check.cpp, plain and with -fsanitize=address,undefined) against trees rebuilt from scratch there and
against the Python model below, the C declarations and the index comment, the Python mirror of the constants, the NULL refusals,
and `pool-replay`: its argument errors for logs with commitments and its unchanged output for a log without them."""
import json
import os
import re
import subprocess

import pytest

from conftest import ROOT

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
CSRC = os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd", "csrc")
M64 = (1 << 64) - 1
SEED = 0x5EED


def mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def toy_hash(a, b):
    return mix((mix(a ^ 0x9E3779B97F4A7C15) * 3 + b) & M64)


def model_root(leaves, depth):
    """client/merkle.ts:150-176 with the toy hash: the root of a fresh tree holding `leaves`, level by level"""
    dflt = [0]
    for _ in range(depth):
        dflt.append(toy_hash(dflt[-1], dflt[-1]))
    level = list(leaves)
    for l in range(depth):
        level = [toy_hash(level[j], level[j + 1] if j + 1 < len(level) else dflt[l]) for j in range(0, len(level), 2)]
    return level[0] if level else dflt[depth]


@pytest.fixture(scope="module")
def check_exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("merkle_prefix")
    src = os.path.join(ROOT, "tests", "host", "merkle_prefix_check.cpp")
    exes = []
    for name, extra in (("plain", []), ("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = str(d / ("merkle_prefix_check_" + name))
        subprocess.run(["g++", "-O2", "-std=c++17", "-I", CSRC, src, "-o", exe] + extra, check=True)
        exes.append(exe)
    return exes


def test_three_cases_and_frontier_against_trees_rebuilt_from_scratch(check_exes):
    outs = []
    for exe in check_exes:
        out = subprocess.run([exe, "%x" % SEED], capture_output=True, text=True)
        assert out.returncode == 0, (exe, out.returncode, out.stdout[-300:], out.stderr[-2000:])
        assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
        outs.append(out.stdout)
    assert outs[0] == outs[1]
    lines = outs[0].strip().split("\n")
    assert len(lines) == 12
    repeats = 0
    for depth in range(1, 7):
        full = 1 << depth
        head = re.fullmatch(r"depth (\d+) sizes (\d+) nodes (\d+) zero_leaves (\d+)", lines[2 * depth - 2])
        # every stored size m, every n <= m; per pair every node of every level
        assert [int(g) for g in head.groups()[:3]] == [depth, (full + 1) * (full + 2) // 2, (full + 1) * (full + 2) // 2 * (2 * full - 1)]
        leaves = []
        for i in range(full):
            v = mix((SEED + depth * 1000 + i) & M64)
            leaves.append(0 if v % 4 == 0 else v)
        assert int(head.group(4)) == leaves.count(0)
        roots = [int(x, 16) for x in lines[2 * depth - 1].split()[1:]]
        assert roots == [model_root(leaves[:n], depth) for n in range(full + 1)], depth
        # a zero-valued leaf is the default leaf: appending it does not change the root
        for n in range(full):
            assert (roots[n + 1] == roots[n]) == (leaves[n] == 0), (depth, n)
        repeats += leaves.count(0)
    assert repeats >= 6          # the seed does exercise repeated roots


def test_header_declares_the_calls_and_constants():
    hdr = open(os.path.join(ROOT, "include", "spp.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    for decl in (
            "#define SPP_TREE_SIZE_NOW UINT64_MAX /* the tree's size at the call */",
            "#define SPP_TREE_NO_SIZE UINT64_MAX /* in outputs: no prefix of this tree has that root */",
            "int spp_merkle_tree_root_at(spp_merkle_tree* t, uint64_t size, uint8_t root[32]);",
            "int spp_merkle_tree_proofs_at(spp_merkle_tree* t, uint64_t size, size_t n, const uint64_t* indices, uint8_t* siblings_out);",
            "int spp_merkle_tree_prefix_roots(spp_merkle_tree* t, uint64_t first_size, size_t count, uint8_t* roots); "
            "/* sizes first_size .. first_size+count-1 */",
            "int spp_merkle_tree_find_roots(spp_merkle_tree* t, size_t count, const uint8_t* roots, uint64_t* sizes, "
            "uint32_t* matches /* optional */);",
            "int spp_withdraw_rows_from_tree_at(spp_merkle_tree* t, uint64_t size, size_t count, const uint8_t* notes, uint8_t* rows);",
            "int spp_prove_withdraw_notes_at_device(spp_circuit* c, spp_merkle_tree* t, uint64_t size, size_t count, const void* d_notes, "
            "const void* d_rs, void* d_proofs, void* d_pws, void* d_status);",
            "int spp_prove_withdraw_notes_at(spp_circuit* c, spp_merkle_tree* t, uint64_t size, size_t count, const uint8_t* notes, "
            "const uint8_t* rs, uint8_t* proofs, uint8_t* pws, int32_t* status);",
            "int spp_pool_root_sizes(spp_pool* pool, spp_merkle_tree* t, uint64_t sizes[33], uint64_t* best /* optional */);"):
        assert decl in flat, decl
    index = hdr[:hdr.index("#ifndef SPP_H")]
    for name in ("spp_merkle_tree_root_at", "_proofs_at", "_prefix_roots", "spp_withdraw_rows_from_tree_at", "spp_prove_withdraw_notes_at(_device)",
                 "spp_merkle_tree_find_roots", "spp_pool_root_sizes"):
        assert name in index, name
    for ref in ("deposit.rs:31-36", "payroll-demo.ts:285-292", "on-chain.ts:93-125,202-235"):
        assert ref in index and ref in hdr[hdr.index("#ifndef SPP_H"):], ref
    body = hdr[hdr.index("#ifndef SPP_H"):]
    assert "client/merkle.ts:150-156" in body and "SPP_TREE_INDEX_SALT" in body
    assert "does not depend on leaves inserted before or after the call" in re.sub(r"\s*\n \*\s*", " ", body)


def test_library_exports_the_calls_and_python_mirrors_the_constants():
    import spp
    from spp import lib, prover, witness
    L = spp.load_library()
    for name in ("spp_merkle_tree_root_at", "spp_merkle_tree_proofs_at", "spp_merkle_tree_prefix_roots", "spp_merkle_tree_find_roots",
                 "spp_withdraw_rows_from_tree_at", "spp_prove_withdraw_notes_at_device", "spp_prove_withdraw_notes_at", "spp_pool_root_sizes"):
        assert hasattr(L, name), name
    assert lib.SPP_TREE_SIZE_NOW == lib.SPP_TREE_NO_SIZE == (1 << 64) - 1
    for m in ("root_at", "proofs_at", "prefix_roots", "find_roots"):
        assert callable(getattr(witness.ShieldedPoolMerkleTree, m)), m
    assert callable(witness.Pool.root_sizes)
    import inspect
    assert "size" in inspect.signature(witness.ShieldedPoolMerkleTree.withdraw_rows).parameters
    assert "size" in inspect.signature(prover.CircuitHandle.prove_withdraw_notes).parameters
    assert "size" in inspect.signature(prover.CircuitHandle.prove_withdraw_notes_device).parameters


def test_the_calls_refuse_null_without_a_device():
    import ctypes
    import spp
    L = spp.load_library()
    now = (1 << 64) - 1
    buf = ctypes.create_string_buffer(4096)
    vp = ctypes.cast(buf, ctypes.c_void_p)
    calls = (lambda: L.spp_merkle_tree_root_at(None, 0, vp),
             lambda: L.spp_merkle_tree_root_at(None, now, vp),
             lambda: L.spp_merkle_tree_proofs_at(None, 0, 0, None, None),
             lambda: L.spp_merkle_tree_proofs_at(None, now, 1, vp, vp),
             lambda: L.spp_merkle_tree_prefix_roots(None, 0, 1, vp),
             lambda: L.spp_merkle_tree_prefix_roots(None, 0, 0, None),
             lambda: L.spp_merkle_tree_find_roots(None, 1, bytes(32), vp, None),
             lambda: L.spp_merkle_tree_find_roots(None, 0, None, None, None),
             lambda: L.spp_withdraw_rows_from_tree_at(None, 0, 1, bytes(160), vp),
             lambda: L.spp_withdraw_rows_from_tree_at(None, now, 0, bytes(160), vp),
             lambda: L.spp_prove_withdraw_notes_at_device(None, None, 0, 1, vp, vp, vp, vp, vp),
             lambda: L.spp_prove_withdraw_notes_at(None, None, 0, 1, bytes(160), None, vp, vp, vp),
             lambda: L.spp_prove_withdraw_notes_at(None, None, now, 0, bytes(160), None, vp, vp, vp),
             lambda: L.spp_pool_root_sizes(None, None, vp, None))
    for k, call in enumerate(calls):
        L.spp_verify(None, 0, None, 0, None, 0, None)     # leaves another message behind
        assert call() == -1 and "NULL" in spp.last_error(), k


GOOD_LOG = [{"deposit": {"root": "00" * 32}}, {"submit_audit": {"proof": "00" * 388, "pw": "0x" + "00" * 76}},
            {"withdraw": {"proof": "00" * 388, "pw": "00" * 172, "recipient": "11" * 32}}, {"deposit": {"root": "0x" + "22" * 32}}]


def test_cli_pool_replay_commitment_errors_touch_no_device(tmp_path, monkeypatch, capsys):
    from spp import cli, prover
    def no_device(*a, **k):
        raise AssertionError("a device context was opened")
    monkeypatch.setattr(cli, "Context", no_device)
    monkeypatch.setattr(prover.Context, "__init__", no_device)
    wvk, avk, log = (str(tmp_path / n) for n in ("w.vk", "a.vk", "log.jsonl"))
    open(wvk, "wb").write(b"x"); open(avk, "wb").write(b"y")
    lines = [json.dumps(g) for g in GOOD_LOG]
    assert cli.parse_pool_commitments(lines) is None
    with_c = [json.dumps({"deposit": {"root": "00" * 32, "commitment": "0x%064x" % 5}}), "", lines[1], lines[2],
              json.dumps({"deposit": {"root": "22" * 32, "commitment": "%064x" % (R - 1)}})]
    assert cli.parse_pool_commitments(with_c) == [5, R - 1]
    assert [k for k, _ in cli.parse_pool_log(with_c)] == ["deposit", "submit_audit", "withdraw", "deposit"]   # the extra key is no error there
    for bad, what in (({"deposit": {"root": "00" * 32}}, "line 2"),                                    # some with, some without
                      ({"deposit": {"root": "00" * 32, "commitment": "00" * 31}}, "line 2"),
                      ({"deposit": {"root": "00" * 32, "commitment": "%064x" % R}}, "line 2"),
                      ({"deposit": {"root": "00" * 32, "commitment": "zz" * 32}}, "line 2"),
                      ({"deposit": {"root": "00" * 32, "commitment": 7}}, "line 2")):
        open(log, "w").write(with_c[0] + "\n" + json.dumps(bad) + "\n")
        assert cli.main(["pool-replay", wvk, avk, log]) == 2
        err = capsys.readouterr().err
        assert "spp pool-replay:" in err and what in err and "commitment" in err, err
    open(log, "w").write(json.dumps(GOOD_LOG[0]) + "\n" + with_c[0] + "\n")                            # the first one without
    assert cli.main(["pool-replay", wvk, avk, log]) == 2 and "line 1" in capsys.readouterr().err
    three = "".join(json.dumps({"deposit": {"root": "00" * 32, "commitment": "%064x" % v}}) + "\n" for v in (1, 2, 3))
    open(log, "w").write(three)
    assert cli.main(["pool-replay", wvk, avk, log, "--depth", "1"]) == 2                              # three leaves, room for two
    assert "depth 1" in capsys.readouterr().err
    assert cli.main(["pool-replay", wvk, avk, log, "--depth", "0"]) == 2
    assert cli.main(["pool-replay", wvk, avk, log, "--depth", "33"]) == 2


def test_cli_pool_replay_without_commitments_prints_what_it_printed(tmp_path, monkeypatch, capsys):
    """no device: a Pool that answers with fixed codes.  The lines are the result names and nothing else, and no tree is made."""
    from spp import cli, lib, witness
    seen = []

    class FakeContext:
        def __init__(self, device):
            pass

        def close(self):
            pass

    class FakePool:
        def __init__(self, ctx, wvk, avk, capacity, verifier="each", group=0):
            seen.append(("pool", capacity, verifier, group))

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

        def settle_log(self, instructions):
            seen.append(("log", [ins[0] for ins in instructions]))
            return [0, 1, 3, 0], [0, 0, 0, 0]

    def no_tree(*a, **k):
        raise AssertionError("a log without commitments made a tree")
    monkeypatch.setattr(cli, "Context", FakeContext)
    monkeypatch.setattr(witness, "Pool", FakePool)
    monkeypatch.setattr(witness, "ShieldedPoolMerkleTree", no_tree)
    wvk, avk, log = (str(tmp_path / n) for n in ("w.vk", "a.vk", "log.jsonl"))
    open(wvk, "wb").write(b"x"); open(avk, "wb").write(b"y")
    open(log, "w").write("".join(json.dumps(g) + "\n" for g in GOOD_LOG))
    assert cli.main(["pool-replay", wvk, avk, log]) == 0
    assert capsys.readouterr().out == "OK\nAUDIT_EXISTS\nBAD_ROOT\nOK\n"
    assert seen == [("pool", 1, "each", 0), ("log", ["deposit", "submit_audit", "withdraw", "deposit"])]
    assert lib.POOL_RESULT_NAMES[3] == "BAD_ROOT"
