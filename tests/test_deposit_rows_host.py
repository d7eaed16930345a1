"""The walk of k_deposit_rows on the host (no GPU): csrc/deposit_rows.hpp compiled with g++ into a stand-alone program
(tests/host/deposit_rows_check.cpp, plain and with -fsanitize=address,undefined) and compared with big-integer rows the Python model
(tests/deposit_model.py) writes for a 70-leaf tree of depth 16; the model itself against a tree rebuilt from scratch by oracle.hashes."""
import os
import random
import subprocess

import pytest

from conftest import ROOT
import deposit_model as M

CSRC = os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd", "csrc")
N_LEAVES = 70


@pytest.fixture(scope="module")
def model_rows():
    rng = random.Random(0xD0)
    leaves = [rng.randrange(M.R) for _ in range(N_LEAVES)]
    leaves[5] = 0                                   # a zero-valued leaf: the root does not move
    t, rows = M.Tree(), []
    for i, leaf in enumerate(leaves):
        sibs = t.siblings_for_append(i)
        rows.append(M.row_from_parts((1, 2), 3, 4, i, sibs, commitment=leaf))
        t.append(leaf)
    return leaves, rows


def test_model_rows_are_the_roots_and_paths_of_trees_rebuilt_from_scratch(model_rows):
    from oracle import hashes as H
    leaves, rows = model_rows
    for i in (0, 1, 2, 3, 6, 31, 32, 63, 64, 69):
        before, after = H.MerkleTree(), H.MerkleTree()
        for leaf in leaves[:i]:
            before.insert(leaf); after.insert(leaf)
        after.insert(leaves[i])
        assert rows[i][0] == before.root() and rows[i][1] == after.root(), i
        assert rows[i][8:] == before.proof(i) == after.proof(i), i
        assert rows[i][4] == i and rows[i][2] == leaves[i]
    assert rows[5][0] == rows[5][1] and rows[6][0] != rows[6][1]


@pytest.fixture(scope="module")
def check_exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("deposit_rows")
    srcs = [os.path.join(ROOT, "tests", "host", "deposit_rows_check.cpp"), os.path.join(CSRC, "circuit.cpp")]
    exes = []
    for name, extra in (("plain", []), ("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = str(d / ("deposit_rows_check_" + name))
        subprocess.run(["g++", "-O2", "-std=c++17", "-I", CSRC] + srcs + ["-o", exe] + extra, check=True)
        exes.append(exe)
    return exes


def test_walk_against_the_model_plain_and_sanitized(check_exes, model_rows, tmp_path):
    leaves, rows = model_rows
    vec = str(tmp_path / "vectors.txt")
    with open(vec, "w") as f:
        f.write("%d %d\n" % (M.DEPTH, len(leaves)))
        f.write("".join("%064x\n" % v for v in leaves))
        for row in rows:
            f.write(" ".join("%064x" % v for v in row[:2] + row[8:]) + "\n")
    for exe in check_exes:
        out = subprocess.run([exe, vec], capture_output=True, text=True)
        assert out.returncode == 0, (exe, out.returncode, out.stdout[-300:], out.stderr[-2000:])
        assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
        assert out.stdout == "rows %d walks %d\n" % (N_LEAVES, 3 * N_LEAVES)


def test_a_wrong_vector_is_noticed(check_exes, model_rows, tmp_path):
    leaves, rows = model_rows
    vec = str(tmp_path / "bad.txt")
    with open(vec, "w") as f:
        f.write("%d %d\n" % (M.DEPTH, len(leaves)))
        f.write("".join("%064x\n" % v for v in leaves))
        for i, row in enumerate(rows):
            words = row[:2] + row[8:]
            if i == 37:
                words[2 + 3] = (words[2 + 3] + 1) % M.R
            f.write(" ".join("%064x" % v for v in words) + "\n")
    out = subprocess.run([check_exes[0], vec], capture_output=True, text=True)
    assert out.returncode == 1 and "leaf 37" in out.stderr and "sibling 3" in out.stderr
