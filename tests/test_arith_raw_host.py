"""CPU: the raw-word vectors of tests/arith_vectors.py through the g++ build of csrc/arith_probe.hpp (tests/host/arith_raw_check.cpp),
judged by the same big-integer predicates tests/test_gpu_arith.py applies to the gfx950 build.  It shows the vectors and the
expectations are right before a GPU sees them, and it executes what the older host checks never reached: Fp::inv() on words
whose low limb is zero (strip()'s shift by 31)."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import arith_vectors as V
from conftest import ROOT

CSRC = os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd", "csrc")


def build_twin(exe):
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", CSRC, os.path.join(ROOT, "tests", "host", "arith_raw_check.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return build_twin(str(tmp_path_factory.mktemp("arith_raw") / "arith_raw_check"))


def run_twin(exe, tmp_path, bs):
    """the batches through the host twin: (rows of result words per batch, the twin's report)"""
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<II", 0x31565241, len(bs)))
        for b in bs:
            f.write(struct.pack("<5I", b.selector, b.arg, len(b.rows), b.in_words, b.out_words))
            f.write(np.asarray(b.rows, dtype="<u4").tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "OK %d" % sum(len(b.rows) for b in bs), r.stdout + r.stderr
    words = np.fromfile(fout, dtype="<u4")
    outs, at = [], 0
    for b in bs:
        k = len(b.rows) * b.out_words
        outs.append(words[at:at + k].reshape(len(b.rows), b.out_words).tolist())
        at += k
    assert at == len(words)
    return outs, r.stdout


def test_operation_table_matches_the_dispatch_header():
    hdr = open(os.path.join(CSRC, "arith_probe.hpp")).read()
    ops = {m[0]: tuple(int(x) for x in m[1:]) for m in re.findall(r"^\s*X\((\w+), (\d+), (\d+), (\d+), ([012])\)", hdr, re.M)}
    assert ops == V.OPS and len(ops) >= 56


@pytest.mark.parametrize("group", V.GROUPS)
def test_host_build_matches_big_integers(twin, tmp_path, group):
    bs = V.batches(group)
    outs, report = run_twin(twin, tmp_path, bs)
    counts = V.verify_group(group, bs, outs)
    assert all(n >= 20 and n % 64 for n in counts.values()), counts
    print(report)                                            # the cases per operation
    for b in bs:
        assert "%s %s arg %d cases %d\n" % (b.field, b.op, b.arg, len(b.rows)) in report
    if group == "inv":
        # at least one case per field enters the zero-low-word branch of strip(); the twin counts the provable ones from the words
        for field in (V.FR, V.FQ):
            n = int(re.search(r"^%s FP_INV zero_low_word_branch (\d+)$" % field, report, re.M).group(1))
            p = V.MOD[field]
            ws = [V.from_words8(r) for b in bs if b.field == field and b.op == "FP_INV" for r in b.rows]
            assert n == sum(V.inv_enters_zero_low_word_branch(w, p) for w in ws) and n >= 200, (field, n)


@pytest.mark.parametrize("group", V.HINT_GROUPS)
def test_host_build_of_the_solver_hints_matches_big_integers(twin, tmp_path, group):
    """csrc/gnark_hints.hpp -- BigS<12>, big_mul_acc and the three hints of the solver kernels -- through the same probe dispatch:
    every case is judged in Python integers, and every branch class the vectors name (V.HINT_CLASSES) holds at least one case."""
    bs = V.batches(group)
    outs, report = run_twin(twin, tmp_path, bs)
    counts = V.verify_group(group, bs, outs)
    print(group, counts)
    print(report)
    assert all(len(b.rows) % 64 for b in bs)
    for b in bs:
        assert "%s %s arg %d cases %d\n" % (b.field, b.op, b.arg, len(b.rows)) in report
    assert sorted(counts) == sorted(V.HINT_CLASSES[group]) and min(counts.values()) > 0, counts
