"""Ragged MSM tables on the host (csrc/msm_ragged.hpp, csrc/msm_classes.hpp through tests/host/msm_ragged_check.cpp): the table
layout whose 64-row blocks differ in length, the range classes of the audit circuit's wires, the split of the HBM budget that
counts what a window bit really costs, and the soundness of the classes on solved witnesses."""
import json
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd", "csrc")
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617

# bases per set of the audit circuit (A, B1, K, Z, CB, CS, B2) as tests/golden/msm_plan.json records them
AUDIT_SIZES = json.load(open(os.path.join(ROOT, "tests", "golden", "msm_plan.json")))["sets"]["audit"]["sizes"]


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ragged") / "msm_ragged_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "msm_ragged_check.cpp"),
                    os.path.join(CSRC, "circuit.cpp"), os.path.join(CSRC, "circuit_audit.cpp"), "-o", exe], check=True)
    return exe


def _classes(check_exe, tmp_path, args, name):
    out = str(tmp_path / (name + "_bounds.txt"))
    proc = subprocess.run([check_exe] + args + [out], capture_output=True, text=True, timeout=900)
    assert proc.returncode == 0 and proc.stdout.strip().splitlines()[-1].startswith("OK msm_classes"), proc.stdout + proc.stderr
    counts = {}
    for line in proc.stdout.splitlines():
        f = line.split()
        if f and f[0] == "CLASSES":
            counts[f[1]] = tuple(int(f[k]) for k in (3, 5, 7, 9))   # wide, bits, limbs, lookups
    bounds = {}
    for line in open(out):
        w, b, _kind = (int(x) for x in line.split())
        bounds[w] = b
    return counts, bounds


def _audit_classes(check_exe, tmp_path, rlwe_pk):
    pk_txt = tmp_path / "pk.txt"
    pk_txt.write_text(" ".join(str(int(v)) for v in list(rlwe_pk["a"]) + list(rlwe_pk["b"])))
    return _classes(check_exe, tmp_path, ["audit", str(pk_txt)], "audit")


def test_ragged_layout_on_random_class_vectors(check_exe):
    """Offsets strictly increase, block b spans E_b * 64 points, every (row, d <= bound) lies inside its block, the total is the
    sum of the blocks; all-wide input is exactly msm_table_elems(N, c, 1) with the uniform index for every (row, d)."""
    proc = subprocess.run([check_exe, "layout"], capture_output=True, text=True, timeout=900)
    assert proc.returncode == 0 and proc.stdout.strip().splitlines()[-1].startswith("OK msm_ragged layout"), proc.stdout


def test_audit_circuit_class_counts(check_exe, tmp_path, rlwe_pk):
    """The audit circuit as the product's builder emits it over tests/golden/rlwe_pk.json: wide / bits / byte limbs / looked-up
    inputs among the wires of A, of B and among the private, uncommitted wires (K).  The expected counts come from the circuit
    (a scan of its solver program made before the classes existed), not from the code under test."""
    counts, bounds = _audit_classes(check_exe, tmp_path, rlwe_pk)
    assert counts["A"] == (27376, 762, 4352, 2112)
    assert counts["B"] == (5441, 762, 4352, 2112)
    assert counts["K"] == (27946, 762, 0, 0)
    assert len(bounds) == 762 + 4352 + 2112 and 0 not in bounds
    assert sorted(set(bounds.values())) == [1, 128, 255]     # bits; r, e1, e2 in [-128, 127]; byte limbs


def _plan(check_exe, sizes, classes, budget):
    proc = subprocess.run([check_exe, "plan"] + [str(v) for v in list(sizes) + list(classes)] + [repr(budget)], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    lines = [l.split() for l in proc.stdout.splitlines() if l.startswith("PLAN")]
    return [int(v) for v in lines[0][2:]], float(lines[1][2])


def test_window_planner_counts_what_a_bit_costs(check_exe):
    """The audit set sizes under the 240 GB budget: with the class counts every flat set reaches 16 bits inside the budget; with
    every base wide the planner gives the windows recorded in profiles/round3_bench_default_run.json (K and Z at 15 bits)."""
    bits, used = _plan(check_exe, AUDIT_SIZES, [762, 4352, 2112, 762, 4352, 2112, 762], 240e9)
    print("ragged: bits", bits, "bytes %.4g" % used)
    assert bits == [16, 16, 16, 16, 9, 9, 16] and used <= 240e9
    recorded = json.load(open(os.path.join(ROOT, "profiles", "round3_bench_default_run.json")))["config"]["msm_windows"]
    bits, used = _plan(check_exe, AUDIT_SIZES, [0] * 7, 240e9)
    print("all wide: bits", bits, "bytes %.4g" % used)
    assert bits == [recorded[k] for k in ("A", "B1", "K", "Z", "CB", "CS", "B2(G2)")] == [16, 16, 15, 15, 9, 9, 16] and used <= 240e9


def _check_bounds(witness, bounds):
    worst = 0
    for w, b in bounds.items():
        v = witness[w] % R
        v = v if v <= R // 2 else v - R
        assert abs(v) <= b, "wire %d: value %d outside its class bound %d" % (w, v, b)
        worst = max(worst, abs(v))
    return worst


def test_classes_hold_on_a_solved_audit_witness(check_exe, tmp_path, audit_artifacts, rlwe_pk):
    """Every narrow wire's signed value is within its bound on the witness the oracle's CPU solver finds for the audit inputs the
    CPU suite already uses."""
    from oracle import circuit as C, rlwe
    _, bounds = _audit_classes(check_exe, tmp_path, rlwe_pk)
    c = C.Circuit(audit_artifacts["sppc"])
    d = rlwe.audit_inputs(rlwe_pk["a"], rlwe_pk["b"], 12345, random.Random(999))
    w = C.solve(c, rlwe.audit_input_vector(d), lambda w: 0x1234567)
    assert C.first_unsatisfied(c, w) == -1
    assert len(bounds) == 7226 and max(bounds) < c.n_wires
    assert _check_bounds(w, bounds) > 1


def test_classes_hold_on_a_solved_withdraw_witness(check_exe, tmp_path, withdraw_artifacts, withdraw_kat):
    from oracle import circuit as C
    counts, bounds = _classes(check_exe, tmp_path, ["withdraw"], "withdraw")
    c = C.Circuit(withdraw_artifacts["sppc"])
    w = C.solve(c, C.withdraw_inputs(withdraw_kat), lambda w: 0xabcdef)
    assert C.first_unsatisfied(c, w) == -1
    assert len(bounds) > 0 and max(bounds) < c.n_wires and counts["A"][1] > 0
    assert _check_bounds(w, bounds) >= 1
