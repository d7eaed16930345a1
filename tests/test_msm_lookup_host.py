"""Lookup-inverse wires on the host (csrc/msm_lookup.hpp through tests/host/msm_lookup_check.cpp, built with the address and
undefined-behaviour sanitizers): the scan over the audit and withdraw circuits against counts made here from the circuit files,
and the second level of the byte-bucket sum -- recoding, windows, signs, running sum, Horner -- against oracle/bn254.py."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd", "csrc")
OP_END, OP_BATCH_DIV, OP_COUNT8, OP_GRUMPKIN = 0, 3, 6, 10
OP_LEN = {1: 2, 2: 2, 12: 2, 3: 3, 8: 3, 11: 3, 6: 4, 4: 4, 5: 4, 7: 4, 9: 1}


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lookup") / "msm_lookup_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "msm_lookup_check.cpp"), os.path.join(CSRC, "circuit.cpp"),
                    os.path.join(CSRC, "circuit_audit.cpp"), "-o", exe], check=True)
    return exe


def _scan(check_exe, tmp_path, args, name):
    out = str(tmp_path / (name + "_lookups.txt"))
    proc = subprocess.run([check_exe] + args + [out], capture_output=True, text=True, timeout=900)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    n = int([l for l in proc.stdout.splitlines() if l.startswith("LOOKUPS")][-1].split()[1])
    pairs = [tuple(int(x) for x in line.split()) for line in open(out)]
    assert len(pairs) == n
    return pairs


def expected_lookup_inverses(circ):
    """(wire, hint row) of every lookup inverse, from the circuit file alone: the rows of an OP_BATCH_DIV whose A row is one wire
    with coefficient 1, whose C row is the constant one and whose B row plus the hint row at the same position of the preceding
    OP_COUNT8 is the challenge wire."""
    from oracle.bn254 import R
    out, pc, pr = [], 0, circ.program
    h0 = nh = 0
    while pr[pc] != OP_END:
        op = pr[pc]
        if op == OP_COUNT8:
            h0, nh = pr[pc + 1], pr[pc + 2]
        if op == OP_BATCH_DIV:
            for i in range(min(pr[pc + 2], nh)):
                k = pr[pc + 1] + i
                aw, ac = circ.A.row(k)
                cw, cc = circ.C.row(k)
                if len(aw) != 1 or ac[0] != 1 or aw[0] == 0 or tuple(cw) != (0,) or cc[0] != 1:
                    continue
                form = {}
                for m, row in ((circ.B, k), (circ.H, h0 + i)):
                    for w, c in zip(*m.row(row)):
                        form[w] = (form.get(w, 0) + c) % R
                form[circ.challenge_wire] = (form.get(circ.challenge_wire, 0) - 1) % R
                if aw[0] not in form and not any(form.values()):
                    out.append((aw[0], h0 + i))
        pc += 5 + pr[pc + 4] if op == OP_GRUMPKIN else OP_LEN[op]
    return out


def test_audit_circuit_has_6464_contiguous_lookup_inverses(check_exe, tmp_path, rlwe_pk, audit_artifacts):
    from oracle import circuit as C
    pk_txt = tmp_path / "pk.txt"
    pk_txt.write_text(" ".join(str(int(v)) for v in list(rlwe_pk["a"]) + list(rlwe_pk["b"])))
    pairs = _scan(check_exe, tmp_path, ["audit", str(pk_txt)], "audit")
    assert len(pairs) == 6464
    wires = [w for w, _ in pairs]
    hints = [h for _, h in pairs]
    assert wires == list(range(wires[0], wires[0] + 6464))          # one per div call of the builder's loop
    assert hints == list(range(hints[0], hints[0] + 6464))
    assert pairs == expected_lookup_inverses(C.Circuit(audit_artifacts["sppc"]))


def test_withdraw_circuit_matches_an_independent_count(check_exe, tmp_path, withdraw_artifacts):
    from oracle import circuit as C
    pairs = _scan(check_exe, tmp_path, ["withdraw"], "withdraw")
    want = expected_lookup_inverses(C.Circuit(withdraw_artifacts["sppc"]))
    print("withdraw: %d lookup inverses" % len(want))
    assert pairs == want and len(want) > 0
    assert _scan(check_exe, tmp_path, ["file", withdraw_artifacts["sppc"]], "withdraw_file") == want


@pytest.mark.parametrize("L", [1, 65])
def test_synthetic_lookup_circuit(check_exe, tmp_path, L):
    """tests/synth_lookup_circuits.py, the circuit of the device tests: satisfiable as generated, a looked-up 256 breaks the sum row
    alone, and the scan names exactly the generator's inverse wires with their hint rows."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import synth_circuits as S
    import synth_lookup_circuits as SL
    from oracle import circuit as C
    g = SL.gen_lookup(L)
    sppc = str(tmp_path / "lookup.sppc")
    S.write_sppc(g.desc, sppc)
    circ = C.Circuit(sppc)
    row = g.inputs(5)
    assert C.first_unsatisfied(circ, C.solve(circ, row, lambda w: 0x1234567)) == -1
    bad, sum_row = g.spoil(row, lookup=L // 2)
    assert C.first_unsatisfied(circ, C.solve(circ, bad, lambda w: 0x1234567)) == sum_row
    pairs = _scan(check_exe, tmp_path, ["file", sppc], "synth")
    assert [w for w, _ in pairs] == g.expect["inv_wires"] and [h for _, h in pairs] == list(range(L))
    assert pairs == expected_lookup_inverses(circ)


def test_a_program_with_an_unknown_instruction_has_none(check_exe):
    proc = subprocess.run([check_exe, "unknown"], capture_output=True, text=True, timeout=900)
    assert proc.returncode == 0 and proc.stdout.strip().splitlines()[-1] == "LOOKUPS 0", proc.stdout + proc.stderr


def test_second_level_sum_against_the_oracle(check_exe, tmp_path):
    """256 random points (one the point at infinity, two equal, two opposite) with scalars 0, 1, r - 1, 2^253-sized and random ones:
    the digits of lkb_recode through lkb_window_sum and the Horner give sum_t s_t * P_t as oracle/bn254.py computes it."""
    from oracle import bn254 as O
    rng = random.Random(20260)
    pts = [O.g1_mul(O.G1_GEN, rng.randrange(1, O.R)) for _ in range(256)]
    pts[7] = None
    pts[9] = pts[8]
    pts[11] = O.g1_neg(pts[10])
    half = (O.R - 1) // 2
    special = [0, 1, O.R - 1, half, half + 1, 16, 17, O.R - 16, O.R - 17, (1 << 253) - 1, 31, 32, 33, 2**250]
    sc = [special[t] if t < len(special) else rng.randrange(O.R) for t in range(256)]
    sc[8] = sc[9] = 5                     # equal points, equal digits: a doubling inside a bucket
    sc[10] = sc[11] = 12345               # opposite points, equal digits: a cancellation
    path = tmp_path / "sum_in.txt"
    path.write_text("".join("%064x %064x %064x\n" % (((p[0], p[1]) if p else (0, 0)) + (s,)) for p, s in zip(pts, sc)))
    proc = subprocess.run([check_exe, "sum", str(path)], capture_output=True, text=True, timeout=900)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    got = proc.stdout.strip().splitlines()[-1].split()
    want = O.g1_msm([p for p in pts if p], [s for p, s in zip(pts, sc) if p])
    assert got[0] == "SUM" and (int(got[1], 16), int(got[2], 16)) == tuple(want)
