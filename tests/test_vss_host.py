"""The verifiable sharing of the auditors' key on the host (csrc/vss.hpp through tests/host/vss_check.cpp, built with the address
and undefined-behaviour sanitizers) against tests/vss_model.py: the generators, the common a of a joint key, entries of the window
table, commitments read off the table for special, window-boundary and random scalars, and the receiver's check on crafted
dealings whose Horner accumulator meets its next term."""
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import vss_model as M  # noqa: E402
from oracle import bn254 as O  # noqa: E402


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vss") / "vss_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "vss_check.cpp"), "-o", exe], check=True)
    return exe


def _run(check_exe, args):
    proc = subprocess.run([check_exe] + args, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    return proc.stdout.strip().splitlines()


def test_model_generator_is_the_stated_point():
    """the model's own derivation gives the H the header states, on the curve, of order r, and is not G's small multiple by sight"""
    ctr, h = M.derive_h()
    assert ctr == 1 and h == M.H == (M.H_X, M.H_Y)
    assert O.g1_is_on_curve(h) and O.g1_mul(h, O.R - 1) == O.g1_neg(h) and h[1] < O.P - h[1]
    assert M.a_from_seed(bytes(32))[:3] == [50220146, 81832116, 17395646]


def test_generators(check_exe):
    g, h = (l.split() for l in _run(check_exe, ["gens"]))
    assert g[0] == "G" and (int(g[1], 16), int(g[2], 16)) == M.G == (1, 2)
    assert h[0] == "H" and int(h[1]) == 1 and (int(h[2], 16), int(h[3], 16)) == M.H


def test_a_from_seed(check_exe):
    seeds = [bytes(32), bytes(range(32))]
    lines = _run(check_exe, ["a"] + [s.hex() for s in seeds])
    for seed, line in zip(seeds, lines):
        tok = line.split()
        got = [int(v) for v in tok[1:]]
        assert tok[0] == "A" and len(got) == 1024 and all(v < M.Q for v in got)
        assert got == M.a_from_seed(seed)
    assert [int(v) for v in lines[0].split()[1:4]] == [50220146, 81832116, 17395646]


def test_table_entries(check_exe):
    """first and last d of the first, a middle and the top window, both bases"""
    picks = [(b, w, d) for b in (0, 1) for w in (0, 15, 31) for d in (1, 2, 128, 255)]
    idx = [(b * 32 + w) * 255 + d - 1 for b, w, d in picks]
    lines = _run(check_exe, ["entry"] + [str(i) for i in idx])
    for (b, w, d), i, line in zip(picks, idx, lines):
        tok = line.split()
        want = O.g1_mul((M.G, M.H)[b], d << (8 * w))      # g1_mul reduces mod r: the top window's large d wrap, as the sum does
        assert tok[0] == "E" and int(tok[1]) == i
        assert (int(tok[2], 16), int(tok[3], 16)) == (want or (0, 0)), (b, w, d)


def test_commitments_against_the_model(check_exe, tmp_path):
    pairs = M.scalar_pairs()
    path = tmp_path / "commit.txt"
    path.write_text("".join("%064x %064x\n" % p for p in pairs))
    lines = _run(check_exe, ["commit", str(path)])
    assert len(lines) == len(pairs)
    for (c, cb), line in zip(pairs, lines):
        tok = line.split()
        assert tok[0] == "C" and bytes.fromhex(tok[1]) == O.g1_to_bytes(M.commit(c, cb)), (hex(c), hex(cb))
    assert bytes.fromhex(lines[pairs.index((0, 0))].split()[1]) == bytes(64)


def _record(t, x, rows, rows_b, zero=None, y=None, yb=None, cm=None):
    cm = cm or [O.g1_to_bytes(M.commit(rows[k], rows_b[k])) for k in range(t)]
    y = M.poly_eval(rows, x) if y is None else y
    yb = M.poly_eval(rows_b, x) if yb is None else yb
    text = "%d %d %d\n" % (t, x, 0 if zero is None else 1) + "".join(c.hex() + "\n" for c in cm) + "%064x\n%064x\n" % (y, yb)
    return text + ("" if zero is None else "%064x\n" % zero)


def test_check_on_crafted_addition_edges(check_exe, tmp_path):
    """accepted: dealings whose accumulator equals its next term (the doubling inside the addition), is its opposite (infinity),
    or meets a commitment that is infinity; and what a plain dealing gives, right and wrong"""
    rng = random.Random(52)
    recs, want = [], []
    for t in (2, 3):
        for x in (1, 2, 3, 255, 4294967295):
            for kind in ("equal", "opposite", "infinity"):
                rows, rows_b = M.crafted_dealing(kind, t, x, rng)
                cm = [M.commit(rows[k], rows_b[k]) for k in range(t)]
                hi = None
                for k in range(t - 1, 0, -1):                 # the accumulator before the last step
                    hi = O.g1_add(O.g1_mul(hi, x), cm[k])
                hi = O.g1_mul(hi, x)
                if kind == "equal":
                    assert hi == cm[0] and hi is not None
                elif kind == "opposite":
                    assert hi == O.g1_neg(cm[0]) and M.poly_eval(rows, x) == 0 and M.poly_eval(rows_b, x) == 0
                else:
                    assert cm[1] is None
                recs.append(_record(t, x, rows, rows_b))
                want.append(0)
    # t = 3 with the top commitment at infinity, and every commitment at infinity (y = y' = 0)
    rows, rows_b = [5, 7, 0], [11, 13, 0]
    recs.append(_record(3, 9, rows, rows_b)); want.append(0)
    recs.append(_record(3, 9, [0, 0, 0], [0, 0, 0])); want.append(0)
    # plain dealings: accepted; a wrong y, a wrong y', refused; t = 1
    for t in (1, 2, 3, 5):
        rows, rows_b = [rng.randrange(M.R) for _ in range(t)], [rng.randrange(M.R) for _ in range(t)]
        x = rng.randrange(1, 1 << 32)
        recs.append(_record(t, x, rows, rows_b)); want.append(0)
        recs.append(_record(t, x, rows, rows_b, y=(M.poly_eval(rows, x) + 1) % M.R)); want.append(M.BAD_SHARE)
        recs.append(_record(t, x, rows, rows_b, yb=(M.poly_eval(rows_b, x) + 1) % M.R)); want.append(M.BAD_SHARE)
    # refresh: a zero secret with its blind published passes; a non-zero secret or another blind does not
    rows, rows_b = [0, rng.randrange(M.R)], [rng.randrange(M.R), rng.randrange(M.R)]
    recs.append(_record(2, 3, rows, rows_b, zero=rows_b[0])); want.append(0)
    recs.append(_record(2, 3, rows, rows_b, zero=(rows_b[0] + 1) % M.R)); want.append(M.NOT_ZERO)
    recs.append(_record(2, 3, [1, rows[1]], rows_b, zero=rows_b[0])); want.append(M.NOT_ZERO)
    # no point: a coordinate + p, a point off the curve; the negated point is a point, and a wrong share
    cm = [O.g1_to_bytes(M.commit(rows[k], rows_b[k])) for k in range(2)]
    px, py = O.g1_from_bytes(cm[1])
    recs.append(_record(2, 3, rows, rows_b, cm=[cm[0], (px + O.P).to_bytes(32, "big") + cm[1][32:]])); want.append(M.BAD_POINT)
    recs.append(_record(2, 3, rows, rows_b, cm=[cm[0], cm[1][:32] + ((py + 1) % O.P).to_bytes(32, "big")])); want.append(M.BAD_POINT)
    recs.append(_record(2, 3, rows, rows_b, cm=[cm[0], O.g1_to_bytes(O.g1_neg((px, py)))])); want.append(M.BAD_SHARE)
    path = tmp_path / "check.txt"
    path.write_text("".join(recs))
    got = [int(l.split()[1]) for l in _run(check_exe, ["check", str(path)])]
    assert got == want
