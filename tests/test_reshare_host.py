"""The reshare section of csrc/vss.hpp on the host (through tests/host/reshare_check.cpp, built with the address and
undefined-behaviour sanitizers as a stand-alone program) against tests/reshare_model.py: the weighted sum of dealers' points by
one shared bit scan, for special and window-boundary weights and for points that are equal, opposite and at infinity; the public
commitment of a share; the NOT_SHARE decision; the Lagrange weights and the weighted sum of sub-shares."""
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import reshare_model as RM  # noqa: E402
import vss_model as M  # noqa: E402
from oracle import bn254 as O  # noqa: E402

R = M.R
XS = (1, 2, 255, 4294967295)


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("reshare") / "reshare_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "reshare_check.cpp"), "-o", exe], check=True)
    return exe


def _run(check_exe, args):
    proc = subprocess.run([check_exe] + args, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    return proc.stdout.strip().splitlines()


def _lincomb_record(points, weights, base):
    text = "%d %d %d\n" % (len(points), 0 if weights is None else 1, 0 if base is None else 1)
    text += "".join((p if isinstance(p, bytes) else O.g1_to_bytes(p)).hex() + "\n" for p in points)
    if weights is not None:
        text += "".join("%064x\n" % w for w in weights)
    if base is not None:
        text += O.g1_to_bytes(base).hex() + "\n"
    return text


def _lincombs(check_exe, tmp_path, cases):
    path = tmp_path / "lincomb.txt"
    path.write_text("".join(_lincomb_record(p, w, b) for _, p, w, b in cases))
    lines = _run(check_exe, ["lincomb", str(path)])
    assert len(lines) == len(cases)
    return [(int(l.split()[1]), bytes.fromhex(l.split()[2])) for l in lines]


def test_lincomb_for_special_and_window_weights(check_exe, tmp_path):
    """one output value; weights from special_scalars() and window_scalars(), a weight of 0 among them, on random points"""
    rng = random.Random(61)
    cases = []
    for w in RM.weight_vectors(rng):
        pts = [O.g1_mul(M.G, rng.randrange(1, R)) for _ in w]
        cases.append((str(w), pts, w, None))
    assert any(0 in w for _, _, w, _ in cases)
    for (name, pts, w, _), (flags, got) in zip(cases, _lincombs(check_exe, tmp_path, cases)):
        assert flags == 0 and got == O.g1_to_bytes(RM.lincomb_points(pts, w)), name


def test_lincomb_on_crafted_points(check_exe, tmp_path):
    """equal, opposite and infinity inputs: the partial sum that returns to infinity in the middle of the scan, the all-infinity
    input, a base that cancels or equals the sum, and the plain (unweighted) sums"""
    rng = random.Random(62)
    cases = RM.crafted_lincombs(rng)
    names = [c[0] for c in cases]
    assert "infinity mid-scan" in names and "all infinity" in names
    for (name, pts, w, base), (flags, got) in zip(cases, _lincombs(check_exe, tmp_path, cases)):
        assert flags == 0 and got == O.g1_to_bytes(RM.lincomb_points(pts, w, base)), name
    want = dict(zip(names, (RM.lincomb_points(p, w, b) for _, p, w, b in cases)))
    assert want["opposite"] is None and want["all infinity"] is None and want["every weight 0"] is None and want["base cancels the sum"] is None


def test_lincomb_on_crafted_lanes_of_one_weight_vector(check_exe, tmp_path):
    """what a launch looks like: ONE weight vector, and per lane points that make the partial sum meet +-the next term at the top
    bit, in the middle and at bit 0 of the scan (tests/test_gpu_reshare.py runs the same lanes on the device)"""
    rng = random.Random(67)
    for dealers in (2, 3):
        weights = RM.crafted_weights(rng, dealers)
        lanes = RM.crafted_lanes(weights, rng)
        cases = [(name, pts, weights, None) for name, pts in lanes]
        for (name, pts, w, _), (flags, got) in zip(cases, _lincombs(check_exe, tmp_path, cases)):
            assert flags == 0 and got == O.g1_to_bytes(RM.lincomb_points(pts, w)), (dealers, name)


def test_lincomb_flags_what_is_no_point(check_exe, tmp_path):
    rng = random.Random(63)
    px, py = O.g1_mul(M.G, rng.randrange(1, R))
    good = O.g1_to_bytes((px, py))
    cases = [("x + p", [good, (px + O.P).to_bytes(32, "big") + good[32:]], [3, 5], None),
             ("off the curve", [good[:32] + ((py + 1) % O.P).to_bytes(32, "big"), good], None, None),
             ("a point", [good, O.g1_to_bytes(O.g1_neg((px, py)))], None, None)]
    got = _lincombs(check_exe, tmp_path, cases)
    assert [f for f, _ in got] == [RM.BAD_POINT, RM.BAD_POINT, 0] and got[2][1] == bytes(64)


def _dealing(rng, t):
    rows, rows_b = [rng.randrange(R) for _ in range(t)], [rng.randrange(R) for _ in range(t)]
    return rows, rows_b, b"".join(O.g1_to_bytes(M.commit(c, cb)) for c, cb in zip(rows, rows_b))


def test_share_commitment(check_exe, tmp_path):
    """E_x at x in {1, 2, 255, 4294967295} for t in {1, 2, 3}, with the crafted dealings whose Horner walk meets +-its next term"""
    rng = random.Random(64)
    recs, want = [], []
    for t in (1, 2, 3):
        for x in XS:
            cms = [_dealing(rng, t)[2]]
            if t > 1:
                for kind in ("equal", "opposite", "infinity"):
                    rows, rows_b = M.crafted_dealing(kind, t, x, rng)
                    cms.append(b"".join(O.g1_to_bytes(M.commit(c, cb)) for c, cb in zip(rows, rows_b)))
            for cm in cms:
                recs.append("%d %d\n" % (t, x) + "".join(cm[64 * k:64 * k + 64].hex() + "\n" for k in range(t)))
                want.append(O.g1_to_bytes(RM.share_commitment(t, 1, cm, x, 0)))
    path = tmp_path / "ex.txt"
    path.write_text("".join(recs))
    lines = _run(check_exe, ["ex", str(path)])
    assert [(l.split()[1], bytes.fromhex(l.split()[2])) for l in lines] == [("1", w) for w in want]
    assert bytes(64) in want                                  # the opposite dealings: E_x is infinity


def test_not_share_decision(check_exe, tmp_path):
    """right: the constant term share G + blind H of the share at x; wrong: share + 1, another x's share, the negated point, a
    non-point; infinity on both sides is right"""
    rng = random.Random(65)
    recs, want = [], []
    for t in (1, 2, 3):
        for x in XS:
            rows, rows_b, cm = _dealing(rng, t)
            y, yb = M.poly_eval(rows, x), M.poly_eval(rows_b, x)
            right = M.commit(y, yb)
            cases = [(O.g1_to_bytes(right), 0), (O.g1_to_bytes(M.commit((y + 1) % R, yb)), RM.NOT_SHARE),
                     (O.g1_to_bytes(O.g1_neg(right)), RM.NOT_SHARE), (bytes(64), RM.NOT_SHARE),
                     (O.g1_to_bytes(right)[:32] + ((right[1] + 1) % O.P).to_bytes(32, "big"), RM.BAD_POINT)]
            if t > 1:
                cases.append((O.g1_to_bytes(M.commit(M.poly_eval(rows, x + 1), M.poly_eval(rows_b, x + 1))), RM.NOT_SHARE))
            for c0, flag in cases:
                assert RM.is_share(t, 1, cm, x, 0, c0) == flag
                recs.append("%d %d\n" % (t, x) + "".join(cm[64 * k:64 * k + 64].hex() + "\n" for k in range(t)) + c0.hex() + "\n")
                want.append(flag)
    rows, rows_b = M.crafted_dealing("opposite", 2, 255, rng)   # E_255 is infinity, and so is the commitment of the share (0, 0)
    cm = b"".join(O.g1_to_bytes(M.commit(c, cb)) for c, cb in zip(rows, rows_b))
    recs.append("2 255\n" + cm[:64].hex() + "\n" + cm[64:].hex() + "\n" + bytes(64).hex() + "\n")
    want.append(0)
    path = tmp_path / "isshare.txt"
    path.write_text("".join(recs))
    assert [int(l.split()[1]) for l in _run(check_exe, ["isshare", str(path)])] == want


def test_lagrange_and_weighted_sum(check_exe, tmp_path):
    for xs in ([1], [1, 3], [2, 1, 5], [255, 1, 4294967295], list(range(1, 65))):
        got = [int(l.split()[1], 16) for l in _run(check_exe, ["lagrange"] + [str(x) for x in xs])]
        assert got == M.lagrange_at_zero(xs), xs
    rng = random.Random(66)
    recs, want = [], []
    for dealers in (1, 2, 3, 64):
        w = [rng.choice(M.special_scalars() + [rng.randrange(R)]) for _ in range(dealers)]
        ys = [rng.choice([0, R - 1, rng.randrange(R)]) for _ in range(dealers)]
        recs.append("%d\n" % dealers + "".join("%064x\n" % v for v in w + ys))
        want.append(sum(a * b for a, b in zip(w, ys)) % R)
    path = tmp_path / "wsum.txt"
    path.write_text("".join(recs))
    assert [int(l.split()[1], 16) for l in _run(check_exe, ["wsum", str(path)])] == want
