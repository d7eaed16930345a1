"""The setup ceremony on the host (csrc/setup_contrib.hpp through tests/host/setup_contrib_check.cpp, built with the address and
undefined-behaviour sanitizers): the non-adjacent form of the contribution's scalar, the scaling of points by its digits against
oracle/bn254.py, the point check, and the structural comparison of two proving keys on hand-made byte buffers."""
import os
import random
import struct
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tests"))
MAX_DIGITS = 256


def special_scalars():
    from oracle.bn254 import R
    return [1, 2, 3, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, 1 << 253, (1 << 253) - 1, 15, 16, 17]


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ceremony") / "setup_contrib_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "setup_contrib_check.cpp"), "-o", exe], check=True)
    return exe


def _run(check_exe, args):
    proc = subprocess.run([check_exe] + args, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    return proc.stdout.strip().splitlines()


def test_recoding_is_the_non_adjacent_form(check_exe):
    rng = random.Random(41)
    from oracle.bn254 import R
    ks = special_scalars() + [rng.randrange(1, R) for _ in range(20)]
    lines = _run(check_exe, ["recode"] + ["%064x" % k for k in ks])
    assert len(lines) == len(ks)
    for k, line in zip(ks, lines):
        tok = line.split()
        length, dig = int(tok[1]), [int(t) for t in tok[2:]]
        assert tok[0] == "NAF" and len(dig) == MAX_DIGITS
        assert all(d in (-1, 0, 1) for d in dig)
        assert sum(d << i for i, d in enumerate(dig)) == k
        assert not any(dig[i] and dig[i + 1] for i in range(MAX_DIGITS - 1)), "two adjacent non-zero digits for %x" % k
        # the form has at most one digit more than the binary expansion, its top digit is +1, nothing above it
        assert length <= k.bit_length() + 1 and dig[length - 1] == 1 and not any(dig[length:])
        # ... and it is the sparsest signed-binary form: never more non-zero digits than the binary expansion has ones
        assert sum(1 for d in dig if d) <= bin(k).count("1")


def ceremony_points(rng):
    """generator, infinity, two equal points, a point and its negative, two random points"""
    from oracle import bn254 as O
    a, b = (O.g1_mul(O.G1_GEN, rng.randrange(1, O.R)) for _ in range(2))
    return [O.G1_GEN, None, a, a, b, O.g1_neg(b)] + [O.g1_mul(O.G1_GEN, rng.randrange(1, O.R)) for _ in range(2)]


def test_host_scaling_against_the_oracle(check_exe, tmp_path):
    from oracle import bn254 as O
    rng = random.Random(42)
    pts = ceremony_points(rng)
    assert len(pts) == 8
    want_flags = [2 if p is None else 1 for p in pts]
    for n, k in enumerate(special_scalars() + [rng.randrange(1, O.R) for _ in range(20)]):
        path = tmp_path / ("scale_%d.txt" % n)
        path.write_text("%064x\n" % k + "".join("%064x %064x\n" % (p or (0, 0)) for p in pts))
        got = [l.split() for l in _run(check_exe, ["scale", str(path)])]
        assert [int(g[1]) for g in got] == want_flags
        want = [O.g1_mul(p, k) or (0, 0) for p in pts]
        assert [(int(g[2], 16), int(g[3], 16)) for g in got] == want, "scalar %x" % k


def test_point_check_refuses_what_is_no_point(check_exe, tmp_path):
    from oracle import bn254 as O
    x, y = O.g1_mul(O.G1_GEN, 77)
    cases = [((x, y), 1), ((0, 0), 2), ((x, (y + 1) % O.P), 0), ((x + O.P, y), 0), ((x, y + O.P), 0), ((0, 1), 0), ((1, 0), 0),
             ((x, O.P - y), 1), ((O.P, O.P), 0)]
    path = tmp_path / "decode.txt"
    path.write_text("%064x\n" % 1 + "".join("%064x %064x\n" % c for c, _ in cases))
    got = [int(l.split()[1]) for l in _run(check_exe, ["scale", str(path)])]
    assert got == [f for _, f in cases]


def _key(n_a=3, n_k=5, n_z=7, seed=1):
    """a hand-made container with distinguishable bytes in every field; returns (bytes, offsets of its parts)"""
    rng = random.Random(seed)
    blob = lambda n: bytes(rng.randrange(256) for _ in range(n))
    parts, off = [], {}

    def put(name, b):
        off[name] = sum(len(p) for p in parts)
        parts.append(b)
    put("header", struct.pack("<7I", 0x4B505053, 1, 9, 40, 3, 2, 11))
    for name, size in (("alpha1", 64), ("beta1", 64), ("delta1", 64), ("beta2", 128), ("delta2", 128)):
        put(name, blob(size))
    for name, n, size, wires in (("A", n_a, 64, True), ("B1", 2, 64, True), ("B2", 2, 128, True), ("K", n_k, 64, True), ("Z", n_z, 64, False),
                                 ("CB", 1, 64, True), ("CS", 1, 64, True)):
        put(name + "_count", struct.pack("<I", n))
        if wires:
            put(name + "_wires", struct.pack("<%dI" % n, *range(10, 10 + n)))
        put(name + "_points", blob(size * n))
    return b"".join(parts), off


def _diff(check_exe, tmp_path, before, after):
    b, a = tmp_path / "before.pk", tmp_path / "after.pk"
    b.write_bytes(before)
    a.write_bytes(after)
    tok = _run(check_exe, ["diff", str(b), str(a)])[-1].split()
    assert tok[0] == "DIFF"
    return [int(t) for t in tok[1:]]


OK, FORMAT, OTHER = 0, 1, 2


def test_structural_diff_on_hand_made_buffers(check_exe, tmp_path):
    import sppk_format
    key, off = _key()
    assert sppk_format.Sppk(key).to_bytes() == key              # the restatement and the hand-made buffer agree on the layout
    got = _diff(check_exe, tmp_path, key, key)
    assert got == [OK, 5, 7, off["delta1"], off["delta2"], off["K_points"], off["Z_points"]]
    flip = lambda data, at: data[:at] + bytes([data[at] ^ 1]) + data[at + 1:]
    # every byte a contribution may change, first and last of each range
    for name, size in (("delta1", 64), ("delta2", 128), ("K_points", 5 * 64), ("Z_points", 7 * 64)):
        for at in (off[name], off[name] + size - 1):
            assert _diff(check_exe, tmp_path, key, flip(key, at))[0] == OK, name
    # the bytes next to those ranges: refused (some belong to a count, and the key then no longer parses)
    for at in (off["delta1"] - 1, off["delta1"] + 64, off["delta2"] - 1, off["delta2"] + 128, off["K_points"] - 1, off["K_points"] + 5 * 64,
               off["Z_points"] - 1, off["Z_points"] + 7 * 64):
        assert _diff(check_exe, tmp_path, key, flip(key, at))[0] in (FORMAT, OTHER), at
    # one byte of every other field, the header's words after magic and version, the last byte of the file
    others = [off[n] for n in ("alpha1", "beta1", "beta2", "A_wires", "A_points", "B1_points", "B2_wires", "B2_points", "K_wires", "CB_wires",
                               "CB_points", "CS_points")] + [8, 12, 16, 20, 24, len(key) - 1]
    for at in others:
        assert _diff(check_exe, tmp_path, key, flip(key, at))[0] == OTHER, at
    # other counts: both keys parse, at another length and at the same length (an A entry and a K entry are 68 bytes each)
    other_key, _ = _key(n_k=6, n_z=6)
    assert len(other_key) == len(key) + 4 and _diff(check_exe, tmp_path, key, other_key)[0] == OTHER
    other_key, _ = _key(n_a=2, n_k=6)
    assert len(other_key) == len(key) and _diff(check_exe, tmp_path, key, other_key)[0] == OTHER
    # what does not parse: truncated, one byte more, wrong magic, wrong version, a count that runs past the end, nothing
    for bad in (key[:-1], key + b"\0", flip(key, 0), flip(key, 4), key[:off["K_count"]] + struct.pack("<I", 1 << 30) + key[off["K_count"] + 4:],
                key[:20], b""):
        assert _diff(check_exe, tmp_path, key, bad)[0] == FORMAT
        assert _diff(check_exe, tmp_path, bad, key)[0] == FORMAT


def test_verifying_key_diff(check_exe, tmp_path):
    rng = random.Random(3)
    nk = 4
    vk = bytes(rng.randrange(256) for _ in range(576)) + struct.pack(">I", nk) + bytes(rng.randrange(256) for _ in range(64 * nk + 12 + 256))

    def diff(a, b):
        pa, pb = tmp_path / "a.vk", tmp_path / "b.vk"
        pa.write_bytes(a)
        pb.write_bytes(b)
        return _run(check_exe, ["vkdiff", str(pa), str(pb)])[-1] == "VKDIFF 1"
    flip = lambda data, at: data[:at] + bytes([data[at] ^ 1]) + data[at + 1:]
    assert diff(vk, vk)
    for at in (384, 447, 448, 575):                             # delta1 | delta2
        assert diff(vk, flip(vk, at))
    for at in (0, 64, 128, 256, 383, 576, 580, len(vk) - 1):    # alpha1, beta1, beta2, gamma2, the count, K, the Pedersen key
        assert not diff(vk, flip(vk, at))
    assert not diff(vk, vk[:-1]) and not diff(vk[:-1], vk[:-1]) and not diff(vk, b"")
