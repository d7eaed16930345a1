"""Threshold opening on the CPU, no GPU: the g++ build of csrc/rlwe_partial.hpp (through tests/host/partial_decrypt_check.cpp)
against tests/partial_vectors.py, the restatement over Python integers -- and the restatement against itself: t partials of a
Python Shamir split combine to auditor_vectors.decrypt under the shared key."""
import os
import random
import subprocess

import pytest

from conftest import ROOT
import auditor_vectors as V
import partial_vectors as P

CSRC = os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "partial_decrypt_check.cpp")
R, Q = P.R, P.Q


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("partial_decrypt") / "partial_decrypt_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", CSRC, SRC, "-o", exe], check=True)
    return exe


def run(exe, commands):
    """one answer line (split into tokens) per command"""
    out = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-300:] + out.stderr[-2000:]
    lines = out.stdout.strip().split("\n")
    assert lines[-1] == "OK partial_decrypt %d commands" % len(commands) and len(lines) == len(commands) + 1
    return [ln.split(" ") for ln in lines[:-1]]


def hx(v):
    return "%064x" % v


def dot_command(u, c1):
    return "D " + " ".join(hx(v) for v in u) + " " + " ".join(str(v) for v in c1)


def blind_command(e, rho, xs, me, seeds, ct, k):
    return "B %d %d %d %s %d %s %s %d" % (e, rho, len(xs), " ".join(str(x) for x in xs), me,
                                           "0" if seeds is None else "1 " + " ".join(s.hex() for s in seeds), hx(ct), k)


def test_the_restatement_combines_to_the_decryption_under_the_shared_key():
    """partials made from Python shares, with masks and smudging noise: the masks cancel, q rho vanishes, e stays inside the
    noise budget -- the combined message is decrypt() under the key that was shared; without blinding on ciphertexts that sit
    on every rounding decision"""
    for name in ("2of3", "3of5"):
        t, xs, _ = P.SETS[name]
        shares = P.shares_of(name)
        seeds = P.pair_seeds(xs)
        for i, (c0, c1) in enumerate(P.records(2)):
            e, rho = P.smudge(t, 10 * t + i)
            ct = P.ct_commitment(c0, c1)
            parts = [P.partial(shares[m], xs, m, c0, c1, seeds[m], e[m], rho[m], ct) for m in range(t)]
            msg, flag = P.combine(parts, c0)
            noise = [sum(e[m][k] for m in range(t)) for k in range(P.SLOTS)]
            want = [V.round_slot(c0[k] + p + noise[k]) for k, p in enumerate(V.schoolbook([v if v < R // 2 else v - R for v in P.small_key()], c1))]
            assert flag == 0 and msg == want, (name, i)
            assert len(set(parts[0]) | set(parts[1])) == 128 and min(parts[0]) > 1 << 200        # masked: nothing small shows
    v = V.dialled_vectors()[5]
    t, xs, _ = P.SETS["3of5"]
    shares = P.split(P.centred_key(v["sk"]), t, xs, random.Random(3))
    parts = [P.partial(shares[m], xs, m, v["c0"], v["c1"]) for m in range(t)]
    assert P.combine(parts, v["c0"]) == (v["msg"], 0)
    assert P.combine(parts[:2], v["c0"])[1] == P.BAD_PARTIALS                                     # too few partials: not a small integer


def test_scaled_share_and_dot_product_under_gpp(check):
    t, xs, _ = P.SETS["3of5"]
    lam = P.lagrange_at_zero(xs)
    share = P.shares_of("3of5")[1]
    picks = list(P.SECRET_EDGES) + share[:40]
    got = run(check, ["S %s %d %s" % (hx(lam[1]), len(picks), " ".join(hx(s) for s in picks))])[0]
    assert [int(g, 16) for g in got] == P.scaled_share(lam[1], picks)
    cases = list(P.extreme_dots())
    c0, c1 = P.records(1)[0]
    cases.append(("a scaled share of the small key", P.scaled_share(lam[1], share), c1))
    got = run(check, [dot_command(u, c) for _, u, c in cases])
    for (name, u, c), g in zip(cases, got):
        assert [int(x, 16) for x in g] == P.dot(u, c), name
    # what the first case loads: slot 0 adds one term and subtracts 1 023, slot 63 adds 64
    top = P.dot([R - 1] * P.N, [Q - 1] * P.N)
    assert top[0] == ((R - 1) * (Q - 1) * (1 - 1023)) % R and top[63] == ((R - 1) * (Q - 1) * (64 - 960)) % R


def test_blinding_under_gpp(check):
    ct = P.ct_commitment(*P.records(1)[0])
    cmds, want = [], []
    for name in ("1of1", "2of3", "3of5"):
        t, xs, _ = P.SETS[name]
        seeds = P.pair_seeds(xs)
        for me in range(t):
            for k in (0, 1, 63):
                for with_seeds in (True, False):
                    s = seeds[me] if with_seeds else None
                    e, rho = random.Random(100 * t + 10 * me + k).randint(-1024, 1024), random.Random(k).randrange(1 << 64)
                    cmds.append(blind_command(e, rho, xs, me, s, ct, k))
                    want.append((e + Q * rho + P.blind(k, ct, xs, me, s)) % R)
    for e, rho in P.EXTREME_SMUDGE:
        cmds.append(blind_command(e, rho, [7], 0, None, ct, 5))
        want.append((e + Q * rho) % R)
    # a commitment whose top four bytes differ gives the same mask (bytes 4..31 are what is hashed); another byte does not
    t, xs, _ = P.SETS["2of3"]
    seeds = P.pair_seeds(xs)
    low = ct & ((1 << 224) - 1)
    cmds += [blind_command(0, 0, xs, 0, seeds[0], c, 9) for c in (low, low | 1 << 250, low ^ 1)]
    got = [int(g[0], 16) for g in run(check, cmds)]
    assert got[:len(want)] == want
    a, b, c = got[len(want):]
    assert a == b == P.blind(9, low, xs, 0, seeds[0]) and c != a
    # the two ends of a pair cancel
    assert (P.blind(9, ct, xs, 0, seeds[0]) + P.blind(9, ct, xs, 1, seeds[1])) % R == 0


def test_combination_and_rounding_under_gpp(check):
    values = list(P.COMBINE_EDGES) + [random.Random(5).randrange(R) for _ in range(20)] + [random.Random(6).randrange(-1 << 99, 1 << 99) for _ in range(20)]
    got = run(check, ["C " + hx(v % R) for v in values])
    for v, g in zip(values, got):
        res, bad = P.combine_slot([v % R])
        assert (int(g[0]), int(g[1])) == (res, 1 if bad else 0), v
    assert [P.combine_slot([v % R])[1] for v in P.COMBINE_EDGES[:4]] == [False, False, True, True]
    rng = random.Random(8)
    pairs = [(t, 0) for t in V.TARGETS] + [(Q - 1, Q - 1), (0, 0)]
    for t in V.TARGETS:                                   # every rounding decision again, reached through a sum that wraps or not
        c0 = rng.randrange(Q)
        pairs.append((c0, (t - c0) % Q))
    got = run(check, ["R %d %d" % p for p in pairs])
    assert [int(g[0]) for g in got] == [V.round_slot(a + b) for a, b in pairs]
    assert set(V.TARGETS) <= {(a + b) % Q for a, b in pairs}


def test_the_check_program_under_the_sanitizers(tmp_path):
    """the same program built with -fsanitize=address,undefined on the extremes of the wide accumulator: stand-alone, nothing
    loaded into Python"""
    exe = str(tmp_path / "partial_decrypt_check_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, SRC, "-o", exe],
                   check=True)
    cases = P.extreme_dots()[:4]
    cmds = [dot_command(u, c) for _, u, c in cases] + [blind_command(e, rho, [7], 0, None, 5, 5) for e, rho in P.EXTREME_SMUDGE]
    cmds += ["C " + hx(v % R) for v in P.COMBINE_EDGES]
    got = run(exe, cmds)
    for (name, u, c), g in zip(cases, got):
        assert [int(x, 16) for x in g] == P.dot(u, c), name
