"""The verifiable sharing of the auditors' key in Python integers (oracle.bn254 for the curve, hashlib for SHA-256; no call into
the package): the generators, the common a of a joint key, dealing, the receiver's check, the sum of sub-shares and the joint key.
The tests of csrc/vss.hpp, of the spp_vss_* calls and of `spp dkg-deal` / `dkg-receive` compare with this."""
import hashlib

from oracle import bn254 as O

R, P = O.R, O.P
N, Q = 1024, 167772161
G = O.G1_GEN
BAD_POINT, BAD_SHARE, NOT_ZERO = 1, 2, 4
# what include/spp.h states for H (ctr = 1)
H_X = 0x195fd53357566de91ef7d79dd6133d81aa5fe1504f8ae4de62748144a660f90c
H_Y = 0x13008f0858db79f81776aedb341c12082a7ded53353189557326dba50cf8fc9f


def derive_h():
    """(ctr, H): the first counter whose hash is the x of a curve point, y the smaller root"""
    ctr = 0
    while True:
        x = int.from_bytes(hashlib.sha256(b"spp-vss-pedersen-h" + ctr.to_bytes(4, "big")).digest(), "big") % P
        v = (x * x * x + 3) % P
        y = pow(v, (P + 1) // 4, P)          # P = 3 mod 4
        if y * y % P == v:
            return ctr, (x, min(y, P - y))
        ctr += 1


H = (H_X, H_Y)


def a_from_seed(seed):
    assert len(seed) == 32
    out, ctr = [], 0
    while len(out) < N:
        d = hashlib.sha256(b"spp-dkg-a" + seed + ctr.to_bytes(4, "big")).digest()
        for w in range(8):
            v = int.from_bytes(d[4 * w:4 * w + 4], "big") & 0x0FFFFFFF
            if v < Q and len(out) < N:
                out.append(v)
        ctr += 1
    return out


def commit(c, cb):
    """c G + c' H, None for infinity"""
    return O.g1_add(O.g1_mul(G, c), O.g1_mul(H, cb))


def poly_eval(coeffs, x):
    """sum_k coeffs[k] x^k mod r"""
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def deal(secrets, blinds, coeffs, coeffs_blind, xs):
    """coeffs[k - 1][v]: coefficient of x^k of value v (the layout of shamir_split).  Returns (commitments as bytes, C_k[v] at
    (k n + v) * 64; ys[j][v]; ys_blind[j][v])."""
    n, t = len(secrets), len(coeffs) + 1
    rows, rows_b = [list(secrets)] + [list(r) for r in coeffs], [list(blinds)] + [list(r) for r in coeffs_blind]
    cm = b"".join(O.g1_to_bytes(commit(rows[k][v], rows_b[k][v])) for k in range(t) for v in range(n))
    ys = [[poly_eval([rows[k][v] for k in range(t)], x) for v in range(n)] for x in xs]
    yb = [[poly_eval([rows_b[k][v] for k in range(t)], x) for v in range(n)] for x in xs]
    return cm, ys, yb


def decode_point(raw):
    """(ok, point): 64 canonical bytes of a curve point or of infinity"""
    if raw == b"\0" * 64:
        return True, None
    x, y = int.from_bytes(raw[:32], "big"), int.from_bytes(raw[32:], "big")
    if x >= P or y >= P or (y * y - x * x * x - 3) % P:
        return False, None
    return True, (x, y)


def check_value(t, x, n, commitments, v, y, yb, zero_blind=None):
    """the flags of one value of one dealer (commitments: that dealer's t * n * 64 bytes)"""
    pts = []
    for k in range(t):
        ok, pt = decode_point(commitments[(k * n + v) * 64:(k * n + v) * 64 + 64])
        if not ok:
            return BAD_POINT
        pts.append(pt)
    rhs, xp = None, 1
    for pt in pts:
        rhs = O.g1_add(rhs, O.g1_mul(pt, xp))
        xp = xp * x % R
    flags = 0 if commit(y, yb) == rhs else BAD_SHARE
    if zero_blind is not None and O.g1_mul(H, zero_blind) != pts[0]:
        flags |= NOT_ZERO
    return flags


def share_sum(ys_by_dealer, base=None):
    n = len(ys_by_dealer[0])
    return [((base[v] if base is not None else 0) + sum(ys[v] for ys in ys_by_dealer)) % R for v in range(n)]


def negacyclic(a, s):
    """a * s mod (X^1024 + 1, q) for lists of ints (s may be signed)"""
    import numpy as np
    a64 = np.array(a, dtype=np.int64)
    out = np.zeros(N, dtype=np.int64)
    for j, sj in enumerate(s):
        sj = int(sj)
        if sj == 0:
            continue
        rot = np.concatenate((-a64[N - j:], a64[:N - j])) if j else a64
        out = (out + sj * rot) % Q
    return [int(v) for v in out]


def public_b(a, s, e):
    """b = e - a s"""
    prod = negacyclic(a, s)
    return [(int(ev) - pv) % Q for ev, pv in zip(e, prod)]


def joint_key(a, parts):
    """parts: [(s_i, e_i)] signed lists.  Returns (sum b_i mod q, sum s_i as signed ints)"""
    b = [0] * N
    for s, e in parts:
        b = [(x + y) % Q for x, y in zip(b, public_b(a, s, e))]
    return b, [sum(int(s[v]) for s, _ in parts) for v in range(N)]


def lagrange_at_zero(xs):
    lam = []
    for i, xi in enumerate(xs):
        num = den = 1
        for j, xj in enumerate(xs):
            if i != j:
                num = num * (-xj) % R
                den = den * (xi - xj) % R
        lam.append(num * pow(den, -1, R) % R)
    return lam


def reconstruct(xs, ys_rows):
    lam = lagrange_at_zero(xs)
    return [sum(l * row[v] for l, row in zip(lam, ys_rows)) % R for v in range(len(ys_rows[0]))]


def special_scalars():
    return [0, 1, 2, R - 1, (R - 1) // 2, (R + 1) // 2]


def window_scalars():
    """2^(8 w) for every window boundary below r, and 2^(8 w) - 1 with all-0xFF windows below"""
    out = []
    for w in range(1, 32):
        if (1 << (8 * w)) < R:
            out += [1 << (8 * w), (1 << (8 * w)) - 1]
    return out


def scalar_pairs(seed=51):
    """(c, c') pairs for commitments: every pair of special scalars ((0, 0) among them), the window scalars against each other
    and against 0, 20 random pairs"""
    import random
    rng = random.Random(seed)
    sp = special_scalars()
    pairs = [(c, cb) for c in sp for cb in sp]
    ws = window_scalars()
    pairs += [(s, ws[(i * 7 + 3) % len(ws)]) for i, s in enumerate(ws)] + [(s, 0) for s in ws[:4]] + [(0, s) for s in ws[-4:]]
    pairs += [(rng.randrange(R), rng.randrange(R)) for _ in range(20)]
    return pairs


def crafted_dealing(kind, t, x, rng):
    """One value whose check meets an addition edge; returns (rows, rows_blind): t coefficients each, constant term first.
    kind 'equal': C_0 = x C_1 (the last Horner step adds a point to itself); 'opposite': C_0 = -x C_1 (x^(t-1) terms cancel to
    infinity at that step); 'infinity': a C_k in the middle (k = 1) is the point at infinity."""
    rows = [rng.randrange(1, R) for _ in range(t)]
    rows_b = [rng.randrange(1, R) for _ in range(t)]
    if kind == "infinity":
        rows[1] = rows_b[1] = 0
    else:
        sign = 1 if kind == "equal" else -1
        # Horner: acc_1 = sum_{k>=1} x^(k-1) C_k, then x acc_1 + C_0: make C_0 = +- x acc_1
        for r_ in (rows, rows_b):
            hi = sum(r_[k] * pow(x, k, R) for k in range(1, t)) % R
            r_[0] = sign * hi % R
    return rows, rows_b
