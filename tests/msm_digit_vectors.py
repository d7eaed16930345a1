"""The recoding contract of the table walks as data: the reference digits of a scalar, written from the contract of k_msm_digits
(csrc/kernels_msm.hip) and not from its loop, and per window width c the scalar families that reach the places where a recoder
goes wrong.

Contract.  Let v be the signed representative of s mod r: v = s for s <= (r-1)/2, else s - r.  The planes hold the unique digits
d_j in [-2^(c-1), 2^(c-1) - 1], 0 <= j < W = ceil(254/c), with sum_j d_j 2^(c j) = v as integers.  (|v| < 2^253 <= 2^(cW - 1), so W
digits always suffice; the asymmetric range is what lets c = 16 fit int16: -2^15 exists there, +2^15 does not.)

Three consumers: tests/test_msm_digit_vectors_host.py (the families hold what they are for, by the reference alone),
tests/test_gpu_msm_digits.py (the planes of the device against the reference) and tests/test_gpu_msm_windows.py (both walks at
every width, over the same families)."""
import random

from oracle import bn254 as B

R = B.R
HALF_R = (R - 1) // 2
WIDTHS = tuple(range(4, 17))
FAMILIES = ("edges", "chain", "allmax", "toponly", "carrytop", "sparse")


def windows(c):
    return (254 + c - 1) // c


def padded_batch(P):
    """Proofs per row of the planes: a batch of 64 or more is rounded up to whole waves (msm_padded_batch, csrc/msm_plan.hpp)."""
    return (P + 63) // 64 * 64 if P >= 64 else P


def signed(s):
    s %= R
    return s if s <= HALF_R else s - R


def digits(s, c):
    """The W reference digits of the scalar s at width c, lowest window first."""
    v, half, out = signed(s), 1 << (c - 1), []
    for _ in range(windows(c)):
        d = ((v + half) % (1 << c)) - half
        v = (v - d) >> c
        out.append(d)
    assert v == 0, (s, c)
    return out


def top_window(c):
    """jt: the highest window in which a single set bit 2^(c jt) is still a scalar below (r-1)/2."""
    return 252 // c


def _shifted_down(v, c):
    while v > HALF_R:
        v >>= c
    return v


def families(c):
    """name -> list of scalars in [0, r), for window width c."""
    W, half, jt = windows(c), 1 << (c - 1), top_window(c)
    top = 1 << (c * jt)
    chain = _shifted_down(sum(half << (c * j) for j in range(W)), c)
    allmax = _shifted_down(sum((half - 1) << (c * j) for j in range(W)), c)
    return {
        "edges": [0, 1, R - 1, HALF_R, HALF_R + 1, 255, half - 1, half, half + 1, (1 << c) - 1, 1 << c],
        "chain": [chain, R - chain],
        "allmax": [allmax, R - allmax],
        "toponly": [top, R - top, HALF_R >> (c * jt) << (c * jt)],
        "carrytop": [top - 1, R - (top - 1)],
        "sparse": [top + 5, R - (top + 5), top - 3, top + half - 1],
    }


def random_scalars(n, seed):
    """n scalars in [0, r) that do not depend on the width (a width's tests share them, and so does the oracle's cache)."""
    rng = random.Random(seed)
    return [rng.randrange(R) for _ in range(n)]


def with_edges(row, c, p=0):
    """A copy of row with the edge scalars of width c spread over it: at other bases for every p, among the other scalars."""
    row = list(row)
    edges = families(c)["edges"]
    where = [(7 * p + 11 * k) % len(row) for k in range(len(edges))]
    assert len(set(where)) == len(edges)
    for i, v in zip(where, edges):
        row[i] = v
    return row


def flat_walk_rows(c, n):
    """The nine scalar rows of a flat-walk call at width c over n bases (tests/test_gpu_msm_windows.py).  Row 0: random with the
    edges.  Rows 1..6: one family each across all bases, cycling through its members.  Row 7: every scalar below 2^(c-1) -- only
    pass 0 has work, every pass above it sums to infinity.  Row 8: digits in windows 0 and jt only, every third scalar folded."""
    fam, half, jt = families(c), 1 << (c - 1), top_window(c)
    rng = random.Random(500 + c)
    rows = [with_edges(random_scalars(n, 88), c)]
    for k, name in enumerate(FAMILIES):
        m = fam[name]
        rows.append([m[(i + k) % len(m)] for i in range(n)])
    rows.append([rng.randrange(half) for _ in range(n)])
    sparse = []
    for i in range(n):
        s = rng.randrange(1, half) + (rng.randrange(1, min(3, HALF_R >> (c * jt)) + 1) << (c * jt))
        assert s <= HALF_R
        sparse.append(s if i % 3 else R - s)
    rows.append(sparse)
    return rows
