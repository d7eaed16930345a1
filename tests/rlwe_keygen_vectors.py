"""What the committed fixtures pin of the reference's key generation (scripts/rlwe_keygen.py with random.Random(42)), derived on
the CPU once per process and shared by tests/test_rlwe_keygen_host.py and tests/test_gpu_rlwe_keygen.py:
    sk      rlwe_decrypt.json's sk_mod_q, centred
    a, b    rlwe_pk.json
    e       centred(b + a*sk mod (X^1024 + 1, q)), which must lie in [-3, 3]
    c1      the degree-1 Shamir coefficient of every key coefficient, y1 - sk mod r from share 1
and the schoolbook negacyclic product in numpy int64 that the device results are compared with."""
import functools
import json
import os

import numpy as np

from conftest import GOLDEN

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
Q = 167772161
N = 1024
BOUND = 3


def negacyclic(a, s):
    """a * s mod (X^1024 + 1) over the integers, int64: a in [0, q), |s| <= 128: |terms| < 2^35, |sums| < 2^45"""
    full = np.convolve(np.asarray(a, dtype=np.int64), np.asarray(s, dtype=np.int64))
    out = full[:N].copy()
    out[:N - 1] -= full[N:]
    return out


def public_b(sk, a, e):
    """b = e - a*sk mod (X^1024 + 1, q) in [0, q)   (rlwe_keygen.py:110-116)"""
    return np.mod(np.asarray(e, dtype=np.int64) - negacyclic(a, sk), Q).astype(np.uint32)


def centred(v, mod=Q):
    v = int(v) % mod
    return v - mod if v > mod // 2 else v


@functools.lru_cache(maxsize=None)
def fixture_key():
    """dict(sk, a, e, b, sk_mod_q: lists of ints; c1: [int] * 1024; shares: the fixture's two shares; share3_head)"""
    d = json.load(open(os.path.join(GOLDEN, "rlwe_decrypt.json")))
    pk = json.load(open(os.path.join(GOLDEN, "rlwe_pk.json")))
    sk = [centred(v) for v in d["sk_mod_q"]]
    a, b = [int(v) for v in pk["a"]], [int(v) for v in pk["b"]]
    e = [centred(int(x)) for x in (np.asarray(b, dtype=np.int64) + negacyclic(a, sk)) % Q]
    assert max(abs(v) for v in sk) <= BOUND and max(abs(v) for v in e) <= BOUND
    s1, s2 = d["shares"]
    assert (s1["x"], s2["x"], d["share3_x"]) == (1, 2, 3)
    y1, y2 = ([int(v, 16) for v in s["y"]] for s in (s1, s2))
    c1 = [(y - s) % R for y, s in zip(y1, sk)]
    return dict(sk=sk, a=a, e=e, b=b, sk_mod_q=[int(v) for v in d["sk_mod_q"]], c1=c1, y1=y1, y2=y2,
                share3_head=[int(v, 16) for v in d["share3_y_head"]], shares=d["shares"])


def edge_keys():
    """the six edge cases of tests/host/rlwe_keygen_check.cpp as arrays [6, 1024]: (sk int8, a uint32, e int8)"""
    rng = np.random.default_rng(20240607)
    small = lambda: rng.integers(-BOUND, BOUND + 1, N).astype(np.int8)
    unif = lambda: rng.integers(0, Q, N).astype(np.uint32)
    x1023 = np.zeros(N, dtype=np.int8)
    x1023[N - 1] = 1
    cases = [(small(), unif(), small()),                                               # a random key
             (np.zeros(N, dtype=np.int8), unif(), small()),                            # sk = 0
             (np.full(N, 3, dtype=np.int8), np.full(N, Q - 1, dtype=np.uint32), small()),   # sk = +3, a = q - 1
             (np.full(N, -3, dtype=np.int8), unif(), small()),                         # sk = -3
             (small(), np.zeros(N, dtype=np.uint32), small()),                         # a = 0
             (x1023, unif(), np.full(N, -3, dtype=np.int8))]                           # sk = X^1023: every product wraps
    return tuple(np.stack([c[k] for c in cases]) for k in range(3))
