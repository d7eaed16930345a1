"""Threshold opening (csrc/rlwe_partial.hpp, k_rlwe_partial, k_rlwe_combine) restated over Python integers, and the crafted
inputs its tests share.

Plain Python, deterministic seeds.  Nothing here comes from the code under test: the product is auditor_vectors.schoolbook over
unbounded integers, the rounding auditor_vectors.round_slot, the mask oracle.bn254.expand_message_xmd (48 bytes, mod r) under
the tag "spp-partial-mask", the ciphertext commitment oracle.hashes.poseidon2_sponge over oracle.rlwe.pack_values, and the
shares come from split() below -- a Python Shamir split over BN254 Fr -- not from the device.

    scaled share   u[j] = lambda_i s_i[j] mod r,  lambda_i = prod_{j != i} (-x_j) / (x_i - x_j)
    partial        p_i[k] = (u * c1 mod X^1024 + 1)[k] + e[k] + q rho[k] + sum_{j != i} sgn(x_i, x_j) M(seed_ij, ct, k)   mod r
    combination    w[k] = sum_i p_i[k] mod r, centred; |w| >= 2^104 flags the record (bit 8); byte = round_slot(c0[k] + w)
"""
import functools
import random

import auditor_vectors as V

R, Q, N, SLOTS = V.R, V.Q, V.N, V.SLOTS
DST = b"spp-partial-mask"
BAD_PARTIALS = 8
SMALL = 1 << 104
assert len(DST) == 16


# ------------------------------------------------------------------------------------------------------------- the restatement
def lagrange_at_zero(xs):
    out = []
    for i, xi in enumerate(xs):
        num = den = 1
        for j, xj in enumerate(xs):
            if j != i:
                num = num * (-xj) % R
                den = den * (xi - xj) % R
        out.append(num * pow(den, R - 2, R) % R)
    return out


def split(secrets, t, xs, rng):
    """ys[j][i] = f_i(xs[j]) mod r, f_i of degree t - 1 with constant term secrets[i] and coefficients from rng"""
    ys = [[0] * len(secrets) for _ in xs]
    for i, s in enumerate(secrets):
        coeffs = [s % R] + [rng.randrange(R) for _ in range(t - 1)]
        for j, x in enumerate(xs):
            acc = 0
            for c in reversed(coeffs):
                acc = (acc * x + c) % R
            ys[j][i] = acc
    return ys


def centred_key(sk_mod_q):
    """a key given mod q as the Fr values an auditor set shares: v for v <= q // 2, else v - q (mod r)"""
    return [(v if v <= Q // 2 else v - Q) % R for v in sk_mod_q]


def scaled_share(lam, share):
    return [lam * s % R for s in share]


def dot(u, c1):
    """(u * c1)[k] mod r for the 64 slots: the unreduced integer product, reduced once"""
    return [v % R for v in V.schoolbook(u, c1)]


def ct_commitment(c0, c1):
    from oracle import hashes, rlwe
    return hashes.poseidon2_sponge(rlwe.pack_values([int(v) for v in c0]) + rlwe.pack_values([int(v) for v in c1]))


def mask(seed, ct, k):
    from oracle import bn254
    msg = bytes(seed) + ct.to_bytes(32, "big")[4:] + k.to_bytes(4, "big")
    assert len(msg) == 64
    return int.from_bytes(bn254.expand_message_xmd(msg, DST, 48), "big") % R


def blind(k, ct, xs, me, seeds=None, e=None, rho=None):
    b = (0 if e is None else int(e[k])) + Q * (0 if rho is None else int(rho[k]))
    if seeds is not None:
        for j, x in enumerate(xs):
            if j != me:
                m = mask(seeds[j], ct, k)
                b += m if xs[me] < x else -m
    return b % R


def partial(share, xs, me, c0, c1, seeds=None, e=None, rho=None, ct=None):
    """the 64 field elements auditor `me` (position in xs) publishes for one ciphertext"""
    u = scaled_share(lagrange_at_zero(xs)[me], share)
    ct = ct_commitment(c0, c1) if ct is None and seeds is not None else ct
    return [(d + blind(k, ct, xs, me, seeds, e, rho)) % R for k, d in enumerate(dot(u, c1))]


def combine_slot(values):
    """(residue mod q of the centred sum, inconsistent?)"""
    w = sum(values) % R
    if w > (R - 1) // 2:
        w -= R
    return w % Q, abs(w) >= SMALL


def combine(partials, c0):
    """partials: [t][64] -> (64 message bytes, 0 or BAD_PARTIALS)"""
    slots = [combine_slot([p[k] for p in partials]) for k in range(SLOTS)]
    return [V.round_slot(int(c0[k]) + res) for k, (res, _) in enumerate(slots)], BAD_PARTIALS if any(b for _, b in slots) else 0


def be(values):
    return b"".join(int(v).to_bytes(32, "big") for v in values)


def unbe(raw):
    return [int.from_bytes(raw[i:i + 32], "big") for i in range(0, len(raw), 32)]


# ----------------------------------------------------------------------------------------------------------------- the inputs
def pair_seeds(xs, tag=0):
    """seeds[i][j] = the 32 bytes auditors i and j share (position in xs), the same at both ends; seeds[i][i] is filler"""
    t = len(xs)
    rng = random.Random(9000 + 31 * t + tag)
    s = [[None] * t for _ in range(t)]
    for i in range(t):
        for j in range(i, t):
            s[i][j] = s[j][i] = bytes(rng.randrange(256) for _ in range(32))
    return s


SETS = {  # name: (t, xs of the participating set, m)
    "1of1": (1, [1], 1),
    "2of3": (2, [3, 1], 3),
    "3of5": (3, [5, (1 << 32) - 1, 2], 5),
}
assert all(len(xs) == t and (t == 1 or xs != sorted(xs)) for t, xs, _ in SETS.values())


@functools.lru_cache(maxsize=None)
def small_key():
    """a key as spp_rlwe_keygen_batch makes it: coefficients in [-3, 3], as Fr values"""
    rng = random.Random(4711)
    return tuple(rng.randint(-3, 3) % R for _ in range(N))


@functools.lru_cache(maxsize=None)
def shares_of(name, key=None):
    """the shares (one list of 1024 per member of the set) of `key` (default small_key()) under SETS[name]"""
    t, xs, _ = SETS[name]
    return split(list(small_key() if key is None else key), t, xs, random.Random(600 + t))


@functools.lru_cache(maxsize=None)
def records(count):
    return tuple(V.clean_record(7000 + i) for i in range(count))


def smudge(count, tag, bound=1024):
    rng = random.Random(8100 + tag)
    return ([[rng.randint(-bound, bound) for _ in range(SLOTS)] for _ in range(count)],
            [[rng.randrange(1 << 64) for _ in range(SLOTS)] for _ in range(count)])


# ---- extremes of the wide accumulator and the blinding
TOP_LIMBS = int.from_bytes(bytes.fromhex("2fffffff" + "ffffffff" * 7), "big")     # limbs 0x2fffffff, 0xffffffff x 7: below r
assert TOP_LIMBS < R
SINGLE_J = (0, 63, 64, 1023)
SECRET_EDGES = (0, 1, R - 1, (R - 1) // 2, (R + 1) // 2, TOP_LIMBS)


@functools.lru_cache(maxsize=None)
def extreme_dots():
    """[(name, u[1024], c1[1024])]: scaled shares handed to the dot product as they are (lambda = 1, t = 1)"""
    rng = random.Random(555)
    dense = [rng.randrange(R) for _ in range(N)]
    out = [("u all r-1, c1 all q-1", [R - 1] * N, [Q - 1] * N),            # slot 0: one added term, 1 023 subtracted; slot 63: 64 added
           ("u all top limbs, c1 all q-1", [TOP_LIMBS] * N, [Q - 1] * N),
           ("u all top limbs, c1 all 2^28-1", [TOP_LIMBS] * N, [(1 << 28) - 1] * N)]     # the header's own bound on c1
    for j in SINGLE_J:
        c1 = [0] * N
        c1[j] = Q - 1
        out.append(("dense u, c1[%d] = q-1" % j, dense, c1))
    out.append(("dense u, dense c1", dense, [rng.randrange(Q) for _ in range(N)]))
    return tuple(out)


EXTREME_SMUDGE = ((1 << 20, (1 << 64) - 1), (-(1 << 20), (1 << 64) - 1), (-(1 << 20), 0), (0, 0), (-1, 1), (-(1 << 31), 5), ((1 << 31) - 1, 5))
COMBINE_EDGES = (SMALL - 1, -(SMALL - 1), SMALL, -SMALL, 0, 1, -1, Q, -Q, (R - 1) // 2, -((R - 1) // 2), (1 << 110) + 12345, SMALL + Q)
