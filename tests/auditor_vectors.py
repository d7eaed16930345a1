"""Crafted inputs for the auditor side -- k_rlwe_decrypt, phase 1 of k_audit_open, the sk_mod_q output of k_shamir_combine -- and
what they must give, from Python integers only.

Plain Python, deterministic seeds.  Nothing here comes from the code under test or from the oracle's numpy path: the expected
message bytes are schoolbook() + round_slot(), the restatement of scripts/rlwe_decrypt.py:101-118 over unbounded integers, and
the expected key coefficients are centred_mod_q(), shamir.ts:97-120 / rlwe_decrypt.py:73-91.  tests/test_auditor_vectors_host.py
holds them against oracle.rlwe and the g++ build of csrc/audit_open.hpp; tests/test_gpu_auditor_edges.py runs them on the device.

Decryption has three decisions per slot (ao_decrypt_slot): the centring at q/2, the floor division of a negative value, and
round-half-to-even at k Delta + Delta/2.  Honest ciphertexts (noise <= 18 435 against Delta/2 = 327 680) and random ones (a tie
with probability 1e-7 per slot) never sit on one.  DIALLED ciphertexts do: under a signed monomial key +-X^s the product sk*c1 is
a signed rotation of c1, and c0[t] is chosen so that (c0 + sk*c1)[t] mod q is exactly a listed residue.  q = 256 Delta + 1, so
q // 2 = 128 Delta, Delta / 2 is an integer, and with v the centred value, (k, rem) = divmod(v, Delta):
    a TIE is 2 rem == Delta.  k even: the byte stays k (half-up would give k + 1);  k odd: it becomes k + 1 either way.
    tie_targets() lists both classes among TARGETS: k even for k = 0, 2, -2 and -128, k odd for k = 1, 127, -1 and -3 (the
    residues k Delta + Delta/2 + d with k >= 128 wrap at the centring: 128 Delta + Delta/2 + 1 is the tie -128 Delta + Delta/2).
    byte_128_targets() lists the eight residues that decode to byte 128: with a positive value 128 Delta = q // 2, the tie
    127 Delta + Delta/2 (k odd, rounded up) and the two values after it; with a negative value -128 Delta = q // 2 + 1, the
    tie -128 Delta + Delta/2 (k even, kept) and the two values before it.
The target list is rotated by s (and by the ciphertext's seed), so every target meets a slot t >= s, which reads the unwrapped
half of SK2, and a slot t < s, which reads the negated half.

EXTREMES load the 64-bit accumulator, which is folded every 128 terms: 128 (q - 1)^2 ~ 2^61.6 is the most it may hold.
OUT-OF-RANGE records carry one coefficient >= q; their expectation is the message of the residues, which is what k_audit_open
decrypts (and flags), and what spp_rlwe_decrypt_batch refuses to look at.
"""
import functools
import operator
import random

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
Q = 167772161
DELTA = Q // 256
HALF = DELTA // 2
N = 1024
SLOTS = 64
assert Q == 256 * DELTA + 1 and 2 * HALF == DELTA and Q // 2 == 128 * DELTA


# ------------------------------------------------------------------------------------------------------------- the restatement
def schoolbook(sk, c1):
    """(sk * c1 mod X^1024 + 1)[t] for the 64 message slots, over the integers, unreduced:
    sum_j sk[t - j] c1[j] for j <= t, minus sum_j sk[t - j + 1024] c1[j] for j > t.  sk, c1: any integers."""
    rev = [int(v) for v in reversed(sk)]            # rev[1023 - i] = sk[i]
    neg = [-v for v in rev]
    c1 = [int(v) for v in c1]
    out = []
    for t in range(SLOTS):
        row = rev[N - 1 - t:] + neg[:N - 1 - t]     # sk[t], sk[t-1], ..., sk[0], -sk[1023], ..., -sk[t+1]
        out.append(sum(map(operator.mul, row, c1)))
    return out


def round_slot(noisy):
    """residue of c0 + sk*c1 -> message byte: centre at q // 2, divmod by Delta, half to even, mod 256"""
    v = noisy % Q
    if v > Q // 2:
        v -= Q
    k, rem = divmod(v, DELTA)
    if 2 * rem > DELTA or (2 * rem == DELTA and k % 2 == 1):
        k += 1
    return k % 256


def decrypt(sk, c0, c1):
    """the 64 message bytes; coefficients of any size count as their residues, as any sum mod q has it"""
    return [round_slot(int(a) + b) for a, b in zip(c0, schoolbook(sk, c1))]


def decode_owner(msg):
    """rlwe_decrypt.py:127-132"""
    return (sum(int(m) << (8 * i) for i, m in enumerate(msg[:32])), sum(int(m) << (8 * i) for i, m in enumerate(msg[32:])))


# ----------------------------------------------------------------------------------------------------------------- the targets
TIE_K = (0, 1, 2, 127, 128, 254, 255)
# residues mod q.  -(k Delta + Delta/2 + d) = (255 - k) Delta + Delta/2 + (1 - d) mod q, so some negatives are listed positives: once each
TARGETS = tuple(dict.fromkeys([sgn * (k * DELTA + HALF + d) % Q for k in TIE_K for d in (-1, 0, 1) for sgn in (1, -1)] +
                              [0, 1, Q - 1,                       # the smallest values on both sides of zero
                               Q // 2, Q // 2 + 1,                # the two sides of the centring
                               DELTA, DELTA - 1, Q - DELTA]))     # the step itself
assert len(TARGETS) == 38 <= SLOTS


def classify(target):
    """(k, rem) of the centred value of a residue"""
    v = target % Q
    if v > Q // 2:
        v -= Q
    return divmod(v, DELTA)


def tie_targets():
    """(ties with k even, ties with k odd) among TARGETS"""
    ties = [t for t in TARGETS if 2 * classify(t)[1] == DELTA]
    return [t for t in ties if classify(t)[0] % 2 == 0], [t for t in ties if classify(t)[0] % 2 == 1]


def byte_128_targets():
    """(centred value > 0, centred value < 0) among the targets that decode to byte 128"""
    hit = [t for t in TARGETS if round_slot(t) == 128]
    return [t for t in hit if t <= Q // 2], [t for t in hit if t > Q // 2]


# --------------------------------------------------------------------------------------------------------------------- vectors
MONOMIAL_S = (0, 1, 63, 64, 1023)


def monomial_key(s, sign):
    sk = [0] * N
    sk[s] = 1 if sign > 0 else Q - 1
    return sk


def _vector(name, key, sk, c0, c1, **more):
    return dict(name=name, key=key, sk=sk, c0=c0, c1=c1, msg=decrypt(sk, c0, c1), **more)


def dialled(s, sign, seed=0):
    """One ciphertext under sign * X^s whose slot t sits exactly on targets[t]: the 38 TARGETS and 26 random residues (so that no
    two ciphertexts decrypt alike), the whole rotated by s + seed.  c1 random in [0, q)."""
    rng = random.Random(1000003 * seed + 2 * s + (sign > 0))
    sk = monomial_key(s, sign)
    c1 = [rng.randrange(Q) for _ in range(N)]
    rot = (s + seed) % SLOTS
    filled = list(TARGETS) + [rng.randrange(Q) for _ in range(SLOTS - len(TARGETS))]
    targets = [filled[(t + rot) % SLOTS] for t in range(SLOTS)]
    prod = schoolbook(sk, c1)
    c0 = [(targets[t] - prod[t]) % Q for t in range(SLOTS)]
    v = _vector("dialled %sX^%d #%d" % ("+" if sign > 0 else "-", s, seed), ("monomial", s, sign), sk, c0, c1, targets=targets)
    assert v["msg"] == [round_slot(t) for t in targets]
    return v


@functools.lru_cache(maxsize=None)
def dialled_vectors():
    """one dialled ciphertext per signed monomial key"""
    return tuple(dialled(s, sign) for s in MONOMIAL_S for sign in (1, -1))


POOL_KEY = (63, -1)     # -X^63: slots 0..62 read the negated half of SK2, slot 63 the other one


@functools.lru_cache(maxsize=None)
def dialled_pool(count=129):
    """`count` distinct dialled ciphertexts under one key, for the batch shapes of k_audit_open; #0 is in dialled_vectors()"""
    pool = tuple(dialled(POOL_KEY[0], POOL_KEY[1], seed) for seed in range(count))
    assert len(set(tuple(v["c1"]) for v in pool)) == count == len(set(tuple(v["msg"]) for v in pool))
    return pool


@functools.lru_cache(maxsize=None)
def extreme_vectors():
    rng = random.Random(20250)
    out = []
    top = [Q - 1] * N
    out.append(_vector("all q-1", "top", top, [Q - 1] * SLOTS, top))                    # every fold holds 128 (q-1)^2
    alt = [0 if i % 2 == 0 else Q - 1 for i in range(N)]
    for j in (127, 128, 1023):                                                           # last term of a fold, first of the next, last of all
        c1 = [0] * N
        c1[j] = Q - 1
        out.append(_vector("alternating key, c1[%d] = q-1" % j, "alternating", alt, [rng.randrange(Q) for _ in range(SLOTS)], c1))
    c1 = [0] * N
    for j in (127, 128, 1023):
        c1[j] = Q - 1
    out.append(_vector("alternating key, c1[127, 128, 1023] = q-1", "alternating", alt, [rng.randrange(Q) for _ in range(SLOTS)], c1))
    dense = [rng.randrange(Q) for _ in range(N)]
    out.append(_vector("dense key, c1 all q-1", "dense", dense, [rng.randrange(Q) for _ in range(SLOTS)], top))
    return tuple(out)


def by_key(vectors):
    """[(sk, [vectors under it])] in order of first appearance: one device call takes one key"""
    groups = {}
    for v in vectors:
        groups.setdefault(v["key"], (v["sk"], []))[1].append(v)
    return list(groups.values())


# ---- out of range
BAD_VALUES = (Q, Q + 1, 2 * Q - 1, (1 << 32) - 1)
BAD_POSITIONS = (("c0", 0), ("c0", 63), ("c1", 0), ("c1", 1), ("c1", 2), ("c1", 3), ("c1", 255), ("c1", 256), ("c1", 1020),
                 ("c1", 1021), ("c1", 1022), ("c1", 1023))


@functools.lru_cache(maxsize=None)
def range_key():
    rng = random.Random(31337)
    return [rng.randrange(Q) for _ in range(N)]


def clean_record(i):
    """a ciphertext with all coefficients below q, distinct for every i, under range_key()"""
    rng = random.Random(424242 + i)
    return [rng.randrange(Q) for _ in range(SLOTS)], [rng.randrange(Q) for _ in range(N)]


def inject(c0, c1, where, index, value):
    c0, c1 = list(c0), list(c1)
    (c0 if where == "c0" else c1)[index] = value
    return c0, c1


@functools.lru_cache(maxsize=None)
def out_of_range_vectors():
    """every listed position with every listed value, each in a base ciphertext of its own; msg: the message of the residues"""
    out = []
    for p, (where, index) in enumerate(BAD_POSITIONS):
        for b, value in enumerate(BAD_VALUES):
            c0, c1 = inject(*clean_record(1000 + 4 * p + b), where, index, value)
            v = _vector("%s[%d] = %d" % (where, index, value), "range", range_key(), c0, c1, where=where, index=index, value=value)
            assert v["msg"] == decrypt(range_key(), [x % Q for x in c0], [x % Q for x in c1])
            out.append(v)
    return tuple(out)


RANGE_BATCH = 65
RANGE_RECORDS = (0, 5, 10, 15, 20, 25, 30, 35, 40, 50, 62, 64)      # record 64 is alone in the second block


@functools.lru_cache(maxsize=None)
def out_of_range_batch():
    """65 records under range_key(): position p of BAD_POSITIONS injected into record RANGE_RECORDS[p] with value p mod 4 of
    BAD_VALUES, clean records between them.  Returns (clean, injected, bad): two lists of 65 (c0, c1, msg) and the injected
    records' indices; clean[i] and injected[i] differ in that one coefficient only."""
    assert len(RANGE_RECORDS) == len(BAD_POSITIONS) and max(RANGE_RECORDS) == RANGE_BATCH - 1
    sk = range_key()
    clean, injected = [], []
    for i in range(RANGE_BATCH):
        c0, c1 = clean_record(i)
        clean.append((c0, c1, decrypt(sk, c0, c1)))
        if i in RANGE_RECORDS:
            p = RANGE_RECORDS.index(i)
            c0, c1 = inject(c0, c1, BAD_POSITIONS[p][0], BAD_POSITIONS[p][1], BAD_VALUES[p % len(BAD_VALUES)])
            injected.append((c0, c1, decrypt(sk, c0, c1)))
        else:
            injected.append(clean[i])
    return clean, injected, list(RANGE_RECORDS)


# ---------------------------------------------------------------------------------------------------------------------- Shamir
SECRETS = (0, 1, 3, R - 1, R - 3, (R - 1) // 2, (R + 1) // 2, Q - 1, Q, Q + 1, R - Q, R - Q - 1, 1 << 32, (1 << 64) - 1, 1 << 224,
           7 * Q, R - 7 * Q)
SHAMIR_T = (1, 2, 3, 64)
SHAMIR_N = (1, 255, 256, 257)       # the 256-thread block of k_shamir_combine and its tail


def centred_mod_q(v):
    """shamir.ts:97-120 / rlwe_decrypt.py:73-91: v if v <= (r - 1) / 2, else v - r; then Python's % q"""
    assert 0 <= v < R
    return (v if v <= (R - 1) // 2 else v - R) % Q


@functools.lru_cache(maxsize=None)
def secret_pool():
    """the listed secrets, 20 random field elements, then further random ones up to 257 values, all distinct"""
    rng = random.Random(977)
    pool = list(SECRETS) + [rng.randrange(R) for _ in range(20)]
    while len(pool) < max(SHAMIR_N):
        pool.append(rng.randrange(R))
    assert len(set(pool)) == len(pool)
    return tuple(pool)


def share_xs(t):
    """t distinct share indices, unsorted, 2^32 - 1 among them"""
    rng = random.Random(50 + t)
    xs = [(1 << 32) - 1] + [1, 1 << 31, 7, 2][:t - 1]
    xs += list(range(100, 100 + t - len(xs)))
    rng.shuffle(xs)
    if xs == sorted(xs):
        xs.reverse()
    assert len(xs) == t == len(set(xs)) and 0 not in xs and (t == 1 or xs != sorted(xs))
    return xs


@functools.lru_cache(maxsize=None)
def shamir_case(t, n):
    """dict(xs: [t], ys: [t][n], secrets: [n], sk_mod_q: [n]).  Value i is secret_pool()[(i + 5 t) mod 257], shared by a random
    polynomial of degree t - 1 with that constant term: ys[j][i] = f_i(xs[j]) mod r."""
    rng = random.Random(7919 * t + n)
    pool = secret_pool()
    secrets = [pool[(i + 5 * t) % len(pool)] for i in range(n)]
    xs = share_xs(t)
    ys = [[0] * n for _ in range(t)]
    for i, s in enumerate(secrets):
        coeffs = [s] + [rng.randrange(R) for _ in range(t - 1)]
        for j, x in enumerate(xs):
            acc = 0
            for c in reversed(coeffs):
                acc = (acc * x + c) % R
            ys[j][i] = acc
    return dict(t=t, n=n, xs=xs, ys=ys, secrets=secrets, sk_mod_q=[centred_mod_q(s) for s in secrets])


def shamir_shapes():
    return [(t, n) for t in SHAMIR_T for n in SHAMIR_N]
