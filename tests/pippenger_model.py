"""The general-base Pippenger MSM (csrc/kernels_pippenger.hip) in Python integers (oracle.bn254 for the curve; no call into the
package): the signed 16-bit recoding, the bucket layout of a window's sorted list with the 256-entry segments and the fix-up path
each bucket takes, builders for scalars with chosen window values, the synthetic generator of spp_msm_g1_pippenger_bench_shard, a
closed-form oracle over a pool of points with known logarithms, and the crafted cases of tests/test_gpu_pippenger_edges.py, each
with the shape it claims (tests/test_pippenger_model_host.py holds every case to its claim under layout()).

The closed form: every base is P_j = k_j G with k_j known, so sum_i s_i P_idx(i) = (sum_i k_idx(i) s_i mod r) G -- ONE scalar
multiplication whatever n is, which is what lets sizes beyond the reach of orc_msm_g1 be compared byte for byte."""
import random
from collections import namedtuple

from oracle import bn254 as O

R = O.R
HALF = (R - 1) // 2                 # the recoder folds a scalar to |s| <= HALF
W, C = 16, 16                       # windows, bits per window
B = 1 << (C - 1)                    # buckets per window: bucket = |digit| - 1
SEG = 256                           # entries of a window's sorted list per lane of k_pip_segments
FIX_SEQ = 12                        # a bucket spanning s1 - s0 <= 12 segments is joined by one lane, beyond by a wave
PART1, PART2 = 16384, 8192          # points per level-1 sort piece, entries per level-2 piece
TILE = 1 << 20                      # points per counting workgroup
CHUNK = 16                          # buckets per chunk of k_pip_chunks (2048 chunks per window)
TOP_MAX = HALF >> (C * (W - 1))     # the largest value the top window of a folded scalar can hold (0x1832)


# ------------------------------------------------------------------------------------------------------------------ recoding
def digits_and_carry(s):
    """The rule above k_pip_digits: fold to |s| <= (r-1)/2, recode from the bottom; a window value above keep_max carries, where
    keep_max is 2^15 - 1 for a + fold and 2^15 for a - fold; the stored digit has the fold sign applied.  Returns (the 16 digits,
    the carry out of the top window)."""
    assert 0 <= s < R
    neg = s > HALF
    mag = R - s if neg else s
    keep_max = B if neg else B - 1
    carry, out = 0, []
    for j in range(W):
        d = ((mag >> (C * j)) & 0xffff) + carry
        if d > keep_max:
            d -= 1 << C
            carry = 1
        else:
            carry = 0
        out.append(-d if neg else d)
    return out, carry


def digits(s):
    return digits_and_carry(s)[0]


def scalar_with(window_values, negate=False):
    """The scalar whose MAGNITUDE has the given 16-bit window values ({window: value} or a list from window 0 up); negate gives
    r - that (a - fold).  The magnitude has to be one the recoder can meet: at most (r-1)/2."""
    items = window_values.items() if isinstance(window_values, dict) else enumerate(window_values)
    mag = 0
    for j, v in items:
        assert 0 <= j < W and 0 <= v < (1 << C)
        mag += v << (C * j)
    assert mag <= HALF, "not a folded magnitude"
    return (R - mag) % R if negate else mag


def scalar_from_digits(digs):
    """The scalar sum_j digs[j] 2^(16 j) mod r, for signed digits ({window: digit} or a list)."""
    items = digs.items() if isinstance(digs, dict) else enumerate(digs)
    return sum(d << (C * j) for j, d in items) % R


# -------------------------------------------------------------------------------------------------------------------- layout
def layout(scalars):
    """Per window j a dict: total (entries of the sorted list = scalars with a non-zero digit there), counts {bucket: entries},
    offsets {bucket: exclusive offset in the list}, buckets {bucket: dict(count, offset, s0, s1, path, ends_on_boundary, members)}
    for the non-empty buckets.  s0 / s1: first and last 256-entry segment the bucket touches; path: 'direct' (one segment, written
    by its segment lane), 'sequential' (k_pip_fixup, s1 - s0 <= 12) or 'heavy' (k_pip_fixup_heavy); members: [(i, negative)] in
    index order (the device's order inside a bucket comes from atomics and is not this one)."""
    memo = {}
    per = [dict() for _ in range(W)]
    for i, s in enumerate(scalars):
        dg = memo.get(s)
        if dg is None:
            dg = memo[s] = digits(s)
        for j, d in enumerate(dg):
            if d:
                per[j].setdefault(abs(d) - 1, []).append((i, d < 0))
    out = []
    for j in range(W):
        off, counts, offsets, buckets = 0, {}, {}, {}
        for b in sorted(per[j]):
            cnt = len(per[j][b])
            s0, s1 = off // SEG, (off + cnt - 1) // SEG
            path = "direct" if s0 == s1 else "sequential" if s1 - s0 <= FIX_SEQ else "heavy"
            counts[b], offsets[b] = cnt, off
            buckets[b] = dict(count=cnt, offset=off, s0=s0, s1=s1, path=path, ends_on_boundary=(off + cnt) % SEG == 0,
                              members=per[j][b])
            off += cnt
        out.append(dict(total=off, counts=counts, offsets=offsets, buckets=buckets))
    return out


# -------------------------------------------------------------------------------------------------- pool and the closed form
class Pool:
    """Points with known logarithms to the group's generator.  The last entry is infinity (logarithm 0, all-zero bytes); three
    entries are tied to entry 0 = P: Q = 2^16 P, -P and 2 P."""

    def __init__(self, group, n_random, seed):
        assert group in ("g1", "g2")
        self.group = group
        self.size = 64 if group == "g1" else 128
        rng = random.Random(seed)
        logs = [rng.randrange(1, 1 << 64) for _ in range(n_random)]
        self.P_IDX = 0
        self.Q_IDX, self.NEG_IDX, self.TWO_IDX, self.WIDE_IDX, self.INF_IDX = range(n_random, n_random + 5)
        logs += [(logs[0] << 16) % R, R - logs[0], 2 * logs[0], rng.randrange(1, R), 0]
        self.logs = logs
        self.finite = n_random + 4              # indices [0, finite) are finite points
        self._bytes = {}

    def __len__(self):
        return len(self.logs)

    def _log_to_bytes(self, k):
        if self.group == "g1":
            return O.g1_to_bytes(O.g1_mul(O.G1_GEN, k))
        return O.g2_to_bytes(O.g2_mul(O.G2_GEN, k % R) if k % R else None)

    def point_bytes(self, j):
        b = self._bytes.get(j)
        if b is None:
            b = self._bytes[j] = self._log_to_bytes(self.logs[j])
        return b

    def bases(self, idx):
        return b"".join(self.point_bytes(j) for j in idx)

    def log(self, idx, scalars):
        assert len(idx) == len(scalars)
        return sum(self.logs[j] * s for j, s in zip(idx, scalars)) % R

    def expected(self, idx, scalars):
        """(sum_i k_idx(i) s_i mod r) G, serialised as spp_msm_g1_pippenger / spp_msm_g2_pippenger return it"""
        return self._log_to_bytes(self.log(idx, scalars))


_POOLS = {}


def pool(group):
    """251 entries for G1, 16 for G2 (the Python twist arithmetic is slow), built once"""
    if group not in _POOLS:
        _POOLS[group] = Pool(group, 246, 0x9199) if group == "g1" else Pool(group, 11, 0x9299)
    return _POOLS[group]


def log_to_g1_bytes(k):
    return O.g1_to_bytes(O.g1_mul(O.G1_GEN, k))


# ------------------------------------------------------------------------------------------------------ the device generator
LCG_A, LCG_C, M64 = 6364136223846793005, 1442695040888963407, (1 << 64) - 1
RINV = pow(1 << 256, -1, R)


def lcg_jump(x, steps):
    """x after `steps` steps of x -> a x + c mod 2^64, in O(log steps)"""
    a, c, acc_a, acc_c = LCG_A, LCG_C, 1, 0
    while steps:
        if steps & 1:
            acc_a, acc_c = acc_a * a & M64, (acc_c * a + c) & M64
        a, c = a * a & M64, (a + 1) * c & M64
        steps >>= 1
    return (acc_a * x + acc_c) & M64


def iter_bench_points(n, seed, small_permille, first=0):
    """Points [first, first + n) of spp_msm_g1_pippenger_bench_shard's sequence as (k, limbs, small): base k G; the scalar is the
    byte limbs & 0xff when small, otherwise the raw limbs written into Montgomery storage, i.e. the field element limbs 2^-256."""
    per = 6 if small_permille else 5                         # generator steps per point
    x = lcg_jump((seed * LCG_A + LCG_C) & M64, per * first)
    for _ in range(n):
        x = (x * LCG_A + LCG_C) & M64
        k = x | 1
        limbs = 0
        for q in range(4):
            x = (x * LCG_A + LCG_C) & M64
            limbs |= x << (64 * q)
        limbs &= (1 << 253) - 1                              # the top 32-bit limb is masked to 29 bits
        small = False
        if small_permille:
            x = (x * LCG_A + LCG_C) & M64
            small = (x >> 20) % 1000 < small_permille
        yield k, limbs, small


def bench_points(n, seed, small_permille, first=0):
    """[(k_i, s_i)]: base k_i G and the scalar as a field element, for points [first, first + n) of the sequence"""
    return [(k, limbs & 0xff if small else limbs * RINV % R) for k, limbs, small in iter_bench_points(n, seed, small_permille, first)]


def bench_log(n, seed, small_permille, first=0):
    """sum_i k_i s_i mod r over the same points, without keeping them (2^-256 is taken out of the sum of the raw-limb scalars)"""
    raw = byte = 0
    for k, limbs, small in iter_bench_points(n, seed, small_permille, first):
        if small:
            byte += k * (limbs & 0xff)
        else:
            raw += k * limbs
    return (raw * RINV + byte) % R


# -------------------------------------------------------------------------------------------------------------------- claims
Case = namedtuple("Case", "name idx scalars claim")


def window_logs(pl, idx, scalars):
    """logarithm of every window sum: sum_i digit_ij k_idx(i) mod r"""
    out = [0] * W
    for i, s in zip(idx, scalars):
        for j, d in enumerate(digits(s)):
            out[j] += d * pl.logs[i]
    return [v % R for v in out]


def _bucket_log(pl, idx, entry):
    return sum(-pl.logs[idx[i]] if neg else pl.logs[idx[i]] for i, neg in entry["members"]) % R


def check_claim(pl, case):
    """Holds a crafted case to every statement of its claim; returns a line saying what was confirmed.  Claim keys:
      digits {i: 16 digits}            the recoding of scalars[i], written out by hand in the builder
      only_windows [j..]               exactly these windows have entries
      buckets {(j, b): {field: v}}     fields of layout()[j]['buckets'][b] (count, offset, s0, s1, path, ends_on_boundary)
      bucket_set {j: [b..]}            the non-empty buckets of window j are exactly these
      bucket_logs {(j, b): log}        logarithm of the bucket's sum (0: the bucket sums to infinity)
      uniform {(j, b): log}            every entry of the bucket is the same base with the same sign, so each full segment's partial
                                       has logarithm 256 * log whatever the order, and the bucket has at least two full segments
      chunks {(j, c1, c2): +1 | -1}    chunk sums S (and T) of chunks c1, c2 are equal (+1) or opposite (-1), both non-zero, and no
                                       other chunk of the window is occupied
      window_logs {j: log}             logarithm of the window sum
      horner_equal j                   the host's Horner accumulator, shifted, equals window sum j (non-zero) when it is added
      horner_zero j                    the accumulator is infinity after window j is added, and some lower window is non-empty
      inf [i..]                        these positions hold the pool's infinity; all_inf: every position does
      pieces (level1, level2)          sort pieces per window: every window's list has all n entries
      zero_result                      the expected sum is infinity"""
    idx, scalars, claim = case.idx, case.scalars, case.claim
    assert len(idx) == len(scalars) and set(claim) <= {
        "digits", "only_windows", "buckets", "bucket_set", "bucket_logs", "uniform", "chunks", "window_logs", "horner_equal",
        "horner_zero", "inf", "all_inf", "pieces", "zero_result"}, case.name
    lay = layout(scalars)
    said = []
    for i, want in claim.get("digits", {}).items():
        assert digits(scalars[i]) == list(want), (case.name, i, hex(scalars[i]), digits(scalars[i]), want)
    if "digits" in claim:
        said.append("%d recodings as written" % len(claim["digits"]))
    if "only_windows" in claim:
        assert [j for j in range(W) if lay[j]["total"]] == sorted(claim["only_windows"]), case.name
        said.append("entries only in windows %s" % sorted(claim["only_windows"]))
    for (j, b), fields in claim.get("buckets", {}).items():
        got = lay[j]["buckets"].get(b)
        assert got is not None, (case.name, j, b, "empty")
        for f, v in fields.items():
            assert got[f] == v, (case.name, j, b, f, got[f], v)
        said.append("window %d bucket %d: %s" % (j, b, ", ".join("%s=%s" % fv for fv in sorted(fields.items()))))
    for j, want in claim.get("bucket_set", {}).items():
        assert sorted(lay[j]["buckets"]) == sorted(want), (case.name, j, sorted(lay[j]["buckets"]))
        said.append("window %d occupies exactly buckets %s" % (j, sorted(want)))
    for (j, b), want in claim.get("bucket_logs", {}).items():
        assert _bucket_log(pl, idx, lay[j]["buckets"][b]) == want % R, (case.name, j, b)
        said.append("window %d bucket %d sums to %s" % (j, b, "infinity" if want % R == 0 else "the claimed point"))
    for (j, b), want in claim.get("uniform", {}).items():
        e = lay[j]["buckets"][b]
        assert len({(idx[i], neg) for i, neg in e["members"]}) == 1, (case.name, j, b)
        i0, neg0 = e["members"][0]
        assert (-pl.logs[idx[i0]] if neg0 else pl.logs[idx[i0]]) % R == want % R and want % R
        first_full = (e["offset"] + SEG - 1) // SEG
        assert (e["offset"] + e["count"]) // SEG - first_full >= 2, (case.name, j, b, "fewer than two full segments")
        said.append("window %d bucket %d: one base, one sign, full-segment partials all 256 P" % (j, b))
    for (j, c1, c2), sign in claim.get("chunks", {}).items():
        S, T = {}, {}
        for b, e in lay[j]["buckets"].items():
            v = _bucket_log(pl, idx, e)
            S[b // CHUNK] = (S.get(b // CHUNK, 0) + v) % R
            T[b // CHUNK] = (T.get(b // CHUNK, 0) + (b % CHUNK + 1) * v) % R
        assert sorted(S) == sorted({c1, c2}) and S[c1] and T[c1], (case.name, j, sorted(S))
        assert S[c2] == sign * S[c1] % R and T[c2] == sign * T[c1] % R, (case.name, j, c1, c2)
        said.append("window %d chunks %d and %d: %s S and T" % (j, c1, c2, "equal" if sign == 1 else "opposite"))
    wl = None
    if {"window_logs", "horner_equal", "horner_zero"} & set(claim):
        wl = window_logs(pl, idx, scalars)
    for j, want in claim.get("window_logs", {}).items():
        assert wl[j] == want % R, (case.name, j)
        said.append("window %d sums to the claimed point" % j)
    if "horner_equal" in claim or "horner_zero" in claim:
        acc, before, after = 0, {}, {}
        for j in range(W - 1, -1, -1):
            acc = (acc << C) % R
            before[j] = acc
            acc = (acc + wl[j]) % R
            after[j] = acc
        if "horner_equal" in claim:
            j = claim["horner_equal"]
            assert before[j] == wl[j] != 0, (case.name, j)
            said.append("Horner adds window %d to an equal accumulator" % j)
        if "horner_zero" in claim:
            j = claim["horner_zero"]
            assert after[j] == 0 and wl[j] != 0 and any(lay[q]["total"] for q in range(j)), (case.name, j)
            said.append("Horner accumulator is infinity after window %d, lower windows non-empty" % j)
    if "inf" in claim:
        assert all(idx[i] == pl.INF_IDX for i in claim["inf"]) and pl.logs[pl.INF_IDX] == 0, case.name
        assert any(s % R for i, s in enumerate(scalars) if idx[i] == pl.INF_IDX)       # infinity meets non-zero digits
        said.append("infinity at %d positions, among them %s" % (sum(1 for i in idx if i == pl.INF_IDX), sorted(claim["inf"])))
    if claim.get("all_inf"):
        assert all(i == pl.INF_IDX for i in idx) and any(scalars), case.name
        said.append("every base at infinity")
    if "pieces" in claim:
        n = len(scalars)
        assert all(lay[j]["total"] == n for j in range(W)), case.name
        assert ((n + PART1 - 1) // PART1, (n + PART2 - 1) // PART2) == tuple(claim["pieces"]), case.name
        said.append("n=%d: %d level-1 and %d level-2 pieces in every window" % ((n,) + tuple(claim["pieces"])))
    if claim.get("zero_result"):
        assert pl.log(idx, scalars) == 0, case.name
        said.append("sum is infinity")
    return "%s (n=%d): %s" % (case.name, len(scalars), "; ".join(said))


# ------------------------------------------------------------------------------------------------------------- crafted cases
EDGE_VALUES = (1, B - 1, B, B + 1, (1 << C) - 1)
TOP_VALUES = (1, TOP_MAX - 1, TOP_MAX)           # what |s| <= (r-1)/2 leaves of the list in the top window


def _single_window_digits(j, v, negate):
    """By hand: window value v alone in window j.  + fold: v < 2^15 stays, v >= 2^15 becomes v - 2^16 and carries 1.
    - fold: v <= 2^15 stays (stored -v), v > 2^15 becomes v - 2^16 (stored 2^16 - v) and carries (stored -1)."""
    d = [0] * W
    if negate:
        if v <= B:
            d[j] = -v
        else:
            d[j], d[j + 1] = (1 << C) - v, -1
    else:
        if v < B:
            d[j] = v
        else:
            d[j], d[j + 1] = v - (1 << C), 1
    return d


def case_digit_edges(pl, seed=1):
    """One launch of 300 scalars: every edge value alone in every window with both fold signs, runs of 0xffff, 0x8000 in every
    window at once, carry chains into the top window, the special scalars; random bases; random scalars fill up to 300."""
    rng = random.Random(seed)
    sc, dg = [], {}

    def put(s, want):
        dg[len(sc)] = want
        sc.append(s)
    for j in range(W):
        for v in (EDGE_VALUES if j < W - 1 else TOP_VALUES):
            for negate in (False, True):
                put(scalar_with({j: v}, negate), _single_window_digits(j, v, negate))
    # runs of 0xffff over windows [a, a + len): + fold: -1 at a, zeros, +1 at a + len;  - fold: the same negated
    for a, ln in ((0, 2), (5, 2), (13, 2), (0, 3), (7, 3), (12, 3), (0, 15)):
        for negate in (False, True):
            want = [0] * W
            want[a], want[a + ln] = -1, 1
            put(scalar_with({j: 0xffff for j in range(a, a + ln)}, negate), [-x for x in want] if negate else want)
    # 0x8000 in every window below the top one (the top window cannot hold it).  + fold: window 0 carries (-2^15), every later one
    # is 0x8001 and carries (-0x7fff), the chain ends as +1 (or top + 1) in the top window.  - fold: 2^15 stays everywhere: no carry.
    for top in (0, TOP_MAX - 1):
        vals = {j: B for j in range(W - 1)}
        vals[W - 1] = top
        put(scalar_with(vals), [-B] + [-(B - 1)] * (W - 2) + [top + 1])
        put(scalar_with(vals, True), [-B] * (W - 1) + [-top])
    # a carry chain of 0xffff that ends in a top window already at TOP_MAX - 1
    vals = {j: 0xffff for j in range(W - 1)}
    vals[W - 1] = TOP_MAX - 1
    put(scalar_with(vals), [-1] + [0] * (W - 2) + [TOP_MAX])
    put(scalar_with(vals, True), [1] + [0] * (W - 2) + [-TOP_MAX])
    # 0, 1, r - 1, (r -+ 1) / 2: the last two are +HALF and -(HALF), the largest magnitudes
    put(0, [0] * W)
    put(1, [1] + [0] * (W - 1))
    put(R - 1, [-1] + [0] * (W - 1))
    sc += [HALF, HALF + 1]                         # (their digits are held to sum_j d_j 2^(16 j) = +-HALF by the host test)
    assert HALF + 1 == (R + 1) // 2
    while len(sc) < 300:
        sc.append(rng.randrange(R))
    idx = [rng.randrange(pl.finite) for _ in sc]
    return Case("digit_edges", idx, sc, dict(digits=dg))


def weight_buckets(window):
    """buckets 0, 1, 15, 16, 17, 16 2^k - 1 and 16 2^k for k = 0..10, and 2^15 - 1: every single-bit chunk number and chunk 2047;
    in the top window only those a folded scalar can reach (digit <= TOP_MAX)"""
    bs = {0, 1, 15, 16, 17, B - 1}
    for k in range(11):
        bs |= {16 * (1 << k) - 1, 16 * (1 << k)}
    if window == W - 1:
        bs = {b for b in bs if b + 1 <= TOP_MAX}
    return sorted(bs)


def case_bucket_weights(pl, window, seed=2):
    """One point in each bucket of weight_buckets(window); digit b + 1, and -2^15 for bucket 2^15 - 1 (the only digit that reaches it)"""
    rng = random.Random(seed + window)
    bs = weight_buckets(window)
    sc = [scalar_from_digits({window: -(b + 1) if b + 1 == B else b + 1}) for b in bs]
    idx = [rng.randrange(pl.finite) for _ in bs]
    claim = dict(only_windows=[window], bucket_set={window: bs}, buckets={(window, b): dict(count=1) for b in bs})
    return Case("bucket_weights_w%d" % window, idx, sc, claim)


def case_chunk_pair(pl, window, k, opposite, b=5):
    """The same base in buckets b and b + 16 2^k (chunks 0 and 2^k, the same place inside the chunk), nothing else: the two chunk
    sums are equal -- or opposite, and the window sums to infinity -- where the trees of k_pip_bits meet them."""
    b2 = b + 16 * (1 << k)
    sc = [scalar_from_digits({window: b + 1}), scalar_from_digits({window: -(b2 + 1) if opposite else b2 + 1})]
    idx = [pl.P_IDX + 1, pl.P_IDX + 1]
    claim = dict(only_windows=[window], bucket_set={window: [b, b2]}, chunks={(window, 0, 1 << k): -1 if opposite else 1})
    return Case("chunk_pair_w%d_k%d_%s" % (window, k, "opposite" if opposite else "equal"), idx, sc, claim)


def case_bucket_cancels(pl, window=7, b=40):
    """one base twice in one bucket with opposite signs (the bucket is infinity), next to an occupied bucket"""
    sc = [scalar_from_digits({window: b + 1}), scalar_from_digits({window: -(b + 1)}), scalar_from_digits({window: b + 2})]
    idx = [3, 3, 4]
    claim = dict(only_windows=[window], bucket_set={window: [b, b + 1]}, bucket_logs={(window, b): 0})
    return Case("bucket_cancels", idx, sc, claim)


def case_horner_equal(pl):
    """P with 2^16 and Q = 2^16 P with 1: window sums P (window 1) and 2^16 P (window 0); the accumulator equals the next sum"""
    k = pl.logs[pl.P_IDX]
    return Case("horner_equal", [pl.P_IDX, pl.Q_IDX], [1 << 16, 1],
                dict(only_windows=[0, 1], window_logs={1: k, 0: k << 16}, horner_equal=0))


def case_horner_cancel(pl, seed=3):
    """P with 2^48 and Q = 2^16 P with r - 2^32: window sums P (window 3) and -2^16 P (window 2) cancel to infinity, and the run
    goes on through windows 1 and 0, which eight small scalars fill"""
    rng = random.Random(seed)
    k = pl.logs[pl.P_IDX]
    sc = [1 << 48, R - (1 << 32)] + [rng.randrange(1, 1 << 30) for _ in range(8)]       # (window 1 below 2^14: no carry into 2)
    idx = [pl.P_IDX, pl.Q_IDX] + [rng.randrange(1, pl.finite - 4) for _ in range(8)]
    return Case("horner_cancel", idx, sc, dict(only_windows=[0, 1, 2, 3], window_logs={3: k, 2: -(k << 16)}, horner_zero=2))


def case_all_zero(pl, seed=4):
    rng = random.Random(seed)
    return Case("all_zero", [rng.randrange(pl.finite) for _ in range(300)], [0] * 300, dict(only_windows=[], zero_result=True))


def case_top_window_only(pl, seed=5):
    """a single non-zero window, the top one: digits 1, 2, TOP_MAX and some between, both signs"""
    rng = random.Random(seed)
    ds = [1, 2, TOP_MAX, -1, -TOP_MAX] + [rng.randrange(1, TOP_MAX) for _ in range(7)]
    sc = [scalar_from_digits({W - 1: d}) for d in ds]
    idx = [rng.randrange(pl.finite) for _ in ds]
    return Case("top_window_only", idx, sc, dict(only_windows=[W - 1], bucket_set={W - 1: sorted({abs(d) - 1 for d in ds})}))


SEGMENT_COUNTS = (255, 256, 257, 512, 3073, 3329, 16385, 16641)
SEGMENT_FILLINGS = ("random", "same", "half")


def case_segments(pl, c, window, filling, seed=6):
    """A bucket of c entries at digit 1 of `window` (offset 0 of the window's list), a bucket of 300 at digit 2 behind it, and 200
    random scalars around them.  Fillings: random bases; one base throughout (the partial of every full segment is 256 P, the
    fix-up adds equal points); one base, half with +d and half with -d, so the bucket sums to infinity (an odd c takes one entry
    of 2 P to get there) -- the order inside the bucket is the device's, so this filling claims the sum and nothing about partials."""
    rng = random.Random(seed * 1000003 + c * 31 + window)
    d1, d2 = scalar_from_digits({window: 1}), scalar_from_digits({window: 2})
    n1 = R - d1
    if filling == "random":
        body = [(rng.randrange(pl.finite), d1) for _ in range(c)] + [(rng.randrange(pl.finite), d2) for _ in range(300)]
    elif filling == "same":
        body = [(pl.P_IDX, d1)] * c + [(pl.P_IDX, d2)] * 300
    else:
        pos = c // 2
        body = [(pl.P_IDX, d1)] * pos
        body += [(pl.P_IDX, n1)] * (c - pos) if c % 2 == 0 else [(pl.P_IDX, n1)] * (c - pos - 2) + [(pl.P_IDX, d1), (pl.TWO_IDX, n1)]
        body += [(pl.P_IDX, d2)] * 150 + [(pl.P_IDX, R - d2)] * 150
    assert len(body) == c + 300
    # random scalars whose digit in `window` is neither +-1 nor +-2 (they sort behind the two buckets)
    rest = []
    while len(rest) < 200:
        s = rng.randrange(R)
        if abs(digits(s)[window]) not in (1, 2):
            rest.append((rng.randrange(pl.finite), s))
    allp = body + rest
    rng.shuffle(allp)
    idx, sc = [p[0] for p in allp], [p[1] for p in allp]
    s1 = (c - 1) // SEG
    path = "direct" if s1 == 0 else "sequential" if s1 <= FIX_SEQ else "heavy"
    e2 = (c + 299) // SEG
    claim = dict(buckets={(window, 0): dict(count=c, offset=0, s0=0, s1=s1, path=path, ends_on_boundary=c % SEG == 0),
                          (window, 1): dict(count=300, offset=c, s0=c // SEG, s1=e2, path="sequential")})
    if filling == "same" and c >= 2 * SEG:
        claim["uniform"] = {(window, 0): pl.logs[pl.P_IDX]}
    if filling == "half":
        claim["bucket_logs"] = {(window, 0): 0, (window, 1): 0}
    return Case("segments_c%d_w%d_%s" % (c, window, filling), idx, sc, claim)


def case_infinity_bases(pl, n=1000, seed=7):
    """infinity at index 0, at n - 1 and at ~10 % of the places between, under random scalars and a crowded bucket"""
    rng = random.Random(seed)
    idx = [pl.INF_IDX if rng.randrange(10) == 0 else rng.randrange(pl.finite) for _ in range(n)]
    idx[0] = idx[n - 1] = pl.INF_IDX
    sc = [rng.randrange(1, R) for _ in range(n)]
    for i in range(100, 100 + 2 * SEG + 40):                         # infinity inside a bucket that spans segments, too
        sc[i] = 9
    idx[100], idx[300] = pl.INF_IDX, pl.INF_IDX
    return Case("infinity_bases", idx, sc, dict(inf=[0, 100, 300, n - 1], buckets={(0, 8): dict(path="sequential")}))


def case_all_infinity(pl, n=300, seed=8):
    rng = random.Random(seed)
    return Case("all_infinity", [pl.INF_IDX] * n, [rng.randrange(1, R) for _ in range(n)], dict(all_inf=True, zero_result=True))


SORT_SIZES = (8191, 8192, 8193, 16383, 16384, 16385, 32769)


def case_sort_pieces(pl, n, seed=9):
    """n random scalars with all 16 digits non-zero (so every window's list has exactly n entries), random bases: n around the
    sizes of one level-2 piece (8192), one level-1 piece (16384) and of two of them"""
    rng = random.Random(seed * 65537 + n)
    sc = []
    while len(sc) < n:
        s = rng.randrange(R)
        if all(digits(s)):
            sc.append(s)
    idx = [rng.randrange(pl.finite) for _ in range(n)]
    return Case("sort_pieces_n%d" % n, idx, sc, dict(pieces=((n + PART1 - 1) // PART1, (n + PART2 - 1) // PART2)))


def all_cases(group):
    """every crafted case of tests/test_gpu_pippenger_edges.py for the group, as (builder, args) so that they are built lazily"""
    pl = pool(group)
    out = [(case_digit_edges, (pl,)), (case_horner_equal, (pl,)), (case_horner_cancel, (pl,)), (case_infinity_bases, (pl,)),
           (case_all_infinity, (pl,))]
    if group == "g1":
        out += [(case_bucket_weights, (pl, w)) for w in (0, 7, 15)]
        out += [(case_chunk_pair, (pl, 7, k, opp)) for k in range(11) for opp in (False, True)]
        out += [(case_bucket_cancels, (pl,)), (case_all_zero, (pl,)), (case_top_window_only, (pl,))]
        out += [(case_segments, (pl, c, w, f)) for c in SEGMENT_COUNTS for w in (0, W - 1) for f in SEGMENT_FILLINGS]
        out += [(case_sort_pieces, (pl, n)) for n in SORT_SIZES]
    else:
        out += [(case_segments, (pl, c, w, f)) for c in (257, 3073, 3329) for w in (0, W - 1) for f in ("same", "half")]
    return out
