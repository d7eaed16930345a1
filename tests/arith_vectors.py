"""Raw-word vectors for the arithmetic headers (csrc/bn254.hpp, csrc/f29.hpp, csrc/gnark_hints.hpp) and the predicate every result
must satisfy.

Plain Python: the references are Python integers only (oracle.bn254 supplies the curve sums of the accumulator scripts).  The
operands are the WORDS the header functions see -- nothing is converted on the way in or out -- so the limb patterns that break a
carry chain, a shift count or a limb selection can be chosen: a fixed edge list per operation plus N_RANDOM seeded random cases.
Every generated case is run and asserted; the generator asserts the preconditions the headers state (operand < 2p, limb bounds,
column sums < 2^64) before anything is sent, so a bad vector fails as a vector and not as a wrong result.

The groups of gnark_hints.hpp (bigs, hint_glv, hint_emul, hint_gk) also name the BRANCH each case takes -- search radius and ring
position of the scalar decomposition, sign of its quotients, sign of a carry, the ladder's equal-point cases -- and verify_group
returns the cases per class, so a test can demand that no class is empty.

Two runners consume the same batches: tests/test_gpu_arith.py (spp_debug_arith, the gfx950 compile) and tests/test_arith_raw_host.py
(tests/host/arith_raw_check.cpp, the g++ compile of the same dispatch header).
"""
import functools
import math
import random

from oracle import bn254 as B
from oracle import hashes as H
from spp import ccs

FR, FQ = "fr", "fq"
MOD = {FR: B.R, FQ: B.P}
FIELD_BITS = {FR: 0x000, FQ: 0x100}          # SPP_ARITH_FR / SPP_ARITH_FQ (include/spp.h)
R256 = 1 << 256                              # Montgomery radix of Fp
R261 = 1 << 261                              # Montgomery radix of F29
M29 = (1 << 29) - 1
N_RANDOM = 2000                              # random cases per operation: the count tests/host/f29_check.cpp uses

# name -> (code, in_words, out_words, fields): the X-macro list of csrc/arith_probe.hpp (test_arith_raw_host.py compares the two);
# fields 0 = Fr and Fq, 1 = Fq only, 2 = Fr only
OPS = {
    "FP_MUL": (1, 16, 8, 0), "FP_SQR": (2, 8, 8, 0), "FP_ADD": (3, 16, 8, 0), "FP_SUB": (4, 16, 8, 0), "FP_NEG": (5, 8, 8, 0),
    "FP_DBL": (6, 8, 8, 0), "FP_MUL_SMALL": (7, 8, 8, 0), "FP_INV": (8, 8, 8, 0), "FP_INV_FERMAT": (9, 8, 8, 0),
    "FP_TO_CANONICAL": (10, 8, 8, 0), "FP_FROM_U256": (11, 8, 8, 0), "FP_IS_ZERO": (12, 8, 1, 0), "FP_EQ": (13, 16, 1, 0),
    "FQ2_MUL": (16, 32, 16, 1), "FQ2_SQR": (17, 16, 16, 1), "FQ2_INV": (18, 16, 16, 1),
    "F29_FROM_WORDS": (32, 8, 9, 0), "F29_TO_WORDS": (33, 9, 8, 0), "F29_NORM": (34, 9, 9, 0), "F29_MUL": (35, 18, 9, 0),
    "F29_SQR": (36, 9, 9, 0), "F29_MUL2": (37, 36, 9, 0), "F29_SUB_NORM_6P_1": (38, 18, 9, 0), "F29_SUB_NORM_2P_1": (39, 18, 9, 0),
    "F29_SUB3_NORM_4P_3": (40, 27, 9, 0), "F29_SUB_LAZY_6P_1": (41, 18, 9, 0), "F29_NEG_LAZY_2P_1": (42, 9, 9, 0),
    "F29_NEG_LAZY_4P_1": (43, 9, 9, 0), "F29_ADD_NORM": (44, 18, 9, 0), "F29_ADD_LAZY": (45, 18, 9, 0),
    "F29_IS_ZERO_MOD_P_7": (46, 9, 1, 0), "F29_IS_ZERO_MOD_P_3": (47, 9, 1, 0), "F29_FROM_FP": (48, 8, 9, 0),
    "F29_TO_FP": (49, 9, 8, 0), "F29_SCALED_TO_FP": (50, 9, 8, 0),
    "F29X2_MUL": (64, 36, 18, 1), "F29X2_SQR": (65, 18, 18, 1),
    "SCRIPT_G1_29": (96, 145, 54, 1), "SCRIPT_G1_29_DISTINCT": (97, 145, 54, 1), "SCRIPT_G1": (98, 145, 54, 1),
    "SCRIPT_G2_29": (99, 273, 106, 1), "SCRIPT_G2_29_DISTINCT": (100, 273, 106, 1), "SCRIPT_G2": (101, 273, 106, 1),
    "HINT_GLV_SPLIT": (128, 32, 9, 2), "HINT_EMUL_REDUCE": (129, 64, 136, 2), "HINT_GRUMPKIN_MUL": (130, 16, 17, 2),
    "BIGS_ADD": (136, 24, 12, 2), "BIGS_SUB": (137, 24, 12, 2), "BIGS_NEGATE": (138, 12, 12, 2), "BIGS_LT": (139, 24, 1, 2),
    "BIGS_SAR64": (140, 12, 12, 2), "BIGS_LOW64_ZERO": (141, 12, 1, 2), "BIGS_ADD_SMALL_MUL": (142, 24, 12, 2),
    "BIG_MUL_ACC_4X4_12": (144, 20, 12, 2), "BIG_MUL_ACC_2X2_12": (145, 16, 12, 2), "BIG_MUL_ACC_8X8_8": (146, 24, 8, 2),
}


# ---------------------------------------------------------------------------------------------------------------- words and limbs
def words8(v):
    assert 0 <= v < R256
    return [(v >> (32 * i)) & 0xffffffff for i in range(8)]


def from_words8(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


def limbs9(v):
    """the normalised 9 x 29-bit limbs of v (limb 8 takes what is left)"""
    assert 0 <= v < 1 << (232 + 32)
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def val9(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


def lifted(p, k, m):
    """limbs of k*p with every low limb >= m * (2^29 - 1): the SUBC_kP_m constants (csrc/gen_consts.py states the rule)"""
    lowmin = m * M29
    c = limbs9(k * p)
    for i in range(8):
        while c[i] < lowmin:
            c[i] += 1 << 29
            c[i + 1] -= 1
    assert c[8] > 0 and val9(c) == k * p and all(x < 1 << 32 for x in c)
    return c


class Batch:
    """n cases of one operation: rows of operand words, and check(i, row, out) -> None or a message; classes(row, out) -> the
    names of the branch classes a case belongs to (the groups of gnark_hints.hpp)"""

    def __init__(self, group, field, op, rows, check, arg=0, classes=None):
        code, iw, ow, fields = OPS[op]
        assert fields == 0 or field == (FQ if fields == 1 else FR)
        self.group, self.field, self.op, self.arg, self.check, self.classes = group, field, op, arg, check, classes
        self.selector, self.in_words, self.out_words = FIELD_BITS[field] | code, iw, ow
        rows = [list(r) for r in rows]
        if len(rows) % 64 == 0:                       # the probe runs blocks of 64 lanes: keep a ragged last block
            rows.append(list(rows[0]))
        assert rows and all(len(r) == iw and all(0 <= x < 1 << 32 for x in r) for r in rows), op
        self.rows = rows

    def name(self):
        return "%s %s%s" % (self.field, self.op, "(arg=%d)" % self.arg if self.arg else "")

    def verify(self, out_rows):
        """asserts every case; the message names the operation, the case and the operand words"""
        assert len(out_rows) == len(self.rows), (self.name(), len(out_rows), len(self.rows))
        for i, (row, out) in enumerate(zip(self.rows, out_rows)):
            out = [int(x) for x in out]
            assert len(out) == self.out_words
            msg = self.check(i, row, out)
            assert msg is None, "%s case %d: %s\n  operands: %s\n  result:   %s" % (
                self.name(), i, msg, " ".join("%08x" % x for x in row), " ".join("%08x" % x for x in out))
        return len(self.rows)


# ---------------------------------------------------------------------------------------------------------------- Fp operands
def top2p(p):
    return ((2 * p) >> 232) - 1


def maxlimb_word(p):
    """all eight low 29-bit limbs all ones under the largest top limb that keeps the word < 2p (maxlimb_words(top2p), f29_check.cpp)"""
    return val9([M29] * 8 + [top2p(p)])


def fp_edge_words(p):
    rng = random.Random(0xF9 ^ (p & 0xffff))
    e = [0, 1, 2, p - 1, p, p + 1, 2 * p - 2, 2 * p - 1]
    k = 0
    while 1 << k < 2 * p:
        e.append(1 << k)
        k += 1
    for step in (29, 32):
        j = 1
        while (1 << (step * j)) - 1 < 2 * p:
            e.append((1 << (step * j)) - 1)
            j += 1
    e += [0xffffffff << (32 * i) for i in range(8) if 0xffffffff << (32 * i) < 2 * p]
    e.append(maxlimb_word(p))
    topmax = (2 * p - 1) >> 232
    for top in (0, 1, topmax):                       # top 29-bit limb 0, 1 and its maximum, under random low limbs
        bound = (2 * p - (top << 232)) if top == topmax else 1 << 232
        e.append((top << 232) + rng.randrange(min(bound, 1 << 232)))
    e += [R256 % p, R256 * R256 % p]
    assert all(0 <= v < 2 * p for v in e)
    return e


def fp_core_words(p):
    """the edges that are not a lone power of two: crossed with each other in full for the binary operations"""
    e = [0, 1, 2, p - 1, p, p + 1, 2 * p - 2, 2 * p - 1, maxlimb_word(p), R256 % p, R256 * R256 % p, (1 << 254), (1 << 232) - 1,
         (1 << 253) - 1, (1 << 224) - 1, 0xffffffff, 0xffffffff << 96, (1 << 29) - 1, 1 << 29, ((2 * p - 1) >> 232) << 232]
    assert all(0 <= v < 2 * p for v in e)
    return e


def fp_random_words(p, seed, n=N_RANDOM):
    rng = random.Random(seed)
    return [rng.randrange(2 * p) for _ in range(n)]


def fp_pairs(p, seed):
    e, c = fp_edge_words(p), fp_core_words(p)
    pairs = [(a, a) for a in e] + [(e[i], e[(i + 7) % len(e)]) for i in range(len(e))]
    pairs += [(a, b) for a in c for b in c]
    pairs += [(a, b) for a in e for b in (1, p - 1, 2 * p - 1, maxlimb_word(p))]
    rng = random.Random(seed)
    pairs += [(rng.randrange(2 * p), rng.randrange(2 * p)) for _ in range(N_RANDOM)]
    return pairs


def _cong(out, want, p, bound=None, what="value"):
    if (out - want) % p:
        return "%s %x is not congruent to %x" % (what, out, want % p)
    if bound is not None and not out < bound:
        return "%s %x is not below %x" % (what, out, bound)
    return None


# ---------------------------------------------------------------------------------------------------------------- Fp group
def fp_batches(field):
    p = MOD[field]
    rinv = pow(R256, -1, p)
    singles = fp_edge_words(p) + fp_random_words(p, 11)
    pairs = fp_pairs(p, 12)
    srows = [words8(a) for a in singles]
    prows = [words8(a) + words8(b) for a, b in pairs]
    out = []

    def bin_op(op, f):
        def chk(i, row, o):
            a, b = from_words8(row[:8]), from_words8(row[8:])
            return _cong(from_words8(o), f(a, b), p, 2 * p)
        out.append(Batch("fp", field, op, prows, chk))

    def un_op(op, f, rows=srows, arg=0, exact_zero=False):
        def chk(i, row, o):
            a, r = from_words8(row), from_words8(o)
            if exact_zero and a in (0, p) and r != 0:
                return "result of the word %s must be exactly 0" % ("0" if a == 0 else "p")
            return _cong(r, f(a), p, 2 * p)
        out.append(Batch("fp", field, op, rows, chk, arg))

    bin_op("FP_MUL", lambda a, b: a * b * rinv)
    bin_op("FP_ADD", lambda a, b: a + b)
    bin_op("FP_SUB", lambda a, b: a - b)
    un_op("FP_SQR", lambda a: a * a * rinv)
    un_op("FP_NEG", lambda a: -a, exact_zero=True)
    un_op("FP_DBL", lambda a: 2 * a)
    for k in (0, 1, 2, 3, 0x8000, 0xffff):
        un_op("FP_MUL_SMALL", lambda a, k=k: k * a, rows=srows if k in (3, 0xffff) else srows[:len(fp_edge_words(p)) + 100], arg=k)

    def chk_canon(i, row, o):
        want = from_words8(row) * rinv % p
        return None if from_words8(o) == want else "expected exactly %x" % want
    out.append(Batch("fp", field, "FP_TO_CANONICAL", srows, chk_canon))

    rng = random.Random(13)                            # from_u256 takes any 256-bit word
    u256 = fp_edge_words(p) + [R256 - 1, R256 - 2, 5 * p, 5 * p - 1, 5 * p + 1, 3 * p, 4 * p - 1, 0xffffffff << 224, 1 << 255]
    u256 += [k * p + d for k in range(2, 6) for d in (-1, 0, 1)] + [rng.randrange(R256) for _ in range(N_RANDOM)]
    assert all(0 <= v < R256 for v in u256)
    out.append(Batch("fp", field, "FP_FROM_U256", [words8(v) for v in u256],
                     lambda i, row, o: _cong(from_words8(o), from_words8(row) * R256, p, 2 * p)))

    def chk_is_zero(i, row, o):
        want = 1 if from_words8(row) in (0, p) else 0
        return None if o[0] == want else "expected %d" % want
    out.append(Batch("fp", field, "FP_IS_ZERO", srows + [words8(p ^ (1 << k)) for k in range(0, 254, 7)], chk_is_zero))

    eq_pairs = pairs + [(a, a + p) for a in singles if a < p] + [(a + p, a) for a in singles[:400] if a < p]
    eq_pairs += [(a, a ^ (1 << k)) for a in (0, p, p - 1, maxlimb_word(p)) for k in range(0, 253, 5) if a ^ (1 << k) < 2 * p]

    def chk_eq(i, row, o):
        want = 1 if (from_words8(row[:8]) - from_words8(row[8:])) % p == 0 else 0
        return None if o[0] == want else "expected %d" % want
    out.append(Batch("fp", field, "FP_EQ", [words8(a) + words8(b) for a, b in eq_pairs], chk_eq))
    return out


# ---------------------------------------------------------------------------------------------------------------- inv group
def inv_words(p):
    e = fp_edge_words(p)
    e += [p - (1 << k) for k in range(1, 253)]          # the first difference u - v is a pure power of two
    e += [p + (1 << k) for k in range(0, 254)]          # the non-canonical twin
    for k in (32, 33, 47, 63, 64, 65, 95, 96, 128, 160, 192, 224, 250):   # 2^k * odd: low words zero, small and large odd parts
        big = (((2 * p - 1) >> k) - 1) | 1
        for odd in (3, 5, 0xffffffff, (1 << 61) - 1, big, big - 2, ((p >> k) - 1) | 1):
            if odd > 0 and (odd << k) < 2 * p:
                e.append(odd << k)
    e += fp_random_words(p, 21)
    assert all(0 <= v < 2 * p for v in e)
    return e


def inv_enters_zero_low_word_branch(word, p):
    """Provably true for words whose first strip() meets a zero low word: the canonical word is a non-zero multiple of 2^32 (the
    strip of v before the loop), or it is p - 2^k with k >= 32 (v is odd, the first difference u - v = 2^k is stripped)."""
    c = word - p if word >= p else word
    if c != 0 and c & 0xffffffff == 0:
        return True
    d = p - c
    return c & 1 == 1 and d > 0 and d & (d - 1) == 0 and d >= 1 << 32


def inv_batches(field):
    p = MOD[field]
    ws = inv_words(p)
    rows = [words8(a) for a in ws]
    assert sum(inv_enters_zero_low_word_branch(a, p) for a in ws) >= 200

    def chk(i, row, o):
        a, r = from_words8(row), from_words8(o)
        if a % p == 0:
            return None if r == 0 else "inv of the word %s must be exactly 0" % ("0" if a == 0 else "p")
        return _cong(r, R256 * R256 * pow(a, -1, p), p, 2 * p)

    def chk_fermat(i, row, o):
        a, r = from_words8(row), from_words8(o)
        return _cong(r, 0 if a % p == 0 else R256 * R256 * pow(a, -1, p), p, 2 * p)
    return [Batch("inv", field, "FP_INV", rows, chk), Batch("inv", field, "FP_INV_FERMAT", rows, chk_fermat)]


def check_inv_agreement(batches, outs):
    """inv and inv_fermat agree after reduction, case by case"""
    by_op = {b.op: (b, o) for b, o in zip(batches, outs)}
    (bi, oi), (bf, of) = by_op["FP_INV"], by_op["FP_INV_FERMAT"]
    assert bi.rows == bf.rows
    p = MOD[bi.field]
    for i, (x, y) in enumerate(zip(oi, of)):
        assert from_words8(x) % p == from_words8(y) % p, "%s inv and inv_fermat differ on case %d: %s" % (
            bi.field, i, " ".join("%08x" % w for w in bi.rows[i]))


# ---------------------------------------------------------------------------------------------------------------- Fq2 group
def fq2_batches():
    p = MOD[FQ]
    rinv = pow(R256, -1, p)
    rng = random.Random(31)
    core = fp_core_words(p)
    el = [(a, b) for a in core[:11] for b in core[:11]] + [(rng.randrange(2 * p), rng.randrange(2 * p)) for _ in range(N_RANDOM)]
    prs = [(el[i], el[(i * 7 + 3) % 121]) for i in range(121)] + [(el[i], el[i]) for i in range(121)]
    prs += [(el[121 + i], el[121 + (i + 1) % N_RANDOM]) for i in range(N_RANDOM)]
    w2 = lambda a: words8(a[0]) + words8(a[1])
    r2 = lambda o: (from_words8(o[:8]), from_words8(o[8:]))

    def both(o, want):
        got = r2(o)
        return _cong(got[0], want[0], p, 2 * p, "c0") or _cong(got[1], want[1], p, 2 * p, "c1")

    def chk_mul(i, row, o):
        a, b = r2(row[:16]), r2(row[16:])
        return both(o, ((a[0] * b[0] - a[1] * b[1]) * rinv, (a[0] * b[1] + a[1] * b[0]) * rinv))

    def chk_sqr(i, row, o):
        a = r2(row)
        return both(o, ((a[0] * a[0] - a[1] * a[1]) * rinv, 2 * a[0] * a[1] * rinv))

    def chk_inv(i, row, o):
        a = r2(row)
        n = (a[0] * a[0] + a[1] * a[1]) % p
        if n == 0:
            assert a[0] % p == 0 and a[1] % p == 0     # -1 is no square in Fq
            return both(o, (0, 0))
        d = R256 * R256 * pow(n, -1, p)
        return both(o, (a[0] * d, -a[1] * d))
    return [Batch("fq2", FQ, "FQ2_MUL", [w2(a) + w2(b) for a, b in prs], chk_mul),
            Batch("fq2", FQ, "FQ2_SQR", [w2(a) for a in el], chk_sqr),
            Batch("fq2", FQ, "FQ2_INV", [w2(a) for a in el], chk_inv)]


# ---------------------------------------------------------------------------------------------------------------- F29 operands
def ext9(p, mult, topk):
    """limbs at exactly the bound a call site of madd_any states: mult x (2^29 - 1) in the low limbs (1x, 2x = 2^30 - 2, 3x), the
    top limb that of topk * p (the value bound)"""
    return [mult * M29] * 8 + [(topk * p) >> 232]


def rand9(rng, p, mult=1, topk=8):
    return [rng.randrange(mult * M29 + 1) for _ in range(8)] + [rng.randrange(((topk * p) >> 232) + 1)]


def one_limb_set(p):
    z = [0] * 9
    out = [z]
    for k in range(9):
        for v in ((1, M29) if k < 8 else (1, (8 * p) >> 232)):
            l = list(z)
            l[k] = v
            out.append(l)
    return out


def _assert_columns(prods, p):
    """the preconditions of reduce(): every 64-bit column of the products plus the reduction's own additions stays below 2^64,
    and the top limb of the result fits its word"""
    col = [0] * 18
    for a, b in prods:
        assert all(x < 1 << 32 for x in a + b)
        for i in range(9):
            for j in range(9):
                col[i + j] += a[i] * b[j]
    assert all(c + 9 * (1 << 58) + (1 << 40) < 1 << 64 for c in col), "column sum"
    total = sum(val9(a) * val9(b) for a, b in prods)
    assert total // R261 + p + 1 < 1 << (232 + 32)
    return total


def _chk_reduced(l, total, p, what="value"):
    """the contract of F29::reduce on column sums `total`: congruent to total / R', limbs 0..7 normalised, < total / R' + p"""
    if any(x > M29 for x in l[:8]):
        return "%s: a low limb is not below 2^29" % what
    return _cong(val9(l), total * pow(R261, -1, p), p, total // R261 + p + 1, what)


def f29_mul_operands(p, seed):
    rng = random.Random(seed)
    e1, e2, e3 = ext9(p, 1, 8), ext9(p, 2, 4), ext9(p, 3, 8)
    pairs = [(e1, e1), (e2, ext9(p, 1, 2)), (e2, e1), (e1, e3), (e3, e1), (ext9(p, 1, 2), e2)]     # 1x1, 2x1, 1x3
    ols = one_limb_set(p)
    pairs += [(a, b) for a in ols for b in (e1, ols[1], ols[-1], ols[2])] + [(a, a) for a in ols]
    pairs += [(limbs9(a), limbs9(b)) for a in (0, 1, p - 1, p, p + 1, 8 * p - 1, maxlimb_word(p)) for b in (1, p, 8 * p - 1, maxlimb_word(p))]
    for m1, m2, t1, t2 in ((1, 1, 8, 8), (2, 1, 4, 2), (1, 3, 8, 8)):
        pairs += [(rand9(rng, p, m1, t1), rand9(rng, p, m2, t2)) for _ in range(N_RANDOM // 2)]
    return pairs


def f29_batches(field):
    p = MOD[field]
    rng = random.Random(41)
    out = []
    r9 = lambda row, k: row[9 * k:9 * k + 9]

    # ---- products -------------------------------------------------------------------------------------------------------
    pairs = f29_mul_operands(p, 42)
    for a, b in pairs:
        _assert_columns([(a, b)], p)
    out.append(Batch("f29", field, "F29_MUL", [a + b for a, b in pairs],
                     lambda i, row, o: _chk_reduced(o, val9(r9(row, 0)) * val9(r9(row, 1)), p)))
    sq = [ext9(p, 1, 8), ext9(p, 2, 4)] + one_limb_set(p) + [limbs9(v) for v in (1, p - 1, p, p + 1, 8 * p - 1, maxlimb_word(p))]
    sq += [rand9(rng, p, m, 8) for m in (1, 1, 1, 2) for _ in range(N_RANDOM // 4)]       # the code squares 1x operands (Pp, Rr)
    for a in sq:
        assert all(x < 1 << 31 for x in a)              # mac_sqr doubles limbs in 32 bits
        _assert_columns([(a, a)], p)
    out.append(Batch("f29", field, "F29_SQR", sq, lambda i, row, o: _chk_reduced(o, val9(row) ** 2, p)))
    e1, e2, e3 = ext9(p, 1, 8), ext9(p, 2, 2), ext9(p, 3, 8)
    quads = [(e1, e3, e2, ext9(p, 1, 2)), (e1, e3, e2, e1), (e3, e1, e1, e2), (e1, e1, e1, e1)]     # mul2 as 1x3 + 2x1 (Y3 of madd_any)
    ols = one_limb_set(p)
    quads += [(a, e3, b, e1) for a in ols[:4] + ols[-2:] for b in ols[:4] + ols[-2:]]
    quads += [(rand9(rng, p, 1, 4), rand9(rng, p, 3, 8), rand9(rng, p, 2, 2), rand9(rng, p, 1, 2)) for _ in range(N_RANDOM)]
    for a, b, c, d in quads:
        _assert_columns([(a, b), (c, d)], p)            # the products-sum per column < 2^64
    out.append(Batch("f29", field, "F29_MUL2", [a + b + c + d for a, b, c, d in quads],
                     lambda i, row, o: _chk_reduced(o, val9(r9(row, 0)) * val9(r9(row, 1)) + val9(r9(row, 2)) * val9(r9(row, 3)), p)))

    # ---- additive forms: exact integers -----------------------------------------------------------------------------------
    def exact(o, want, normalised):
        if normalised and any(x > M29 for x in o[:8]):
            return "a low limb is not below 2^29"
        return None if val9(o) == want else "value %x, expected exactly %x" % (val9(o), want)

    def sub_ops(op, k, m, nsub, normalised, a_mult=1, a_top=8):
        """a - b (- 2c) + k*p for subtrahends whose low limbs stay within m * (2^29 - 1) and whose top limbs C(8) + a8 covers"""
        C = lifted(p, k, m)
        rows = []

        def add(a, subs):
            w = [subs[0][i] + (2 * subs[1][i] if nsub == 2 else 0) for i in range(9)]
            assert all(w[i] <= m * M29 for i in range(8)) and all(a[i] + C[i] + 8 < 1 << 32 for i in range(9)), op
            assert a[8] + C[8] - w[8] >= 0, op
            rows.append(a + subs[0] + (subs[1] if nsub == 2 else []))
        lowmax = [M29] * 8
        tops = lambda a8: (C[8] + a8) if nsub == 1 else (C[8] + a8) // 3
        amax = ext9(p, a_mult, a_top)
        zero = [0] * 9
        for a in (zero, amax, limbs9(p), limbs9(1)):
            t = tops(a[8])
            cands = [zero, lowmax + [0], lowmax + [t], [0] * 8 + [t], limbs9(1), [M29] + [0] * 8, [0, M29] + [0] * 7]
            if m == 3 and nsub == 1:
                cands.append([3 * M29] * 8 + [t])
            for b in cands:
                add(a, (b, b) if nsub == 2 else (b,))
        for a in one_limb_set(p):
            add(a, ((lowmax + [0],) * 2) if nsub == 2 else (lowmax + [0],))
        for _ in range(N_RANDOM):
            a = rand9(rng, p, a_mult, a_top)
            t = tops(a[8])
            if nsub == 2:
                add(a, ([rng.randrange(M29 + 1) for _ in range(8)] + [rng.randrange(t + 1)],
                        [rng.randrange(M29 + 1) for _ in range(8)] + [rng.randrange(t + 1)]))
            else:
                add(a, ([rng.randrange(m * M29 + 1) for _ in range(8)] + [rng.randrange(t + 1)],))

        def chk(i, row, o):
            want = val9(r9(row, 0)) - val9(r9(row, 1)) - (2 * val9(r9(row, 2)) if nsub == 2 else 0) + k * p
            return exact(o, want, normalised)
        out.append(Batch("f29", field, op, rows, chk))

    sub_ops("F29_SUB_NORM_6P_1", 6, 1, 1, True)
    sub_ops("F29_SUB_NORM_2P_1", 2, 1, 1, True)
    sub_ops("F29_SUB3_NORM_4P_3", 4, 3, 2, True)
    sub_ops("F29_SUB_LAZY_6P_1", 6, 1, 1, False)

    def neg_op(op, k):
        C = lifted(p, k, 1)
        rows = [[0] * 9, [M29] * 8 + [C[8]], [M29] * 8 + [0], [0] * 8 + [C[8]], limbs9(1), limbs9(p), limbs9(p + 1), list(C)]
        rows += one_limb_set(p)[:17] + [[rng.randrange(M29 + 1) for _ in range(8)] + [rng.randrange(C[8] + 1)] for _ in range(N_RANDOM)]
        assert all(b[i] <= C[i] for b in rows for i in range(9))
        out.append(Batch("f29", field, op, rows, lambda i, row, o: exact(o, k * p - val9(row), False)))
    neg_op("F29_NEG_LAZY_2P_1", 2)
    neg_op("F29_NEG_LAZY_4P_1", 4)

    adds = [(ext9(p, 1, 8), ext9(p, 1, 8)), (ext9(p, 3, 8), ext9(p, 3, 8)), ([0] * 9, [0] * 9), (limbs9(1), [M29] * 8 + [0]),
            ([M29] * 8 + [0], limbs9(1)), (ext9(p, 2, 4), ext9(p, 1, 8))]
    adds += [(a, ext9(p, 1, 8)) for a in one_limb_set(p)]
    adds += [(rand9(rng, p, m, 8), rand9(rng, p, 1, 8)) for m in (1, 1, 2, 3) for _ in range(N_RANDOM // 4)]
    assert all(a[i] + b[i] + 8 < 1 << 32 for a, b in adds for i in range(9))
    out.append(Batch("f29", field, "F29_ADD_NORM", [a + b for a, b in adds],
                     lambda i, row, o: exact(o, val9(r9(row, 0)) + val9(r9(row, 1)), True)))
    out.append(Batch("f29", field, "F29_ADD_LAZY", [a + b for a, b in adds],
                     lambda i, row, o: exact(o, val9(r9(row, 0)) + val9(r9(row, 1)), False)))

    # ---- layout and domain changes ------------------------------------------------------------------------------------------
    words = fp_edge_words(p) + [R256 - 1, 0xffffffff << 224, 1 << 255, (1 << 232) - 1, 1 << 232] + fp_random_words(p, 43)
    words += [rng.randrange(R256) for _ in range(200)]

    def chk_from_words(i, row, o):
        want = limbs9(from_words8(row))
        return None if o == want else "expected limbs %s" % " ".join("%08x" % x for x in want)
    out.append(Batch("f29", field, "F29_FROM_WORDS", [words8(v) for v in words], chk_from_words))

    def chk_to_words(i, row, o):
        want = words8(val9(row))
        return None if o == want else "expected words %s" % " ".join("%08x" % x for x in want)
    out.append(Batch("f29", field, "F29_TO_WORDS", [limbs9(v) for v in words], chk_to_words))   # normalised limbs, value < 2^256

    top = (1 << 32) - 8                                  # a limb plus the carry from below (<= 7) must fit its word
    norms = [ext9(p, 1, 8), ext9(p, 2, 4), ext9(p, 3, 8), [top] * 8 + [0x7fffffff], [0] * 9, [M29 + 1] + [M29] * 7 + [0],
             [top] + [M29] * 7 + [5]] + one_limb_set(p)
    norms += [[1 << 29 if j == k else 0 for j in range(9)] for k in range(8)] + [[top if j == k else 0 for j in range(9)] for k in range(8)]
    norms += [[rng.randrange(top + 1) for _ in range(8)] + [rng.randrange(1 << 31)] for _ in range(N_RANDOM)]
    assert all(x <= top for r in norms for x in r)
    out.append(Batch("f29", field, "F29_NORM", norms, lambda i, row, o: exact(o, val9(row), True)))

    fpw = fp_edge_words(p) + fp_random_words(p, 44)
    k_in = R261 * R261 * pow(R256, -1, p) % p            # mont29(x*R, K29_IN) = x*R'
    out.append(Batch("f29", field, "F29_FROM_FP", [words8(v) for v in fpw],
                     lambda i, row, o: _chk_reduced(o, from_words8(row) * k_in, p)))            # == a * R'/R, below a*K/R' + p
    acc = [limbs9(v) for v in (0, 1, p - 1, p, p + 1, 2 * p, 8 * p - 1, maxlimb_word(p), val9(ext9(p, 1, 8)))] + one_limb_set(p)
    acc += [rand9(rng, p, 1, 8) for _ in range(N_RANDOM)]
    assert all(val9(a) < (1 << 232) * (((8 * p) >> 232) + 1) and all(x <= M29 for x in a[:8]) for a in acc)
    one = R256 % p

    def chk_to_fp(i, row, o, k=one):
        r = from_words8(o)
        total = val9(row) * k
        return _cong(r, total * pow(R261, -1, p), p, min(2 * p, total // R261 + p + 1))
    out.append(Batch("f29", field, "F29_TO_FP", acc, chk_to_fp))                                 # x*R' -> x*R
    out.append(Batch("f29", field, "F29_SCALED_TO_FP", acc, lambda i, row, o: chk_to_fp(i, row, o, 1 << 251)))   # zz*R'^2/R -> zz*R
    return out


# ---------------------------------------------------------------------------------------------------------------- is_zero_mod_p
def is_zero_batches(field):
    p = MOD[field]
    rng = random.Random(51)
    vals = []
    for k in range(9):
        for d in (0, 1, -1, 1 << 29, -(1 << 29), 1 << 232, -(1 << 232)):
            if k * p + d >= 0:
                vals.append(k * p + d)
    for k in range(9):                                   # the low limb of k*p under other limbs: passes the filter, fails the compare
        for _ in range(20):
            vals.append((rng.randrange((8 * p) >> 29) << 29) | ((k * p) & M29))
        for j in range(1, 9):
            vals.append((k * p) ^ (1 << (29 * j + rng.randrange(20))))
    vals += [rng.randrange(8 * p) for _ in range(N_RANDOM)]
    rows = [limbs9(v) for v in vals]
    out = []
    for kmax in (7, 3):
        def chk(i, row, o, kmax=kmax):
            v = val9(row)
            want = 1 if v % p == 0 and v // p <= kmax else 0
            return None if o[0] == want else "expected %d" % want
        out.append(Batch("is_zero_mod_p", field, "F29_IS_ZERO_MOD_P_%d" % kmax, rows, chk))
    return out


# ---------------------------------------------------------------------------------------------------------------- F29x2
def f29x2_batches():
    p = MOD[FQ]
    rng = random.Random(61)
    out = []
    r9 = lambda row, k: row[9 * k:9 * k + 9]
    for k in (2, 4, 6, 8):                               # CA = SUBC_kP_1 dominates a1: low limbs <= 2^29 - 1, top limb <= CA(8)
        C = lifted(p, k, 1)
        top = min(C[8], (8 * p) >> 232)
        a1max = [M29] * 8 + [top]
        n1 = lambda: [rng.randrange(M29 + 1) for _ in range(8)] + [rng.randrange(top + 1)]
        e1 = ext9(p, 1, 8)
        muls = [(e1, a1max, e1, e1), (e1, [0] * 9, e1, e1), ([0] * 9, a1max, [0] * 9, e1), ([0] * 9,) * 4, (limbs9(1), limbs9(1), limbs9(1), limbs9(1))]
        muls += [(rand9(rng, p), n1(), rand9(rng, p), rand9(rng, p)) for _ in range(N_RANDOM // 4)]
        for a0, a1, b0, b1 in muls:
            na1 = [C[i] - a1[i] for i in range(9)]
            assert all(x >= 0 for x in na1)
            _assert_columns([(a0, b0), (na1, b1)], p)
            _assert_columns([(a0, b1), (a1, b0)], p)

        def chk_mul(i, row, o, k=k):
            a0, a1, b0, b1 = (val9(r9(row, j)) for j in range(4))
            return (_chk_reduced(o[:9], a0 * b0 + (k * p - a1) * b1, p, "c0") or _chk_reduced(o[9:], a0 * b1 + a1 * b0, p, "c1"))
        out.append(Batch("f29x2", FQ, "F29X2_MUL", [a + b + c + d for a, b, c, d in muls], chk_mul, arg=k))
        sqs = [(e1, a1max), (e1, [0] * 9), ([0] * 9, a1max), ([0] * 9, [0] * 9), (limbs9(1), limbs9(1)), (limbs9(p), limbs9(p))]
        sqs += [(rand9(rng, p), n1()) for _ in range(N_RANDOM // 4)]
        for a0, a1 in sqs:
            s = [a0[i] + a1[i] for i in range(9)]
            d = [a0[i] + C[i] - a1[i] for i in range(9)]
            assert all(x >= 0 for x in d)
            _assert_columns([(s, d)], p)
            _assert_columns([([2 * x for x in a0], a1)], p)

        def chk_sqr(i, row, o, k=k):
            a0, a1 = val9(r9(row, 0)), val9(r9(row, 1))
            return _chk_reduced(o[:9], (a0 + a1) * (a0 - a1 + k * p), p, "c0") or _chk_reduced(o[9:], 2 * a0 * a1, p, "c1")
        out.append(Batch("f29x2", FQ, "F29X2_SQR", [a + b for a, b in sqs], chk_sqr, arg=k))
    return out


# ---------------------------------------------------------------------------------------------------------------- scripts
def _mont(x, noncanonical=False):
    w = x * R256 % B.P
    return w + B.P if noncanonical and w + B.P < 2 * B.P else w


def script_cases(g2):
    """(table of <= 8 affine points, steps [(index, negate)]) -- the same shapes for G1 and G2"""
    add, mul, gen = (B.g2_add, B.g2_mul, B.G2_GEN) if g2 else (B.g1_add, B.g1_mul, B.G1_GEN)
    neg = B.g2_neg if g2 else B.g1_neg
    rng = random.Random(71 + g2)
    pts = [mul(gen, rng.randrange(1, B.R)) for _ in range(5)]
    P, Q, S, T, U = pts
    PQ, nPQ = add(P, Q), neg(add(P, Q))
    table = [P, Q, S, T, U, PQ, nPQ, add(PQ, S)]
    cases = [
        [(0, 0)], [(0, 1)], [(0, 0), (1, 0)], [(0, 1), (1, 1)],
        [(0, 0), (0, 0)], [(0, 0), (0, 0), (1, 0), (2, 1)],                    # the same point twice from infinity, then further adds
        [(0, 1), (0, 1), (3, 0)],                                              # the same with negated entries
        [(0, 0), (0, 1)], [(0, 0), (0, 1), (1, 0), (2, 0)],                    # P then -P: cancellation, restart from infinity
        [(0, 1), (0, 0), (4, 1)],
        [(0, 0), (1, 0), (5, 0)], [(0, 0), (1, 0), (5, 0), (2, 0), (3, 1)],    # P, Q, then the entry P+Q: doubling with non-trivial ZZ
        [(0, 0), (1, 0), (6, 1)],                                              # ... as the negated entry -(P+Q)
        [(0, 0), (1, 0), (6, 0)], [(0, 0), (1, 0), (6, 0), (2, 0)],            # P, Q, then -(P+Q): cancellation with non-trivial ZZ
        [(0, 0), (1, 0), (5, 1), (3, 1), (4, 0)],                              # ... as the negated entry P+Q
        [(0, 0), (1, 0), (2, 0), (7, 0)], [(0, 1), (1, 1), (2, 1), (7, 0)],    # P+Q+S met as an entry: doubling / cancellation later on
        [(0, 1), (1, 1), (2, 1), (3, 1), (4, 1)],                              # negated entries throughout
        [(0, 0), (1, 1), (2, 0), (3, 1), (4, 0), (0, 0), (1, 1), (5, 0), (6, 0), (2, 1), (7, 0), (3, 0), (0, 1), (4, 1), (1, 0), (5, 1)],   # 16 steps
        [(i % 5, (i * 5 // 3) & 1) for i in range(16)],
    ]
    for _ in range(20):
        cases.append([(rng.randrange(8), rng.randrange(2)) for _ in range(rng.randrange(1, 17))])
    return table, cases


def _script_row(g2, table, steps, noncanonical):
    assert len(table) <= 8 and len(steps) <= 16 and all(pt is not None for pt in table)
    row = [len(steps)] + [i | (n << 8) for i, n in steps] + [0] * (16 - len(steps))
    for pt in table:
        coords = (pt[0][0], pt[0][1], pt[1][0], pt[1][1]) if g2 else pt
        for c in coords:
            row += words8(_mont(c, noncanonical))
    return row + [0] * ((32 if g2 else 16) * (8 - len(table)))


def script_batches(g2):
    add, neg = (B.g2_add, B.g2_neg) if g2 else (B.g1_add, B.g1_neg)
    table, cases = script_cases(g2)
    aw = 32 if g2 else 16
    rinv = pow(R256, -1, B.P)
    sfx = "G2" if g2 else "G1"
    group = "scripts_g2" if g2 else "scripts_g1"

    def walk(steps, distinct):
        """the affine sum; with distinct, a step whose entry has the accumulator's x adds nothing and returns false"""
        acc, ret = None, 0
        for s, (i, n) in enumerate(steps):
            e = neg(table[i]) if n else table[i]
            if distinct and acc is not None and acc[0] == e[0]:
                continue
            acc = add(acc, e)
            ret |= 1 << s
        return acc, ret

    def point_check(o, want):
        if o[0] != (1 if want is None else 0):
            return "inf flag %d, expected %s" % (o[0], "infinity" if want is None else "a point")
        ws = [from_words8(o[1 + 8 * j:9 + 8 * j]) for j in range(aw // 8)]
        if want is None:
            return None if not any(ws) else "infinity must come back as zero words"
        coords = (want[0][0], want[0][1], want[1][0], want[1][1]) if g2 else want
        for j, (w, c) in enumerate(zip(ws, coords)):
            if not w < 2 * B.P or w * rinv % B.P != c:
                return "coordinate %d is %x, expected %x" % (j, w * rinv % B.P, c)
        return None

    out = []
    for op, distinct in (("SCRIPT_%s_29" % sfx, False), ("SCRIPT_%s" % sfx, False), ("SCRIPT_%s_29_DISTINCT" % sfx, True)):
        steps_list = list(cases)
        pair_of = {}
        if distinct:
            # every script that meets a same-x step also runs with those steps taken out: all limbs must match
            for ci, steps in enumerate(cases):
                _, ret = walk(steps, True)
                if ret != (1 << len(steps)) - 1:
                    pair_of[ci] = len(steps_list)
                    steps_list.append([st for s, st in enumerate(steps) if (ret >> s) & 1])
            assert len(pair_of) >= 8
        rows = [_script_row(g2, table, steps, noncanonical=(ci % 3 == 2)) for ci, steps in enumerate(steps_list)]
        want = [walk(steps, distinct) for steps in steps_list]

        def chk(i, row, o, want=want, distinct=distinct):
            acc, ret = want[i]
            if distinct and o[1 + aw] != ret:
                return "madd_distinct returned %s per step, expected %s" % (bin(o[1 + aw]), bin(ret))
            return point_check(o, acc)
        b = Batch(group, FQ, op, rows, chk)
        b.pair_of = pair_of
        out.append(b)
    return out


def check_distinct_limbs_unchanged(batch, out_rows):
    """madd_distinct leaves every limb unchanged on a same-x step: the script with those steps removed ends in the same limbs"""
    for ci, cj in batch.pair_of.items():
        a, b = [int(x) for x in out_rows[ci]], [int(x) for x in out_rows[cj]]
        aw = batch.out_words - 2 - (72 if batch.out_words == 106 else 36)
        assert a[0] == b[0] and a[2 + aw:] == b[2 + aw:], "%s case %d: a same-x step changed the accumulator's limbs\n  %s\n  %s" % (
            batch.name(), ci, " ".join("%08x" % x for x in a[2 + aw:]), " ".join("%08x" % x for x in b[2 + aw:]))


# ---------------------------------------------------------------------------------------------------------------- BigS<12>, big_mul_acc
M384 = 1 << 384


def wordsn(v, n):
    assert 0 <= v < 1 << (32 * n)
    return [(v >> (32 * i)) & 0xffffffff for i in range(n)]


def from_words(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


def big(v):
    """a signed value as the 12 two's-complement words of Big384"""
    assert -(1 << 383) <= v < 1 << 383
    return wordsn(v % M384, 12)


def signed384(u):
    return u - M384 if u >> 383 else u


def bigs_edge_values():
    e = [0, 1, -1, 2, -2, (1 << 383) - 1, -(1 << 383), -(1 << 383) + 1, 1 << 382, (1 << 382) - 1, -(1 << 382), -(1 << 382) - 1, -(1 << 382) + 1]
    for k in range(32, 384, 32):                          # every word boundary, from both sides and in both signs
        e += [1 << k, -(1 << k), (1 << k) - 1, -(1 << k) - 1, -(1 << k) + 1]
    e += [signed384(0xffffffff << (32 * i)) for i in range(12)]                       # one all-ones word
    e += [signed384(int("ffffffff00000000" * 6, 16)), signed384(int("00000000ffffffff" * 6, 16))]
    return list(dict.fromkeys(e))


def _rand_signed(rng, maxbits=383):
    return rng.choice((1, -1)) * rng.getrandbits(rng.randrange(maxbits + 1))


LT_DOMAIN = 1 << 382      # the bound the header comment of BigS::lt states: |a|, |b| < 2^382


def lt_class(a, b):
    if not -(1 << 383) <= a - b < 1 << 383:
        return "lt overflowing difference"
    return "lt in the stated domain" if abs(a) < LT_DOMAIN and abs(b) < LT_DOMAIN else "lt beyond the domain, difference fits"


def bigs_batches():
    rng = random.Random(81)
    e = bigs_edge_values()
    singles = e + [_rand_signed(rng) for _ in range(N_RANDOM)]
    singles += [-(rng.getrandbits(300) << 64) for _ in range(50)] + [rng.getrandbits(300) << 64 for _ in range(20)]   # low 64 bits zero
    singles += [rng.choice((1, -1)) * (rng.getrandbits(200) << 32 | 1) << 32 for _ in range(20)]                      # w[0] = 0, w[1] != 0
    singles += [rng.choice((1, -1)) * ((rng.getrandbits(200) << 64) | rng.getrandbits(32) | 1) for _ in range(20)]    # w[1] = 0, w[0] != 0
    pairs = [(a, b) for a in e for b in e]
    # differences just below and exactly 2^383, from both sides
    h, t = 1 << 382, 1 << 383
    pairs += [(h, -h), (h - 1, -h), (-h, h), (-h - 1, h), (0, -t), (-1, -t), (t - 1, -1), (t - 1, 0), (-t, 1), (-t, 0), (t - 1, -t), (-t, t - 1)]
    pairs += [(_rand_signed(rng), _rand_signed(rng)) for _ in range(N_RANDOM)]
    pairs += [(_rand_signed(rng, 260), _rand_signed(rng, 260)) for _ in range(N_RANDOM // 4)]       # the magnitudes of dev_glv_split
    pairs += [(a, a + d) for a in (_rand_signed(rng, 381) for _ in range(100)) for d in (-1, 0, 1)]  # equal high words
    srows = [big(a) for a in singles]
    prows = [big(a) + big(b) for a, b in pairs]
    sg = lambda w: signed384(from_words(w))
    out = []

    def exact(o, want):
        return None if from_words(o) == want % M384 else "expected %x" % (want % M384)

    def carries(x, y, sub):
        """the carry (borrow) out of each of the 12 words of x + y (x - y) on the raw words"""
        return [(((x % (1 << 32 * k)) - (y % (1 << 32 * k))) < 0) if sub else (((x % (1 << 32 * k)) + (y % (1 << 32 * k))) >> (32 * k))
                for k in range(1, 13)]

    def cls_addsub(name, sub):
        def f(row, o):
            c = carries(from_words(row[:12]), from_words(row[12:]), sub)
            return [name, name + (" borrowing" if sub else " carrying") + " through all 12 words"] if all(c) else [name]
        return f
    out.append(Batch("bigs", FR, "BIGS_ADD", prows, lambda i, row, o: exact(o, sg(row[:12]) + sg(row[12:])), classes=cls_addsub("add", False)))
    out.append(Batch("bigs", FR, "BIGS_SUB", prows, lambda i, row, o: exact(o, sg(row[:12]) - sg(row[12:])), classes=cls_addsub("sub", True)))

    def cls_negate(row, o):
        a = sg(row)
        return ["negate", "negate of 0 (the carry runs through all 12 words)"] if a == 0 else ["negate", "negate of -2^383"] if a == -(1 << 383) else ["negate"]
    out.append(Batch("bigs", FR, "BIGS_NEGATE", srows, lambda i, row, o: exact(o, -sg(row)), classes=cls_negate))

    def chk_lt(i, row, o):
        a, b = sg(row[:12]), sg(row[12:])
        if o[0] not in (0, 1):
            return "not a truth value"
        if lt_class(a, b) == "lt overflowing difference":
            return None                                  # outside the domain: the result is recorded (lt_overflow_record), not judged
        return None if o[0] == (1 if a < b else 0) else "expected %d" % (a < b)
    out.append(Batch("bigs", FR, "BIGS_LT", prows, chk_lt, classes=lambda row, o: [lt_class(sg(row[:12]), sg(row[12:]))]))

    def cls_sar(row, o):
        a = sg(row)
        return ["sar64 non-negative"] if a >= 0 else ["sar64 negative, low 64 bits %s" % ("zero" if a % (1 << 64) == 0 else "non-zero")]
    out.append(Batch("bigs", FR, "BIGS_SAR64", srows, lambda i, row, o: exact(o, sg(row) >> 64), classes=cls_sar))

    def chk_low(i, row, o):
        want = 1 if from_words(row) % (1 << 64) == 0 else 0
        return None if o[0] == want else "expected %d" % want
    out.append(Batch("bigs", FR, "BIGS_LOW64_ZERO", srows, chk_low,
                     classes=lambda row, o: ["low64_zero %s" % ("true" if row[0] | row[1] == 0 else "one word zero" if 0 in row[:2] else "false")]))
    core = [0, 1, -1, (1 << 383) - 1, -(1 << 383), 1 << 128, -(1 << 128) + 1, signed384(int("ffffffff00000000" * 6, 16))]
    mrows = [big(a) + big(b) for a in e for b in core] + prows[len(e) ** 2:len(e) ** 2 + 12 + 300]
    for m in (0, 1, -1, 2, -3, 5, -5, 37, 64, -64):
        out.append(Batch("bigs", FR, "BIGS_ADD_SMALL_MUL", mrows, lambda i, row, o, m=m: exact(o, sg(row[:12]) + m * sg(row[12:])), arg=m & 0xffff,
                         classes=lambda row, o, m=m: ["add_small_mul m %s 0" % ("<" if m < 0 else ">" if m else "=")]))
    # big_mul_acc, the three shapes in use: [accumulator nw, a na, b nb] -> (accumulator + a * b) mod 2^(32 nw)
    for op, nw, na, nb in (("BIG_MUL_ACC_4X4_12", 12, 4, 4), ("BIG_MUL_ACC_2X2_12", 12, 2, 2), ("BIG_MUL_ACC_8X8_8", 8, 8, 8)):
        full, prod = 1 << (32 * nw), 1 << (32 * min(nw, na + nb))
        accs = [0, 1, full - 1, full - prod, prod - 1, full - 2, (full - 1) ^ (prod - 1) ^ 0xffffffff, rng.getrandbits(32 * nw)]
        ops = lambda n: [0, 1, (1 << (32 * n)) - 1, 1 << 31, 0xffffffff, 1 << (32 * (n - 1)), (1 << (32 * n)) - (1 << 32), rng.getrandbits(32 * n)]
        rows = [(c, a, b) for c in accs for a in ops(na) for b in ops(nb)]
        rows += [(rng.getrandbits(32 * nw), rng.getrandbits(32 * na), rng.getrandbits(32 * nb)) for _ in range(N_RANDOM // 2)]
        rows += [(full - 1 - rng.getrandbits(rng.randrange(32 * nw)), rng.getrandbits(32 * na), rng.getrandbits(32 * nb)) for _ in range(N_RANDOM // 2)]
        dec = lambda row, nw=nw, na=na: (from_words(row[:nw]), from_words(row[nw:nw + na]), from_words(row[nw + na:]))

        def chk(i, row, o, full=full, dec=dec):
            c, a, b = dec(row)
            return None if from_words(o) == (c + a * b) % full else "expected %x" % ((c + a * b) % full)

        def cls(row, o, op=op, full=full, prod=prod, dec=dec):
            c, a, b = dec(row)
            r = [op]
            if c and a * b:
                r.append(op + " into a non-zero accumulator")
            if prod < full and (c % prod) + a * b >= prod:
                r.append(op + " carry out of the last written word")
            if c + a * b >= full:
                r.append(op + " truncated at nw")
            return r
        out.append(Batch("bigs", FR, op, [wordsn(c, nw) + wordsn(a, na) + wordsn(b, nb) for c, a, b in rows], chk, classes=cls))
    return out


def lt_overflow_record(bs, outs):
    """(operand words, result) of every BIGS_LT case whose difference overflows 384 bits: what two builds must agree on"""
    b, o = next((b, o) for b, o in zip(bs, outs) if b.op == "BIGS_LT")
    sg = lambda w: signed384(from_words(w))
    return [(tuple(row), int(out[0])) for row, out in zip(b.rows, o) if lt_class(sg(row[:12]), sg(row[12:])) == "lt overflowing difference"]


# ---------------------------------------------------------------------------------------------------------------- dev_glv_split
GLV_STEP_CAP = 60         # |b| + 5 <= 60: inside the 64 steps the device spends on a quotient (beyond the cap its answer is undefined)


def glv_split_basis(s, v1, v2, bits=ccs.GLV_BITS):
    """ccs.glv_split with the basis (v1, v2) given, det > 0, and the same search order: (found, s1, s2, radius, (i1, i2), b1, b2)
    where glv_split raises"""
    det = v1[0] * v2[1] - v2[0] * v1[1]
    assert det > 0
    b1 = (2 * s * v2[1] + det) // (2 * det)
    b2 = (-2 * s * v1[1] + det) // (2 * det)
    for radius in range(0, 6):
        for i1 in range(-radius, radius + 1):
            for i2 in range(-radius, radius + 1):
                if max(abs(i1), abs(i2)) != radius:
                    continue
                x = s - (b1 + i1) * v1[0] - (b2 + i2) * v2[0]
                y = -(b1 + i1) * v1[1] - (b2 + i2) * v2[1]
                if 0 <= x < 1 << bits and 0 <= y < 1 << bits:
                    return 1, x, y, radius, (i1, i2), b1, b2
    return 0, 0, 0, None, None, b1, b2


def glv_words(v1, v2):
    """the 28 constant words of OP_GLV (ccs._glv_constants) for a basis"""
    det = v1[0] * v2[1] - v2[0] * v1[1]
    assert 0 < det < 1 << 256 and all(abs(v) < 1 << 128 for v in v1 + v2)
    w = []
    for v in v1 + v2:
        w += wordsn(abs(v), 4) + [1 if v < 0 else 0]
    return w + wordsn(det, 8)


def glv_basis_of(words):
    v = [(-1 if words[5 * k + 4] else 1) * from_words(words[5 * k:5 * k + 4]) for k in range(4)]
    return (v[0], v[1]), (v[2], v[3])


def glv_skewed_bases(n, seed=83):
    """bases of two long, nearly parallel vectors (their difference is the short one): Babai rounding then lands up to half a long
    vector from the target and the search has to walk rings (r, -r): radius 2 .. 5 and scalars with no pair at all.  The lattice
    is {(x, y): x = lam * y mod det} for the lam the basis itself fixes.  -> [(v1, v2, lam, q = det, largest scalar within the cap)]"""
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        x, y = (rng.randrange(1 << 125, 1 << 127) * rng.choice((1, -1)) for _ in range(2))
        d1, d2 = (rng.randrange(1 << 121, 1 << 126) * rng.choice((1, -1)) for _ in range(2))
        u1, u2 = (x, y), (x + d1, y + d2)
        det = u1[0] * u2[1] - u2[0] * u1[1]
        if det < 0:
            u1, u2, det = u2, u1, -det
        if det == 0 or det >> 256 or max(abs(v) for v in u1 + u2) >> 128 or math.gcd(u1[1], det) != 1 or math.gcd(u2[1], det) != 1:
            continue
        smax = min(1 << 128, (GLV_STEP_CAP - 6) * det // max(abs(u1[1]), abs(u2[1])))       # |b| <= s |v_y| / det + 1
        if smax < 1 << 120:
            continue
        lam = u1[0] * pow(u1[1], -1, det) % det
        assert (u2[0] - lam * u2[1]) % det == 0
        out.append((u1, u2, lam, det, smax))
    return out


@functools.lru_cache(maxsize=None)
def glv_cases():
    """[(v1, v2, lam, q, scalar)]: (a) the container's constants, (b) other bases of the same lattice, (c) skewed bases and sublattices"""
    rng = random.Random(82)
    lam, q = ccs.GLV_LAMBDA, ccs.Q_BASE
    v1, v2 = glv_basis_of(ccs._glv_constants())
    assert v1[0] * v2[1] - v2[0] * v1[1] == q
    fixed = [0, 1, 2, (1 << 64) - 1, (1 << 64) + 1, (1 << 127) - 1, 1 << 127, (1 << 127) + 1, (1 << 128) - 1, lam % (1 << 128)]
    for n in (1, 2):                                     # b1 = floor((2 s v2y + det) / (2 det)) first reaches n at this scalar
        sn = -(-(2 * n - 1) * q // (2 * v2[1]))
        assert glv_split_basis(sn - 1, v1, v2)[5] == n - 1 and glv_split_basis(sn, v1, v2)[5] == n
        fixed += [sn - 1, sn, sn + 1]
    assert all(0 <= s < 1 << 128 for s in fixed)
    cases = [(v1, v2, lam, q, s) for s in fixed + [rng.getrandbits(128) for _ in range(N_RANDOM)]]
    add = lambda a, b, k=1: (a[0] + k * b[0], a[1] + k * b[1])
    neg = lambda a: (-a[0], -a[1])
    for u1, u2 in ((neg(v2), v1), (neg(v1), neg(v2)), (add(v1, v2), v2), (v2, neg(v1)), (add(v1, v2, 2), v2)):
        assert u1[0] * u2[1] - u2[0] * u1[1] == q
        cases += [(u1, u2, lam, q, s) for s in fixed + [rng.getrandbits(128) for _ in range(N_RANDOM // 4)]]
    for u1, u2 in (((2 * v1[0], 2 * v1[1]), v2), (v1, (2 * v2[0], 2 * v2[1])), (add(v1, v2), add(v2, v1, -1))):   # index-2 sublattices
        assert u1[0] * u2[1] - u2[0] * u1[1] == 2 * q
        cases += [(u1, u2, lam, q, s) for s in fixed + [rng.getrandbits(128) for _ in range(100)]]
    for u1, u2, l2, q2, smax in glv_skewed_bases(24):
        cases += [(u1, u2, l2, q2, s) for s in [0, 1, smax - 1] + [rng.randrange(smax) for _ in range(120)]]
    for u1, u2, _, _, s in cases:                         # every base keeps the true quotients inside the device's step cap
        _, _, _, _, _, b1, b2 = glv_split_basis(s, u1, u2)
        assert abs(b1) + 5 <= GLV_STEP_CAP and abs(b2) + 5 <= GLV_STEP_CAP and 0 <= s < 1 << 128
    return cases


def glv_batches():
    cases = glv_cases()
    lattice = {tuple(glv_words(u1, u2)): (lam, q) for u1, u2, lam, q, _ in cases}

    def expect(row):
        v1, v2 = glv_basis_of(row[:28])
        return glv_split_basis(from_words(row[28:]), v1, v2)

    def chk(i, row, o):
        found, x, y = expect(row)[:3]
        got = (o[0], from_words(o[1:5]), from_words(o[5:9]))
        if got != (found, x, y):
            return "expected found %d s1 %x s2 %x" % (found, x, y)
        if found:
            lam, q = lattice[tuple(row[:28])]
            s = from_words(row[28:])
            if not (0 <= got[1] < 1 << 127 and 0 <= got[2] < 1 << 127 and (got[1] - lam * got[2] - s) % q == 0):
                return "s1 - lambda s2 = s (mod q) or the range 2^127 does not hold"
        return None

    def cls(row, o):
        found, _, _, radius, pos, b1, b2 = expect(row)
        r = ["not found" if not found else "radius >= 3" if radius >= 3 else "radius %d" % radius]
        if found and radius:
            r.append("ring position %s%s" % ("+0-"[(pos[0] < 0) + (pos[0] <= 0)], "+0-"[(pos[1] < 0) + (pos[1] <= 0)]))
        return r + [n for n, c in (("b1 < 0", b1 < 0), ("b1 > 0", b1 > 0), ("b2 < 0", b2 < 0), ("b2 > 0", b2 > 0)) if c]
    return [Batch("hint_glv", FR, "HINT_GLV_SPLIT", [glv_words(u1, u2) + wordsn(s, 4) for u1, u2, _, _, s in cases], chk, classes=cls)]


# ---------------------------------------------------------------------------------------------------------------- dev_emulated_reduce<6, 6>
B64 = 1 << 64
EMUL_CMAX = 1 << 58       # |c_i| of the random generator (see emul_cases)


def limbs64(v, n):
    assert 0 <= v < 1 << (64 * n)
    return [(v >> (64 * i)) & (B64 - 1) for i in range(n)]


def emul_limbs(k, r, c):
    """a_0 .. a_5 of a(X) = k(X) p(X) + r(X) + (2^64 - X) c(X) for the free carries c_0 .. c_4 (c_5 = k_3 p_3 closes the identity:
    a has no X^6); None when a limb leaves [0, r_BN254)"""
    q = ccs.Q_BASE
    assert 0 <= k < 1 << 256 and 0 <= r < q and len(c) == 5
    kl, pl, rl = limbs64(k, 4), limbs64(q, 4), limbs64(r, 4) + [0, 0]
    c = list(c) + [kl[3] * pl[3]]
    a = []
    for i in range(6):
        a.append(sum(kl[x] * pl[i - x] for x in range(4) if 0 <= i - x < 4) + rl[i] + B64 * c[i] - (c[i - 1] if i else 0))
    return a if all(0 <= v < MOD[FR] for v in a) else None


def emul_reference(a):
    """ccs._emulated_mul_hint on the limbs a (b = [1], 64-bit limbs, n = nq = 4, six carries) -> (k, r, signed carries); the carries
    are recomputed as integers here and must be the field elements the hint returns"""
    q = ccs.Q_BASE
    ref = ccs._emulated_mul_hint([64, 4, 6, 4] + limbs64(q, 4) + list(a) + [1], 14)
    k, r = sum(v << (64 * i) for i, v in enumerate(ref[:4])), sum(v << (64 * i) for i, v in enumerate(ref[4:8]))
    kl, pl, rl = limbs64(k, 4), limbs64(q, 4), limbs64(r, 4) + [0, 0]
    cs, c = [], 0
    for i in range(6):
        num = a[i] - sum(kl[x] * pl[i - x] for x in range(4) if 0 <= i - x < 4) - rl[i] + c
        assert num % B64 == 0
        c = num // B64
        cs.append(c)
    assert [v % MOD[FR] for v in cs] == ref[8:] and cs[5] == kl[3] * pl[3]
    return k, r, cs


@functools.lru_cache(maxsize=None)
def emul_cases():
    """(edge cases, random cases, keep rate of the random generator) as limb lists.

    The random generator picks k < 2^256, r < q and carries |c_i| <= 2^58 and keeps a case when every limb is in [0, r_BN254): a limb
    is a_i = sum k_x p_y + r_i + 2^64 c_i - c_(i-1) with sum k_x p_y around 2^126, so a negative carry of 2^58 (2^122 after the
    shift) leaves the limb non-negative unless the k limbs under it are small.  Measured keep rate: 0.98 (asserted >= 0.9 below).
    A second family draws the LIMBS at random (a_i < r_BN254, the value below 2^256 q so the quotient fits): every such row is in the
    domain, and its carries run up to 2^190 in both signs, which the constructive family cannot reach."""
    rng = random.Random(84)
    q, p = ccs.Q_BASE, MOD[FR]
    ones = (1 << 256) - 1
    cm = EMUL_CMAX
    kbig = ones - (1 << 70)                              # every limb of k large: the limbs stay positive under a carry of -2^58
    edges = [emul_limbs(0, 0, [0] * 5)]                                                        # a = 0
    edges += [emul_limbs(kk, rr, [0] * 5) for kk, rr in ((0, q - 1), (1, 0), (1, 1), (2, 0))]   # a(2^64) = q - 1, q, q + 1, 2 q
    edges += [emul_limbs(kbig, 0, [5, -7, 11, -13, 17]), emul_limbs(kbig, q - 1, [5, -7, 11, -13, 17]), emul_limbs(ones, q - 1, [0] * 5)]
    edges += [emul_limbs(ones, 12345, [1, 2, 3, 4, 5]), emul_limbs(0, q - 1, [1, 1, 1, 0, 0])]
    for kk in (int("ffffffffffffffff0000000000000000" * 2, 16), int("0000000000000000ffffffffffffffff" * 2, 16)):   # all-ones limb next to a zero limb
        edges += [emul_limbs(kk, rng.randrange(q), [0] * 5), emul_limbs(kk, rng.randrange(q), [3, -3, 3, -3, 3])]
    edges += [emul_limbs(0, rng.randrange(q), [0] * 5), emul_limbs(rng.getrandbits(192), rng.randrange(q), [0] * 5)]   # all carries zero
    for j in range(5):
        for v in (-1, cm, -cm, 1):                       # a carry of -1, and +- the largest magnitude the generator uses, at every place
            c = [0] * 5
            c[j] = v
            edges.append(emul_limbs(kbig, rng.randrange(q), c))
    edges += [emul_limbs(kbig, rng.randrange(q), [cm] * 5), emul_limbs(kbig, rng.randrange(q), [-cm] * 5)]
    edges.append(emul_limbs(kbig, rng.randrange(q), [-cm, cm, -cm, cm, -cm]))
    k1 = rng.getrandbits(128)                            # upper limbs a_4 = a_5 = 0 under a non-zero k: c_4 = 0, c_3 = k_1 p_3
    edges.append(emul_limbs(k1, rng.randrange(q), [0, 0, 0, (k1 >> 64) * (q >> 192), 0]))
    edges.append(emul_limbs(rng.getrandbits(64), rng.randrange(q), [0] * 5))
    assert all(a is not None for a in edges), "an edge case left the domain"                   # none may be dropped
    assert edges[-2][4:] == [0, 0] and edges[-1][4:] == [0, 0] and all(edges[5][4:])
    kept, tried = [], 0
    while len(kept) < N_RANDOM:
        tried += 1
        a = emul_limbs(rng.getrandbits(256), rng.randrange(q), [rng.randrange(-cm, cm + 1) for _ in range(5)])
        if a is not None:
            kept.append(a)
    rate = len(kept) / tried
    assert rate >= 0.9, rate
    free = []
    while len(free) < N_RANDOM // 2:
        a = [rng.randrange(p) for _ in range(5)] + [rng.getrandbits(rng.randrange(1, 190))]
        if sum(v << (64 * i) for i, v in enumerate(a)) < q << 256:
            free.append(a)
    for top in ((q << 256) - 1, (q << 256) - q, (q << 256) - q - 1):                            # the largest quotient a row can have
        lo, a5 = top % (1 << 320), top >> 320
        free.append(limbs64(lo % (1 << 256), 4) + [lo >> 256, a5])
    return edges, kept + free, rate


def emul_batches():
    edges, rand, _ = emul_cases()
    q = ccs.Q_BASE
    qc = words8(q) + words8(pow(q, -1, R256))
    limbs = lambda row: [from_words8(row[8 * i:8 * i + 8]) for i in range(6)]

    def chk(i, row, o):
        k, r, cs = emul_reference(limbs(row))
        if from_words8(o[:8]) != k:
            return "quotient, expected %x" % k
        if from_words8(o[8:16]) != r:
            return "remainder, expected %x" % r
        for j in range(6):
            raw = signed384(from_words(o[16 + 12 * j:28 + 12 * j]))
            if raw != cs[j]:
                return "carry %d is %d, expected %d" % (j, raw, cs[j])
            if from_words8(o[88 + 8 * j:96 + 8 * j]) != cs[j] % MOD[FR]:
                return "carry %d as a field element, expected %x" % (j, cs[j] % MOD[FR])
        d6 = -(from_words(o[6:8]) * (q >> 192))           # the X^6 coefficient of a - k p - r: the identity closes when carry_5 + d_6 = 0
        if signed384(from_words(o[76:88])) + d6 != 0:
            return "carry_5 + d_6 != 0"
        return None

    def cls(row, o):
        a = limbs(row)
        k, r, cs = emul_reference(a)
        r_ = ["remainder zero" if r == 0 else "remainder q - 1" if r == q - 1 else "remainder other",
              "upper limbs a_4, a_5 %s" % ("zero" if a[4] == 0 and a[5] == 0 else "non-zero" if a[4] and a[5] else "one zero")]
        if k == (1 << 256) - 1:
            r_.append("quotient maximal")
        if not any(cs):
            r_.append("all carries zero")
        if any(c < 0 for c in cs):
            r_.append("a carry negative")
        if -1 in cs:
            r_.append("a carry -1")
        if any(abs(c) == EMUL_CMAX for c in cs[:5]):
            r_.append("a carry at +-2^58")
        if any(abs(c) >> 180 for c in cs):
            r_.append("a carry beyond 2^180")
        return r_
    rows = [sum((words8(v) for v in a), []) + qc for a in edges + rand]
    return [Batch("hint_emul", FR, "HINT_EMUL_REDUCE", rows, chk, classes=cls)]


# ---------------------------------------------------------------------------------------------------------------- dev_grumpkin_mul
def gk_add(P, Q_):
    """affine addition on y^2 = x^3 - 17 over Fr; None is the point at infinity"""
    p = MOD[FR]
    if P is None:
        return Q_
    if Q_ is None:
        return P
    if P[0] == Q_[0]:
        if (P[1] + Q_[1]) % p == 0:
            return None
        l = 3 * P[0] * P[0] * pow(2 * P[1], -1, p) % p
    else:
        l = (Q_[1] - P[1]) * pow(Q_[0] - P[0], -1, p) % p
    x = (l * l - P[0] - Q_[0]) % p
    return x, (l * (P[0] - x) - P[1]) % p


def gk_mul(k):
    """k * G by double-and-add from the top bit, and the names of the ladder's special steps k passes through"""
    G = (1, ccs.GRUMPKIN_GY)
    acc, seen = None, set()
    for bit in range(k.bit_length() - 1, -1, -1):
        acc = gk_add(acc, acc)
        if (k >> bit) & 1:
            if acc is None and bit != k.bit_length() - 1:
                seen.add("ladder restarts from infinity")
            elif acc == G:
                seen.add("ladder adds G to G (H = 0, Rr = 0)")
            elif acc is not None and acc[0] == G[0]:
                seen.add("ladder adds G to -G")
            acc = gk_add(acc, G)
    return acc, seen


@functools.lru_cache(maxsize=None)
def gk_cases():
    """[(k, k * G or None, special steps)]"""
    rng = random.Random(85)
    o = ccs.Q_BASE
    ks = [0, 1, 2, 3, 1 << 127, (1 << 128) - 1, 1 << 128, 1 << 255, (1 << 256) - 1, o - 1, o, o + 1, 2 * o, 2 * o + 1]
    ks += [o + 2, 2 * o + 4, 2 * o + 5, 4 * o - 1]         # (o + 2) >> 1 = (o + 1) / 2: doubled it is G again, and the last bit adds G
    ks += [rng.getrandbits(256) for _ in range(N_RANDOM // 10)]
    ks += [rng.getrandbits(rng.randrange(1, 129)) + (rng.getrandbits(rng.randrange(0, 129)) << 128) for _ in range(N_RANDOM // 10)]   # (lo, hi)
    assert all(0 <= k < 1 << 256 for k in ks)
    assert gk_mul(o)[0] is None and gk_mul(1)[0] == (1, ccs.GRUMPKIN_GY)
    for k in (2, 3, (1 << 128) - 1, ks[20] % MOD[FR], ks[-1] % MOD[FR]):
        assert gk_mul(k)[0] == tuple(H.fixed_base_scalar_mul(k))
    return [(k,) + gk_mul(k) for k in ks]


def gk_batches():
    cases = {k: (pt, seen) for k, pt, seen in gk_cases()}
    p = MOD[FR]
    rinv = pow(R256, -1, p)
    gy = words8(ccs.GRUMPKIN_GY * R256 % p)

    def chk(i, row, o):
        k = from_words8(row[:8])
        want = cases[k][0]
        assert (want is None) == (k % ccs.Q_BASE == 0)
        if o[0] != (0 if want is None else 1):
            return "finite flag %d" % o[0]
        x, y = from_words8(o[1:9]), from_words8(o[9:17])
        if want is None:
            return None if x == 0 and y == 0 else "the point at infinity must come back as zero words"
        if not (x < 2 * p and y < 2 * p and (x * rinv % p, y * rinv % p) == want):
            return "expected (%x, %x)" % want
        return None

    def cls(row, o):
        k = from_words8(row[:8])
        pt, seen = cases[k]
        return ["finite" if pt is not None else "k = 0 mod the group order"] + sorted(seen)
    return [Batch("hint_gk", FR, "HINT_GRUMPKIN_MUL", [words8(k) + gy for k, _, _ in gk_cases()], chk, classes=cls)]


# ---------------------------------------------------------------------------------------------------------------- the groups
GROUPS = ("fp", "inv", "fq2", "f29", "is_zero_mod_p", "f29x2", "scripts_g1", "scripts_g2")
HINT_GROUPS = ("bigs", "hint_glv", "hint_emul", "hint_gk")       # csrc/gnark_hints.hpp: verify_group returns cases per branch class
_MUL_ACC = ["BIG_MUL_ACC_%s%s" % (sh, c) for sh in ("4X4_12", "2X2_12", "8X8_8") for c in ("", " into a non-zero accumulator", " truncated at nw")]
HINT_CLASSES = {                                                  # every class must hold at least one case
    "bigs": _MUL_ACC + ["BIG_MUL_ACC_4X4_12 carry out of the last written word", "BIG_MUL_ACC_2X2_12 carry out of the last written word",
                        "add", "add carrying through all 12 words", "sub", "sub borrowing through all 12 words", "negate", "negate of -2^383",
                        "negate of 0 (the carry runs through all 12 words)", "add_small_mul m < 0", "add_small_mul m = 0", "add_small_mul m > 0",
                        "low64_zero false", "low64_zero one word zero", "low64_zero true", "lt in the stated domain",
                        "lt beyond the domain, difference fits", "lt overflowing difference", "sar64 non-negative",
                        "sar64 negative, low 64 bits zero", "sar64 negative, low 64 bits non-zero"],
    # ring positions: (sign of i1, sign of i2) of the pair the search returns at radius >= 1; (+, +) is not reached by any base here
    "hint_glv": ["radius 0", "radius 1", "radius 2", "radius >= 3", "not found", "b1 < 0", "b1 > 0", "b2 < 0", "b2 > 0"] +
                ["ring position " + p for p in ("+-", "+0", "-+", "--", "-0", "0+", "0-")],
    "hint_emul": ["remainder zero", "remainder q - 1", "remainder other", "quotient maximal", "all carries zero", "a carry negative", "a carry -1",
                  "a carry at +-2^58", "a carry beyond 2^180", "upper limbs a_4, a_5 zero", "upper limbs a_4, a_5 one zero",
                  "upper limbs a_4, a_5 non-zero"],
    "hint_gk": ["finite", "k = 0 mod the group order", "ladder adds G to G (H = 0, Rr = 0)", "ladder adds G to -G", "ladder restarts from infinity"],
}


def batches(group):
    if group == "fp":
        return fp_batches(FR) + fp_batches(FQ)
    if group == "inv":
        return inv_batches(FR) + inv_batches(FQ)
    if group == "fq2":
        return fq2_batches()
    if group == "f29":
        return f29_batches(FR) + f29_batches(FQ)
    if group == "is_zero_mod_p":
        return is_zero_batches(FR) + is_zero_batches(FQ)
    if group == "f29x2":
        return f29x2_batches()
    if group == "scripts_g1":
        return script_batches(False)
    if group == "scripts_g2":
        return script_batches(True)
    if group == "bigs":
        return bigs_batches()
    if group == "hint_glv":
        return glv_batches()
    if group == "hint_emul":
        return emul_batches()
    if group == "hint_gk":
        return gk_batches()
    raise KeyError(group)


def verify_group(group, bs, outs):
    """all predicates of a group on the results `outs[k]` (rows of words) of batch bs[k]; returns {batch name: cases}, for the
    groups of gnark_hints.hpp {branch class: cases}"""
    counts = {}
    if group in HINT_GROUPS:
        counts = {c: 0 for c in HINT_CLASSES.get(group, ())}
        for b, o in zip(bs, outs):
            b.verify(o)
            for row, out in zip(b.rows, o):
                for c in b.classes(row, [int(x) for x in out]):
                    counts[c] = counts.get(c, 0) + 1
        return counts
    for b, o in zip(bs, outs):
        counts[b.name()] = b.verify(o)
        if getattr(b, "pair_of", None):
            check_distinct_limbs_unchanged(b, o)
    if group == "inv":
        for f in (FR, FQ):
            sel = [(b, o) for b, o in zip(bs, outs) if b.field == f]
            check_inv_agreement([b for b, _ in sel], [o for _, o in sel])
    return counts
