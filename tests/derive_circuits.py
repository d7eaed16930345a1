"""Circuits crafted for the derivation of a key from a powers-of-tau transcript (spp_setup_from_ptau): synth_circuits.Desc objects whose
matrices put the column gather, its combine step and the Z points on their edges, and transcripts' secrets chosen to make points meet.

The derivation reads only the matrices, n_public, challenge_wire and committed, so the rows here are not satisfiable and the program
is OP_END alone.  A generator returns a `Crafted`: `desc`, the wires it names (`wire`), and `expect`: the properties the circuit is
built to have, computed from the matrices by the model below (`model`), never by hand.  tests/test_derive_circuits_host.py recomputes
them on its own, so a generator that drifts off its edge fails without a GPU.  Expected keys never come from here: the tests take
them from ptau_format.derived_key.

The gather as the library plans it, restated from csrc/ptau.hpp's documentation and not imported from the code under test: a column
is the list of its (row, coefficient) terms in the order matrix A, matrix B, matrix C, each in row order and inside a row in the order
stored; the G1 gather has the columns A_j, B_j and K_j = A_j on beta L | B_j on alpha L | C_j on L of every wire j, the G2 gather the
columns B_j; a column of t terms is cut into ceil(t / 16) chunks, one lane each; a coefficient c is applied as min(c, R - c) with a
sign, in a loop of the magnitude's bit length."""
import random

from synth_circuits import Desc, R

CHUNK = 16                               # PT_GATHER_CHUNK
WAVE = 64

# secrets of the transcripts the GPU tests derive from
TAU = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % R
ALPHA = 0x0FEDCBA987654321DEADBEEF00C0FFEE0123456789ABCDEF0FEDCBA987654321 % R
BETA = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R


class Crafted:
    def __init__(self, name, desc, wire, expect):
        self.name, self.desc, self.wire, self.expect = name, desc, wire, expect


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
def magnitude(c):
    c %= R
    return R - c if c > (R - 1) // 2 else c


def _columns(desc):
    cols = {m: [[] for _ in range(desc.n_wires)] for m in "ABC"}
    for m in "ABC":
        for k, terms in enumerate(getattr(desc, m)):
            for w, v in terms:
                cols[m][w].append((k, v))
    return cols


def _chunks(t):
    return -(-t // CHUNK)


def _row_sums(col):
    out = {}
    for k, v in col:
        out[k] = (out.get(k, 0) + v) % R
    return out


def model(desc):
    """the facts a test may rely on; `vanish` holds for a transcript with tau off the domain:
         always: the wires whose A, B or K column sums to infinity whatever the secrets (every row's coefficients sum to zero)
         K_equal / K_opposite: the wires whose K column does under alpha == beta / under beta == -alpha, and not always"""
    cols = _columns(desc)
    W = desc.n_wires
    lens = {m: [len(c) for c in cols[m]] for m in "ABC"}
    klen = [lens["A"][j] + lens["B"][j] + lens["C"][j] for j in range(W)]
    g1 = sum(_chunks(lens["A"][j]) + _chunks(lens["B"][j]) + _chunks(klen[j]) for j in range(W))
    g2 = sum(_chunks(lens["B"][j]) for j in range(W))
    bits = {magnitude(v).bit_length() for m in "ABC" for c in cols[m] for _, v in c}
    zero = lambda sums: all(v == 0 for v in sums.values())
    always = {m: [j for j in range(W) if cols[m][j] and zero(_row_sums(cols[m][j]))] for m in "AB"}
    k_always, k_equal, k_opposite = [], [], []
    for j in range(W):
        if not klen[j]:
            continue
        a, b, c = (_row_sums(cols[m][j]) for m in "ABC")
        rows = set(a) | set(b) | set(c)
        if zero(a) and zero(b) and zero(c):
            k_always.append(j)
        elif zero(c) and all((a.get(k, 0) + b.get(k, 0)) % R == 0 for k in rows):      # alpha (a_k + b_k) + c_k
            k_equal.append(j)
        elif zero(c) and all((a.get(k, 0) - b.get(k, 0)) % R == 0 for k in rows):      # alpha (b_k - a_k) + c_k
            k_opposite.append(j)
    return {"domain_log": desc.domain_log, "n_wires": W, "col_len": lens, "k_len": klen, "chunks_g1": g1, "chunks_g2": g2,
            "max_col": max(klen), "max_col_chunks": max(_chunks(t) for t in klen), "bit_lengths": bits,
            "vanish": {"A": always["A"], "B": always["B"], "K": k_always, "K_equal": k_equal, "K_opposite": k_opposite}}


def _finish(name, d, wire, public, challenge, committed):
    """wires [0, public) are the public ones; no instruction but OP_END"""
    d.n_public, d.n_secret = public, d.n_wires - public
    d.challenge_wire, d.committed = challenge, sorted(committed)
    d.finish()
    return Crafted(name, d, wire, model(d))


def _rows(d, n, a, b, c):
    """n constraints from three {row: terms} dictionaries"""
    for k in range(n):
        d.row(a.get(k, []), b.get(k, []), c.get(k, []))


# ---------------------------------------------------------------------------------------------------------------------
# every kind of coefficient
# ---------------------------------------------------------------------------------------------------------------------
def coefficient_kinds():
    """the scalar loop's edges: the zero, the one-addition and the sign cases, a word boundary of every word from both sides (bit
    length 32 k: the first word read is full; 32 k + 1: one bit of the first word, then a reload), the largest magnitude"""
    rng = random.Random(0xC0EF)
    ks = [0, 1, R - 1, 2, R - 2, 3, (1 << 28) - 1]
    for k in range(1, 8):
        ks += [1 << (32 * k - 1), (1 << (32 * k)) - 1, 1 << (32 * k)]
    ks += [(R - 1) // 2, (R + 1) // 2, R - (1 << 32), R - ((1 << 32) - 1)]
    return ks + [rng.randrange(1, R) for _ in range(2)]


def coeff_kinds():
    """wire i carries coefficient_kinds()[i] once in A, once in B and once in C, on three rows of a 32-row domain; the first three
    wires are public, one is the challenge wire and three are committed"""
    ks = coefficient_kinds()
    d, n = Desc(0, 0), 32
    d.new_wire(len(ks) - 1)
    a, b, c = {}, {}, {}
    for i, v in enumerate(ks):
        a.setdefault(5 * i % n, []).append((i, v))
        b.setdefault((5 * i + 11) % n, []).append((i, v))
        c.setdefault((5 * i + 22) % n, []).append((i, v))
    _rows(d, n, a, b, c)
    wire = {"kind_%d" % i: i for i in range(len(ks))}
    return _finish("coeff_kinds", d, wire, 3, ks.index(1 << 32), [ks.index(1 << 63), ks.index((R - 1) // 2), len(ks) - 1])


# ---------------------------------------------------------------------------------------------------------------------
# column lengths around the chunk, a column of more than a wave of chunks
# ---------------------------------------------------------------------------------------------------------------------
SHAPE_LENGTHS = (0, 1, 15, 16, 17, 32, 33)
K_LENGTHS = (15, 16, 17)                 # wires whose K column (A | B | C) has exactly this many terms
LONG_TERMS = CHUNK * WAVE + 1
FILLERS = 62                             # wires with one term in B


def column_shapes():
    """100 constraints on a 128-row domain.  Wire 0 (the constant, as in the audit circuit) has LONG_TERMS terms in A and in B,
    (wire, c) repeated inside rows, mostly small coefficients and a few full-size ones; one wire per length of SHAPE_LENGTHS with
    that many terms in each of A, B and C on distinct rows; one wire per length of K_LENGTHS with that many terms in all; FILLERS
    wires with one term in B between them, so that there are more wires than a wave has lanes"""
    rng = random.Random(0x5A9E)
    d, n = Desc(1, 0), 100
    a, b, c = {}, {}, {}
    full = [(R - 1) // 2, (R + 1) // 2, 1 << 224, R - (1 << 160)]

    def coeff(i):
        if i % 131 == 7:
            return rng.choice(full + [rng.randrange(1, R)])
        return rng.choice([1, R - 1, 2, R - 3, rng.randrange(2, 1 << 20), R - rng.randrange(2, 1 << 28), 1 << 32, (1 << 32) - 1])
    wire = {"long": 0, "public": 1}
    for m in (a, b):
        for i in range(LONG_TERMS):
            m.setdefault(i % n, []).append((0, coeff(i)))
    a.setdefault(3, []).append((1, 5))
    c.setdefault(4, []).append((1, R - 9))
    for i in range(FILLERS):             # the wires named below come after a wave of others: the combine step of the G2 gather, one
        w = d.new_wire()                 # lane per wire, runs two workgroups and meets them in the second
        b.setdefault(rng.randrange(n), []).append((w, coeff(i)))
    for t in SHAPE_LENGTHS:
        w = wire["len_%d" % t] = d.new_wire()
        for m in (a, b, c):
            for j, k in enumerate(rng.sample(range(n), t)):
                m.setdefault(k, []).append((w, coeff(j + 1)))
    for t in K_LENGTHS:
        w = wire["k_len_%d" % t] = d.new_wire()
        for j, k in enumerate(rng.sample(range(n), t)):
            (a, b, c)[j % 3].setdefault(k, []).append((w, coeff(j + 1)))
    _rows(d, n, a, b, c)
    return _finish("column_shapes", d, wire, 2, wire["len_17"], [wire["len_16"], wire["len_33"], wire["k_len_16"]])


# ---------------------------------------------------------------------------------------------------------------------
# an accumulator that meets the point it holds, or its negative
# ---------------------------------------------------------------------------------------------------------------------
def meetings():
    """20 constraints on a 32-row domain; see the wires' names below.  BIG is a full-size coefficient."""
    rng = random.Random(0x3EE7)
    BIG = rng.randrange(1 << 250, (R - 1) // 2)
    d, n = Desc(1, 0), 20
    a, b, c = {}, {}, {}
    wire = {"one": 0, "public": 1}
    a.setdefault(0, []).append((0, 1))
    b.setdefault(1, []).append((1, 7))
    c.setdefault(2, []).append((1, R - 2))
    row = iter(range(3, n))

    def new(name):
        wire[name] = d.new_wire()
        return wire[name]
    # 1. (w, c), (w, c) in one row of A and of B: P + P in the mixed addition (c = 1), in the general addition (multi-bit c)
    for name, v in (("twice_1", 1), ("twice_minus_1", R - 1), ("twice_5", 5), ("twice_big", BIG)):
        w, k = new(name), next(row)
        a.setdefault(k, []).extend([(w, v), (w, v)])
        b.setdefault(k, []).extend([(w, v), (w, v)])
    # 2. c in A and in B of one row, nothing in C: the K column is c beta L_k + c alpha L_k, a doubling under alpha == beta and
    #    infinity under beta == -alpha; `_then` carries a further term, so the sum restarts from infinity
    for name, v in (("ab_1", 1), ("ab_6", 6), ("ab_big", BIG), ("ab_1_committed", 1)):
        w, k = new(name), next(row)
        a.setdefault(k, []).append((w, v))
        b.setdefault(k, []).append((w, v))
    for name, v in (("ab_1_then", 1), ("ab_big_then", BIG)):
        w, k = new(name), next(row)
        a.setdefault(k, []).append((w, v))
        b.setdefault(k, []).append((w, v))
        c.setdefault((k + 5) % n, []).append((w, 3))
    #    c in A and -c in B: infinity under alpha == beta
    w, k = new("ab_opposite_6"), next(row)
    a.setdefault(k, []).append((w, 6))
    b.setdefault(k, []).append((w, R - 6))
    # 3. two full chunks, the second the first with every coefficient negated: the combine step adds P and -P.  In one row of A and
    #    of B (so in G1 and G2, whatever the secrets) ...
    cs = [1, 2, R - 1, 3, BIG, 1 << 32, (1 << 32) - 1, R - 5] + [rng.randrange(2, 1 << 20) for _ in range(CHUNK - 8)]
    w, k = new("chunks_cancel"), next(row)
    for m in (a, b):
        m.setdefault(k, []).extend([(w, v) for v in cs] + [(w, R - v) for v in cs])
    #    ... and over 16 rows in the K column: A's chunk on beta L against B's on alpha L, opposite partials under beta == -alpha, equal
    #    partials (a doubling in the combine step) under alpha == beta
    w = new("k_chunks")
    for j, v in enumerate(cs):
        a.setdefault(j, []).append((w, v))
        b.setdefault(j, []).append((w, v))
    # 4. (w, c), (w, R - c) in one row: P - P in the mixed and in the general addition; `_then`: with a term after the pair
    for name, v in (("cancel_1", 1), ("cancel_big", BIG)):
        w, k = new(name), next(row)
        a.setdefault(k, []).extend([(w, v), (w, R - v)])
        b.setdefault(k, []).extend([(w, v), (w, R - v)])
    for name, v in (("cancel_1_then", 1), ("cancel_9_then", 9)):
        w, k = new(name), next(row)
        a.setdefault(k, []).extend([(w, v), (w, R - v), (w, 4)])
        b.setdefault(k, []).extend([(w, v), (w, R - v), (w, R - 1)])
    _rows(d, n, a, b, c)
    return _finish("meetings", d, wire, 2, wire["twice_5"], [wire["ab_1_committed"], wire["twice_big"], wire["cancel_9_then"]])


# ---------------------------------------------------------------------------------------------------------------------
# the smallest domain
# ---------------------------------------------------------------------------------------------------------------------
def smallest():
    """two constraints, domain_log 1: one Z point, one stage, logn - 1 == 0 in the pass kernel's shifts"""
    rng = random.Random(0x5317)
    d = Desc(1, 0)
    wire = {"one": 0, "public": 1, "challenge": d.new_wire(), "committed": d.new_wire(), "private": d.new_wire()}
    big = [rng.randrange(1, R) for _ in range(2)]
    d.row([(0, 1), (1, 2), (4, R - 3)], [(2, 5), (3, 1)], [(4, 1), (3, 7)])
    d.row([(3, big[0]), (2, R - 1)], [(4, big[1]), (1, 1)], [(2, 1), (0, 1 << 32)])
    return _finish("smallest", d, wire, 2, wire["challenge"], [wire["committed"]])


GENERATORS = {"coeff_kinds": coeff_kinds, "column_shapes": column_shapes, "meetings": meetings, "smallest": smallest}
