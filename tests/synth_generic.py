"""Synthetic circuits that carry the generic solver instructions (OP_SOLVE_ROW, OP_LIMBS, OP_COUNTN of csrc/circuit.hpp), built on
synth_circuits.Desc / write_sppc, for the cooperative solver's planner and kernel.

Besides the generators: `model`, a big-integer execution of a program with the instructions 1, 12 .. 15 written from the comments
in csrc/circuit.hpp (not from the kernels), and `twin`, the all-inputs container of the same rows (every wire an input, program =
the commitment step) through which oracle.native sets up and proves the same statement: the oracle does not know the instructions
13 .. 18.  A generator returns a synth_circuits.Synth whose `expect` names the generic rows and divisions it was built with."""
import random

import synth_circuits as S
from synth_circuits import R, OP_END, OP_SOLVE_C, OP_COMMIT, OP_MASK

OP_SOLVE_ROW, OP_LIMBS, OP_COUNTN = 13, 14, 15
NONE32 = 0xFFFFFFFF
LIMBS_REVERSED = 1 << 31
OP_LEN = dict(S.OP_LEN)
OP_LEN.update({OP_SOLVE_ROW: 5, OP_LIMBS: 5, OP_COUNTN: 5})


class GDesc(S.Desc):
    """Desc plus the generic instructions.  An OP_SOLVE_ROW names coefficients (1 / cf, the inverse of a constant other factor) by
    their index in the container's table, which write_sppc fills in order of first appearance in A, B, C, H: the values are parked
    in a hint row no instruction reads, and `finish` turns the values into indices."""

    def __init__(self, n_pub_inputs, n_secret):
        super().__init__(n_pub_inputs, n_secret)
        self._fix = []                    # (program position, coefficient value)
        self.generic_rows = self.generic_divs = 0

    def _coef(self, value):
        self._fix.append((len(self.program), value % R))
        self.program.append(0)

    def solve_row(self, side, mine, other, third, cf=1):
        """One row solved for a fresh wire `out`, the last term (coefficient cf) of side `side` (0 A, 1 B, 2 C).
        side 2: mine = the rest of C, other / third = A / B:  out = (<A><B> - <rest>) / cf
        side 0: mine = the rest of A, other = B, third = C:   out = (<C> / <B> - <rest>) / cf      (side 1: A and B swapped)
        An `other` made of wire-0 terms alone is a constant: its inverse goes into the instruction; else it is inverted at run time."""
        out = self.new_wire()
        mine = list(mine) + [(out, cf)]
        if side == 2:
            k = self.row(other, third, mine)
        elif side == 0:
            k = self.row(mine, other, third)
        else:
            k = self.row(other, mine, third)
        self.program += [OP_SOLVE_ROW, k, side]
        if cf % R == 1:
            self.program.append(NONE32)
        else:
            self._coef(pow(cf, -1, R))
        constant = side != 2 and all(w == 0 for w, _ in other)
        if constant:
            self._coef(pow(sum(v for _, v in other) % R, -1, R))
        else:
            self.program.append(NONE32)
            self.generic_divs += side != 2
        self.generic_rows += 1
        return out

    def limbs(self, form, n, width, reversed_=False):
        h, out0 = self.hrow(form), self.new_wire(n)
        self.program += [OP_LIMBS, h, n, width | (LIMBS_REVERSED if reversed_ else 0), out0]
        return out0

    def countn(self, forms, size):
        h0 = len(self.H)
        for f in forms:
            self.hrow(f)
        out0 = self.new_wire(size)
        self.program += [OP_COUNTN, h0, len(forms), out0, size]
        return out0

    def finish(self):
        if self._fix:
            self.hrow([(0, v) for _, v in self._fix])          # parks the values in the coefficient table
        index, n = {}, 0
        for m in (self.A, self.B, self.C, self.H):
            for terms in m:
                for _, v in terms:
                    if v not in index:
                        index[v] = n
                        n += 1
        for pos, v in self._fix:
            self.program[pos] = index[v]
        return super().finish()


def instructions(desc):
    pc = 0
    while desc.program[pc] != OP_END:
        yield pc, desc.program[pc]
        pc += OP_LEN[desc.program[pc]]


def coefficient_table(desc):
    """the container's coefficient table as write_sppc lays it out"""
    seen, table = set(), []
    for m in (desc.A, desc.B, desc.C, desc.H):
        for terms in m:
            for _, v in terms:
                if v not in seen:
                    seen.add(v)
                    table.append(v)
    return table


def model(desc, inputs, challenge=None, rs=(0, 0), stop_at_commit=False):
    """Every wire from the inputs, instruction by instruction, in Python integers.  challenge: the value of the challenge wire, set
    at the commitment boundary (None: 0)."""
    from oracle import circuit as C
    coeffs = coefficient_table(desc)
    w = [0] * desc.n_wires
    w[0] = 1
    for i, v in enumerate(inputs):
        w[1 + i] = v % R

    def dot(terms):
        return sum(v * w[x] for x, v in terms) % R

    def inv0(v):
        return pow(v, -1, R) if v % R else 0
    pr = desc.program
    for pc, op in instructions(desc):
        if op == OP_SOLVE_C:
            k = pr[pc + 1]
            w[desc.C[k][-1][0]] = (dot(desc.A[k]) * dot(desc.B[k]) - dot(desc.C[k][:-1])) % R
        elif op == OP_SOLVE_ROW:
            k, side, inv_ci, odiv_ci = pr[pc + 1:pc + 5]
            sides = (desc.A[k], desc.B[k], desc.C[k])
            out, cf = sides[side][-1]
            rest = dot(sides[side][:-1])
            if side == 2:
                v = dot(desc.A[k]) * dot(desc.B[k]) - rest
            else:
                other = dot(sides[1 - side])
                oi = coeffs[odiv_ci] if odiv_ci != NONE32 else inv0(other)      # a zero factor gives 0
                v = dot(desc.C[k]) * oi - rest
            if inv_ci != NONE32:
                assert coeffs[inv_ci] * cf % R == 1
                v *= coeffs[inv_ci]
            w[out] = v % R
        elif op == OP_LIMBS:
            h, n, width_w, out0 = pr[pc + 1:pc + 5]
            width, rev = width_w & 0x7FFFFFFF, width_w >> 31
            v = dot(desc.H[h])
            for i in range(n):
                w[out0 + (n - 1 - i if rev else i)] = (v >> (i * width)) & ((1 << width) - 1)
        elif op == OP_COUNTN:
            h0, n, out0, size = pr[pc + 1:pc + 5]
            for j in range(size):
                w[out0 + j] = 0
            for i in range(n):
                v = dot(desc.H[h0 + i])
                if v < size:
                    w[out0 + v] += 1
        elif op == OP_MASK:
            w[pr[pc + 1]] = C.mask_value(*rs)
        elif op == OP_COMMIT:
            if stop_at_commit:
                return w
            w[desc.challenge_wire] = 0 if challenge is None else challenge % R
        else:
            raise ValueError(op)
    return w


def twin(desc):
    """the same rows with every wire an input: the program is the commitment step alone"""
    t = S.Desc(desc.n_public - 1, desc.n_wires - desc.n_public)
    t.A, t.B, t.C = [list(r) for r in desc.A], [list(r) for r in desc.B], [list(r) for r in desc.C]
    t.H = [list(r) for r in desc.H]                    # the same coefficient table, so the same container but for the program
    t.committed, t.challenge_wire = list(desc.committed), desc.challenge_wire
    t.program = [OP_COMMIT]
    t.finish()
    assert (t.n_wires, t.n_constraints, t.domain_log) == (desc.n_wires, desc.n_constraints, desc.domain_log)
    return t


# ---------------------------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------------------------
N_IN = 8


def _make(name, body, n_in=N_IN, small_inputs=None, zero_rows=()):
    """body(d, v, rng) -> the wire tied to the public input; small_inputs(rng) -> the secret inputs where random field elements will
    not do; zero_rows: the rows built to stay unsatisfied (a zero divisor)"""
    rng = random.Random(sum(map(ord, name)))
    d = GDesc(1, n_in)
    v = [d.sec(i) for i in range(n_in)]
    tie_src = body(d, v, rng)
    tie = S._tie(d, tie_src)
    d.commit(v[:2], v[0])
    d.finish()

    def inputs(seed, **kw):
        r = random.Random(seed)
        vals = small_inputs(r, **kw) if small_inputs else [r.randrange(1, R) for _ in range(n_in)]
        w = model(d, [0] + vals, stop_at_commit=True)
        return [w[tie_src]] + vals

    def spoil(row):
        return [(row[0] + 1) % R] + row[1:], tie
    return S.Synth(name, d, inputs, spoil, {"generic_rows": d.generic_rows, "generic_divs": d.generic_divs, "zero_rows": tuple(zero_rows)})


def _base_chain(d, v, rng, n=8):
    cur = v[0]
    for j in range(n):
        cur = d.solve_row(2, [(v[(j + 1) % len(v)], j + 2)], [(cur, 1), (0, j + 1)], [(v[(j + 2) % len(v)], 1)], cf=1 if j % 2 else j + 3)
    return cur


def _tail_chain(d, v, cur, n=7):
    """n more rows behind `cur`: with it a run long enough for the level planner, fed by the hints in front of it"""
    for j in range(n):
        cur = d.solve_row(j % 3, [(v[j % len(v)], 1)], [(0, j + 2)] if j % 2 else [(cur, 1), (v[1], 1)], [(cur, 1), (0, j + 1)], cf=j + 1)
    return cur


def gen_sides():
    """one row of each side, cf = 1 and cf != 1, the other factor a constant and a form inverted at run time: ten dependent rows"""
    def body(d, v, rng):
        cur = v[0]
        for cf in (1, 7):
            cur = d.solve_row(2, [(v[1], 3)], [(cur, 1), (v[2], 1)], [(v[3], 5), (0, 2)], cf=cf)
        for side in (0, 1):
            for cf in (1, rng.randrange(2, R)):
                for other in ([(0, 9)], [(cur, 1), (v[4], 2)]):
                    cur = d.solve_row(side, [(v[5], 4), (0, 1)], other, [(cur, 3), (v[6], 1)], cf=cf)
        return cur
    return _make("sides", body)


def gen_chain(n=40):
    """a chain of n dependent rows: levels of one row, the sides in turn, every third division at run time"""
    def body(d, v, rng):
        cur = v[0]
        for j in range(n):
            side = j % 3
            if side == 2:
                cur = d.solve_row(2, [(v[j % 8], j + 1)], [(cur, 1), (0, 1)], [(cur, rng.randrange(R)), (v[(j + 3) % 8], 1)], cf=1 + j % 2)
            else:
                other = [(v[(j + 1) % 8], 1), (cur, 1)] if j % 2 else [(0, j + 2)]
                cur = d.solve_row(side, [(v[(j + 2) % 8], 1)], other, [(cur, 1), (0, 5)], cf=1 if j % 4 else 11)
        return cur
    return _make("chain%d" % n, body)


def gen_level(n):
    """one level of n independent rows behind the base chain (64: one pass of the wave at one lane per row; 65: a second pass)"""
    def body(d, v, rng):
        base = _base_chain(d, v, rng)
        outs = []
        for j in range(n):
            if j % 4 == 3:        # (every row reads the chain's end, so that the n rows are a level of their own)
                outs.append(d.solve_row(0, [(v[j % 8], 1)], [(0, j + 2)], [(v[(j + 1) % 8], 1), (base, 1)], cf=j + 2))
            else:
                outs.append(d.solve_row(2, [], [(v[j % 8], 1), (base, 1)], [(v[(j + 1) % 8], j + 2)]))
        # one row that reads them all, so that a wrong value anywhere reaches the tied wire
        return d.solve_row(2, [(base, 1)], [(o, j + 1) for j, o in enumerate(outs)], [(0, 1)])
    return _make("level%d" % n, body)


def gen_mixed():
    """a run that mixes OP_SOLVE_C and OP_SOLVE_ROW: a dependent chain that alternates, and four independent rows of each kind"""
    def body(d, v, rng):
        cur = v[0]
        for j in range(12):
            if j % 2:
                cur = d.solve_c([(cur, 1), (v[1], -1)], [(cur, 1), (v[1], -1)] if j % 4 == 1 else [(v[2], j)], [(v[3], 1)])
            else:
                cur = d.solve_row(j % 3, [(v[4], 1)], [(cur, 1), (v[5], 1)], [(cur, 2), (0, 3)], cf=j + 1)
        side = [d.solve_c([(v[j], 1)], [(v[j + 1], 1)]) for j in range(4)] + \
               [d.solve_row(1, [], [(0, 4)], [(v[j], 1), (cur, 1)]) for j in range(4)]
        return d.solve_c([(o, j + 1) for j, o in enumerate(side)], [(cur, 1)])
    return _make("mixed", body)


def gen_divs(n, zeros=()):
    """n independent rows out_i * (x_i - y_i) = z_i solved for out_i (side 0, divisor inverted at run time) in front of the base
    chain: one level holds the n divisions and the chain's first row.  `zeros`: the rows whose divisor the inputs make zero; they
    get 0 and, z_i being non-zero, stay unsatisfied."""
    def body(d, v, rng):
        outs = [d.solve_row(0, [], [(v[3 * i], 1), (v[3 * i + 1], -1)], [(v[3 * i + 2], 1)]) for i in range(n)]
        base = _base_chain(d, v, rng)
        return d.solve_row(2, [(base, 1)], [(o, i + 1) for i, o in enumerate(outs)], [(0, 1)])

    def vals(r):
        out = []
        for i in range(n):
            x = r.randrange(1, R)
            y = x if i in zeros else (x + r.randrange(1, R - 1)) % R
            out += [x, y, r.randrange(1, R)]
        return out + [r.randrange(1, R) for _ in range(max(0, N_IN - 3 * n))]
    name = "divs%d%s" % (n, "_zero" if zeros else "")
    return _make(name, body, n_in=max(N_IN, 3 * n), small_inputs=vals, zero_rows=zeros)


def gen_longrow():
    """a component of 32 rows whose last row has 600 terms -- its record fits no chunk, the component takes the table form --
    beside an independent component of 32 rows that is streamed"""
    def body(d, v, rng):
        a = v[0]
        for j in range(31):
            a = d.solve_row(2 if j % 2 else 0, [(v[1], j + 1)], [(a, 1), (v[2], 1)], [(a, 1), (0, 2)] if j % 2 == 0 else [(v[3], 1)], cf=j + 2)
        big = d.solve_row(2, [(v[i % 8], rng.randrange(R)) for i in range(598)], [(a, 1)], [(v[4], 1)], cf=5)
        b = v[5]
        for j in range(32):
            b = d.solve_row(2, [(v[6], 1)], [(b, 1), (0, j + 1)], [(b, 1), (v[7], 1)])
        d.row([(b, 1)], [(0, 1)], [(b, 1)])          # (no solved row joins the two: they stay components of their own)
        return big
    return _make("longrow", body)


def gen_limbs():
    """six OP_LIMBS in a row (one per lane): widths 64 (four limbs), 128 and 128 reversed (two limbs), twice over; every value is put
    together again by a row"""
    def body(d, v, rng):
        base = _base_chain(d, v, rng)
        srcs = [v[1], v[2], v[3], base, v[4], v[5]]
        outs = []
        for j, src in enumerate(srcs):
            width, n, rev = ((64, 4, False), (128, 2, False), (128, 2, True))[j % 3]
            outs.append((d.limbs([(src, 1), (0, j)], n, width, rev), n, width, rev, src, j))
        for o, n, width, rev, src, j in outs:
            d.row([(o + (n - 1 - i if rev else i), 1 << (width * i)) for i in range(n)], [(0, 1)], [(src, 1), (0, j)])
        return _tail_chain(d, v, d.solve_row(2, [(base, 1)], [(o, 1) for o, *_ in outs] + [(o + 1, 3) for o, *_ in outs], [(0, 1)]))
    return _make("limbs", body)


def gen_countn(nq=426, size=64):
    """OP_COUNTN: nq queries over the table 0 .. size - 1; the inputs are small, so most queries v_i + c fall inside, those with a large
    c and the negated ones outside"""
    def body(d, v, rng):
        base = _base_chain(d, v, rng)
        forms = []
        for i in range(nq):
            if i % 17 == 5:
                forms.append([(v[i % 8], -1), (0, -1)])              # R - 1 - v: outside
            else:
                forms.append([(v[i % 8], 1), (0, i % 23)])           # up to 40 + 22: the top ones outside
        cnt = d.countn(forms, size)
        return _tail_chain(d, v, d.solve_row(2, [(base, 1)], [(cnt + j, j + 1) for j in range(size)], [(0, 1)]))

    def vals(r):
        return [r.randrange(0, 48) for _ in range(N_IN)]
    return _make("countn", body, small_inputs=vals)


def gen_tracks():
    """two independent components of 40 rows each in one run: more than one track is in use"""
    def body(d, v, rng):
        a, b = v[0], v[1]
        for j in range(40):
            a = d.solve_row(2, [(v[2], 1)], [(a, 1), (0, j + 1)], [(a, 1), (v[3], 1)], cf=j % 3 + 1)
            b = d.solve_row(j % 2, [(v[4], 1)], [(b, 1), (v[5], 1)] if j % 5 == 0 else [(0, j + 2)], [(b, 3), (0, 1)])
        d.row([(b, 1)], [(0, 1)], [(b, 1)])
        return a
    return _make("tracks", body)


CASES = {
    "sides": gen_sides,
    "chain40": gen_chain,
    "level64": lambda: gen_level(64),
    "level65": lambda: gen_level(65),
    "mixed": gen_mixed,
    "divs1": lambda: gen_divs(1),
    "divs64": lambda: gen_divs(64),
    "divs65": lambda: gen_divs(65),
    "divs70_zero": lambda: gen_divs(70, zeros=(0, 63, 69)),
    "longrow": gen_longrow,
    "limbs": gen_limbs,
    "countn": gen_countn,
    "tracks": gen_tracks,
}
