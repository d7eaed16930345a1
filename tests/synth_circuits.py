"""Synthetic circuits for the load-time planners: a writer of the SPPC container (version 2, the layout oracle/circuit.py reads),
generators that put a circuit on one side of a planning threshold, and a restatement in Python of what the planners should make
of a circuit (`plan_model`), so that a generator that drifts off its threshold fails on the CPU.

A generator returns a `Synth`: the circuit description (`desc`), `inputs(seed)` -> a satisfying input row (public then secret),
`spoil(row)` -> (a row that breaks exactly one constraint, that constraint), and `expect`: the plan facts the circuit is built to
have, each named after the threshold it sits on.  Expected witnesses and proofs never come from here: the tests take them from
oracle.circuit.solve and oracle.native.

The planning constants are restated from the planners' documentation, not imported from the code under test."""
import random
import struct

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
(OP_END, OP_SOLVE_C, OP_SOLVE_A, OP_BATCH_DIV, OP_BITS, OP_LIMBS8, OP_COUNT8, OP_POSEIDON, OP_POSEIDON2, OP_COMMIT, OP_GRUMPKIN,
 OP_INV_H, OP_MASK) = range(13)
OP_LEN = {OP_SOLVE_C: 2, OP_SOLVE_A: 2, OP_MASK: 2, OP_BATCH_DIV: 3, OP_INV_H: 3, OP_COUNT8: 4, OP_BITS: 4, OP_LIMBS8: 4, OP_COMMIT: 1}
CIRCUIT_SYNTH = 100                    # neither withdraw (1) nor audit (2): the generic batch entry points are under test

# the thresholds under test
SMALL_ROW_MIN, SMALL_ROW_REST, LONG_ROW_MIN = 64, 32, 512
SMALL_COEF_LIMIT = 1 << 30             # |coefficient| below this is "small"
LOOKUP_CST_MAX = 32000
RUN_MAX = 8                            # constraints per run of identical B rows
ROWS_KERNEL_LANES = 65536              # n_runs * P below this: 16 lanes per row
WIDE_DIV_MIN = 64
DIV_WAVE_MAX = 16384                   # n * P up to this: one division per lane
DIV_BIG_CHUNK_P = 256                  # P from this on: chunks of 32, below: chunks of 4
COOP_CHUNK = 1024
COOP_RUN_MIN, COOP_COMPONENT_MIN, COOP_PAR_MIN, COOP_TRACKS = 8, 32, 4, 4


class Desc:
    """a circuit as Python data; rows are lists of (wire, coefficient as an int mod R)"""

    def __init__(self, n_pub_inputs, n_secret):
        self.id = CIRCUIT_SYNTH
        self.n_public = n_pub_inputs + 1           # with the constant one (wire 0)
        self.n_secret = n_secret
        self.n_wires = 1 + n_pub_inputs + n_secret
        self.A, self.B, self.C, self.H = [], [], [], []
        self.program = []
        self.committed = []
        self.challenge_wire = 0

    # ---- building ----
    def pub(self, i):
        return 1 + i

    def sec(self, i):
        return self.n_public + i

    def new_wire(self, n=1):
        w = self.n_wires
        self.n_wires += n
        return w

    def row(self, a, b, c):
        self.A.append([(w, v % R) for w, v in a])
        self.B.append([(w, v % R) for w, v in b])
        self.C.append([(w, v % R) for w, v in c])
        return len(self.A) - 1

    def hrow(self, terms):
        self.H.append([(w, v % R) for w, v in terms])
        return len(self.H) - 1

    def solve_c(self, a, b, c_rest=()):
        """out = <a,w> <b,w> - <c_rest,w>: the row with the output last on the C side (coefficient 1) and its instruction"""
        out = self.new_wire()
        k = self.row(a, b, list(c_rest) + [(out, 1)])
        self.program += [OP_SOLVE_C, k]
        return out

    def commit(self, wires, phase2_wire):
        """the commitment every shipped circuit carries: a mask wire with the row mask * 1 = mask, the committed list, the phase
        boundary, and one row that reads the challenge after it.  Returns the wire that row defines."""
        mask = self.new_wire()
        self.program += [OP_MASK, mask]
        self.row([(mask, 1)], [(0, 1)], [(mask, 1)])
        self.committed = sorted(set(list(wires) + [mask]))
        self.program += [OP_COMMIT]
        self.challenge_wire = self.new_wire()
        return self.solve_c([(self.challenge_wire, 1)], [(phase2_wire, 1)])

    def finish(self):
        self.program += [OP_END]
        self.n_constraints = len(self.A)
        self.domain_log = max(1, (self.n_constraints - 1).bit_length())
        return self

    def n_inputs(self):
        return self.n_public - 1 + self.n_secret


def write_sppc(desc, path):
    """the container, field by field as Circuit.__init__ of the oracle reads it"""
    index, coeffs = {}, []

    def cid(v):
        if v not in index:
            index[v] = len(coeffs)
            coeffs.append(v)
        return index[v]

    def sparse(rows):
        rowptr, flat = [0], []
        for terms in rows:
            for w, v in terms:
                flat += [w, cid(v)]
            rowptr.append(len(flat) // 2)
        return struct.pack("<2I", len(rows), len(flat) // 2) + struct.pack("<%dI" % len(rowptr), *rowptr) + struct.pack("<%dI" % len(flat), *flat)
    mats = [sparse(m) for m in (desc.A, desc.B, desc.C, desc.H)]
    head = struct.pack("<13I", 0x43505053, 2, desc.id, desc.n_public, desc.n_secret, desc.n_wires, desc.n_constraints, desc.domain_log,
                       desc.challenge_wire, len(coeffs), len(desc.committed), len(desc.program), 0)
    body = b"".join(v.to_bytes(32, "little") for v in coeffs) + b"".join(mats) + \
        struct.pack("<%dI" % len(desc.committed), *desc.committed) + struct.pack("<%dI" % len(desc.program), *desc.program)
    with open(path, "wb") as f:
        f.write(head + body)


def instructions(desc):
    """(pc, opcode) of every instruction of the program"""
    pc = 0
    while desc.program[pc] != OP_END:
        yield pc, desc.program[pc]
        pc += OP_LEN[desc.program[pc]]


class Synth:
    def __init__(self, name, desc, inputs, spoil, expect):
        self.name, self.desc, self.inputs, self.spoil, self.expect = name, desc, inputs, spoil, expect


# ---------------------------------------------------------------------------------------------------------------------
# what the planners should make of a circuit
# ---------------------------------------------------------------------------------------------------------------------
def small_signed(v):
    v %= R
    if v < SMALL_COEF_LIMIT:
        return v
    if R - v < SMALL_COEF_LIMIT:
        return -(R - v)
    return None


def lookup_wires(desc):
    """{wire: cst} of the looked-up values of OP_COUNT8 that name one wire (coefficient 1) plus a small constant"""
    out = {}
    pc = 0
    pr = desc.program
    while pr[pc] != OP_END:
        if pr[pc] == OP_COUNT8:
            for h in range(pr[pc + 1], pr[pc + 1] + pr[pc + 2]):
                wire, nw, cst, ok = 0, 0, 0, True
                for w, v in desc.H[h]:
                    s = small_signed(v)
                    if s is None:
                        ok = False
                    elif w == 0:
                        cst += s
                    elif s == 1:
                        wire, nw = w, nw + 1
                    else:
                        ok = False
                if ok and nw == 1 and -LOOKUP_CST_MAX <= cst <= LOOKUP_CST_MAX and wire not in out:
                    out[wire] = cst
        pc += OP_LEN[pr[pc]]
    return out


def plan_model(desc, small_sum_bound=1 << 63):
    """The plan facts of spp_circuit_plan_stats, from the description and the documented thresholds alone.
    small_sum_bound: a row is summed as integers only if sum |coefficient| * max |slot value| stays below it (None: no such rule)."""
    st = {}
    nc = desc.n_constraints
    runs, length = 0, 0
    for k in range(nc):
        if k == 0 or length >= RUN_MAX or not desc.B[k] or desc.B[k] != desc.B[k - 1]:
            runs, length = runs + 1, 0
        length += 1
    st["n_runs"] = runs
    st["max_row_terms"] = max([len(r) for m in (desc.A, desc.B, desc.C) for r in m] + [0])
    lk = lookup_wires(desc)
    slots = dict(lk)
    slots[0] = None
    sm, lg = 0, 0
    small_flag = set()
    if lk:
        for mi, m in enumerate((desc.A, desc.B, desc.C)):
            for k, terms in enumerate(m):
                if len(terms) < SMALL_ROW_MIN or len(terms) > 1 << 20:
                    continue
                q = [(w, small_signed(v)) for w, v in terms if w in slots and small_signed(v) is not None]
                if len(q) < SMALL_ROW_MIN or len(terms) - len(q) > SMALL_ROW_REST:
                    continue
                if small_sum_bound is not None:
                    tot = sum(abs(s) * (1 if w == 0 else max(abs(lk[w]), abs(255 - lk[w]))) for w, s in q)
                    if tot >= small_sum_bound:
                        continue
                sm += 1
                small_flag.add((mi, k))
    for mi, m in enumerate((desc.A, desc.B, desc.C)):
        for k, terms in enumerate(m):
            if len(terms) > LONG_ROW_MIN and (mi, k) not in small_flag:
                lg += 1
    st["sm_nrows"], st["sm_nslots"], st["lg_n"] = sm, (len(lk) + 1 if sm else 0), lg
    # the schedule: wide steps cut the program into sequential stretches
    pr = desc.program
    stretches, seg, pc = [], 0, 0
    st["max_wide_div"] = st["wide_steps"] = st["wide_divs"] = 0
    while pr[pc] != OP_END:
        op, n = pr[pc], OP_LEN[pr[pc]]
        wide = (op == OP_BATCH_DIV and pr[pc + 2] >= WIDE_DIV_MIN) or op == OP_COUNT8 or op == OP_COMMIT
        if wide:
            if pc > seg:
                stretches.append((seg, pc))
            seg = pc + n
            if op != OP_COMMIT:
                st["wide_steps"] += 1
            if op == OP_BATCH_DIV:
                st["wide_divs"] += 1
                st["max_wide_div"] = max(st["max_wide_div"], pr[pc + 2])
        pc += n
    if pc > seg:
        stretches.append((seg, pc))
    items = {"seq": 0, "par": 0, "levels": 0, "level_stream": 0}
    chunks_total, tracks = 0, 0
    for a, b in stretches:
        its, c = _coop_items(desc, a, b)
        chunks_total += c
        for kind, _, _, _ in its:
            items[kind] += 1
        tracks = max(tracks, _tracks(its))
    st["items_seq"], st["items_par"], st["items_levels"], st["items_level_stream"] = items["seq"], items["par"], items["levels"], items["level_stream"]
    st["stream_chunks"], st["tracks"] = chunks_total, tracks
    return st


# the facts the device's plan must share with this model; the number of sequential items and the dealing over tracks follow from
# cost weights and are asserted only where a generator names them (`expect`)
PLAN_KEYS = ("n_runs", "max_row_terms", "sm_nrows", "sm_nslots", "lg_n", "max_wide_div", "wide_steps", "wide_divs", "items_par",
             "items_levels", "items_level_stream", "stream_chunks")


def record_words(desc, k):
    """words of one row's record in the level stream: 4 + 2 per term (a square row carries its B side only, C without the output)"""
    na = 0 if desc.A[k] == desc.B[k] else len(desc.A[k])
    return 4 + 2 * (na + len(desc.B[k]) + len(desc.C[k]) - 1)


def level_words(desc, rows):
    """words of a level record that holds `rows`: 2 + one offset word and one record per row"""
    return 2 + sum(1 + record_words(desc, k) for k in rows)


def run_levels(desc, rows):
    """dependency level of every row of a run of OP_SOLVE_C rows: 0 for a row that reads no wire written earlier in the run, else
    1 + the highest level among the rows that write one of its inputs"""
    level_of, lev = {}, []
    for k in rows:
        lv = max([level_of[w] for w in _row_reads(desc, k) if w in level_of] + [0])
        level_of[desc.C[k][-1][0]] = lv + 1
        lev.append(lv)
    return lev


def sublevel_lanes(desc, rows):
    """(rows, lanes per row) of every sub-level of a run that forms one component: a level is cut where its record would pass
    COOP_CHUNK - 1 words; lanes double while below 16, below the longest linear form of the sub-level, and rows x 2 x lanes <= 64"""
    lev = run_levels(desc, rows)
    out = []
    for lv in sorted(set(lev)):
        mine = [k for k, l in zip(rows, lev) if l == lv]
        i = 0
        while i < len(mine):
            words, sub = 2, []
            while i < len(mine) and words + 1 + record_words(desc, mine[i]) <= COOP_CHUNK - 1:
                words += 1 + record_words(desc, mine[i])
                sub.append(mine[i])
                i += 1
            assert sub, "a row no chunk holds"
            longest = max([1] + [n for k in sub for n in (0 if desc.A[k] == desc.B[k] else len(desc.A[k]), len(desc.B[k]), len(desc.C[k]) - 1)])
            g = 1
            while g < 16 and g < longest and len(sub) * g * 2 <= 64:
                g *= 2
            out.append((len(sub), g))
    return out


def _row_reads(desc, k, solve_c=True):
    rd = [w for w, _ in desc.A[k]] + [w for w, _ in desc.B[k]] + [w for w, _ in (desc.C[k][:-1] if solve_c else desc.C[k])]
    return rd


def _op_rw(desc, pc):
    """(wires read, wires written, uses the scratch rows) of the instruction at pc"""
    pr = desc.program
    op = pr[pc]
    if op == OP_SOLVE_C:
        return _row_reads(desc, pr[pc + 1]), [desc.C[pr[pc + 1]][-1][0]], False
    if op in (OP_SOLVE_A, OP_BATCH_DIV):
        ks = [pr[pc + 1]] if op == OP_SOLVE_A else range(pr[pc + 1], pr[pc + 1] + pr[pc + 2])
        rd, wr = [], []
        for k in ks:
            rd += [w for w, _ in desc.B[k]] + [w for w, _ in desc.C[k]]
            wr.append(desc.A[k][0][0])
        return rd, wr, True
    if op in (OP_BITS, OP_LIMBS8):
        return [w for w, _ in desc.H[pr[pc + 1]]], list(range(pr[pc + 3], pr[pc + 3] + pr[pc + 2])), False
    if op == OP_INV_H:
        return [w for w, _ in desc.H[pr[pc + 1]]], [pr[pc + 2]], False
    if op == OP_MASK:
        return [], [pr[pc + 1]], False
    raise ValueError(op)


def _coop_items(desc, a, b):
    """items (kind, reads, writes, scratch) of the sequential stretch [a, b) and the chunks of level stream they take"""
    pr = desc.program
    its, chunks = [], 0
    seq0 = pc = a

    def flush(end):
        if end > seq0:
            rd, wr, scr = [], [], False
            q = seq0
            while q < end:
                r, w, s = _op_rw(desc, q)
                rd, wr, scr = rd + r, wr + w, scr or s
                q += OP_LEN[pr[q]]
            its.append(("seq", rd, wr, scr))
    while pc < b:
        op = pr[pc]
        if op == OP_SOLVE_C:
            e = pc
            while e < b and pr[e] == OP_SOLVE_C:
                e += 2
            ks = [pr[q + 1] for q in range(pc, e, 2)]
            if len(ks) < COOP_RUN_MIN:
                pc = e
                continue
            flush(pc)
            level_of, writer, lev = {}, {}, []
            parent = list(range(len(ks)))

            def find(x):
                while parent[x] != x:
                    parent[x] = parent[parent[x]]
                    x = parent[x]
                return x
            for i, k in enumerate(ks):
                lv = 0
                for w in _row_reads(desc, k):
                    if w in level_of:
                        lv = max(lv, level_of[w])
                        ra, rb = find(i), find(writer[w])
                        if ra != rb:
                            parent[ra] = rb
                out = desc.C[k][-1][0]
                level_of[out], writer[out] = lv + 1, i
                lev.append(lv)
            size = {}
            for i in range(len(ks)):
                size[find(i)] = size.get(find(i), 0) + 1
            comps = []
            for i in range(len(ks)):
                r = find(i)
                if size[r] >= COOP_COMPONENT_MIN and r not in comps:
                    comps.append(r)
            if any(size[find(i)] < COOP_COMPONENT_MIN for i in range(len(ks))):
                comps.append(None)
            for cid in comps:
                mine = [i for i in range(len(ks)) if (find(i) == cid if cid is not None else size[find(i)] < COOP_COMPONENT_MIN)]
                by_level = {}
                for i in mine:
                    by_level.setdefault(lev[i], []).append(ks[i])
                used, nchunks, fits = 0, 0, True
                for lv in sorted(by_level):
                    rows, i = by_level[lv], 0
                    while i < len(rows) and fits:
                        words, cnt = 2, 0
                        while i < len(rows) and words + 1 + record_words(desc, rows[i]) <= COOP_CHUNK - 1:
                            words += 1 + record_words(desc, rows[i])
                            i, cnt = i + 1, cnt + 1
                        if cnt == 0:
                            fits = False
                            break
                        if used and used + words > COOP_CHUNK - 1:
                            nchunks, used = nchunks + 1, 0
                        used += words
                    if not fits:
                        break
                if used:
                    nchunks += 1
                rd = [w for i in mine for w in _row_reads(desc, ks[i])]
                wr = [desc.C[ks[i]][-1][0] for i in mine]
                if fits:
                    chunks += nchunks
                    its.append(("level_stream", rd, wr, False))
                else:
                    its.append(("levels", rd, wr, False))
            pc = seq0 = e
        elif op in (OP_BITS, OP_LIMBS8, OP_INV_H):
            e, written, group = pc, set(), []
            while e < b and pr[e] in (OP_BITS, OP_LIMBS8, OP_INV_H):
                rd, wr, _ = _op_rw(desc, e)
                if any(w in written for w in rd):
                    break
                written.update(wr)
                group.append(e)
                e += OP_LEN[pr[e]]
            if len(group) < COOP_PAR_MIN:
                pc = e if group else pc + OP_LEN[op]
                continue
            flush(pc)
            rd, wr = [], []
            for q in group:
                r, w, _ = _op_rw(desc, q)
                rd, wr = rd + r, wr + w
            its.append(("par", rd, wr, False))
            pc = seq0 = e
        else:
            pc += OP_LEN[op]
    flush(b)
    return its, chunks


def _tracks(its):
    """tracks in use: independent components of the items, those that use the scratch rows together on track 0, the others dealt
    over the tracks; with c components without scratch use and any number with, min(4, ...) tracks are in use"""
    n = len(its)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    writer = {}
    for i, (_, rd, wr, _) in enumerate(its):
        for w in rd:
            if w in writer:
                ra, rb = find(i), find(writer[w])
                if ra != rb:
                    parent[ra] = rb
        for w in wr:
            writer[w] = i
    roots = {find(i) for i in range(n)}
    scratch = {find(i) for i in range(n) if its[i][3]}
    free = len(roots - scratch)
    # with scratch users track 0 starts loaded: the free components go to the emptier tracks first
    return min(COOP_TRACKS, (1 if scratch else 0) + free)


# ---------------------------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------------------------
def _tie(d, wire, pub_index=0):
    """wire * 1 = public input: the constraint a spoiled public input breaks, alone"""
    return d.row([(wire, 1)], [(0, 1)], [(d.pub(pub_index), 1)])


def gen_tiny():
    """five constraints (domain 2^3), one committed wire (the mask alone), a square row"""
    d = Desc(1, 1)
    x = d.sec(0)
    y = d.solve_c([(x, 1)], [(x, 1)])
    tie = _tie(d, y)
    z = d.commit([], x)
    d.solve_c([(z, 1), (y, 1)], [(x, 1)])
    d.finish()

    def inputs(seed):
        v = random.Random(seed).randrange(R)
        return [v * v % R, v]

    def spoil(row):
        return [(row[0] + 1) % R] + row[1:], tie
    return Synth("tiny", d, inputs, spoil, {"domain_log": 3, "n_committed": 1})


LOOKUP_CSTS = (0, 3, -32000, 32000)


def gen_rows(n_runs=260, with_1025=False, nl=64):
    """Row paths of the matrix evaluation.  `nl` input wires are looked up with offsets 0, +3, -32000, +32000 in turn (and are the
    committed wires: 65 with the mask), 40 input wires are general.  One row per case, each with a B row of its own unless it belongs
    to a run; filler rows bring the runs of identical B rows to `n_runs`."""
    ng = 40
    d = Desc(1, nl + ng)
    rng = random.Random(1234)
    L = [d.sec(i) for i in range(nl)]
    G = [d.sec(nl + i) for i in range(ng)]
    csts = [LOOKUP_CSTS[i % 4] for i in range(nl)]
    uniq = [2]

    def own_b():
        uniq[0] += 1
        return [(G[uniq[0] % ng], 1), (0, uniq[0])]

    def small_terms(n, coef=None):
        return [(L[i % nl], coef(i) if coef else rng.choice((-1, 1)) * rng.randrange(1, 1 << 28)) for i in range(n)]

    def wide_terms(n):
        return [(G[i % ng], rng.randrange(1 << 31, R - (1 << 31))) for i in range(n)]
    ex = {"small": 0, "long": 0}

    def case(side, terms, small=False, long=False):
        if side == "A":
            d.solve_c(terms, own_b())
        elif side == "B":
            d.solve_c(own_b(), terms)
        else:
            d.solve_c([(G[3], 1)], own_b(), terms)
        ex["small"] += small
        ex["long"] += long
    # the lookup and its range constraint: every looked-up value is counted iff it is a byte
    h0 = len(d.H)
    for i in range(nl):
        d.hrow([(L[i], 1)] + ([(0, csts[i])] if csts[i] else []))
    cnt0 = d.new_wire(256)
    d.program += [OP_COUNT8, h0, nl, cnt0]
    range_row = d.row([(cnt0 + j, 1) for j in range(256)], [(0, 1)], [(0, nl)])
    _tie(d, G[0])
    # SMALL_ROW_MIN: 63 / 64 / 65 qualifying terms on each side (a C row has the output as one other term)
    for side in "ABC":
        for n in (63, 64, 65):
            case(side, small_terms(n), small=n >= SMALL_ROW_MIN)
    # SMALL_ROW_REST: 64 qualifying terms and 32 / 33 others
    case("A", small_terms(64) + wide_terms(32), small=True)
    case("A", small_terms(64) + wide_terms(33))
    # the coefficient bound: +-(2^30 - 1) is small, +-2^30 is not (it counts as one of the others)
    top = SMALL_COEF_LIMIT - 1
    case("A", small_terms(64, lambda i: top if i % 2 else -top), small=True)
    case("A", small_terms(63) + [(L[5], SMALL_COEF_LIMIT)])
    case("A", small_terms(64, lambda i: top) + [(L[5], SMALL_COEF_LIMIT), (L[6], -SMALL_COEF_LIMIT)], small=True)
    # LONG_ROW_MIN: 512 / 513 terms, small and not small
    case("A", small_terms(512), small=True)
    case("A", small_terms(513), small=True)
    case("A", wide_terms(512))
    case("A", wide_terms(513), long=True)
    case("B", wide_terms(513), long=True)
    case("C", wide_terms(512), long=True)             # 513 terms with the output
    case("C", wide_terms(511))                        # 512 with the output
    if with_1025:
        case("A", wide_terms(1025), long=True)
    # a row with repeated wires, a row with no terms
    case("A", [(L[0], 5), (L[0], 7), (G[1], 3), (G[1], 4), (L[0], -2)])
    d.row([], [(G[2], 1)], [])
    # runs of identical B rows of length 1, 8, 9 and 17; the shared row general, small and long in turn
    for kind in ("general", "small", "long"):
        for length in (1, 8, 9, 17):
            shared = {"general": lambda: wide_terms(3), "small": lambda: small_terms(64), "long": lambda: wide_terms(513)}[kind]()
            for j in range(length):
                d.solve_c([(G[(7 * j + length) % ng], 1), (0, j + 1)], shared)
            ex["small"] += length if kind == "small" else 0
            ex["long"] += length if kind == "long" else 0
    phase2 = d.commit(L, L[0])
    # filler: rows with B rows of their own until the runs number n_runs
    d.n_constraints = len(d.A)
    have = plan_model_runs(d)
    assert have <= n_runs, (have, n_runs)
    for _ in range(n_runs - have):
        d.solve_c([(phase2, 1)], own_b())
    d.finish()

    def inputs(seed):
        r = random.Random(seed)
        lv = []
        for i in range(nl):
            lo = -csts[i]
            # both ends of [-cst, 255 - cst] on the first wires of every offset, random bytes elsewhere
            v = lo if i < 4 else lo + 255 if i < 8 else lo + r.randrange(256)
            lv.append(v % R)
        gv = [r.randrange(R) for _ in range(ng)]
        return [gv[0]] + lv + gv

    def spoil(row, wire=0, above=True):
        """lookup wire `wire` one step outside its range: only the range constraint can tell"""
        bad = list(row)
        bad[1 + wire] = ((255 - csts[wire] + 1) if above else (-csts[wire] - 1)) % R
        return bad, range_row
    name = "rows%d%s" % (n_runs, "_1025" if with_1025 else "")
    return Synth(name, d, inputs, spoil, {"n_runs": n_runs, "sm_nrows": ex["small"], "lg_n": ex["long"], "sm_nslots": nl + 1,
                                            "max_row_terms": 1025 if with_1025 else 513, "n_committed": nl + 1,
                                            "domain_log": 11 if n_runs > 512 else 9})


def plan_model_runs(desc):
    runs, length = 0, 0
    for k in range(len(desc.A)):
        if k == 0 or length >= RUN_MAX or not desc.B[k] or desc.B[k] != desc.B[k - 1]:
            runs, length = runs + 1, 0
        length += 1
    return runs


def gen_widest_small_row(nterms=1 << 18, n_runs=256):
    """The widest integer row the planner should admit: one A row of 2^18 terms on a -32000-offset lookup wire, coefficient
    2^30 - 1, with the wire's value near 32 255: the sum is (2^30 - 1) * 2^18 * 32255 = 0.984 * 2^63.  With 2^19 terms the sum
    passes 2^63 and the row must not be summed as integers.  Filler rows bring the runs to `n_runs`, so that 256 proofs take the
    run kernel, the only one that reads small rows."""
    nl = 2
    d = Desc(1, nl + 1)
    L = [d.sec(0), d.sec(1)]
    g = d.sec(2)
    h0 = len(d.H)
    d.hrow([(L[0], 1), (0, -32000)])
    d.hrow([(L[1], 1)])
    cnt0 = d.new_wire(256)
    d.program += [OP_COUNT8, h0, nl, cnt0]
    range_row = d.row([(cnt0 + j, 1) for j in range(256)], [(0, 1)], [(0, nl)])
    _tie(d, g)
    big_row = len(d.A)
    d.solve_c([(L[0], SMALL_COEF_LIMIT - 1)] * nterms, [(g, 1)])
    z = d.commit(L, L[1])
    d.n_constraints = len(d.A)
    for j in range(n_runs - plan_model_runs(d)):
        d.solve_c([(z, 1)], [(g, 1), (0, j + 2)])
    d.finish()

    def inputs(seed):
        r = random.Random(seed)
        v = 32255 - (seed % 3)                # at and just under the top of [32000, 32255]
        gv = r.randrange(R)
        return [gv, v, r.randrange(256), gv]

    def spoil(row):
        bad = list(row)
        bad[1] = 32256
        return bad, range_row
    fits = nterms * (SMALL_COEF_LIMIT - 1) * 32255 < 1 << 63        # else the row is no integer row: it is long
    return Synth("widest_small_row%d" % nterms, d, inputs, spoil, {"n_runs": n_runs, "sm_nrows": 1 if fits else 0, "lg_n": 0 if fits else 1,
                                                                    "max_row_terms": nterms, "sm_nslots": 3 if fits else 0, "domain_log": 9,
                                                                    "big_row": big_row})


def gen_div(n):
    """OP_BATCH_DIV of n divisions out_i (x_i - y_i) = (x_i - y_i) z_i, with t_i = (x_i - y_i) z_i solved first: a zero denominator
    makes the C side vanish with it, and the division yields 0.  The zero positions are chosen by the input row."""
    d = Desc(1, 3 * n)
    x = [d.sec(3 * i) for i in range(n)]
    y = [d.sec(3 * i + 1) for i in range(n)]
    z = [d.sec(3 * i + 2) for i in range(n)]
    t = [d.solve_c([(x[i], 1), (y[i], -1)], [(z[i], 1)]) for i in range(n)]
    out = [d.new_wire() for _ in range(n)]
    k0 = len(d.A)
    for i in range(n):
        d.row([(out[i], 1)], [(x[i], 1), (y[i], -1)], [(t[i], 1)])
    d.program += [OP_BATCH_DIV, k0, n]
    # out_i = z_i unless the denominator is zero; the sum ties the quotients to the public input
    s = d.solve_c([(o, i + 1) for i, o in enumerate(out)], [(0, 1)])
    tie = _tie(d, s)
    d.commit(out[:1], out[0])
    d.finish()

    def inputs(seed, zeros=()):
        r = random.Random(seed)
        row, tot = [], 0
        for i in range(n):
            xv, zv = r.randrange(R), r.randrange(R)
            yv = xv if i in zeros else r.randrange(R)
            if yv == xv and i not in zeros:
                yv = (yv + 1) % R
            row += [xv, yv, zv]
            tot += 0 if i in zeros else (i + 1) * zv
        return [tot % R] + row

    def spoil(row):
        return [(row[0] + 1) % R] + row[1:], tie
    wide = n >= WIDE_DIV_MIN
    return Synth("div%d" % n, d, inputs, spoil, {"max_wide_div": n if wide else 0, "wide_divs": 1 if wide else 0, "wide_steps": 1 if wide else 0})


def gen_ops(par_run=4, broken=False):
    """BITS / LIMBS8 / INV_H / COUNT8 on edge values chosen by the inputs.  `par_run` independent instructions stand in a row (3 stay
    sequential, 4 go one per lane); `broken`: the third of them reads what the second wrote, which ends the run there."""
    d = Desc(1, 6)
    v = [d.sec(i) for i in range(6)]
    hv = [d.hrow([(w, 1)]) for w in v]
    # 254 bits of v0 and 32 bytes of v1, each put together again by one row
    bits0 = d.new_wire(254)
    d.program += [OP_BITS, hv[0], 254, bits0]
    d.row([(bits0 + i, 1 << i) for i in range(254)], [(0, 1)], [(v[0], 1)])
    limbs0 = d.new_wire(32)
    d.program += [OP_LIMBS8, hv[1], 32, limbs0]
    d.row([(limbs0 + i, 1 << (8 * i)) for i in range(32)], [(0, 1)], [(v[1], 1)])
    # inverse hint of v2 (0 for 0): v2 * inv = flag, flag * v2 = v2
    inv = d.new_wire()
    d.program += [OP_INV_H, hv[2], inv]
    flag = d.solve_c([(v[2], 1)], [(inv, 1)])
    d.row([(flag, 1)], [(v[2], 1)], [(v[2], 1)])
    # a run of independent instructions (an OP_SOLVE_C in front of it ends the run of the three above)
    sep = d.solve_c([(v[3], 1)], [(v[3], 1)])
    outs = []
    for j in range(par_run):
        src = v[3 + j % 3]
        if broken and j == 2:
            h = d.hrow([(outs[1], 1), (src, 1)])          # reads the second instruction's first output
        else:
            h = d.hrow([(src, 1), (0, j)])
        o = d.new_wire(16)
        d.program += [OP_BITS if j % 2 == 0 else OP_LIMBS8, h, 16, o]
        outs.append(o)
    d.solve_c([(o, 1) for o in outs], [(sep, 1)])
    # lookup of sums of two wires (no range class follows from these): the histogram counts the values below 256 only
    hc = len(d.H)
    pairs = [(v[3], v[4]), (v[4], v[5]), (v[3], v[5]), (v[0], v[1]), (v[2], v[2])]
    for a, b in pairs:
        d.hrow([(a, 1), (b, 1)])
    cnt0 = d.new_wire(256)
    d.program += [OP_COUNT8, hc, len(pairs), cnt0]
    total = d.solve_c([(cnt0 + j, j + 1) for j in range(256)], [(0, 1)])
    tie = _tie(d, total)
    d.commit([limbs0, limbs0 + 1, bits0], limbs0)
    d.finish()

    def inputs(seed, vals=None):
        r = random.Random(seed)
        vals = list(vals) if vals is not None else [r.randrange(R) for _ in range(6)]
        sums = [(vals[3] + vals[4]) % R, (vals[4] + vals[5]) % R, (vals[3] + vals[5]) % R, (vals[0] + vals[1]) % R, 2 * vals[2] % R]
        total = sum(s + 1 for s in sums if s < 256) % R
        return [total] + vals

    def spoil(row):
        return [(row[0] + 1) % R] + row[1:], tie
    name = "ops%d%s" % (par_run, "_broken" if broken else "")
    return Synth(name, d, inputs, spoil, {"items_par": 1 if par_run >= COOP_PAR_MIN and not broken else 0, "wide_steps": 1})


# edge rows for gen_ops: v0 (bits), v1 (bytes), v2 (inverse), v3..v5 (looked up in pairs)
OPS_EDGE_VALUES = [
    [R - 1, R - 1, 0, 0, 0, 255],              # all-ones patterns; lookups 0, 255, 255, R-2 (not a byte), 0
    [0, 0, R - 1, 255, 1, 0],                  # zeros; lookups 256 (not counted), 1, 255
    [1 << 253, (1 << 64) + 5, 1, (1 << 64) + 5, 0, 250],   # a low word below 256 under a high word that is not zero
    [R - 1, 0, 5, R - 1, 1, 255],              # R - 1 + 1 wraps to 0
]


def gen_levels(kind, n=8):
    """The level planner of the cooperative solver, one small circuit per case:
    chain:      n dependent OP_SOLVE_C rows in one run (7 stays sequential, 8 becomes levels; 40: a deep chain), square rows
                and +-1 coefficients among them
    wide:       one level of n independent rows (200: more rows than lanes, cut across two chunks)
    edge:       one level of independent rows whose record takes exactly n words (1022, 1023 fit a chunk; 1024 is cut)
    bigrow:     a run with one row of 600 terms: its record cannot fit a chunk, the table-driven form takes the run
    components: chains of n, 10 and 10 rows in one run (n = 32: an item of its own beside the lump of small ones; 31: one lump)
    tracks:     six chains of n rows in one run and a division that reads the third: six components for four tracks
    lanes:      levels of 4 rows with 20-term forms (16 lanes per row), with 2-term forms (2), and 40 rows of 1-term forms (1)"""
    rng = random.Random(99)
    n_in = 8
    d = Desc(1, n_in)
    v = [d.sec(i) for i in range(n_in)]
    ex = {}
    tie_src = None
    if kind == "chain":
        cur = v[0]
        for j in range(n):
            if j % 3 == 0:
                cur = d.solve_c([(cur, 1), (v[1], -1)], [(cur, 1), (v[1], -1)])          # square, +-1 only
            elif j % 3 == 1:
                cur = d.solve_c([(cur, 1), (0, -1)], [(v[2], 1)], [(v[3], -1), (cur, 1)])
            else:
                cur = d.solve_c([(cur, rng.randrange(R)), (v[4], 3)], [(cur, 1), (v[5], rng.randrange(R))])
        tie_src = cur
        stream = n >= COOP_RUN_MIN
        ex = {"items_level_stream": 1 if stream else 0, "items_levels": 0, "stream_chunks": 1 if stream else 0}
    elif kind == "wide":
        outs = [d.solve_c([(v[j % n_in], 1)], [(v[(j + 1) % n_in], j + 2)]) for j in range(n)]
        tie_src = outs[0]
        per = 9                                                   # words per row: offset + 4 + 2 * 2 terms
        first = (COOP_CHUNK - 1 - 2) // per
        ex = {"items_level_stream": 1, "items_levels": 0, "stream_chunks": -(-n // first), "rows_per_sublevel": first}
    elif kind == "edge":
        # m rows, T terms in all: 2 + 5 m + 2 T = n words
        m = 9 if n % 2 else 10
        T = (n - 2 - 5 * m) // 2
        assert 2 + 5 * m + 2 * T == n
        base, extra = divmod(T, m)
        outs = []
        for j in range(m):
            na = base + (1 if j < extra else 0) - 1
            outs.append(d.solve_c([(v[i % n_in], rng.randrange(R)) for i in range(na)], [(v[j % n_in], 1)]))
        tie_src = outs[0]
        ex = {"items_level_stream": 1, "items_levels": 0, "stream_chunks": 1 if n <= COOP_CHUNK - 1 else 2, "level_words": n, "level_rows": m}
    elif kind == "bigrow":
        outs = [d.solve_c([(v[j], 1)], [(v[j + 1], 1)]) for j in range(7)]
        outs.append(d.solve_c([(v[i % n_in], rng.randrange(R)) for i in range(600)], [(outs[0], 1)]))
        tie_src = outs[-1]
        ex = {"items_level_stream": 0, "items_levels": 1, "stream_chunks": 0}
    elif kind in ("components", "tracks"):
        lens = [n, 10, 10] if kind == "components" else [n] * 6
        curs = [v[c] for c in range(len(lens))]
        for j in range(max(lens)):               # interleaved: the rows of the chains alternate in the run
            for c, ln in enumerate(lens):
                if j < ln:
                    curs[c] = d.solve_c([(curs[c], 1), (0, c + 1)], [(curs[c], 1), (0, j + 1)])
        if kind == "tracks":
            # one division on the third chain: its component uses the scratch rows and must run on track 0
            q = d.new_wire()
            k = d.row([(q, 1)], [(curs[2], 1), (0, 5)], [(curs[2], 3)])
            d.program += [OP_SOLVE_A, k]
            tie_src = d.solve_c([(q, 1)], [(0, 1)])
            ex = {"items_level_stream": 6, "items_levels": 0, "tracks": 4}
        else:
            tie_src = curs[0]
            ex = {"items_level_stream": 2 if n >= COOP_COMPONENT_MIN else 1, "items_levels": 0}
    elif kind == "lanes":
        l0 = [d.solve_c([(v[i % n_in], rng.randrange(R)) for i in range(20)], [(v[j], 1)]) for j in range(4)]
        l1 = [d.solve_c([(l0[j], 1), (v[j], 2)], [(l0[(j + 1) % 4], 1), (0, 1)]) for j in range(4)]
        l2 = [d.solve_c([(l1[j % 4], 1)], [(v[j % n_in], 1)]) for j in range(40)]
        tie_src = d.solve_c([(o, j + 1) for j, o in enumerate(l2)], [(0, 1)])
        ex = {"items_level_stream": 1, "items_levels": 0, "stream_chunks": 1}
    else:
        raise ValueError(kind)
    tie = _tie(d, tie_src)
    d.commit(v[:2], v[0])
    d.finish()

    def inputs(seed):
        from oracle import circuit as C
        r = random.Random(seed)
        vals = [r.randrange(R) for _ in range(n_in)]
        w = C.solve(_as_circuit(d), [0] + vals, lambda w_: 0)       # the tied wire is solved before the commitment
        return [w[tie_src]] + vals

    def spoil(row):
        return [(row[0] + 1) % R] + row[1:], tie
    return Synth("levels_%s%d" % (kind, n), d, inputs, spoil, ex)


class _Sparse:
    def __init__(self, rows):
        self._rows = rows
        self.rows = len(rows)

    def row(self, k):
        return [w for w, _ in self._rows[k]], [v for _, v in self._rows[k]]


def _as_circuit(d):
    """the description in the shape oracle.circuit.solve walks (no file in between)"""
    class Cc:
        pass
    c = Cc()
    c.A, c.B, c.C, c.H = _Sparse(d.A), _Sparse(d.B), _Sparse(d.C), _Sparse(d.H)
    c.program, c.n_wires, c.challenge_wire, c.n_constraints = d.program, d.n_wires, d.challenge_wire, d.n_constraints
    c.n_inputs = d.n_inputs
    return c


def contents_equal(desc, circ):
    """the description against what oracle.circuit.Circuit read back from the written file"""
    if (circ.id, circ.n_public, circ.n_secret, circ.n_wires, circ.n_constraints, circ.domain_log, circ.challenge_wire) != \
            (desc.id, desc.n_public, desc.n_secret, desc.n_wires, desc.n_constraints, desc.domain_log, desc.challenge_wire):
        return False
    if circ.committed != desc.committed or circ.program != desc.program or circ.aux:
        return False
    for m, rows in ((circ.A, desc.A), (circ.B, desc.B), (circ.C, desc.C), (circ.H, desc.H)):
        if m.rows != len(rows):
            return False
        for k, terms in enumerate(rows):
            ws, cs = m.row(k)
            if list(ws) != [w for w, _ in terms] or list(cs) != [v for _, v in terms]:
                return False
    return True


# every generator under a name: the host tests walk all of them, the GPU tests pick theirs
CASES = {
    "tiny": gen_tiny,
    "rows260": lambda: gen_rows(260),
    "rows1030": lambda: gen_rows(1030),
    "rows1030_1025": lambda: gen_rows(1030, with_1025=True),
    "widest_small_row": gen_widest_small_row,
    "widest_small_row_x2": lambda: gen_widest_small_row(1 << 19),
    "div63": lambda: gen_div(63),
    "div64": lambda: gen_div(64),
    "div65": lambda: gen_div(65),
    "div100": lambda: gen_div(100),
    "ops3": lambda: gen_ops(3),
    "ops4": lambda: gen_ops(4),
    "ops4_broken": lambda: gen_ops(4, broken=True),
    "chain7": lambda: gen_levels("chain", 7),
    "chain8": lambda: gen_levels("chain", 8),
    "chain40": lambda: gen_levels("chain", 40),
    "wide200": lambda: gen_levels("wide", 200),
    "edge1022": lambda: gen_levels("edge", 1022),
    "edge1023": lambda: gen_levels("edge", 1023),
    "edge1024": lambda: gen_levels("edge", 1024),
    "bigrow": lambda: gen_levels("bigrow"),
    "components31": lambda: gen_levels("components", 31),
    "components32": lambda: gen_levels("components", 32),
    "tracks32": lambda: gen_levels("tracks", 32),
    "tracks180": lambda: gen_levels("tracks", 180),
    "lanes": lambda: gen_levels("lanes"),
}
