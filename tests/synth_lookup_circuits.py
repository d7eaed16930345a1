"""Synthetic circuits with a log-derivative range check, as Builder::finalize_lookups (csrc/circuit.cpp) emits it: L byte inputs
are looked up, every lookup i gets the wire inv_i = 1 / (X - b_i) by a deferred division, the 256 table entries the wires
q_j = m_j / (X - j), and one row asserts sum inv_i = sum q_j.  The inv_i are the lookup-inverse wires of csrc/msm_lookup.hpp; a few
dozen other wires stand beside them.  Written with tests/synth_circuits.py's Desc / write_sppc."""
import random

from synth_circuits import (Desc, Synth, R, OP_BATCH_DIV, OP_COUNT8, _tie)

N_GENERAL = 24


def gen_lookup(L):
    d = Desc(1, L + N_GENERAL)
    b = [d.sec(i) for i in range(L)]
    g = [d.sec(L + i) for i in range(N_GENERAL)]
    # the other wires: a chain of products over the general inputs, tied to the public input
    y = d.solve_c([(g[0], 1)], [(g[0], 1)])
    tie = _tie(d, y)
    acc = y
    for i in range(1, N_GENERAL):
        acc = d.solve_c([(acc, 1), (g[i], 3)], [(g[(i * 7) % N_GENERAL], 1), (0, i)])
    # the lookup: hint rows of the looked-up values, multiplicities, commitment, challenge
    h0 = len(d.H)
    for w in b:
        d.hrow([(w, 1)])
    m0 = d.new_wire(256)
    d.program += [OP_COUNT8, h0, L, m0]
    d.commit(b + [m0 + j for j in range(256)], acc)
    X = d.challenge_wire
    k0 = len(d.A)
    inv = []
    for w in b:
        o = d.new_wire()
        d.row([(o, 1)], [(w, -1), (X, 1)], [(0, 1)])
        inv.append(o)
    q = []
    for j in range(256):
        o = d.new_wire()
        d.row([(o, 1)], ([(0, -j)] if j else []) + [(X, 1)], [(m0 + j, 1)])
        q.append(o)
    d.program += [OP_BATCH_DIV, k0, L + 256]
    sum_row = d.row([(o, 1) for o in inv] + [(o, -1) for o in q], [(0, 1)], [])
    d.finish()

    def inputs(seed, values=None):
        """values: the L looked-up bytes (default: random)"""
        r = random.Random(seed)
        gv = [r.randrange(R) for _ in range(N_GENERAL)]
        bv = list(values) if values is not None else [r.randrange(256) for _ in range(L)]
        assert len(bv) == L
        return [gv[0] * gv[0] % R] + [v % R for v in bv] + gv

    def spoil(row, lookup=0, value=256):
        """lookup `lookup` takes a value outside the table: only the sum row can tell"""
        bad = list(row)
        bad[1 + lookup] = value % R
        return bad, sum_row
    return Synth("lookup%d" % L, d, inputs, spoil, {"lookup_inverses": L, "inv_wires": inv, "tie": tie})
