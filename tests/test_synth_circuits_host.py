"""The synthetic circuits (tests/synth_circuits.py) on the CPU: every generator writes a container the oracle reads back unchanged,
gives rows the oracle's solver satisfies, spoils exactly the constraint it names, sets up and proves with the C oracle, and has the
shape it is meant to have -- each assertion names the threshold the generator sits on, so a generator that drifts off it fails
here and not on the device."""
import os
import pytest

import synth_circuits as S


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """name -> (Synth, paths, oracle circuit, oracle prover), each made once"""
    from oracle import circuit as C, native
    d = tmp_path_factory.mktemp("synth")
    cache = {}

    def get(name):
        if name not in cache:
            g = S.CASES[name]()
            sppc, pk, vk = (os.path.join(str(d), name + "." + e) for e in ("sppc", "pk", "vk"))
            S.write_sppc(g.desc, sppc)
            native.setup(sppc, b"\x05" * 32, pk, vk)
            cache[name] = (g, dict(sppc=sppc, pk=pk, vk=vk), C.Circuit(sppc), native.Prover(sppc, pk))
        return cache[name]
    return get


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_generator_roundtrip_solve_spoil_prove(built, name):
    from oracle import circuit as C, groth16
    g, art, circ, orc = built(name)
    assert S.contents_equal(g.desc, circ)                                   # the writer against the oracle's reader
    assert circ.id not in (1, 2) and circ.committed and circ.challenge_wire
    assert any(circ.challenge_wire in circ.A.row(k)[0] for k in range(circ.n_constraints)), "no row reads the challenge"
    assert {S.OP_MASK, S.OP_COMMIT} <= {op for _, op in S.instructions(g.desc)}
    for seed in (1, 2):
        row = g.inputs(seed)
        rc, proof, pw, wires = orc.prove(row, 3 + seed, 4 + seed, want_wires=True)
        assert rc == 0
        w = C.solve(circ, row, lambda w_: wires[circ.challenge_wire], rs=(3 + seed, 4 + seed))
        assert w == wires                                                   # the two oracle solvers agree
        assert C.first_unsatisfied(circ, w) == -1
    assert groth16.verify(open(art["vk"], "rb").read(), proof, pw)
    bad, k = g.spoil(row)
    assert C.first_unsatisfied(circ, C.solve(circ, bad, lambda w_: wires[circ.challenge_wire], rs=(5, 6))) == k
    assert orc.prove(bad, 5, 6)[0] != 0


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_generator_sits_on_its_threshold(name):
    g = S.CASES[name]()
    model = S.plan_model(g.desc)
    for key, want in g.expect.items():
        if key in model:
            assert model[key] == want, (name, key, model[key], want)
    if "domain_log" in g.expect:
        assert g.desc.domain_log == g.expect["domain_log"]
    if "n_committed" in g.expect:
        assert len(g.desc.committed) == g.expect["n_committed"]


def test_row_path_shapes():
    """SMALL_ROW_MIN = 64, SMALL_ROW_REST = 32, LONG_ROW_MIN = 512, runs of at most 8, n_runs * P against 65 536"""
    g = S.CASES["rows260"]()
    d = g.desc
    lk = S.lookup_wires(d)
    assert sorted(set(lk.values())) == [-32000, 0, 3, 32000] and len(lk) == 64
    assert len(d.committed) == 65                                           # more than 64 committed wires

    def counts(terms):
        q = sum(1 for w, v in terms if (w in lk or w == 0) and S.small_signed(v) is not None)
        return q, len(terms) - q
    by_counts = {}
    for side, m in (("A", d.A), ("B", d.B), ("C", d.C)):
        for k, terms in enumerate(m):
            by_counts.setdefault((side,) + counts(terms), []).append(k)
    for side, rest in (("A", 0), ("B", 0), ("C", 1)):
        for q in (63, 64, 65):                                              # SMALL_ROW_MIN from both sides, on every side
            assert (side, q, rest) in by_counts, (side, q)
    assert ("A", 64, 32) in by_counts and ("A", 64, 33) in by_counts        # SMALL_ROW_REST from both sides
    assert ("A", 63, 1) in by_counts and ("A", 64, 2) in by_counts          # a 2^30 coefficient is one of the others
    coefs = {S.small_signed(v) for m in (d.A,) for terms in m for _, v in terms if S.small_signed(v) is not None}
    assert (1 << 30) - 1 in coefs and -((1 << 30) - 1) in coefs
    assert any(v in (1 << 30, S.R - (1 << 30)) for terms in d.A for _, v in terms)
    lens = {(side, len(t)) for side, m in (("A", d.A), ("B", d.B), ("C", d.C)) for t in m}
    assert {("A", 512), ("A", 513), ("B", 513), ("C", 512), ("C", 513)} <= lens    # LONG_ROW_MIN from both sides
    assert ("A", 0) in lens and ("C", 0) in lens                            # a row with no terms
    assert any(len({w for w, _ in t}) < len(t) for t in d.A if len(t) < 8 and t)   # a row with repeated wires
    # runs of identical B rows: lengths 1, 8, 9, 17 for a general, a small and a long shared row
    runs, k = [], 0
    while k < d.n_constraints:
        e = k + 1
        while e < d.n_constraints and d.B[e] and d.B[e] == d.B[k]:
            e += 1
        runs.append((e - k, len(d.B[k])))
        k = e
    for nterms in (3, 64, 513):
        assert {1, 8, 9, 17} <= {ln for ln, nt in runs if nt == nterms}, nterms
    # 260 runs: 252 proofs stay below 65 536 lanes, 256 proofs reach it
    n_runs = S.plan_model(d)["n_runs"]
    assert n_runs * 252 < S.ROWS_KERNEL_LANES <= n_runs * 256
    # lookup inputs at both ends of their ranges, the spoiled ones one step outside
    row = g.inputs(1)
    for i in range(4):
        cst = S.LOOKUP_CSTS[i]
        assert row[1 + i] == (-cst) % S.R and row[1 + 4 + i] == (255 - cst) % S.R
        assert g.spoil(row, wire=i, above=True)[0][1 + i] == (256 - cst) % S.R
        assert g.spoil(row, wire=i, above=False)[0][1 + i] == (-cst - 1) % S.R
    # the P <= 64 && max_row_terms > 1024 clause needs n_runs * 64 >= 65 536 to decide anything
    for name, longest in (("rows1030", 513), ("rows1030_1025", 1025)):
        m = S.plan_model(S.CASES[name]().desc)
        assert m["max_row_terms"] == longest and m["n_runs"] * 64 >= S.ROWS_KERNEL_LANES


def test_spoiled_lookup_values_break_the_range_constraint_alone(built):
    from oracle import circuit as C
    g, art, circ, orc = built("rows260")
    row = g.inputs(3)
    for wire in range(4):
        for above in (False, True):
            bad, k = g.spoil(row, wire=wire, above=above)
            assert C.first_unsatisfied(circ, C.solve(circ, bad, lambda w_: 7)) == k
            assert orc.prove(bad, 1, 2)[0] != 0


def test_widest_small_row_shape():
    """one A row of 2^18 terms, coefficient 2^30 - 1, on a -32000-offset wire whose value reaches 32 255: the integer sum is
    0.984 * 2^63, inside a signed 64-bit accumulator; one more doubling of the row would not be"""
    g = S.CASES["widest_small_row"]()
    d = g.desc
    big = d.A[g.expect["big_row"]]
    assert len(big) == 1 << 18 and {v for _, v in big} == {(1 << 30) - 1} and len({w for w, _ in big}) == 1
    assert S.lookup_wires(d)[big[0][0]] == -32000
    top = max(g.inputs(s)[1] for s in range(3))
    assert top == 32255
    assert len(big) * ((1 << 30) - 1) * top < 1 << 63 <= 2 * len(big) * ((1 << 30) - 1) * top
    m = S.plan_model(d)
    assert m["sm_nrows"] == 1 and m["n_runs"] * 256 >= S.ROWS_KERNEL_LANES
    # twice the terms: every other rule still admits the row, the bound on the sum does not
    d2 = S.CASES["widest_small_row_x2"]().desc
    assert S.plan_model(d2, small_sum_bound=None)["sm_nrows"] == 1
    m2 = S.plan_model(d2)
    assert (m2["sm_nrows"], m2["lg_n"]) == (0, 1) and m2["n_runs"] * 256 >= S.ROWS_KERNEL_LANES


def test_division_shapes():
    """the 64-division cut, n * P against 16 384, chunks of 4 below 256 proofs and of 32 from 256 on"""
    for n in (63, 64, 65, 100):
        d = S.CASES["div%d" % n]().desc
        assert [d.program[pc + 2] for pc, op in S.instructions(d) if op == S.OP_BATCH_DIV] == [n]
        m = S.plan_model(d)
        assert m["wide_divs"] == (1 if n >= S.WIDE_DIV_MIN else 0)
    assert 64 * 256 == S.DIV_WAVE_MAX < 65 * 256                            # 64 divisions, 256 proofs: the last batch of one lane each
    assert 65 % 32 and 65 % 4 and 100 * 192 > S.DIV_WAVE_MAX                # partial last chunks; 255 proofs cut to 192 + 63 still chunk
    g = S.CASES["div65"]()
    row = g.inputs(1, zeros=(0, 15, 31, 64))
    assert all(row[1 + 3 * i] == row[2 + 3 * i] for i in (0, 15, 31, 64)) and row[1 + 3] != row[2 + 3]


def test_level_planner_shapes():
    """runs of 8 rows become levels, records are packed into 1 024-word chunks, components of 32 rows stand alone"""
    def run_rows(d):
        """the rows of the first run of OP_SOLVE_C instructions"""
        rows = []
        for pc, op in S.instructions(d):
            if op != S.OP_SOLVE_C:
                break
            rows.append(d.program[pc + 1])
        return rows
    for n, chunks in ((1022, 1), (1023, 1), (1024, 2)):
        g = S.CASES["edge%d" % n]()
        rows = run_rows(g.desc)
        assert len(rows) == g.expect["level_rows"] >= S.COOP_RUN_MIN
        assert S.level_words(g.desc, rows) == n                             # against COOP_CHUNK - 1 = 1 023 usable words
        assert S.plan_model(g.desc)["stream_chunks"] == chunks
    g = S.CASES["wide200"]()
    rows = run_rows(g.desc)
    assert len(rows) == 200 and {S.record_words(g.desc, k) for k in rows} == {8}
    assert S.level_words(g.desc, rows[:113]) <= 1023 < S.level_words(g.desc, rows[:114])
    g = S.CASES["bigrow"]()
    assert max(S.record_words(g.desc, k) for k in run_rows(g.desc)) > S.COOP_CHUNK     # no chunk can hold it
    assert len(run_rows(S.CASES["chain7"]().desc)) == 7 and len(run_rows(S.CASES["chain8"]().desc)) == 8
    d = S.CASES["chain40"]().desc
    assert len(run_rows(d)) == 40 and S.run_levels(d, run_rows(d)) == list(range(40))      # a dependency chain 40 deep
    assert set(S.run_levels(S.CASES["wide200"]().desc, rows)) == {0}                        # one level
    for n in (7, 8):
        d = S.CASES["chain%d" % n]().desc
        assert max(S.run_levels(d, run_rows(d))) == n - 1
    # lanes per row: 4 rows of 20-term forms get 16, 4 rows of 2-term forms 2, 40 rows of 1-term forms 1
    d = S.CASES["lanes"]().desc
    assert S.sublevel_lanes(d, run_rows(d))[:3] == [(4, 16), (4, 2), (40, 1)]
    assert {g for _, g in S.sublevel_lanes(d, run_rows(d))} >= {16, 2, 1}
    assert S.sublevel_lanes(S.CASES["wide200"]().desc, rows) == [(113, 1), (87, 1)]          # more rows than lanes, cut in two
    d = S.CASES["chain8"]().desc
    assert any(d.A[k] == d.B[k] for k in run_rows(d))                       # a square row
    assert any({v for _, v in d.A[k] + d.B[k]} <= {1, S.R - 1} for k in run_rows(d))   # +-1 coefficients only
    for name, kinds in (("ops3", 0), ("ops4", 1), ("ops4_broken", 0)):
        assert S.plan_model(S.CASES[name]().desc)["items_par"] == kinds     # runs of 3 / 4 independent instructions, a broken run
    d = S.CASES["tracks32"]().desc
    assert S.plan_model(d)["tracks"] == 4
    # six independent components; the one item that uses the scratch rows (the division) reads the third chain and nothing else
    # written in the stretch, so that component -- and no other -- is pinned to track 0
    end = next(pc for pc, op in S.instructions(d) if op == S.OP_COMMIT)
    its, _ = S._coop_items(d, 0, end)
    chains = [i for i, it in enumerate(its) if it[0] == "level_stream"]
    users = [i for i, it in enumerate(its) if it[3]]
    assert len(chains) == 6 and len(users) == 1
    assert all(not set(its[a][2]) & set(its[b][1]) for a in chains for b in chains if a != b)
    assert [c for c in chains if set(its[c][2]) & set(its[users[0]][1])] == [chains[2]]
    assert S.plan_model(S.CASES["components31"]().desc)["items_level_stream"] == 1
    assert S.plan_model(S.CASES["components32"]().desc)["items_level_stream"] == 2


def test_ops_edge_rows_are_satisfiable(built):
    from oracle import circuit as C
    g, art, circ, orc = built("ops4")
    for vals in S.OPS_EDGE_VALUES:
        row = g.inputs(0, vals=vals)
        rc, _, _, wires = orc.prove(row, 9, 10, want_wires=True)
        assert rc == 0, vals
        assert C.solve(circ, row, lambda w_: wires[circ.challenge_wire], rs=(9, 10)) == wires
