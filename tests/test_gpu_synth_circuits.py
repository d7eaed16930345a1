"""Synthetic circuits (tests/synth_circuits.py) through the device prover: every case sets the circuit up on the device (key bytes
against the oracle's), loads it with 6-bit windows, shows by spp_circuit_plan_stats that it takes the path it names, proves a batch
with fixed (r, s) and requires the status words, the witness column the library keeps, and the proof and public-witness bytes of
EVERY row to equal the oracle's -- then the same bytes with each diagnostic switch that takes a path out, and a spoiled row in the
middle of the batch refused alone.  No tolerance anywhere: integers and bytes."""
import os
import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None

import synth_circuits as S

pytestmark = pytest.mark.gpu

SPP_ERR_UNSAT = -4
BATCH_SIZES = [1, 63, 64, 65, 256, 1024, 1025]
SWITCH_VARS = ("SPP_NO_SMALL_ROWS", "SPP_NO_LONG_ROWS", "SPP_NO_COOP", "SPP_NO_LEVEL_STREAM", "SPP_COOP_ONE_TRACK", "SPP_NO_SPLIT", "SPP_H_MODE")
# the default is SPP_H_MODE=2 with every path on; each variant takes one path out (or computes h another way)
VARIANTS = {
    "no_small_rows": {"SPP_NO_SMALL_ROWS": "1"},
    "no_long_rows": {"SPP_NO_LONG_ROWS": "1"},
    "no_coop": {"SPP_NO_COOP": "1"},
    "no_level_stream": {"SPP_NO_LEVEL_STREAM": "1"},
    "one_track": {"SPP_COOP_ONE_TRACK": "1"},
    "no_split": {"SPP_NO_SPLIT": "1"},
    "h_mode0": {"SPP_H_MODE": "0"},
    "h_mode1": {"SPP_H_MODE": "1"},
}


@pytest.fixture(scope="module")
def ctx():
    import spp
    c = spp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def lab(ctx, tmp_path_factory):
    """name -> the generator's circuit written, set up by the oracle AND on the device (the key files must be the same bytes, as in
    test_setup_matches_oracle), read back by the oracle; each made once for the module"""
    from oracle import circuit as C, native
    d = str(tmp_path_factory.mktemp("synth_gpu"))
    cache = {}

    def get(name):
        if name not in cache:
            g = S.CASES[name]()
            sppc, pk, vk, pk2, vk2 = (os.path.join(d, name + "." + e) for e in ("sppc", "pk", "vk", "gpu.pk", "gpu.vk"))
            S.write_sppc(g.desc, sppc)
            native.setup(sppc, b"\x0d" * 32, pk, vk)
            ctx.setup(sppc, b"\x0d" * 32, pk2, vk2)
            same = open(vk2, "rb").read() == open(vk, "rb").read() and open(pk2, "rb").read() == open(pk, "rb").read()
            cache[name] = dict(g=g, sppc=sppc, pk=pk, vk=vk, setup_matches=same, circ=C.Circuit(sppc), orc=native.Prover(sppc, pk), want={})
        return cache[name]
    return get


def _clear(monkeypatch):
    for k in SWITCH_VARS:
        monkeypatch.delenv(k, raising=False)


def _oracle_batch(case, key, rows, rs):
    """proofs and public witnesses of the whole batch from the C oracle, once per (circuit, batch)"""
    from oracle import native
    if key not in case["want"]:
        rc, proofs, pws = native.prove_many(case["orc"], rows, rs)
        assert rc == 0
        case["want"][key] = (proofs, pws)
    return case["want"][key]


def _kept_column(count, split):
    """the row whose witness the library keeps: column 0 of the last piece of the batch (above 64 proofs a batch that is no multiple of
    64 is cut into a body and a tail of count % 64)"""
    return count - count % 64 if (split and count > 64 and count % 64) else 0


def run_case(ctx, lab, monkeypatch, name, count, rows=None, bad=None, variants=tuple(VARIANTS), key=None):
    """The checks every case makes (module docstring).  rows: the batch (default: five generated rows in turn); bad: {index: spoiled
    row} placed into a second batch; variants: the switches to compare across."""
    from oracle import circuit as C
    case = lab(name)
    g, circ, orc = case["g"], case["circ"], case["orc"]
    assert case["setup_matches"], "device setup differs from the oracle's"
    if rows is None:
        pool = [g.inputs(1 + i) for i in range(min(count, 5))]
        rows = [pool[i % len(pool)] for i in range(count)]
    assert len(rows) == count
    rs = [(11 + 3 * i, 1000003 + 7 * i) for i in range(count)]
    want_proofs, want_pws = _oracle_batch(case, key or ("default", count), rows, rs)
    _clear(monkeypatch)
    h = ctx.load_circuit(case["sppc"], case["pk"], 6)
    try:
        stats = h.plan_stats()
        model = S.plan_model(g.desc)
        assert {k: stats[k] for k in S.PLAN_KEYS} == {k: model[k] for k in S.PLAN_KEYS}, (name, stats)
        for k, v in g.expect.items():
            if k in stats:
                assert stats[k] == v, (name, k, stats[k], v)
        proofs, pws, status = h.prove_batch(rows, rs)
        assert status == [0] * count, (name, count)
        i0 = _kept_column(count, True)
        rc, _, _, wires = orc.prove(rows[i0], rs[i0][0], rs[i0][1], want_wires=True)
        assert rc == 0
        assert h.debug_witness() == C.solve(circ, rows[i0], lambda w: wires[circ.challenge_wire], rs=rs[i0]), (name, count, "witness")
        assert proofs == want_proofs and pws == want_pws, (name, count, [i for i in range(count) if proofs[i] != want_proofs[i]][:8])
        if bad:
            spoiled = [bad.get(i, rows[i]) for i in range(count)]
            p2, w2, st2 = h.prove_batch(spoiled, rs)
            assert st2 == [SPP_ERR_UNSAT if i in bad else 0 for i in range(count)], (name, count)
            for i in range(count):
                if i in bad:
                    assert p2[i] == b"\x00" * 388
                else:
                    assert p2[i] == want_proofs[i] and w2[i] == want_pws[i], (name, count, i)
    finally:
        h.close()
    for v in variants:
        if v == "no_split" and not (count > 64 and count % 64):
            continue                                   # nothing to cut
        _clear(monkeypatch)
        for k, val in VARIANTS[v].items():
            monkeypatch.setenv(k, val)
        h = ctx.load_circuit(case["sppc"], case["pk"], 6)
        try:
            off = h.plan_stats()                         # the switch is read: the path it names is out of the plan
            if v == "no_small_rows":
                assert off["sm_nrows"] == 0 and off["sm_nslots"] == 0, (name, v, off)
            if v == "no_long_rows":
                assert off["lg_n"] == 0, (name, v, off)
            if v == "no_level_stream":
                assert off["items_level_stream"] == 0 and off["stream_chunks"] == 0, (name, v, off)
                assert off["items_levels"] == stats["items_levels"] + stats["items_level_stream"], (name, v, off)
            proofs, pws, status = h.prove_batch(rows, rs)
            assert status == [0] * count, (name, count, v)
            assert proofs == want_proofs and pws == want_pws, (name, count, v)
            if v in ("no_coop", "no_split"):             # another solver kernel / an uncut batch: its witness too
                i0 = _kept_column(count, v != "no_split")
                rc, _, _, wires = orc.prove(rows[i0], rs[i0][0], rs[i0][1], want_wires=True)
                assert h.debug_witness() == C.solve(circ, rows[i0], lambda w: wires[circ.challenge_wire], rs=rs[i0]), (name, count, v)
            if bad and v in ("no_small_rows", "no_coop"):
                _, _, st2 = h.prove_batch([bad.get(i, rows[i]) for i in range(count)], rs)
                assert st2 == [SPP_ERR_UNSAT if i in bad else 0 for i in range(count)], (name, count, v)
        finally:
            h.close()
    _clear(monkeypatch)


def _mid(case, count):
    g = case["g"]
    return {count // 2: g.spoil(g.inputs(1 + (count // 2) % 5))[0]}


# ---------------------------------------------------------------------------------------------- batch sizes and domains
@pytest.mark.parametrize("count", BATCH_SIZES)
def test_tiny_circuit_every_batch_size(ctx, lab, monkeypatch, count):
    """domain 2^3 (7 H bases), one committed wire: the batched NTT, coset scaling and QAP step at their smallest, MSM sets of 1 and 7
    bases; 65 and 1025 are no multiples of the wave; 1025 uncut (SPP_NO_SPLIT) is past the cooperative solver's 1 024 proofs and
    past scaled blinding"""
    run_case(ctx, lab, monkeypatch, "tiny", count, bad=_mid(lab("tiny"), count) if count > 1 else None)


# ---------------------------------------------------------------------------------------------- level planner
LEVEL_CASES = ("chain7", "chain8", "chain40", "wide200", "edge1022", "edge1023", "edge1024", "bigrow", "components31", "components32",
               "tracks32", "lanes")


# tracks180 is tracks32 with chains of 180 rows, there for the 2^11 domain alone: it stops at 256 proofs (1 024 oracle proofs of a
# 2^11 circuit cost the CPU several seconds and meet no index that tracks32 at 1 024 / 1 025 and the 2^11 row circuits do not)
@pytest.mark.parametrize("name,count", [(n, c) for n in LEVEL_CASES for c in BATCH_SIZES] + [("tracks180", c) for c in BATCH_SIZES[:5]])
def test_level_planner_cases(ctx, lab, monkeypatch, name, count):
    """runs of 7 / 8 rows, a 40-deep chain (domain 2^6), a 200-row level over two chunks, levels of 1 022 / 1 023 / 1 024 words, a row
    no chunk holds (COOP_LEVELS), components of 31 / 32 rows, six components on four tracks with a division pinned to track 0
    (tracks180: domain 2^11), 16 / 2 / 1 lanes per row"""
    run_case(ctx, lab, monkeypatch, name, count, bad=_mid(lab(name), count) if count > 2 else None)


# ---------------------------------------------------------------------------------------------- BITS / LIMBS8 / INV_H / COUNT8
@pytest.mark.parametrize("name,count", [(n, c) for n in ("ops3", "ops4", "ops4_broken") for c in BATCH_SIZES])
def test_hint_instructions_on_edge_values(ctx, lab, monkeypatch, name, count):
    """254 bits and 32 bytes of R - 1 and of 0, the inverse hint of 0, looked-up sums 0 / 255 / 256 / R - 1 + 1 and one whose low word is
    a byte under a high word that is not zero; runs of 3 (sequential) and 4 (one per lane) independent instructions, a run a
    dependency breaks"""
    g = lab(name)["g"]
    special = [g.inputs(0, vals=v) for v in S.OPS_EDGE_VALUES] + [g.inputs(7)]
    rows = [special[i % len(special)] for i in range(count)]
    run_case(ctx, lab, monkeypatch, name, count, rows=rows, bad={count // 2: g.spoil(rows[count // 2])[0]} if count > 1 else None,
             key=("edges", count))


# ---------------------------------------------------------------------------------------------- wide division
def _div_rows(g, n, count):
    pats = [(), (0,), (15,), (31,), tuple(range(32, 64)), (n - 1,), (0, 1, 2, 3), (3,), (4, 5, 6, 7), tuple(range(n)), (0, 31, 32, 63)]
    pats = [tuple(i for i in p if i < n) for p in pats]
    return [g.inputs(1 + i % 7, zeros=pats[i % len(pats)]) for i in range(count)]


@pytest.mark.parametrize("n,count", [(63, 65), (63, 256), (64, 1), (64, 256), (64, 257), (65, 1), (65, 252), (65, 255), (65, 256),
                                     (65, 1025), (100, 255), (100, 256)])
def test_wide_division_cases(ctx, lab, monkeypatch, n, count):
    """63 divisions stay in the sequential stretch, 64 and 65 are a wide step (plan stats).  The batch sizes lie on both sides of the
    launch-time cuts, which fix P here: n * P = 16 384 exactly (64 x 256) and just above (65 x 256, 64 x 257 uncut), below 256 proofs
    (65 x 255 uncut, 100 x 192) and from 256 on, n no multiple of 4 or 32.  Which kernel a launch took leaves no trace: every form
    must give the oracle's bytes.  Zero denominators first, in the middle and last in a chunk, whole chunks of zeros, every
    denominator zero"""
    name = "div%d" % n
    g = lab(name)["g"]
    rows = _div_rows(g, n, count)
    run_case(ctx, lab, monkeypatch, name, count, rows=rows, bad={count // 2: g.spoil(rows[count // 2])[0]} if count > 1 else None,
             key=("zeros", count))


# ---------------------------------------------------------------------------------------------- row paths
def _lookup_spoils(g, rows, count):
    """the eight out-of-range lookup values (one step below and above each of the four ranges), spread over the batch"""
    bad = {}
    for j, (wire, above) in enumerate((w, a) for w in range(4) for a in (False, True)):
        i = (count // 9) * (j + 1)
        bad[i] = g.spoil(rows[i], wire=wire, above=above)[0]
    return bad


@pytest.mark.parametrize("count", sorted(BATCH_SIZES + [252]))
def test_row_path_thresholds(ctx, lab, monkeypatch, count):
    """260 runs (domain 2^9, 65 committed wires), so n_runs * P is under 65 536 at 252 proofs (cut or not) and reaches it at 256: the
    sizes from 256 on are those at which the small rows (63 / 64 / 65 qualifying terms on each side, 32 / 33 others, +-(2^30 - 1)
    and 2^30), the long rows (512 / 513 terms) and the runs of 1 / 8 / 9 / 17 identical B rows (shared row general, small, long) of
    the plan are read, by the launch rule; the plan stats show the rows are planned, the launch itself leaves no trace.  Lookup values
    sit at both ends of their ranges; one step outside is refused, alone, at every size and under every switch compared"""
    case = lab("rows260")
    g = case["g"]
    pool = [g.inputs(1 + i) for i in range(5)]
    rows = [pool[i % 5] for i in range(count)]
    run_case(ctx, lab, monkeypatch, "rows260", count, rows=rows, bad=_lookup_spoils(g, rows, count) if count > 9 else None)


@pytest.mark.parametrize("name,count", [("rows1030_1025", 64), ("rows1030_1025", 65), ("rows1030", 64)])
def test_1025_term_row_at_64_and_65_proofs(ctx, lab, monkeypatch, name, count):
    """1 030 runs (domain 2^11): 64 proofs reach 65 536 lanes, so `P <= 64 && max_row_terms > 1024` alone decides at 64 proofs, with
    and without the 1 025-term row, and 65 uncut proofs (SPP_NO_SPLIT) are past it.  The threshold fixes P; the launch's choice
    leaves no trace, every form must give the oracle's bytes"""
    run_case(ctx, lab, monkeypatch, name, count, bad=_mid(lab(name), count))


# the two widest rows are one circuit each at 256 proofs; the switches are compared in groups so that a case stays at a few seconds
WIDEST_GROUPS = [(), ("no_small_rows", "no_long_rows"), ("no_coop", "no_level_stream"), ("one_track", "h_mode0", "h_mode1")]


@pytest.mark.parametrize("group", WIDEST_GROUPS, ids=lambda g: "+".join(g) or "spoiled")
def test_widest_integer_row(ctx, lab, monkeypatch, group):
    """2^18 terms x (2^30 - 1) x 32 255 = 0.984 * 2^63: the widest row a signed 64-bit sum holds.  It is planned as an integer row
    (sm_nrows == 1: the bound sum of |coefficient| x largest slot magnitude < 2^63 admits it) and accepted."""
    run_case(ctx, lab, monkeypatch, "widest_small_row", 256, bad=None if group else _mid(lab("widest_small_row"), 256), variants=group)


@pytest.mark.parametrize("group", WIDEST_GROUPS, ids=lambda g: "+".join(g) or "spoiled")
def test_integer_row_past_the_64_bit_sum(ctx, lab, monkeypatch, group):
    """2^19 such terms: every other rule admits the row, its sum 1.97 * 2^63 does not fit.  Without the planner's bound the sum wraps
    and 256 valid rows are refused; with it the row is planned as a long row and the bytes are the oracle's."""
    run_case(ctx, lab, monkeypatch, "widest_small_row_x2", 256, bad=None if group else _mid(lab("widest_small_row_x2"), 256), variants=group)
