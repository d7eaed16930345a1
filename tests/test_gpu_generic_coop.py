"""The generic solver instructions (OP_SOLVE_ROW, OP_LIMBS, OP_COUNTN) through the cooperative solver, on the synthetic circuits of
tests/synth_generic.py.  Every case sets its circuit up on the device and its all-inputs twin by the oracle under the same seed
(same verifying key), loads the circuit with 6-bit windows, and at 1, 3, 64 and 65 proofs requires: the plan statistics name the
generic rows and run-time divisions the circuit was built with and at least one level item; the status words; every wire of the
column the library keeps equal to the big-integer model; proof and public-witness bytes of EVERY row equal to the oracle's on the
twin under the same blinding and mask; the same bytes under SPP_NO_COOP=1 (the lane path: no generic rows in the plan),
SPP_NO_LEVEL_STREAM=1 and SPP_COOP_ONE_TRACK=1; one spoiled row in the middle refused alone.  Integers and bytes: no tolerance."""
import os
import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None

import synth_circuits as S
import synth_generic as SG

pytestmark = pytest.mark.gpu

SPP_ERR_UNSAT = -4
BATCH_SIZES = (1, 3, 64, 65)
SWITCH_VARS = ("SPP_NO_COOP", "SPP_NO_LEVEL_STREAM", "SPP_COOP_ONE_TRACK", "SPP_COOP_MAX", "SPP_NO_SPLIT")
VARIANTS = {"no_coop": "SPP_NO_COOP", "no_level_stream": "SPP_NO_LEVEL_STREAM", "one_track": "SPP_COOP_ONE_TRACK"}
SEED = b"\x0e" * 32


@pytest.fixture(scope="module")
def ctx():
    import spp
    c = spp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def lab(ctx, tmp_path_factory):
    """name -> the circuit written and set up on the device, its twin written and set up by the oracle; once per module"""
    from oracle import native
    d = str(tmp_path_factory.mktemp("generic_gpu"))
    cache = {}

    def get(name):
        if name not in cache:
            g = SG.CASES[name]()
            sppc, pk, vk, tw, opk, ovk = (os.path.join(d, name + "." + e) for e in ("sppc", "pk", "vk", "twin.sppc", "o.pk", "o.vk"))
            S.write_sppc(g.desc, sppc)
            S.write_sppc(SG.twin(g.desc), tw)
            ctx.setup(sppc, SEED, pk, vk)
            native.setup(tw, SEED, opk, ovk)
            same = open(vk, "rb").read() == open(ovk, "rb").read()
            cache[name] = dict(g=g, sppc=sppc, pk=pk, same_vk=same, orc=native.Prover(tw, opk), want={})
        return cache[name]
    return get


def _clear(monkeypatch):
    for k in SWITCH_VARS:
        monkeypatch.delenv(k, raising=False)


def _expected(case, key, rows, rs):
    """per row: (oracle's return code, proof, public witness, every wire by the model), once per (circuit, batch)"""
    if key not in case["want"]:
        g, orc = case["g"], case["orc"]
        cw = g.desc.challenge_wire
        out = []
        for row, (r, s) in zip(rows, rs):
            first = SG.model(g.desc, row, rs=(r, s))                       # phase 1 is right, the challenge is not there yet
            chal = orc.prove(first[1:], r, s, want_wires=True)[3][cw]      # the oracle runs the commitment step
            w = SG.model(g.desc, row, challenge=chal, rs=(r, s))
            rc, proof, pw = orc.prove(w[1:], r, s)
            out.append((rc, proof, pw, w))
        case["want"][key] = out
    return case["want"][key]


def _kept_column(count):
    return count - count % 64 if (count > 64 and count % 64) else 0


def _prove_and_compare(h, name, rows, rs, want, bad=()):
    proofs, pws, status = h.prove_batch(rows, rs)
    for i, (rc, proof, pw, _) in enumerate(want):
        if rc != 0 or i in bad:
            assert status[i] == SPP_ERR_UNSAT and proofs[i] == bytes(388), (name, i, status[i])
        else:
            assert status[i] == 0, (name, i, status[i])
            assert proofs[i] == proof and pws[i] == pw, (name, i)


@pytest.mark.parametrize("name,count", [(n, c) for n in SG.CASES for c in BATCH_SIZES])
def test_generic_circuits_on_the_cooperative_solver(ctx, lab, monkeypatch, name, count):
    case = lab(name)
    g = case["g"]
    assert case["same_vk"], "the device's key of the circuit differs from the oracle's key of its twin"
    pool = [g.inputs(1 + i) for i in range(min(count, 5))]
    rows = [pool[i % len(pool)] for i in range(count)]
    rs = [(11 + 3 * i, 1000003 + 7 * i) for i in range(count)]
    want = _expected(case, count, rows, rs)
    zero = g.expect["zero_rows"]
    assert all((rc != 0) == bool(zero) for rc, _, _, _ in want)
    if zero:            # the rows with a zero divisor get 0: the model says so, and the oracle refuses the witness for them
        k0 = g.desc.program.index(SG.OP_SOLVE_ROW)
        assert [want[0][3][g.desc.A[g.desc.program[k0 + 1] + i][-1][0]] == 0 for i in range(70)] == [i in zero for i in range(70)]
    _clear(monkeypatch)
    h = ctx.load_circuit(case["sppc"], case["pk"], 6)
    try:
        stats = h.plan_stats()
        assert stats["generic_rows"] == g.expect["generic_rows"] and stats["generic_divs"] == g.expect["generic_divs"], (name, stats)
        assert stats["items_levels"] + stats["items_level_stream"] > 0, (name, stats)
        if name == "longrow":
            assert stats["items_levels"] == 1 and stats["items_level_stream"] >= 1, stats
        if name == "limbs":
            assert stats["items_par"] == 1, stats
        if name == "tracks":
            assert stats["tracks"] >= 2, stats
        _prove_and_compare(h, name, rows, rs, want)
        i0 = _kept_column(count)
        assert h.debug_witness() == want[i0][3], (name, count, "witness")
        if count > 1 and not zero:
            mid = count // 2
            spoiled = list(rows)
            spoiled[mid] = g.spoil(rows[mid])[0]
            _prove_and_compare(h, name, spoiled, rs, want, bad=(mid,))
    finally:
        h.close()
    for v, var in VARIANTS.items():
        _clear(monkeypatch)
        monkeypatch.setenv(var, "1")
        h = ctx.load_circuit(case["sppc"], case["pk"], 6)
        try:
            off = h.plan_stats()
            if v == "no_coop":
                assert off["generic_rows"] == 0 and off["generic_divs"] == 0, (name, off)
            else:
                assert off["generic_rows"] == stats["generic_rows"] and off["generic_divs"] == stats["generic_divs"], (name, v, off)
            if v == "no_level_stream":
                assert off["items_level_stream"] == 0 and off["items_levels"] == stats["items_levels"] + stats["items_level_stream"], (name, off)
            _prove_and_compare(h, name + "/" + v, rows, rs, want)
            assert h.debug_witness() == want[_kept_column(count)][3], (name, count, v, "witness")
        finally:
            h.close()
    _clear(monkeypatch)
