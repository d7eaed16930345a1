"""Lookup-inverse wires summed by byte bucket (csrc/msm_lookup.hpp, csrc/kernels_msm_lookup.hip) on synthetic circuits with a
log-derivative range check (tests/synth_lookup_circuits.py), loaded with the throughput layout (window_bits = 0, flat A and K sets)
under a small table budget and with the path's threshold lowered to 64 proofs (SPP_LOOKUP_BUCKETS=64).  Every case: proofs and
public witnesses of every row equal the C oracle's and equal the same library's with the path off (SPP_LOOKUP_BUCKETS=0); a row
that looks up 256 is refused through its status word, alone.  No tolerance: bytes."""
import os

import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None

import synth_circuits as S
import synth_lookup_circuits as SL

pytestmark = pytest.mark.gpu

SPP_ERR_UNSAT = -4


@pytest.fixture(scope="module")
def ctx():
    import spp
    c = spp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def lab(ctx, tmp_path_factory):
    """L -> the circuit written, set up and loaded by the oracle, once for the module"""
    from oracle import native
    d = str(tmp_path_factory.mktemp("lookup_gpu"))
    cache = {}

    def get(L):
        if L not in cache:
            g = SL.gen_lookup(L)
            sppc, pk, vk = (os.path.join(d, "l%d.%s" % (L, e)) for e in ("sppc", "pk", "vk"))
            S.write_sppc(g.desc, sppc)
            native.setup(sppc, b"\x0e" * 32, pk, vk)
            cache[L] = dict(g=g, sppc=sppc, pk=pk, orc=native.Prover(sppc, pk), want={})
        return cache[L]
    return get


def _values(kind, L, i):
    """the looked-up bytes of row i"""
    if kind == "all":         # every byte 0 .. 255 present, in another rotation per row
        return [(t + 37 * i) % 256 for t in range(L)]
    if kind == "equal":       # one bucket: a chain of additions (and another bucket per row)
        return [(11 * i + 5) % 256] * L
    if kind == "ends":        # bytes 0 and 255 only
        return [255 if (t * (i + 3) + i) % 3 else 0 for t in range(L)]
    return None               # random


def _load(ctx, case, monkeypatch, switch):
    monkeypatch.setenv("SPP_TABLE_BUDGET_GB", "0.25")
    monkeypatch.setenv("SPP_LOOKUP_BUCKETS", switch)
    return ctx.load_circuit(case["sppc"], case["pk"], 0)


CASES = [(1, "random", 130), (63, "random", 130), (64, "random", 130), (65, "random", 130), (300, "all", 130), (300, "equal", 130),
         (300, "ends", 130), (300, "all", 64), (300, "all", 65)]


@pytest.mark.parametrize("L,kind,count", CASES)
def test_bucket_sums_give_the_oracles_bytes(ctx, lab, monkeypatch, L, kind, count):
    """L = 1; 63 / 64 / 65 lookups (a partial table block, a full one, a straddle); 300 lookups with every byte present, all equal,
    bytes 0 and 255 only.  130 proofs are a body of 128 on the path and a tail of 2 on the table walks; 64 is the threshold itself;
    65 leaves a tail of one.  Every row is a different witness."""
    from oracle import native
    case = lab(L)
    g = case["g"]
    rows = [g.inputs(100 + i, values=_values(kind, L, i)) for i in range(count)]
    rs = [(13 + 5 * i, 2000003 + 11 * i) for i in range(count)]
    key = (kind, count)
    if key not in case["want"]:
        rc, proofs, pws = native.prove_many(case["orc"], rows, rs)
        assert rc == 0
        case["want"][key] = (proofs, pws)
    want_proofs, want_pws = case["want"][key]
    assert len(set(want_proofs)) == count
    bad_i = count // 2 + 1
    spoiled = list(rows)
    spoiled[bad_i] = g.spoil(rows[bad_i], lookup=L // 2, value=256)[0]

    h = _load(ctx, case, monkeypatch, "64")
    try:
        trows = h.msm_table_rows()
        assert trows[0] == 1 and trows[2] == 1, trows                  # A and K took the flat layout
        assert h.lookup_buckets() == [L, 64]                           # the scan found every inverse; the threshold is the switch's
        proofs, pws, status = h.prove_batch(rows, rs)
        p2, w2, st2 = h.prove_batch(spoiled, rs)
    finally:
        h.close()
    assert status == [0] * count
    assert proofs == want_proofs and pws == want_pws, [i for i in range(count) if proofs[i] != want_proofs[i]][:8]
    assert st2 == [SPP_ERR_UNSAT if i == bad_i else 0 for i in range(count)]
    for i in range(count):
        if i == bad_i:
            assert p2[i] == b"\x00" * 388
        else:
            assert p2[i] == want_proofs[i] and w2[i] == want_pws[i], i

    h = _load(ctx, case, monkeypatch, "0")
    try:
        assert h.lookup_buckets() == [0, 0]
        proofs0, pws0, status0 = h.prove_batch(rows, rs)
    finally:
        h.close()
    assert status0 == [0] * count and proofs0 == proofs and pws0 == pws
