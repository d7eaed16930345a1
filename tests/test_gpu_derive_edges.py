"""spp_setup_from_ptau on the circuits of tests/derive_circuits.py and on transcripts whose secrets make points meet: every assertion
is byte equality of the derived (pk, vk) with ptau_format.derived_key's big integers, and a mismatch names the first section and wire
that differ.  Every kind of coefficient through the gather's scalar loop in G1 and G2, columns around the chunk size and one of more
than a wave of chunks, sums that double, cancel and restart, alpha == beta and alpha or beta = -1, tau on the domain (the transform
meets equal and opposite points in every stage), tau a primitive 2n-th root (every Z point through the doubling), the smallest domain,
and a transcript larger than the circuit needs.

Transcripts and expected keys are big-integer products in Python (about 2 ms in G1, 12 ms in G2): each is built once for the module."""
import os
import sys

import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import spp
    c = spp.Context(0)
    yield c
    c.close()


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return path


class Bench:
    """the module's circuits on disk, its transcripts and its expected keys, each made once"""

    def __init__(self, tmp):
        import derive_circuits as D
        import synth_circuits as S
        self.tmp = tmp
        self.crafted = {name: gen() for name, gen in D.GENERATORS.items()}
        self.sppc = {}
        for name, g in self.crafted.items():
            self.sppc[name] = str(tmp / (name + ".sppc"))
            S.write_sppc(g.desc, self.sppc[name])
        self._transcripts, self._keys, self._count = {}, {}, 0

    def transcript(self, log, secrets):
        import ptau_format as F
        if (log, secrets) not in self._transcripts:
            self._transcripts[(log, secrets)] = F.transcript(log, *secrets)
        return self._transcripts[(log, secrets)]

    def want(self, name, secrets):
        import ptau_format as F
        if (name, secrets) not in self._keys:
            self._keys[(name, secrets)] = F.derived_key(self.crafted[name].desc, *secrets)
        return self._keys[(name, secrets)]

    def derive(self, ctx, name, transcript_bytes):
        self._count += 1
        pt, pk, vk = (str(self.tmp / ("d%d%s" % (self._count, e))) for e in (".ptau", ".pk", ".vk"))
        _write(pt, transcript_bytes)
        ctx.setup_from_ptau(self.sppc[name], pt, pk, vk)
        return _read(pk), _read(vk)


@pytest.fixture(scope="module")
def bench(tmp_path_factory):
    return Bench(tmp_path_factory.mktemp("edges"))


def first_difference(got, want):
    """the first (section, wire) at which two (pk, vk) pairs differ, None when they are equal"""
    import sppk_format as S
    if got == want:
        return None
    try:
        g, w = S.Sppk(got[0]), S.Sppk(want[0])
    except ValueError as e:
        return "the proving key does not parse: %s" % e
    for field in ("header", "alpha1", "beta1", "delta1", "beta2", "delta2"):
        if getattr(g, field) != getattr(w, field):
            return "pk " + field
    for sec in ("A", "B1", "B2", "K", "Z", "CB", "CS"):
        if sec in w.wires and g.wires[sec] != w.wires[sec]:
            extra, missing = sorted(set(g.wires[sec]) - set(w.wires[sec])), sorted(set(w.wires[sec]) - set(g.wires[sec]))
            return "section %s lists other wires: %s too many, %s missing" % (sec, extra, missing)
        names = w.wires.get(sec, list(range(len(w.points[sec]))))
        if len(g.points[sec]) != len(w.points[sec]):
            return "section %s has %d points, not %d" % (sec, len(g.points[sec]), len(w.points[sec]))
        bad = [names[i] for i in range(len(names)) if g.points[sec][i] != w.points[sec][i]]
        if bad:
            return "section %s, wire %d (in all: %s)" % (sec, bad[0], bad) if sec != "Z" else "Z points %s" % bad
    gv, wv = S.Vk(got[1]), S.Vk(want[1])
    for field in ("alpha1", "beta1", "beta2", "gamma2", "delta1", "delta2", "tail"):
        if getattr(gv, field) != getattr(wv, field):
            return "vk " + field
    return "vk K %s" % [i for i in range(max(len(gv.K), len(wv.K))) if gv.K[i:i + 1] != wv.K[i:i + 1]]


def _check(ctx, bench, name, secrets, log=None):
    desc = bench.crafted[name].desc
    got = bench.derive(ctx, name, bench.transcript(log or desc.domain_log, secrets))
    diff = first_difference(got, bench.want(name, secrets))
    assert diff is None, "%s: %s" % (name, diff)
    return got


def _z_points(pk_bytes):
    import sppk_format as S
    return S.Sppk(pk_bytes).points["Z"]


def _generic():
    import derive_circuits as D
    return (D.TAU, D.ALPHA, D.BETA)


def test_first_difference_names_section_and_wire(bench):
    """the reporter on a key in big integers with one point of one wire replaced (no GPU call: the other tests' messages depend on it)"""
    import sppk_format as S
    want = bench.want("smallest", (5, 6, 7))
    key = S.Sppk(want[0])
    key.points["B2"][1] = key.points["B2"][0]
    assert first_difference((key.to_bytes(), want[1]), want).startswith("section B2, wire %d " % key.wires["B2"][1])
    key = S.Sppk(want[0])
    key.points["Z"][0] = bytes(64)
    assert first_difference((key.to_bytes(), want[1]), want) == "Z points [0]"
    assert first_difference(want, want) is None


# --------------------------------------------------------------------------------------------------------------------------
# generic secrets: what the columns hold is the edge
# --------------------------------------------------------------------------------------------------------------------------
def test_every_coefficient_kind(ctx, bench):
    """bit lengths 0, 1, 2, 28, 32 k and 32 k + 1 for every word, 253, both signs: the scalar loop of the gather in G1 (A, B1, K on
    three bases) and in G2 (B2), one wire per kind"""
    e = bench.crafted["coeff_kinds"].expect
    assert {0, 1, 32, 33, 224, 225, 253} <= e["bit_lengths"]
    _check(ctx, bench, "coeff_kinds", _generic())


def test_column_lengths_around_the_chunk_and_a_column_of_more_than_a_wave_of_chunks(ctx, bench):
    e = bench.crafted["column_shapes"].expect
    assert e["max_col_chunks"] > 64 and e["chunks_g1"] % 64 and e["chunks_g2"] % 64 and min(e["chunks_g1"], e["chunks_g2"]) > 64
    _check(ctx, bench, "column_shapes", _generic())


def test_a_larger_transcript_gives_the_same_key(ctx, bench):
    """only the prefix is used, and T1 is cut at 2 n - 1 of the circuit, not of the file"""
    assert bench.crafted["column_shapes"].desc.domain_log == 7
    _check(ctx, bench, "column_shapes", _generic(), log=8)


# --------------------------------------------------------------------------------------------------------------------------
# sums that meet what they hold
# --------------------------------------------------------------------------------------------------------------------------
def _meeting_secrets(which):
    import derive_circuits as D
    from oracle.bn254 import R
    return {"alpha_equals_beta": (D.TAU, D.ALPHA, D.ALPHA), "beta_minus_one": (D.TAU, 1, R - 1), "alpha_minus_one": (D.TAU, R - 1, 1)}[which]


@pytest.mark.parametrize("which", ["alpha_equals_beta", "beta_minus_one", "alpha_minus_one"])
def test_meetings_in_the_sums(ctx, bench, which):
    """doublings and cancellations inside a chunk (mixed and general addition, G1 and G2) and between chunks under every
    transcript; alpha == beta doubles the K columns of the `ab` wires and the partials of k_chunks, beta == -alpha cancels them:
    the wire leaves the K section, a committed or public one stays with the point at infinity"""
    import sppk_format as S
    g = bench.crafted["meetings"]
    got_pk, _ = _check(ctx, bench, "meetings", _meeting_secrets(which))
    key, v = S.Sppk(got_pk), g.expect["vanish"]
    gone = set(v["K"]) | set(v["K_equal"] if which == "alpha_equals_beta" else v["K_opposite"])
    assert not gone & set(key.wires["K"]) and (which == "alpha_equals_beta" or gone & set(g.desc.committed))
    assert all((p == bytes(64)) == (w in gone) for w, p in zip(key.wires["CB"], key.points["CB"]))
    assert not (set(v["A"]) & set(key.wires["A"])) and not (set(v["B"]) & (set(key.wires["B1"]) | set(key.wires["B2"])))


# --------------------------------------------------------------------------------------------------------------------------
# degenerate secrets: tau on the domain, tau a primitive 2n-th root
# --------------------------------------------------------------------------------------------------------------------------
K0 = 5                                   # neither 0 nor n / 2 of the 32-row domain


def _on_domain(which):
    import derive_circuits as D
    import ptau_format as F
    from oracle.bn254 import R
    return {"omega_k0": (pow(F.omega(5), K0, R), D.ALPHA, D.BETA), "minus_one": (R - 1, D.ALPHA, D.BETA)}[which]


@pytest.mark.parametrize("name", ["coeff_kinds", "meetings"])
@pytest.mark.parametrize("which", ["omega_k0", "minus_one"])
def test_tau_on_the_domain(ctx, bench, which, name):
    """L_k(tau) is the indicator of one row: every other Lagrange point is infinity, a column is what its terms on that row sum to"""
    assert bench.crafted[name].desc.domain_log == 5
    got_pk, _ = _check(ctx, bench, name, _on_domain(which))
    z = _z_points(got_pk)
    assert len(z) == 31 and all(p == bytes(64) for p in z)


def test_tau_of_order_four_on_the_128_row_domain(ctx, bench):
    """the transcript repeats with period 4: every stage of the transform but the last two sees only equal pairs, sums that double
    and differences at infinity"""
    import derive_circuits as D
    import ptau_format as F
    secrets = (F.omega(2), D.ALPHA, D.BETA)
    t = F.Ptau(bench.transcript(7, secrets))
    assert t.T1[4] == t.T1[0] and t.T1[1] != t.T1[0] and t.T1[2] != t.T1[0] and t.T2[5] == t.T2[1]
    got_pk, _ = _check(ctx, bench, "column_shapes", secrets)
    z = _z_points(got_pk)
    assert len(z) == 127 and all(p == bytes(64) for p in z)


@pytest.mark.parametrize("name", ["coeff_kinds", "column_shapes"])
def test_tau_a_primitive_root_of_twice_the_domain(ctx, bench, name):
    """tau^n = -1: T[i + n] == -T[i], so every Z point is -2 T[i], a doubling inside the mixed addition"""
    import derive_circuits as D
    import ptau_format as F
    from oracle import bn254 as O
    log = bench.crafted[name].desc.domain_log
    secrets = (F.omega(log + 1), D.ALPHA, D.BETA)
    t = F.Ptau(bench.transcript(log, secrets))
    n = 1 << log
    assert all(O.g1_from_bytes(t.T1[i + n]) == O.g1_neg(O.g1_from_bytes(t.T1[i])) for i in range(n - 1))
    got_pk, _ = _check(ctx, bench, name, secrets)
    z = _z_points(got_pk)
    assert len(z) == n - 1 and z[3] == O.g1_to_bytes(O.g1_mul(O.g1_from_bytes(t.T1[3]), O.R - 2))


# --------------------------------------------------------------------------------------------------------------------------
# the smallest domain
# --------------------------------------------------------------------------------------------------------------------------
def test_two_constraints(ctx, bench):
    """domain_log 1: one stage, one Z point; under a generic transcript and under the new one (tau = alpha = beta = 1)"""
    got_pk, _ = _check(ctx, bench, "smallest", _generic())
    assert len(_z_points(got_pk)) == 1
    t0 = str(bench.tmp / "new1.ptau")
    ctx.ptau_new(1, t0)
    got = bench.derive(ctx, "smallest", _read(t0))
    diff = first_difference(got, bench.want("smallest", (1, 1, 1)))
    assert diff is None, diff
    assert _z_points(got[0]) == [bytes(64)]
