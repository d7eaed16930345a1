"""From a powers-of-tau transcript to a key on the GPU: the inverse NTT over group elements through its unit entry points against
oracle/bn254.py big integers, and spp_setup_from_ptau byte for byte against the oracle's seeded setup brought to gamma = delta =
sigma = rho = 1 (tests/ptau_format.py)."""
import os
import random
import sys

import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

TAU = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % 21888242871839275222246405745257275088548364400416034343698204186575808495617
# k_ec_ntt_pass runs one lane per output element in workgroups of 64, a transform's n / 2 sums before its n / 2 differences: n = 64 is
# one workgroup, n = 128 the smallest size with two (and the smallest where whole waves hold only sums or only differences)
LOG_TWO_WORKGROUPS = 7


@pytest.fixture(scope="module")
def ctx():
    import spp
    c = spp.Context(0)
    yield c
    c.close()


def _read(path):
    with open(path, "rb") as f:
        return f.read()


class Group:
    def __init__(self, name):
        from oracle import bn254 as O
        self.name = name
        g1 = name == "g1"
        self.gen, self.size = (O.G1_GEN, 64) if g1 else (O.G2_GEN, 128)
        self.add, self.mul, self.neg = (O.g1_add, O.g1_mul, O.g1_neg) if g1 else (O.g2_add, O.g2_mul, O.g2_neg)
        self.to_bytes = O.g1_to_bytes if g1 else O.g2_to_bytes

    def intt(self, ctx, pts, log):
        call = ctx.ec_intt_g1 if self.name == "g1" else ctx.ec_intt_g2
        out = call(b"".join(self.to_bytes(p) for p in pts), log)
        return [out[self.size * i:self.size * (i + 1)] for i in range(1 << log)]

    def msm(self, ctx, raw_points, scalars):
        return (ctx.msm_g1 if self.name == "g1" else ctx.msm_g2)(b"".join(raw_points), scalars)


@pytest.fixture(scope="module", params=["g1", "g2"])
def G(request):
    return Group(request.param)


def _powers(G, tau, n):
    from oracle import bn254 as O
    return [G.mul(G.gen, pow(tau, i, O.R)) for i in range(n)]


# --------------------------------------------------------------------------------------------------------------------------
# 2. the group inverse NTT
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log", [1, 2, 3, 6])
def test_intt_of_powers_gives_the_lagrange_points(ctx, G, log):
    import ptau_format as F
    got = G.intt(ctx, _powers(G, TAU, 1 << log), log)
    want = [G.to_bytes(G.mul(G.gen, l)) for l in F.lagrange_at(TAU, log)]
    assert got == want, [k for k in range(1 << log) if got[k] != want[k]]


def test_intt_across_two_workgroups(ctx, G):
    """every output through identities over calls that exist and are tested against the oracle: the outputs sum to the generator
    (the L_k sum to one), and sum_k w^(j k) L_k is input j; then 32 outputs against big integers"""
    import ptau_format as F
    from oracle import bn254 as O
    log = LOG_TWO_WORKGROUPS
    n, w = 1 << log, F.omega(log)
    pts = _powers(G, TAU, n)
    got = G.intt(ctx, pts, log)
    assert G.msm(ctx, got, [1] * n) == G.to_bytes(G.gen)
    rng = random.Random(5)
    for j in [0, n - 1] + [rng.randrange(n) for _ in range(6)]:
        assert G.msm(ctx, got, [pow(w, j * k, O.R) for k in range(n)]) == G.to_bytes(pts[j]), j
    L = F.lagrange_at(TAU, log)
    for k in [0, 1, n // 2 - 1, n // 2, n - 1] + [rng.randrange(n) for _ in range(27)]:
        assert got[k] == G.to_bytes(G.mul(G.gen, L[k])), k


@pytest.mark.parametrize("log", [3, LOG_TWO_WORKGROUPS])
def test_intt_of_equal_points(ctx, G, log):
    """the transcript of tau = 1: every first-stage difference is infinity and every sum a doubling; output 0 is the point itself"""
    n = 1 << log
    got = G.intt(ctx, [G.gen] * n, log)
    assert got[0] == G.to_bytes(G.gen) and all(x == bytes(G.size) for x in got[1:])


def test_intt_with_an_opposite_pair_a_repeated_point_and_infinity(ctx, G):
    import ptau_format as F
    from oracle import bn254 as O
    rng = random.Random(6)
    p, q = (G.mul(G.gen, rng.randrange(1, O.R)) for _ in range(2))
    pts = [p, q, q, None, G.neg(p), q, G.neg(q), p]           # (0, 4) opposite and (1, 5) equal in the first stage
    got = G.intt(ctx, pts, 3)
    assert got == [G.to_bytes(x) for x in F.group_intt(pts, 3, G.add, G.mul)]


def test_intt_refuses_what_is_no_point_and_sizes_out_of_range(ctx, G):
    import spp
    from oracle import bn254 as O
    from spp import lib
    g = G.to_bytes(G.gen)
    call = ctx.ec_intt_g1 if G.name == "g1" else ctx.ec_intt_g2
    off_curve = g[:-32] + O.fe_be((int.from_bytes(g[-32:], "big") + 1) % O.P)
    above_q = O.fe_be(int.from_bytes(g[:32], "big") + O.P) + g[32:]
    for points, log in ((g + off_curve, 1), (above_q + g, 1), (g, 0)):
        with pytest.raises(spp.SppError) as e:
            call(points, log)
        assert e.value.code == lib.SPP_ERR_BAD_INPUT


# --------------------------------------------------------------------------------------------------------------------------
# 5. the derivation against the oracle's setup
# --------------------------------------------------------------------------------------------------------------------------
def _circuit(tmp, gen):
    import synth_circuits as S
    sppc = str(tmp / "c.sppc")
    S.write_sppc(gen.desc, sppc)
    return sppc


def _derive(ctx, tmp, sppc, transcript_bytes, tag):
    pt, pk, vk = (str(tmp / (tag + e)) for e in (".ptau", ".pk", ".vk"))
    with open(pt, "wb") as f:
        f.write(transcript_bytes)
    ctx.setup_from_ptau(sppc, pt, pk, vk)
    return _read(pk), _read(vk)


def _against_the_reference(ctx, tmp, gen, seed, kz_points):
    import ptau_format as F
    import sppk_format as S
    import verify_vectors as V
    from oracle import native
    sppc = _circuit(tmp, gen)
    log = gen.desc.domain_log
    tau, alpha, beta, gamma, delta, _, _ = V.trapdoor(seed)
    ref_pk, ref_vk = str(tmp / "ref.pk"), str(tmp / "ref.vk")
    native.setup(sppc, seed, ref_pk, ref_vk)
    want_pk, want_vk = F.derived_from_reference(_read(ref_pk), _read(ref_vk), gamma, delta)
    assert (want_pk, want_vk) == F.derived_key(gen.desc, tau, alpha, beta)      # the two restatements agree
    key = S.Sppk(want_pk)
    assert len(key.points["K"]) + len(key.points["Z"]) == kz_points
    transcript = F.transcript(log, tau, alpha, beta)
    got_pk, got_vk = _derive(ctx, tmp, sppc, transcript, "t")
    assert got_pk == want_pk
    assert got_vk == want_vk
    return sppc, log, (tau, alpha, beta), want_pk, want_vk


def test_derivation_on_the_tiny_circuit(ctx, tmp_path):
    import synth_circuits as S
    g = S.gen_tiny()
    assert g.expect["domain_log"] == 3
    _against_the_reference(ctx, tmp_path, g, b"\x05" * 32, 4 + 7)


def test_derivation_over_several_waves_and_transcripts_of_other_sizes(ctx, tmp_path):
    import ptau_format as F
    import spp
    import synth_circuits as S
    from spp import lib
    g = S.gen_div(20)
    sppc, log, secrets, want_pk, want_vk = _against_the_reference(ctx, tmp_path, g, b"\x06" * 32, 164)   # 101 K + 63 Z points
    assert log == 6
    # a larger transcript serves: a prefix of the powers is a transcript
    assert _derive(ctx, tmp_path, sppc, F.transcript(7, *secrets), "t7") == (want_pk, want_vk)
    # a smaller one does not
    with pytest.raises(spp.SppError) as e:
        _derive(ctx, tmp_path, sppc, F.transcript(5, *secrets), "t5")
    assert e.value.code == lib.SPP_ERR_BAD_INPUT
    # the derivation is deterministic
    assert _derive(ctx, tmp_path, sppc, F.transcript(6, *secrets), "again") == (want_pk, want_vk)


@pytest.mark.parametrize("which", ["tiny", "div"])
def test_derivation_from_the_new_transcript(ctx, tmp_path, which):
    """tau = 1 is the first point of the domain: L_0 = G, every other Lagrange point and every Z point infinity, so A_j = A[0][j] G"""
    import ptau_format as F
    import sppk_format as S
    import synth_circuits as C
    g = C.gen_tiny() if which == "tiny" else C.gen_div(20)
    sppc = _circuit(tmp_path, g)
    t0 = str(tmp_path / "new.ptau")
    ctx.ptau_new(g.desc.domain_log, t0)
    got_pk, got_vk = _derive(ctx, tmp_path, sppc, _read(t0), "new")
    assert (got_pk, got_vk) == F.derived_key(g.desc, 1, 1, 1)
    key = S.Sppk(got_pk)
    assert all(z == bytes(64) for z in key.points["Z"]) and key.wires["A"] == sorted({w for w, v in g.desc.A[0] if v})


def test_derivation_refuses_a_transcript_with_a_bad_point(ctx, tmp_path):
    import ptau_format as F
    import spp
    import synth_circuits as S
    from spp import lib
    g = S.gen_tiny()
    sppc = _circuit(tmp_path, g)
    good = F.transcript(3, 5, 6, 7)
    for case in ("t1_point_off_curve", "t2_point_off_subgroup"):
        data, _, _ = F.tampered(case, good, good, bytes(480), good)
        with pytest.raises(spp.SppError) as e:
            _derive(ctx, tmp_path, sppc, data, case)
        assert e.value.code == lib.SPP_ERR_FORMAT, case
