"""The ceremony end to end on the GPU: sigma contributions on a derived key against big integers with every refusal, the whole
chain transcript contributions -> derive -> delta contribution -> sigma contribution on the withdraw circuit with proofs byte for
byte against the oracle, and the same chain through the command line."""
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

ENTROPY_1 = bytes(range(32))
ENTROPY_2 = bytes(range(100, 132))
ENTROPY_3 = bytes(range(200, 232))


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


# --------------------------------------------------------------------------------------------------------------------------
# 6. sigma
# --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sigma_link(ctx, tmp_path_factory):
    """gen_div(20) derived from the transcript of (5, 6, 7): k0; k0 -> (sigma, ENTROPY_1) k1; k0 -> (delta, ENTROPY_2) kd"""
    import ptau_format as F
    import synth_circuits as S
    tmp = tmp_path_factory.mktemp("sigma")
    p = lambda name: str(tmp / name)
    S.write_sppc(S.gen_div(20).desc, p("c.sppc"))
    _write(p("t.ptau"), F.transcript(6, 5, 6, 7))
    ctx.setup_from_ptau(p("c.sppc"), p("t.ptau"), p("k0.pk"), p("k0.vk"))
    r1 = ctx.setup_contribute_sigma(p("k0.pk"), p("k0.vk"), p("k1.pk"), p("k1.vk"), ENTROPY_1)
    rd = ctx.setup_contribute(p("k0.pk"), p("k0.vk"), p("kd.pk"), p("kd.vk"), ENTROPY_2)
    return dict(tmp=tmp, pk0=p("k0.pk"), vk0=p("k0.vk"), pk1=p("k1.pk"), vk1=p("k1.vk"), r1=r1, pkd=p("kd.pk"), vkd=p("kd.vk"), rd=rd)


def test_sigma_contribution_every_byte(ctx, sigma_link):
    import ptau_format as F
    import sppk_format as S
    from spp import lib
    c = sigma_link
    assert len(S.Sppk(_read(c["pk0"])).points["CS"]) >= 2
    want = F.sigma_contributed(_read(c["pk0"]), _read(c["vk0"]), *F.sigma_secrets(ENTROPY_1))
    assert (_read(c["pk1"]), _read(c["vk1"]), c["r1"]) == want
    again = [str(c["tmp"] / n) for n in ("again.pk", "again.vk")]
    assert ctx.setup_contribute_sigma(c["pk0"], c["vk0"], again[0], again[1], ENTROPY_1) == c["r1"]
    assert (_read(again[0]), _read(again[1])) == want[:2]
    assert ctx.setup_verify_sigma_contribution(c["pk0"], c["vk0"], c["pk1"], c["vk1"], c["r1"]) == (True, lib.SPP_SIGMA_OK)


@pytest.mark.parametrize("case", ["cs_point_replaced", "a_section_byte", "vk_point_kept_old", "z_plus_one", "cs_point_off_curve", "truncated"])
def test_sigma_refusals_name_their_reason(ctx, sigma_link, case):
    import sppk_format as S
    from oracle import bn254 as O
    from spp import lib
    c = sigma_link
    pk, vk, receipt = S.Sppk(_read(c["pk1"])), S.Vk(_read(c["vk1"])), c["r1"]
    pk_bytes = None
    if case == "cs_point_replaced":
        pk.points["CS"][1], want = O.g1_to_bytes(O.g1_mul(O.G1_GEN, 12345)), "SCALING"
    elif case == "a_section_byte":
        pk.points["A"][0], want = pk.points["A"][0][:-1] + bytes([pk.points["A"][0][-1] ^ 1]), "NOT_A_SIGMA_CHANGE"
    elif case == "vk_point_kept_old":
        vk.tail, want = S.Vk(_read(c["vk0"])).tail, "VK"
    elif case == "z_plus_one":
        z = (int.from_bytes(receipt[128:], "big") + 1) % O.R
        receipt, want = receipt[:128] + z.to_bytes(32, "big"), "RECEIPT"
    elif case == "cs_point_off_curve":
        x, y = O.g1_from_bytes(pk.points["CS"][1])
        pk.points["CS"][1], want = O.g1_to_bytes((x, (y + 1) % O.P)), "POINT_INVALID"
    else:
        pk_bytes, want = pk.to_bytes()[:-10], "FORMAT"
    pk_t = _write(str(c["tmp"] / (case + ".pk")), pk.to_bytes() if pk_bytes is None else pk_bytes)
    vk_t = _write(str(c["tmp"] / (case + ".vk")), vk.to_bytes())
    got = ctx.setup_verify_sigma_contribution(c["pk0"], c["vk0"], pk_t, vk_t, receipt)
    assert got == (False, lib.SIGMA_REASON_NAMES.index(want)), "%s: %s" % (case, lib.SIGMA_REASON_NAMES[got[1]])


def test_each_verifier_refuses_the_other_kind_of_link(ctx, sigma_link):
    from spp import lib
    c = sigma_link
    assert ctx.setup_verify_contribution(c["pk0"], c["vk0"], c["pk1"], c["vk1"], c["r1"]) == (False, lib.SPP_CONTRIB_NOT_A_DELTA_CHANGE)
    assert ctx.setup_verify_sigma_contribution(c["pk0"], c["vk0"], c["pkd"], c["vkd"], c["rd"]) == (False, lib.SPP_SIGMA_NOT_A_SIGMA_CHANGE)
    assert ctx.setup_verify_contribution(c["pk0"], c["vk0"], c["pkd"], c["vkd"], c["rd"]) == (True, lib.SPP_CONTRIB_OK)   # a derived key takes delta links


def test_sigma_needs_committed_wires(ctx, tmp_path):
    import spp
    import sppk_format as S
    import synth_circuits as C
    from oracle import native
    from spp import lib
    sppc, pk, vk = (str(tmp_path / ("k." + e)) for e in ("sppc", "pk", "vk"))
    C.write_sppc(C.gen_tiny().desc, sppc)
    native.setup(sppc, b"\x05" * 32, pk, vk)
    key = S.Sppk(_read(pk))
    key.points["CB"], key.wires["CB"], key.points["CS"], key.wires["CS"] = [], [], [], []
    _write(pk, key.to_bytes())
    with pytest.raises(spp.SppError) as e:
        ctx.setup_contribute_sigma(pk, vk, str(tmp_path / "o.pk"), str(tmp_path / "o.vk"), ENTROPY_1)
    assert e.value.code == lib.SPP_ERR_BAD_INPUT


# --------------------------------------------------------------------------------------------------------------------------
# 7. the whole chain on the withdraw circuit
# --------------------------------------------------------------------------------------------------------------------------
def test_whole_chain_on_the_withdraw_circuit(ctx, withdraw_artifacts, withdraw_kat, tmp_path):
    import spp
    from oracle import native, circuit as C
    from spp import lib
    from test_gpu_setup_ceremony import _another_note
    sppc = withdraw_artifacts["sppc"]
    p = lambda name: str(tmp_path / name)
    ctx.ptau_new(14, p("t0.ptau"))
    r1 = ctx.ptau_contribute(p("t0.ptau"), p("t1.ptau"), ENTROPY_1)
    r2 = ctx.ptau_contribute(p("t1.ptau"), p("t2.ptau"), ENTROPY_2)
    assert ctx.ptau_verify_contribution(p("t0.ptau"), p("t1.ptau"), r1) == (True, lib.SPP_PTAU_OK)
    assert ctx.ptau_verify_contribution(p("t1.ptau"), p("t2.ptau"), r2) == (True, lib.SPP_PTAU_OK)
    ctx.setup_from_ptau(sppc, p("t2.ptau"), p("k0.pk"), p("k0.vk"))
    rd = ctx.setup_contribute(p("k0.pk"), p("k0.vk"), p("k1.pk"), p("k1.vk"), ENTROPY_3)
    assert ctx.setup_verify_contribution(p("k0.pk"), p("k0.vk"), p("k1.pk"), p("k1.vk"), rd) == (True, lib.SPP_CONTRIB_OK)
    rs = ctx.setup_contribute_sigma(p("k1.pk"), p("k1.vk"), p("k2.pk"), p("k2.vk"), ENTROPY_1)
    assert ctx.setup_verify_sigma_contribution(p("k1.pk"), p("k1.vk"), p("k2.pk"), p("k2.vk"), rs) == (True, lib.SPP_SIGMA_OK)
    rows, blind = [C.withdraw_inputs(withdraw_kat), _another_note(31)], [(3, 4), (5, 6)]
    h = ctx.load_circuit(sppc, p("k2.pk"), 6)                        # the final key through the existing loader
    try:
        proofs, pws, status = h.prove_batch(rows, blind)
    finally:
        h.close()
    assert status == [0, 0]
    orc = native.Prover(sppc, p("k2.pk"))
    vk_final, vk_derived = _read(p("k2.vk")), _read(p("k0.vk"))
    for row, (r, s), proof, pw in zip(rows, blind, proofs, pws):
        rc, want_proof, want_pw = orc.prove(row, r, s)
        assert rc == 0 and proof == want_proof and pw == want_pw
        assert spp.verify(vk_final, proof, pw)
        assert not spp.verify(vk_derived, proof, pw)
        flipped = proof[:100] + bytes([proof[100] ^ 1]) + proof[101:]
        assert not spp.verify(vk_final, flipped, pw)


# --------------------------------------------------------------------------------------------------------------------------
# 8. the command line: new, two contributions, verify, derive, a sigma contribution and its verification
# --------------------------------------------------------------------------------------------------------------------------
def test_command_line_from_the_transcript_to_a_key(ctx, tmp_path, capsys):
    import ptau_format as F
    import synth_circuits as S
    from spp import cli
    p = lambda *name: str(tmp_path.joinpath(*name))
    S.write_sppc(S.gen_tiny().desc, p("tiny.sppc"))
    assert cli.main(["ptau-new", "3", "--out", p("t.ptau")]) == 0
    assert cli.main(["ptau-contribute", p("t.ptau"), "--out", p("c1"), "--entropy", ENTROPY_1.hex()]) == 0
    assert cli.main(["ptau-contribute", p("c1", "t.ptau"), "--out", p("c2"), "--entropy", ENTROPY_2.hex()]) == 0
    capsys.readouterr()
    assert cli.main(["ptau-verify", p("t.ptau"), p("c1", "t.ptau"), p("c1", "t.receipt"), p("c2", "t.ptau"), p("c2", "t.receipt")]) == 0
    assert "2 links verified" in capsys.readouterr().out
    assert cli.main(["setup-derive", p("tiny.sppc"), p("c2", "t.ptau"), "--out", p("k0")]) == 0
    s1, s2 = F.contribution_secrets(ENTROPY_1), F.contribution_secrets(ENTROPY_2)
    from oracle import bn254 as O
    want = F.derived_key(S.gen_tiny().desc, *(x * y % O.R for x, y in zip(s1[:3], s2[:3])))
    assert (_read(p("k0", "tiny.pk")), _read(p("k0", "tiny.vk"))) == want
    assert cli.main(["setup-contribute-sigma", p("k0", "tiny.pk"), p("k0", "tiny.vk"), "--out", p("k1"), "--entropy", ENTROPY_3.hex()]) == 0
    capsys.readouterr()
    link = [p("k0", "tiny.pk"), p("k0", "tiny.vk"), p("k1", "tiny.pk"), p("k1", "tiny.vk"), p("k1", "tiny.receipt")]
    assert cli.main(["setup-verify-sigma"] + link) == 0
    assert "1 links verified" in capsys.readouterr().out
    assert cli.main(["setup-verify"] + link) == 1                    # the delta verifier does not take a sigma link
    assert "link 1" in capsys.readouterr().out
    assert cli.main(["setup-derive", p("tiny.sppc"), p("missing.ptau"), "--out", p("k9")]) == 2
