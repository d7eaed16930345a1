"""CPU: every case of tests/verify_vectors.py -- simulated proofs, forgeries whose points are all on their curves, malformed
encodings -- gets the verdict it has by construction from the three host verifiers: the Python oracle (groth16.verify), the product's
single-proof verifier (spp.verify) and the g++ build of the header the GPU kernels compile (csrc/verify_one.hpp, through
tests/host/pairing_check.cpp <vk> <proof> <pw>).  Both keys: withdraw (5 public words) and audit (2).

The pure-Python pairing takes about a second per case, so the list is cut into groups of GROUP cases, a test each.  A case on which
the oracle and the construction disagree means the oracle (or the case) is wrong and comes before anything else.
tests/test_gpu_verify_forged.py puts the same list through the gfx950 build."""
import os
import random
import subprocess

import pytest

from conftest import ROOT, GOLDEN
import verify_vectors as V

SEEDS = {"withdraw": b"\x07" * 32, "audit": b"\x09" * 32}               # conftest.py: withdraw_artifacts / audit_artifacts
NPUB = {"withdraw": 5, "audit": 2}
GROUP = 6
SPP_ERR_FORMAT = -7


@pytest.fixture(scope="module")
def keys(withdraw_artifacts, audit_artifacts):
    return {"withdraw": open(withdraw_artifacts["vk"], "rb").read(), "audit": open(audit_artifacts["vk"], "rb").read()}


@pytest.fixture(scope="module")
def case_lists(keys):
    return {k: V.cases(keys[k], V.trapdoor(SEEDS[k]), NPUB[k], random.Random(2024 + NPUB[k])) for k in keys}


@pytest.fixture(scope="module")
def verify_one_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("verify_one") / "pairing_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "pairing_check.cpp"), "-o", exe], check=True)
    return exe


def _spp_verdict(vk, proof, pw):
    """spp.verify answers False, or raises SPP_ERR_FORMAT for a commitment count or a witness header it does not read: both refuse"""
    import spp
    try:
        return spp.verify(vk, proof, pw)
    except spp.SppError as e:
        assert e.code == SPP_ERR_FORMAT, e
        return False


def _verify_one_verdict(exe, d, vk_path, proof, pw):
    pr, pwf = os.path.join(d, "p.proof"), os.path.join(d, "p.pw")
    open(pr, "wb").write(proof)
    open(pwf, "wb").write(pw)
    out = subprocess.run([exe, vk_path, pr, pwf], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split()[:1] == ["VERIFY"], (out.stdout, out.stderr)
    return out.stdout.split()[1] == "1"


def test_case_list_is_complete_and_labelled(case_lists):
    for key, cs in case_lists.items():
        assert len(cs) == V.N_CASES
        by_stage = {s: [c for c in cs if c[4] == s] for s in V.STAGES}
        assert [len(by_stage[s]) for s in V.STAGES] == [24, 5, 10, 4, 12], key
        assert sum(c[0].startswith("generic") for c in cs) >= 4
        # the forgeries aimed at a pairing or at the subgroup test are well-formed in every other respect: canonical coordinates,
        # all five points on their curves, commitment count 1, a matching header
        from oracle import bn254 as B, groth16
        for name, proof, pw, expect, stage in cs:
            if stage in (V.STAGE2, V.STAGE4, V.SUBGROUP):
                assert all(int.from_bytes(proof[o:o + 32], "big") < B.P for o in list(range(0, 256, 32)) + list(range(260, 388, 32))), name
                Ar, Bs, Krs, Cm, PoK = V.split_proof(proof)
                assert all(B.g1_is_on_curve(p) for p in (Ar, Krs, Cm, PoK)) and B.g2_is_on_curve(Bs), name
                assert (groth16._g2_times_r(Bs) is None) == (stage != V.SUBGROUP), name
                assert groth16.parse_public_witness(pw) and all(v < B.R for v in groth16.parse_public_witness(pw)), name


@pytest.mark.parametrize("key", ["withdraw", "audit"])
def test_stage2_forgeries_fail_the_pedersen_pairing_and_nothing_else(keys, case_lists, key):
    """without the proof-of-knowledge check these five would be ACCEPTED: their Groth16 equation holds"""
    from oracle import bn254 as B, groth16
    vk = groth16.parse_vk(keys[key])
    for name, proof, pw, expect, stage in case_lists[key]:
        if stage != V.STAGE2:
            continue
        Ar, Bs, Krs, Cm, PoK = V.split_proof(proof)
        ksum = V.ksum_of(vk, groth16.parse_public_witness(pw), Cm)
        assert B.pairing_product_is_one([(Ar, Bs), (B.g1_neg(vk["alpha1"]), vk["beta2"]), (B.g1_neg(ksum), vk["gamma2"]),
                                         (B.g1_neg(Krs), vk["delta2"])]), name
        assert not expect


@pytest.mark.parametrize("first", range(0, V.N_CASES, GROUP))
@pytest.mark.parametrize("key", ["withdraw", "audit"])
def test_host_verifiers_give_the_verdict_by_construction(keys, case_lists, verify_one_exe, withdraw_artifacts, audit_artifacts, tmp_path, key, first):
    from oracle import groth16
    vk, vk_path = keys[key], {"withdraw": withdraw_artifacts, "audit": audit_artifacts}[key]["vk"]
    group = case_lists[key][first:first + GROUP]
    assert group
    for name, proof, pw, expect, stage in group:
        got = dict(oracle=groth16.verify(vk, proof, pw), spp_verify=_spp_verdict(vk, proof, pw),
                   verify_one=_verify_one_verdict(verify_one_exe, str(tmp_path), vk_path, proof, pw))
        assert got == dict(oracle=expect, spp_verify=expect, verify_one=expect), "%s key, case %r (%s): %r" % (key, name, stage, got)


def test_trapdoor_check_refuses_keys_of_another_setup(keys):
    """the simulator is only for keys of the oracle's seeded setup: another seed's scalars, the other circuit's key and the
    reference's gnark-made keys (whose toxic waste nobody has) are all refused by check_trapdoor, loudly"""
    V.check_trapdoor(keys["withdraw"], V.trapdoor(SEEDS["withdraw"]))
    V.check_trapdoor(keys["audit"], V.trapdoor(SEEDS["audit"]))
    with pytest.raises(AssertionError):
        V.check_trapdoor(keys["withdraw"], V.trapdoor(SEEDS["audit"]))
    with pytest.raises(AssertionError):
        V.check_trapdoor(keys["audit"], V.trapdoor(b"\x08" * 32))
    for name in ("reference_withdraw.vk", "reference_audit.vk"):
        with pytest.raises(AssertionError):
            V.check_trapdoor(open(os.path.join(GOLDEN, name), "rb").read(), V.trapdoor(SEEDS["withdraw"]))


def test_malleations_of_a_real_proof_are_valid_and_krs_of_another_proof_is_not(keys, withdraw_artifacts, withdraw_kat):
    """the same construction tests/test_gpu_verify_forged.py applies to a proof from the GPU prover, here on the oracle's prover"""
    import spp
    from oracle import native, circuit as C
    p = native.Prover(withdraw_artifacts["sppc"], withdraw_artifacts["pk"])
    row = C.withdraw_inputs(withdraw_kat)
    (rc1, proof, pw), (rc2, other, _) = p.prove(row, 3, 4), p.prove(row, 5, 6)
    assert rc1 == 0 and rc2 == 0 and proof[192:256] != other[192:256]
    vk = keys["withdraw"]
    for name, m in V.malleations(vk, proof, random.Random(5)):
        assert m != proof and spp.verify(vk, m, pw), name
        assert not spp.verify(vk, m[:192] + other[192:256] + m[256:], pw), name
