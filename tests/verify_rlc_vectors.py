"""Vectors for the random-linear-combination batch verifier (spp_verify_batch_rlc), on top of tests/verify_vectors.py.

Cancelling pairs: two valid simulated proofs and a point D, bent into (Krs_0 + D, Krs_1 - D) and into (PoK_0 + D, PoK_1 - D).  Each
proof alone is invalid (its Groth16 equation, or its Pedersen equation, is off by e(D, delta) or e(D, G)), but the PRODUCT of the two
equations is one: a combination that weighs the two proofs with equal scalars accepts both.  Only distinct secret scalars refuse them.

Plain Python over the oracle; no GPU, no libspp.  Consumed by tests/test_verify_rlc_host.py and tests/test_gpu_verify_rlc.py."""
from oracle import bn254 as B
from oracle import groth16

import verify_vectors as V

KINDS = ("krs", "pok")


def cancelling_pairs(vk, td, npub, rng):
    """{"krs": [(proof, pw), (proof, pw)], "pok": [...]}, and the points they were made from (for unweighted_product_is_one)"""
    vk = V._vk(vk)
    V.check_trapdoor(vk, td)
    pubs = [[rng.randrange(B.R) for _ in range(npub)] for _ in range(2)]
    pts = [V.simulate_points(vk, td, pub, V._big(rng), V._big(rng), V._big(rng)) for pub in pubs]
    D = B.g1_mul(V.G1, V._big(rng))
    signed = (D, B.g1_neg(D))
    pws = [groth16.public_witness_bytes(pub) for pub in pubs]
    out = {"krs": [], "pok": [], "points": pts, "pubs": pubs, "D": D}
    for (Ar, Bs, Krs, Cm, PoK), pw, d in zip(pts, pws, signed):
        out["krs"].append((V.proof_bytes(Ar, Bs, B.g1_add(Krs, d), Cm, PoK), pw))
        out["pok"].append((V.proof_bytes(Ar, Bs, Krs, Cm, B.g1_add(PoK, d)), pw))
    assert all(len({p for p, _ in out[k]}) == 2 for k in KINDS)
    return out


def unweighted_product_is_one(vk, pairs, kind):
    """the product of the two proofs' equations (stage 4 for "krs", stage 2 for "pok") with all scalars equal to 1, by the oracle's
    pairing: what a combination without distinct scalars checks"""
    vk = V._vk(vk)
    prs = []
    for (proof, pw) in pairs[kind]:
        Ar, Bs, Krs, Cm, PoK = V.split_proof(proof)
        if kind == "krs":
            ksum = V.ksum_of(vk, groth16.parse_public_witness(pw), Cm)
            prs += [(Ar, Bs), (B.g1_neg(vk["alpha1"]), vk["beta2"]), (B.g1_neg(ksum), vk["gamma2"]), (B.g1_neg(Krs), vk["delta2"])]
        else:
            prs += [(PoK, vk["ped_G"]), (Cm, vk["ped_GSigmaNeg"])]
    return B.pairing_product_is_one(prs)


def accepts(cs):
    return [c for c in cs if c[3]]


def cycled(cs, n):
    return [cs[k % len(cs)] for k in range(n)]
