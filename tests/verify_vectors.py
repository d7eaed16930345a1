"""Simulated and forged proofs for the verifiers, with the verdict each must get and the check that must give it.

Plain Python over oracle.bn254 and oracle.groth16; no GPU, no libspp, no files (the key bytes and the setup seed are handed in).

The oracle's trusted setup is deterministic: orc_setup derives tau, alpha, beta, gamma, delta, sigma, rho from its 32-byte seed.
Whoever knows them can make a proof that verifies for ANY public words and ANY chosen Ar, Bs, Cm (the Groth16 simulator):

    PoK = sigma * Cm
    Krs = (1/delta) * (b * Ar - alpha*beta * G1) - (gamma/delta) * ksum,   ksum = K0 + sum pub_i K_i + challenge(Cm) K_last + Cm

which puts e(Ar, Bs) = e(alpha, beta) e(ksum, gamma) e(Krs, delta) and e(PoK, G) e(Cm, GSigmaNeg) = 1 by bilinearity.  So the
verdict of every case below is known BY CONSTRUCTION -- no verifier is asked -- and a proof can be wrong in exactly one place
while every point stays on its curve and every encoding stays canonical, which a flipped byte never manages: such forgeries get
past the format, curve and subgroup checks and are refused by the pairing that is there to refuse them.  Points at infinity,
proof points equal to key points and the textbook malleations of a valid proof are accept cases.

This works only for keys made by the oracle's seeded setup (check_trapdoor refuses any other key).

Two runners consume the same list: tests/test_verify_vectors_host.py (the oracle, spp.verify and the g++ build of verify_one) and
tests/test_gpu_verify_forged.py (k_verify and, behind the pool ledger, k_verify_list).
"""
from oracle import bn254 as B
from oracle import groth16

SETUP_DST = b"spp-groth16-setup-v1"          # oracle/c/groth16.c orc_setup; csrc/spp_setup.cpp uses the same derivation
ACCEPT, STAGE2, STAGE4, SUBGROUP, FORMAT = "accept", "stage2-pok", "stage4-groth16", "subgroup", "format"
STAGES = (ACCEPT, STAGE2, STAGE4, SUBGROUP, FORMAT)
N_CASES = 55                                 # cases() asserts it: a case dropped or added shows here first
G1, G2 = B.G1_GEN, B.G2_GEN


# ---------------------------------------------------------------------------------------------------------------- trapdoor
def trapdoor(seed32):
    """(tau, alpha, beta, gamma, delta, sigma, rho) of the oracle's setup for this seed"""
    seed32 = bytes(seed32)
    assert len(seed32) == 32
    return tuple(B.hash_to_fr(seed32, SETUP_DST, 7))


def _vk(vk):
    return vk if isinstance(vk, dict) else groth16.parse_vk(vk)


def check_trapdoor(vk, td):
    """the key was made from these scalars; a change to the setup's derivation fails here, not inside a case"""
    vk = _vk(vk)
    tau, alpha, beta, gamma, delta, sigma, rho = td
    assert all(0 < v < B.R for v in td), "a setup scalar is zero"
    assert B.g1_mul(G1, alpha) == vk["alpha1"], "alpha * G1 != alpha1"
    assert B.g2_mul(G2, beta) == vk["beta2"], "beta * G2 != beta2"
    assert B.g2_mul(G2, gamma) == vk["gamma2"], "gamma * G2 != gamma2"
    assert B.g2_mul(G2, delta) == vk["delta2"], "delta * G2 != delta2"
    assert B.g2_mul(G2, rho) == vk["ped_G"], "rho * G2 != ped_G"
    assert B.g2_mul(G2, (-rho * sigma) % B.R) == vk["ped_GSigmaNeg"], "-rho*sigma * G2 != ped_GSigmaNeg"


# ---------------------------------------------------------------------------------------------------------------- simulator
def proof_bytes(Ar, Bs, Krs, Cm, PoK, count=1):
    """the 388 bytes groth16.parse_proof reads; None (infinity) is all-zero bytes"""
    out = B.g1_to_bytes(Ar) + B.g2_to_bytes(Bs) + B.g1_to_bytes(Krs) + int(count).to_bytes(4, "big") + B.g1_to_bytes(Cm) + B.g1_to_bytes(PoK)
    assert len(out) == 388
    return out


def split_proof(proof):
    """(Ar, Bs, Krs, Cm, PoK) of a proof whose points are to be reused"""
    p = groth16.parse_proof(proof)
    return p["Ar"], p["Bs"], p["Krs"], p["commitment"], p["pok"]


def ksum_of(vk, pub, Cm):
    vk = _vk(vk)
    assert len(pub) + 2 == len(vk["K"]) and all(0 <= v < B.R for v in pub)
    challenge = B.hash_to_fr(B.g1_to_bytes(Cm), B.DST_COMMITMENT, 1)[0]
    ks = vk["K"][0]
    for v, k in zip(list(pub) + [challenge], vk["K"][1:]):
        ks = B.g1_add(ks, B.g1_mul(k, v))
    return B.g1_add(ks, Cm)


def krs_for(vk, td, pub, Ar, b, Cm):
    """the Krs that balances the Groth16 equation for Ar (a point), Bs = b * G2 and the commitment Cm (a point)"""
    _, alpha, beta, gamma, delta, _, _ = td
    di = B.inv(delta, B.R)
    lhs = B.g1_add(B.g1_mul(Ar, b), B.g1_neg(B.g1_mul(G1, alpha * beta)))
    return B.g1_add(B.g1_mul(lhs, di), B.g1_neg(B.g1_mul(ksum_of(vk, pub, Cm), gamma * di)))


def simulate_points(vk, td, pub, a, b, c):
    vk = _vk(vk)
    Ar, Bs, Cm = B.g1_mul(G1, a), B.g2_mul(G2, b), B.g1_mul(G1, c)
    return Ar, Bs, krs_for(vk, td, pub, Ar, b, Cm), Cm, B.g1_mul(Cm, td[5])


def simulate(vk, td, pub, a, b, c):
    """A proof that verifies for the public words `pub`, with Ar = a*G1, Bs = b*G2, Cm = c*G1 (a scalar of 0: infinity).
    Returns (proof388, pw)."""
    return proof_bytes(*simulate_points(vk, td, pub, a, b, c)), groth16.public_witness_bytes(pub)


def malleations(vk, proof, rng):
    """the three textbook re-randomisations of a VALID proof, from the key alone: [(name, proof)] -- all still valid"""
    vk = _vk(vk)
    Ar, Bs, Krs, Cm, PoK = split_proof(proof)
    s, t = rng.randrange(2, B.R), rng.randrange(2, B.R)
    return [("(-Ar, -Bs)", proof_bytes(B.g1_neg(Ar), B.g2_neg(Bs), Krs, Cm, PoK)),
            ("(s Ar, Bs / s)", proof_bytes(B.g1_mul(Ar, s), B.g2_mul(Bs, B.inv(s, B.R)), Krs, Cm, PoK)),
            ("(Ar, Bs + t delta2, Krs + t Ar)", proof_bytes(Ar, B.g2_add(Bs, B.g2_mul(vk["delta2"], t)), B.g1_add(Krs, B.g1_mul(Ar, t)), Cm, PoK))]


# ---------------------------------------------------------------------------------------------------------------- a twist point outside G2
def fq_sqrt(v):
    r = pow(v, (B.P + 1) // 4, B.P)                                      # q = 3 mod 4
    return r if r * r % B.P == v % B.P else None


def fq2_sqrt(a):
    alpha = fq_sqrt((a[0] * a[0] + a[1] * a[1]) % B.P)
    if alpha is None:
        return None
    for d in ((a[0] + alpha) * pow(2, -1, B.P) % B.P, (a[0] - alpha) * pow(2, -1, B.P) % B.P):
        x0 = fq_sqrt(d)
        if x0:
            y = (x0, a[1] * pow(2 * x0, -1, B.P) % B.P)
            if B.f2_mul(y, y) == (a[0] % B.P, a[1] % B.P):
                return y
    return None


def twist_point_outside_the_subgroup():
    """the twist point with the smallest x = (k, 0), k >= 2: on the curve y^2 = x^3 + 3/(9+u), not of order r (the cofactor is ~2^254)"""
    x = 1
    while True:
        x += 1
        y = fq2_sqrt(B.f2_add(B.f2_mul(B.f2_mul((x, 0), (x, 0)), (x, 0)), B.G2_B))
        if y is not None:
            pt = ((x, 0), y)
            assert B.g2_is_on_curve(pt) and groth16._g2_times_r(pt) is not None
            return pt


# ---------------------------------------------------------------------------------------------------------------- the cases
def _put(data, off, new):
    return data[:off] + new + data[off + len(new):]


def _big(rng):
    return rng.randrange(1 << 253, B.R)                                  # a 254-bit scalar


def cases(vk, td, npub, rng):
    """[(name, proof, pw, expect, stage)]: expect is the verdict by construction, stage the check that must make the decision.
    Every reject case of the stages `stage2-pok`, `stage4-groth16` and `subgroup` has all five points on their curves and all
    encodings canonical, and passes every check in front of its stage."""
    vk = _vk(vk)
    check_trapdoor(vk, td)
    assert npub + 2 == len(vk["K"]) and npub >= 2
    _, alpha, beta, gamma, delta, sigma, _ = td
    pwb = groth16.public_witness_bytes
    words = lambda: [rng.randrange(B.R) for _ in range(npub)]
    out = []

    def accept(name, pub, a, b, c):
        pts = simulate_points(vk, td, pub, a, b, c)
        out.append((name, proof_bytes(*pts), pwb(pub), True, ACCEPT))
        return pts

    # ---- accept
    for i in range(4):
        accept("generic %d" % i, words(), _big(rng), _big(rng), _big(rng))
    accept("public words all 0", [0] * npub, _big(rng), _big(rng), _big(rng))
    accept("public words all r-1", [B.R - 1] * npub, _big(rng), _big(rng), _big(rng))
    w = words()
    w[npub // 2] = 0
    accept("one public word 0", w, _big(rng), _big(rng), _big(rng))
    accept("Cm and PoK infinity", words(), _big(rng), _big(rng), 0)
    accept("Ar infinity", words(), 0, _big(rng), _big(rng))
    accept("Bs infinity", words(), _big(rng), 0, _big(rng))
    accept("Ar, Bs, Cm infinity", words(), 0, 0, 0)
    for name, b in (("G2 generator", 1), ("gamma2", gamma), ("delta2", delta), ("beta2", beta), ("-delta2", B.R - delta)):
        pts = accept("Bs = " + name, words(), _big(rng), b, _big(rng))
        assert pts[1] == {"G2 generator": G2, "gamma2": vk["gamma2"], "delta2": vk["delta2"], "beta2": vk["beta2"],
                          "-delta2": B.g2_neg(vk["delta2"])}[name]
    for name, a in (("G1 generator", 1), ("alpha1", alpha), ("-alpha1", B.R - alpha)):
        pts = accept("Ar = " + name, words(), a, _big(rng), _big(rng))
        assert pts[0] == {"G1 generator": G1, "alpha1": vk["alpha1"], "-alpha1": B.g1_neg(vk["alpha1"])}[name]
    accept("Cm = G1 generator", words(), _big(rng), _big(rng), 1)
    a = _big(rng)
    accept("a b = alpha beta", words(), a, alpha * beta * B.inv(a, B.R) % B.R, _big(rng))
    pub = words()
    base = simulate_points(vk, td, pub, _big(rng), _big(rng), _big(rng))
    for name, pr in malleations(vk, proof_bytes(*base), rng):
        out.append(("malleated " + name, pr, pwb(pub), True, ACCEPT))

    # ---- reject, every point on its curve, every encoding canonical.  `base` (valid under `pub`) is what gets bent.
    Ar, Bs, Krs, Cm, PoK = base
    c2 = _big(rng)
    Cm2 = B.g1_mul(G1, c2)
    PoK2 = B.g1_mul(Cm2, sigma)
    assert Cm2 != Cm and PoK != Cm and PoK is not None
    rej = lambda name, pts, pw, stage: out.append((name, proof_bytes(*pts), pw, False, stage))
    pw = pwb(pub)
    # stage 2: the Pedersen pairing.  Krs always matches the Cm in the proof, so the Groth16 equation would hold.
    rej("-PoK", (Ar, Bs, Krs, Cm, B.g1_neg(PoK)), pw, STAGE2)
    rej("PoK of another commitment", (Ar, Bs, Krs, Cm, PoK2), pw, STAGE2)
    rej("PoK = Cm", (Ar, Bs, Krs, Cm, Cm), pw, STAGE2)
    rej("PoK infinity, Cm finite", (Ar, Bs, Krs, Cm, None), pw, STAGE2)
    a0, b0 = _big(rng), _big(rng)
    inf_cm = simulate_points(vk, td, pub, a0, b0, 0)                     # valid with Cm = PoK = infinity ...
    rej("Cm infinity, PoK finite", inf_cm[:4] + (PoK,), pw, STAGE2)     # ... until a PoK is put beside it
    # stage 4: the Groth16 pairing.  PoK = sigma * Cm throughout.
    rej("Cm', PoK' of another commitment, Krs kept", (Ar, Bs, Krs, Cm2, PoK2), pw, STAGE4)
    rej("-Ar alone", (B.g1_neg(Ar), Bs, Krs, Cm, PoK), pw, STAGE4)
    rej("-Bs alone", (Ar, B.g2_neg(Bs), Krs, Cm, PoK), pw, STAGE4)
    rej("2 Ar", (B.g1_add(Ar, Ar), Bs, Krs, Cm, PoK), pw, STAGE4)
    rej("-Krs", (Ar, Bs, B.g1_neg(Krs), Cm, PoK), pw, STAGE4)
    rej("Krs + G1", (Ar, Bs, B.g1_add(Krs, G1), Cm, PoK), pw, STAGE4)
    rej("Krs infinity", (Ar, Bs, None, Cm, PoK), pw, STAGE4)
    rej("Ar and Krs swapped", (Krs, Bs, Ar, Cm, PoK), pw, STAGE4)
    off1 = list(pub)
    off1[npub - 1] = (off1[npub - 1] + 1) % B.R
    rej("a public word off by 1", base, pwb(off1), STAGE4)
    swapped = list(pub)
    swapped[0], swapped[1] = swapped[1], swapped[0]
    assert swapped != pub
    rej("two public words exchanged", base, pwb(swapped), STAGE4)
    # subgroup: on the twist, not of order r
    T = twist_point_outside_the_subgroup()
    TB = B.g2_add(T, Bs)
    for name, pt in (("Bs = small-x twist point outside G2", T), ("Bs = that point + a valid Bs", TB)):
        assert B.g2_is_on_curve(pt) and groth16._g2_times_r(pt) is not None
        rej(name, (Ar, pt, Krs, Cm, PoK), pw, SUBGROUP)
    # with a finite Ar those two would also fail the Groth16 pairing (the Miller loop of a point outside G2 is not bilinear), so a
    # verifier WITHOUT the subgroup test still refuses them.  With Ar at infinity e(Ar, Bs) = 1 whatever Bs is: only the subgroup
    # test stands between these two and acceptance
    ar_inf = simulate_points(vk, td, pub, 0, _big(rng), _big(rng))
    for name, pt in (("Ar infinity, Bs = small-x twist point outside G2", T), ("Ar infinity, Bs = that point + a valid Bs", B.g2_add(T, ar_inf[1]))):
        assert B.g2_is_on_curve(pt) and groth16._g2_times_r(pt) is not None and ar_inf[0] is None
        rej(name, (None, pt) + ar_inf[2:], pw, SUBGROUP)

    # ---- reject, format and canonical encodings (the proof underneath is valid)
    good = proof_bytes(*base)
    fmt = lambda name, pr, w_: out.append((name, pr, w_, False, FORMAT))
    for count in (0, 2, 0x01000000):
        fmt("commitment count %#x" % count, _put(good, 256, count.to_bytes(4, "big")), pw)
    be = lambda v: v.to_bytes(4, "big")
    fmt("pw header nsec = 1", good, _put(pw, 4, be(1)))
    fmt("pw header npub + 1", good, _put(pw, 0, be(npub + 1)))
    fmt("pw header nvec - 1", good, _put(pw, 8, be(npub - 1)))
    fmt("Ar.x exactly q", _put(good, 0, B.fe_be(B.P)), pw)
    # q is the non-canonical spelling of 0, and no point of G1 has a zero coordinate (3 is no square mod q; the order is odd): the
    # only VALID proofs a reducing decoder could be tricked with are those with a point at infinity, spelt with q for one of the zeros
    fmt("Ar infinity spelt (q, 0)", _put(proof_bytes(*ar_inf), 0, B.fe_be(B.P)), pw)
    bs_inf = simulate_points(vk, td, pub, _big(rng), 0, _big(rng))
    fmt("Bs infinity spelt with Y.A0 = q", _put(proof_bytes(*bs_inf), 64 + 96, B.fe_be(B.P)), pw)
    zero_word = list(pub)
    zero_word[1] = 0
    zpts = simulate_points(vk, td, zero_word, _big(rng), _big(rng), _big(rng))   # valid under the word 0 ...
    fmt("a public word exactly r", proof_bytes(*zpts), _put(pwb(zero_word), 12 + 32, B.fe_be(B.R)))   # ... refused under its alias r
    fmt("Ar = (x, 0)", _put(good, 32, bytes(32)), pw)
    fmt("Ar = (0, y)", _put(good, 0, bytes(32)), pw)

    assert len(out) == N_CASES, len(out)
    assert len({c[0] for c in out}) == N_CASES
    assert all(len(c[1]) == 388 and len(c[2]) == 12 + 32 * npub and c[4] in STAGES and c[3] == (c[4] == ACCEPT) for c in out)
    assert {c[4] for c in out} == set(STAGES)
    return out
