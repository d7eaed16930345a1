"""The powers-of-tau transcript (SPPT) as a Python object, a contribution and its receipt in big integers, and the verifier's four
ratio equations over oracle/bn254.py pairings: a restatement of include/spp.h's protocol with no code shared with the library.

    SPPT: 'SPPT' 1 L (u32 little-endian), n = 2^L | T1: tau^i G1, i < 2n - 1 | T2: tau^i G2, i < n | A1: alpha tau^i G1, i < n |
          B1: beta tau^i G1, i < n | beta2 = beta G2         (G1 points 64 B, G2 points 128 B, no counts)
    receipt: three times  base' | T = k base | z = k + c s  for (t, T1_1), (a, A1_0), (b, B1_0)
"""
import hashlib
import struct

RECEIPT_LEN = 480
TAGS = {"T1": 1, "T2": 2, "A1": 3, "B1": 4}


class Ptau:
    def __init__(self, data):
        if len(data) < 12:
            raise ValueError("truncated")
        magic, version, self.log = struct.unpack_from("<4sII", data, 0)
        if magic != b"SPPT" or version != 1 or not 1 <= self.log <= 20:
            raise ValueError("not an SPPT transcript")
        n = self.n = 1 << self.log
        at = 12
        self.T1 = [data[at + 64 * i:at + 64 * i + 64] for i in range(2 * n - 1)]
        at += 64 * (2 * n - 1)
        self.T2 = [data[at + 128 * i:at + 128 * i + 128] for i in range(n)]
        at += 128 * n
        self.A1 = [data[at + 64 * i:at + 64 * i + 64] for i in range(n)]
        at += 64 * n
        self.B1 = [data[at + 64 * i:at + 64 * i + 64] for i in range(n)]
        at += 64 * n
        self.beta2 = data[at:at + 128]
        if at + 128 != len(data):
            raise ValueError("wrong length for L = %d" % self.log)

    def to_bytes(self):
        return b"".join([struct.pack("<4sII", b"SPPT", 1, self.log)] + self.T1 + self.T2 + self.A1 + self.B1 + [self.beta2])


def _progression(mul, to_bytes, gen, first, ratio, count, r):
    out, k = [], first % r
    for _ in range(count):
        out.append(to_bytes(mul(gen, k)))
        k = k * ratio % r
    return out


def transcript(log, tau, alpha, beta):
    """the transcript of (tau, alpha, beta) for n = 2^log, every point one product with a generator"""
    from oracle import bn254 as O
    n = 1 << log
    t = Ptau.__new__(Ptau)
    t.log, t.n = log, n
    t.T1 = _progression(O.g1_mul, O.g1_to_bytes, O.G1_GEN, 1, tau, 2 * n - 1, O.R)
    t.T2 = _progression(O.g2_mul, O.g2_to_bytes, O.G2_GEN, 1, tau, n, O.R)
    t.A1 = _progression(O.g1_mul, O.g1_to_bytes, O.G1_GEN, alpha, tau, n, O.R)
    t.B1 = _progression(O.g1_mul, O.g1_to_bytes, O.G1_GEN, beta, tau, n, O.R)
    t.beta2 = O.g2_to_bytes(O.g2_mul(O.G2_GEN, beta % O.R))
    return t.to_bytes()


def new(log):
    return transcript(log, 1, 1, 1)


def contribution_secrets(entropy):
    """(t, a, b, k_t, k_a, k_b) of spp_ptau_contribute for 32 bytes of entropy"""
    from oracle import bn254 as O
    return tuple(O.hash_to_fr(bytes(entropy), b"spp-ptau-contribute-v1", 6))


def contributed(data, t, a, b):
    """the transcript after a contribution with secrets t, a, b: every point multiplied on its own"""
    from oracle import bn254 as O
    p = Ptau(data)
    g1 = lambda raw, k: O.g1_to_bytes(O.g1_mul(O.g1_from_bytes(raw), k % O.R))
    g2 = lambda raw, k: O.g2_to_bytes(O.g2_mul(O.g2_from_bytes(raw), k % O.R))
    pw = [pow(t, i, O.R) for i in range(2 * p.n - 1)]
    p.T1 = [g1(x, pw[i]) for i, x in enumerate(p.T1)]
    p.T2 = [g2(x, pw[i]) for i, x in enumerate(p.T2)]
    p.A1 = [g1(x, a * pw[i]) for i, x in enumerate(p.A1)]
    p.B1 = [g1(x, b * pw[i]) for i, x in enumerate(p.B1)]
    p.beta2 = g2(p.beta2, b)
    return p.to_bytes()


def _bases(p):
    return [p.T1[1], p.A1[0], p.B1[0]]


def _challenge(before_bytes, base, base_after, T):
    from oracle import bn254 as O
    return O.hash_to_fr(hashlib.sha256(before_bytes).digest() + base + base_after + T, b"spp-ptau-contribute-c1", 1)[0]


def receipt(before_bytes, after_bytes, secrets):
    """the 480 bytes spp_ptau_contribute returns for these secrets"""
    from oracle import bn254 as O
    out = []
    for j, (base, base_after) in enumerate(zip(_bases(Ptau(before_bytes)), _bases(Ptau(after_bytes)))):
        s, k = secrets[j], secrets[3 + j]
        T = O.g1_to_bytes(O.g1_mul(O.g1_from_bytes(base), k))
        c = _challenge(before_bytes, base, base_after, T)
        out.append(base_after + T + ((k + c * s) % O.R).to_bytes(32, "big"))
    return b"".join(out)


def receipt_holds(before_bytes, after_bytes, rcpt):
    """base' is the file's and z base == T + c base', three times, in big integers"""
    from oracle import bn254 as O
    if len(rcpt) != RECEIPT_LEN:
        return False
    for j, (base, base_after) in enumerate(zip(_bases(Ptau(before_bytes)), _bases(Ptau(after_bytes)))):
        r = rcpt[160 * j:160 * j + 160]
        T, z = r[64:128], int.from_bytes(r[128:], "big")
        c = _challenge(before_bytes, base, r[:64], T)
        lhs = O.g1_mul(O.g1_from_bytes(base), z)
        rhs = O.g1_add(O.g1_from_bytes(T), O.g1_mul(O.g1_from_bytes(r[:64]), c))
        if r[:64] != base_after or z >= O.R or lhs != rhs:
            return False
    return True


def ratio_scalars(before_bytes, after_bytes, section, count):
    """rho_i: the first 128 bits of SHA256(SHA256(before) | SHA256(after) | tag | i as 8 bytes big-endian)"""
    head = hashlib.sha256(before_bytes).digest() + hashlib.sha256(after_bytes).digest() + bytes([TAGS[section]])
    return [int.from_bytes(hashlib.sha256(head + struct.pack(">Q", i)).digest()[:16], "big") for i in range(count)]


def ratio_check(before_bytes, after_bytes, name):
    """one of the verifier's equations TAU_G1, TAU_G2, ALPHA, BETA over the transcript `after`, with oracle/bn254.py pairings"""
    from oracle import bn254 as O
    p = Ptau(after_bytes)
    tau1, tau2 = O.g1_from_bytes(p.T1[1]), O.g2_from_bytes(p.T2[1])
    section = {"TAU_G1": "T1", "TAU_G2": "T2", "ALPHA": "A1", "BETA": "B1"}[name]
    raw = getattr(p, section)
    rho = ratio_scalars(before_bytes, after_bytes, section, len(raw) - 1)
    if name == "TAU_G2":
        pts = [O.g2_from_bytes(x) for x in raw]
        lo = hi = None
        for i, k in enumerate(rho):
            lo, hi = O.g2_add(lo, O.g2_mul(pts[i], k)), O.g2_add(hi, O.g2_mul(pts[i + 1], k))
        return O.pairing_product_is_one([(tau1, lo), (O.g1_neg(O.G1_GEN), hi)])
    pts = [O.g1_from_bytes(x) for x in raw]
    lo, hi = O.g1_msm(pts[:-1], rho), O.g1_msm(pts[1:], rho)
    good = O.pairing_product_is_one([(hi, O.G2_GEN), (O.g1_neg(lo), tau2)])
    if name == "BETA":
        good = good and O.pairing_product_is_one([(pts[0], O.G2_GEN), (O.g1_neg(O.G1_GEN), O.g2_from_bytes(p.beta2))])
    return good


# the tamperings of one honest link that the verifier must refuse, each with the name of the FIRST check that fails
REFUSALS = ["t1_power_replaced", "t1_powers_swapped", "t1_last_power_doubled", "t2_power_replaced", "a1_point_scaled", "b1_point_scaled",
            "beta2_of_another", "t1_0_not_the_generator", "t1_point_off_curve", "t2_point_off_subgroup", "z_plus_one", "t_replaced",
            "another_size", "truncated"]


def tampered(case, before, after, receipt, other_after):
    """(bytes of the file after, receipt, the reason's name) for one tampering of an honest link; other_after: another contribution
    to the same transcript before"""
    import verify_vectors as V
    from oracle import bn254 as O
    p = Ptau(after)
    other = O.g1_to_bytes(O.g1_mul(O.G1_GEN, 12345))
    twice = lambda raw: O.g1_to_bytes(O.g1_mul(O.g1_from_bytes(raw), 2))
    data = None
    if case == "t1_power_replaced":
        p.T1[3], want = other, "TAU_G1"
    elif case == "t1_powers_swapped":
        p.T1[3], p.T1[5], want = p.T1[5], p.T1[3], "TAU_G1"
    elif case == "t1_last_power_doubled":
        p.T1[-1], want = twice(p.T1[-1]), "TAU_G1"
    elif case == "t2_power_replaced":
        p.T2[3], want = O.g2_to_bytes(O.g2_mul(O.G2_GEN, 12345)), "TAU_G2"
    elif case == "a1_point_scaled":
        p.A1[2], want = twice(p.A1[2]), "ALPHA"
    elif case == "b1_point_scaled":
        p.B1[2], want = twice(p.B1[2]), "BETA"
    elif case == "beta2_of_another":
        p.beta2, want = Ptau(other_after).beta2, "BETA"
    elif case == "t1_0_not_the_generator":
        p.T1[0], want = twice(p.T1[0]), "POINT_INVALID"
    elif case == "t1_point_off_curve":
        x, y = O.g1_from_bytes(p.T1[4])
        p.T1[4], want = O.g1_to_bytes((x, (y + 1) % O.P)), "POINT_INVALID"
    elif case == "t2_point_off_subgroup":
        p.T2[2], want = O.g2_to_bytes(V.twist_point_outside_the_subgroup()), "POINT_INVALID"
    elif case == "z_plus_one":
        z = (int.from_bytes(receipt[128:160], "big") + 1) % O.R
        receipt, want = receipt[:128] + z.to_bytes(32, "big") + receipt[160:], "RECEIPT"
    elif case == "t_replaced":
        receipt, want = receipt[:160 + 64] + other + receipt[160 + 128:], "RECEIPT"     # T of the proof for alpha
    elif case == "another_size":
        data, want = new(p.log - 1), "SIZE"
    else:
        data, want = after[:-10], "FORMAT"
    return (p.to_bytes() if data is None else data), receipt, want


# ------------------------------------------------------------------------------------------------------------------------------
# the derivation of a key from a transcript (spp_setup_from_ptau), in big integers
# ------------------------------------------------------------------------------------------------------------------------------
def omega(log):
    """the root of unity of order 2^log that spp_setup.cpp takes: 5^((r - 1) / 2^log)"""
    from oracle import bn254 as O
    return pow(O.FR_GENERATOR, (O.R - 1) >> log, O.R)


def lagrange_at(tau, log):
    """L[k] = L_k(tau) over the domain of size 2^log, as spp_setup.cpp computes it; tau on the domain gives the indicator"""
    from oracle import bn254 as O
    n, w = 1 << log, omega(log)
    pts = [pow(w, k, O.R) for k in range(n)]
    if tau % O.R in pts:
        return [1 if p == tau % O.R else 0 for p in pts]
    scale = (pow(tau, n, O.R) - 1) * pow(n, -1, O.R) % O.R
    return [p * scale * pow(tau - p, -1, O.R) % O.R for p in pts]


def group_intt(points, log, add, mul):
    """(1 / n) sum_i w^(-k i) P_i for every k by the definition: n^2 products of big integers"""
    from oracle import bn254 as O
    n, winv, ninv = 1 << log, pow(omega(log), -1, O.R), pow(1 << log, -1, O.R)
    out = []
    for k in range(n):
        acc = None
        for i, p in enumerate(points):
            acc = add(acc, mul(p, pow(winv, k * i, O.R) * ninv % O.R))
        out.append(acc)
    return out


def _sections(desc, scalars_a, scalars_b, scalars_k):
    from oracle import bn254 as O
    W = desc.n_wires
    cls = [0] * W
    for j in range(desc.n_public):
        cls[j] = 1
    cls[desc.challenge_wire] = 1
    for w in desc.committed:
        cls[w] = 2
    g1 = lambda k: O.g1_to_bytes(O.g1_mul(O.G1_GEN, k % O.R))
    g2 = lambda k: O.g2_to_bytes(O.g2_mul(O.G2_GEN, k % O.R))
    sec = lambda sc, enc, keep: ([j for j in range(W) if keep(j) and sc[j] % O.R], [enc(sc[j]) for j in range(W) if keep(j) and sc[j] % O.R])
    return cls, g1, g2, sec


def derived_key(desc, tau, alpha, beta):
    """(pk bytes, vk bytes) of spp_setup_from_ptau for the synthetic circuit desc (tests/synth_circuits.py) and the transcript of
    (tau, alpha, beta): spp_setup's scalars with gamma = delta = sigma = rho = 1, every point one product with a generator"""
    from oracle import bn254 as O
    W, log = desc.n_wires, desc.domain_log
    n, L = 1 << log, lagrange_at(tau, log)
    aw, bw, cw = ([0] * W for _ in range(3))
    for rows, out in ((desc.A, aw), (desc.B, bw), (desc.C, cw)):
        for k, terms in enumerate(rows):
            for w, v in terms:
                out[w] = (out[w] + v * L[k]) % O.R
    kk = [(beta * aw[j] + alpha * bw[j] + cw[j]) % O.R for j in range(W)]
    cls, g1, g2, sec = _sections(desc, aw, bw, kk)
    zt = (pow(tau, n, O.R) - 1) % O.R
    parts = [struct.pack("<7I", 0x4B505053, 1, desc.id, W, log, desc.n_public, desc.challenge_wire), g1(alpha), g1(beta), g1(1), g2(beta), g2(1)]
    for sc, enc, keep in ((aw, g1, lambda j: True), (bw, g1, lambda j: True), (bw, g2, lambda j: True), (kk, g1, lambda j: cls[j] == 0)):
        wires, pts = sec(sc, enc, keep)
        parts += [struct.pack("<I", len(wires)), struct.pack("<%dI" % len(wires), *wires)] + pts
    parts += [struct.pack("<I", n - 1)] + [g1(zt * pow(tau, i, O.R)) for i in range(n - 1)]
    cb = [struct.pack("<I", len(desc.committed)), struct.pack("<%dI" % len(desc.committed), *desc.committed)] + [g1(kk[w]) for w in desc.committed]
    parts += cb + cb
    vk = [g1(alpha), g1(beta), g2(beta), g2(1), g1(1), g2(1), struct.pack(">I", desc.n_public + 1)]
    vk += [g1(kk[j]) for j in range(desc.n_public)] + [g1(kk[desc.challenge_wire]), struct.pack(">3I", 1, 0, 1), g2(1), g2(O.R - 1)]
    return b"".join(parts), b"".join(vk)


def derived_from_reference(pk_bytes, vk_bytes, gamma, delta):
    """the key spp_setup_from_ptau must give, from the key a seeded setup gave for the same tau, alpha, beta: the private K and
    the Z points times delta, the vk's K and CB times gamma, CS = CB, the delta and gamma points the generators, the commitment
    key (G2, -G2); A, B1, B2, alpha1, beta1, beta2 as they are"""
    import sppk_format as S
    from oracle import bn254 as O
    pk, vk = S.Sppk(pk_bytes), S.Vk(vk_bytes)
    times = lambda raw, k: O.g1_to_bytes(O.g1_mul(O.g1_from_bytes(raw), k))
    g1, g2 = O.g1_to_bytes(O.G1_GEN), O.g2_to_bytes(O.G2_GEN)
    for name in ("K", "Z"):
        pk.points[name] = [times(p, delta) for p in pk.points[name]]
    pk.points["CB"] = [times(p, gamma) for p in pk.points["CB"]]
    pk.points["CS"] = list(pk.points["CB"])
    pk.delta1, pk.delta2 = g1, g2
    vk.K = [times(p, gamma) for p in vk.K]
    vk.gamma2, vk.delta1, vk.delta2 = g2, g1, g2
    vk.tail = vk.tail[:12] + g2 + O.g2_to_bytes(O.g2_neg(O.G2_GEN))
    return pk.to_bytes(), vk.to_bytes()


# ------------------------------------------------------------------------------------------------------------------------------
# sigma contributions (spp_setup_contribute_sigma), in big integers
# ------------------------------------------------------------------------------------------------------------------------------
def sigma_secrets(entropy):
    """(s, k) of spp_setup_contribute_sigma for 32 bytes of entropy"""
    from oracle import bn254 as O
    return tuple(O.hash_to_fr(bytes(entropy), b"spp-groth16-sigma-v1", 2))


def sigma_contributed(pk_bytes, vk_bytes, s, k):
    """(pk, vk, receipt) after a sigma contribution with secret s and nonce k: CS times s, the vk's last G2 point times s"""
    import sppk_format as S
    from oracle import bn254 as O
    pk, vk = S.Sppk(pk_bytes), S.Vk(vk_bytes)
    cs0 = pk.points["CS"][0]
    pk.points["CS"] = [O.g1_to_bytes(O.g1_mul(O.g1_from_bytes(p), s)) for p in pk.points["CS"]]
    vk.tail = vk.tail[:-128] + O.g2_to_bytes(O.g2_mul(O.g2_from_bytes(vk.tail[-128:]), s))
    T = O.g1_to_bytes(O.g1_mul(O.g1_from_bytes(cs0), k))
    c, = O.hash_to_fr(hashlib.sha256(pk_bytes).digest() + cs0 + pk.points["CS"][0] + T, b"spp-groth16-sigma-c1", 1)
    return pk.to_bytes(), vk.to_bytes(), pk.points["CS"][0] + T + ((k + c * s) % O.R).to_bytes(32, "big")
