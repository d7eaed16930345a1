"""The SPPK proving-key container and the gnark raw verifying key as Python objects, for tests that build or tamper with keys: a
restatement of the layout csrc/spp_setup.cpp writes, with no code shared with the library.

    SPPK: 'SPPK' 1 | circuit id, wires, domain log, publics, challenge wire (u32 little-endian) | alpha1 beta1 delta1 (G1, 64 B) |
          beta2 delta2 (G2, 128 B) | A: count, wires, points | B1: the same | B2: count, wires, G2 points | K: count, wires, points |
          Z: count, points | CB: count, wires, points | CS: the same
    vk:   alpha1 beta1 | beta2 gamma2 | delta1 delta2 | count (u32 big-endian) | K points | 1 0 1 (u32 big-endian) | two G2 points
"""
import struct


class Sppk:
    G1_SECTIONS = ("A", "B1", "K", "Z", "CB", "CS")

    def __init__(self, data):
        self.header = data[:28]
        magic, version = struct.unpack_from("<II", data, 0)
        if magic != 0x4B505053 or version != 1:
            raise ValueError("not an SPPK container")
        at = 28
        self.alpha1, self.beta1, self.delta1 = (data[at + 64 * i:at + 64 * i + 64] for i in range(3))
        at += 192
        self.beta2, self.delta2 = data[at:at + 128], data[at + 128:at + 256]
        at += 256
        self.wires, self.points = {}, {}
        for name, size, has_wires in (("A", 64, True), ("B1", 64, True), ("B2", 128, True), ("K", 64, True), ("Z", 64, False),
                                      ("CB", 64, True), ("CS", 64, True)):
            n, = struct.unpack_from("<I", data, at)
            at += 4
            if has_wires:
                self.wires[name] = list(struct.unpack_from("<%dI" % n, data, at))
                at += 4 * n
            self.points[name] = [data[at + size * i:at + size * (i + 1)] for i in range(n)]
            if any(len(p) != size for p in self.points[name]):
                raise ValueError("truncated")
            at += size * n
        if at != len(data):
            raise ValueError("trailing bytes")

    def to_bytes(self):
        out = [self.header, self.alpha1, self.beta1, self.delta1, self.beta2, self.delta2]
        for name in ("A", "B1", "B2", "K", "Z", "CB", "CS"):
            pts = self.points[name]
            out.append(struct.pack("<I", len(pts)))
            if name in self.wires:
                out.append(struct.pack("<%dI" % len(pts), *self.wires[name]))
            out += pts
        return b"".join(out)


class Vk:
    def __init__(self, data):
        self.alpha1, self.beta1 = data[0:64], data[64:128]
        self.beta2, self.gamma2 = data[128:256], data[256:384]
        self.delta1, self.delta2 = data[384:448], data[448:576]
        nk, = struct.unpack_from(">I", data, 576)
        self.K = [data[580 + 64 * i:644 + 64 * i] for i in range(nk)]
        self.tail = data[580 + 64 * nk:]
        if len(self.tail) != 12 + 256:
            raise ValueError("not a verifying key")

    def to_bytes(self):
        return b"".join([self.alpha1, self.beta1, self.beta2, self.gamma2, self.delta1, self.delta2, struct.pack(">I", len(self.K))]
                        + self.K + [self.tail])


def contributed(pk_bytes, vk_bytes, d):
    """(pk, vk) after a contribution with secret d, from oracle/bn254.py big integers: delta times d, K and Z times 1/d."""
    from oracle import bn254 as O
    pk, vk = Sppk(pk_bytes), Vk(vk_bytes)
    di = pow(d, -1, O.R)
    pk.delta1 = O.g1_to_bytes(O.g1_mul(O.g1_from_bytes(pk.delta1), d))
    pk.delta2 = O.g2_to_bytes(O.g2_mul(O.g2_from_bytes(pk.delta2), d))
    for name in ("K", "Z"):
        pk.points[name] = [O.g1_to_bytes(O.g1_mul(O.g1_from_bytes(p), di)) for p in pk.points[name]]
    vk.delta1, vk.delta2 = pk.delta1, pk.delta2
    return pk.to_bytes(), vk.to_bytes()


def contribution_secrets(entropy):
    """(d, k) of spp_setup_contribute for 32 bytes of entropy"""
    from oracle import bn254 as O
    return tuple(O.hash_to_fr(bytes(entropy), b"spp-groth16-contribute-v1", 2))


def receipt_holds(pk_before_bytes, receipt):
    """z * delta1 == T + c * delta1' with c recomputed from the key before, all in big integers"""
    import hashlib
    from oracle import bn254 as O
    delta1 = Sppk(pk_before_bytes).delta1
    d1a, T, z = receipt[:64], receipt[64:128], int.from_bytes(receipt[128:160], "big")
    c, = O.hash_to_fr(hashlib.sha256(pk_before_bytes).digest() + delta1 + d1a + T, b"spp-groth16-contribute-c1", 1)
    lhs = O.g1_mul(O.g1_from_bytes(delta1), z)
    rhs = O.g1_add(O.g1_from_bytes(T), O.g1_mul(O.g1_from_bytes(d1a), c))
    return z < O.R and lhs == rhs
