"""The committee's commitments and verifiable resharing in Python integers (tests/vss_model.py for the sharing, oracle.bn254 for
the curve; no call into the package): the weighted sum of dealers' commitments, the public commitment of a share, the new
member's decisions with their three flags, and crafted inputs for the addition's branches.  The tests of the reshare section of
csrc/vss.hpp, of spp_vss_combine_commitments / spp_vss_share_commitments / spp_vss_reshare_receive and of the `spp dkg-committee`,
`dkg-reshare-deal` and `dkg-reshare-receive` commands compare with this."""
import vss_model as M
from oracle import bn254 as O

R = M.R
BAD_POINT, BAD_SHARE, NOT_SHARE = M.BAD_POINT, M.BAD_SHARE, 8


def points_of(raw):
    """[(ok, point)] of a string of 64-byte points"""
    return [M.decode_point(raw[i:i + 64]) for i in range(0, len(raw), 64)]


def lincomb_points(points, weights=None, base=None):
    """base + sum_d w_d points[d] for points as the model holds them (None: infinity)"""
    acc = base
    for d, pt in enumerate(points):
        acc = O.g1_add(acc, pt if weights is None else O.g1_mul(pt, weights[d] % R))
    return acc


def combine(commitments, weights=None, base=None):
    """(flags per dealer, bad, out bytes or None): out[i] = base[i] + sum_d w_d C_d[i] over the dealers' commitment strings"""
    dec = [points_of(c) for c in commitments]
    flags = [[0 if ok else BAD_POINT for ok, _ in row] for row in dec]
    bad = sum(f != 0 for row in flags for f in row)
    if bad:
        return flags, bad, None
    bpts = [pt for _, pt in points_of(base)] if base is not None else [None] * len(dec[0])
    out = b"".join(O.g1_to_bytes(lincomb_points([row[i][1] for row in dec], weights, bpts[i])) for i in range(len(dec[0])))
    return flags, 0, out


def share_commitment(t, n, committee, x, v):
    """E_x[v] = sum_k x^k D_k[v] as a point (None: infinity)"""
    acc, xp = None, 1
    for k in range(t):
        ok, pt = M.decode_point(committee[(k * n + v) * 64:(k * n + v) * 64 + 64])
        assert ok
        acc = O.g1_add(acc, O.g1_mul(pt, xp))
        xp = xp * x % R
    return acc


def share_commitments(t, n, committee, xs, values=None):
    """bytes per x, every value (or only `values`, the others left as 64 bytes of 0xEE)"""
    pick = range(n) if values is None else values
    out = []
    for x in xs:
        row = [b"\xee" * 64] * n
        for v in pick:
            row[v] = O.g1_to_bytes(share_commitment(t, n, committee, x, v))
        out.append(b"".join(row))
    return out


def is_share(t_old, n, committee, x_old, v, c0_raw):
    """0 or NOT_SHARE: is this constant term the public commitment of the share at x_old?"""
    ok, c0 = M.decode_point(c0_raw)
    if not ok:
        return BAD_POINT
    return 0 if share_commitment(t_old, n, committee, x_old, v) == c0 else NOT_SHARE


def reshare_receive(xs_old, t_new, x_new, n, committee, commitments, ys, ys_blind, values=None):
    """(flags [[int] * n] per old member, bad, share, blind, committee_out).  values: compute committee_out only there (the cost of
    the model's scalar products); the other entries are 64 bytes of 0xEE."""
    t_old = len(xs_old)
    flags = []
    for j, xj in enumerate(xs_old):
        row = []
        for v in range(n):
            f = M.check_value(t_new, x_new, n, commitments[j], v, ys[j][v], ys_blind[j][v])
            if f != BAD_POINT:
                f |= is_share(t_old, n, committee, xj, v, commitments[j][v * 64:v * 64 + 64])
            row.append(f)
        flags.append(row)
    bad = sum(f != 0 for row in flags for f in row)
    if bad:
        return flags, bad, None, None, None
    lam = M.lagrange_at_zero(xs_old)
    share = [sum(l * y[v] for l, y in zip(lam, ys)) % R for v in range(n)]
    blind = [sum(l * y[v] for l, y in zip(lam, ys_blind)) % R for v in range(n)]
    out = [b"\xee" * 64] * (t_new * n)
    for i in (range(t_new * n) if values is None else [k * n + v for k in range(t_new) for v in values]):
        out[i] = O.g1_to_bytes(lincomb_points([O.g1_from_bytes(c[64 * i:64 * i + 64]) for c in commitments], lam))
    return flags, 0, share, blind, b"".join(out)


def crafted_lincombs(rng):
    """[(name, points, weights, base)]: one output value each, for the branches of the shared scan.  Points are multiples of G
    whose scalars make the partial sum meet its next term: equal (the doubling inside the addition), opposite (back to infinity
    in the middle of the scan, then on), an input at infinity, every input at infinity, a weight of 0."""
    G = M.G
    mul = lambda k: O.g1_mul(G, k % R)
    a = rng.randrange(1, R)
    P = mul(a)
    out = []
    # weights 1, 1 on equal points: the second addition of the top bit doubles
    out.append(("equal", [P, P], [1, 1], None))
    # weights 1, 1 on opposite points: infinity at bit 0, and that is the result
    out.append(("opposite", [P, O.g1_neg(P)], [1, 1], None))
    # weights 2, 3 on (P, -P): after the top bit (both set) the partial sum is infinity, it is doubled as infinity, and the scan goes on
    out.append(("infinity mid-scan", [P, O.g1_neg(P)], [2, 3], None))
    # full-size weights whose high parts agree on opposite points: the partial sum stays at infinity for many bits
    w = rng.randrange(1 << 200, R >> 1)
    out.append(("infinity for 100 bits", [P, O.g1_neg(P)], [w, w ^ ((1 << 100) - 1)], None))
    # second point is the first's double with half its weight's place: 2 * P + 1 * (2 P) meets an equal term after a doubling
    out.append(("equal after doubling", [P, mul(2 * a)], [2, 1], None))
    out.append(("opposite after doubling", [P, mul(-2 * a)], [2, 1], mul(5)))
    out.append(("an input at infinity", [P, None, mul(a + 1)], [rng.randrange(R), rng.randrange(R), rng.randrange(R)], None))
    out.append(("all infinity", [None, None], [rng.randrange(R), rng.randrange(R)], None))
    out.append(("all infinity with a base", [None, None], [rng.randrange(R), 1], mul(9)))
    out.append(("a weight of 0", [P, mul(a + 2)], [0, rng.randrange(R)], None))
    out.append(("every weight 0", [P, mul(a + 2)], [0, 0], None))
    out.append(("base cancels the sum", [P, mul(3)], [1, 1], mul(-a - 3)))
    out.append(("base equals the sum", [P, mul(3)], [1, 1], mul(a + 3)))
    # unweighted: equal, opposite, infinity
    out.append(("plain equal", [P, P, P], None, None))
    out.append(("plain opposite", [P, O.g1_neg(P), mul(7)], None, None))
    out.append(("plain infinity", [None, P, None], None, P))
    return out


def crafted_lanes(weights, rng):
    """[(name, points)] for ONE weight vector shared by every lane (what a launch has): per lane the dealers' points, multiples of
    G chosen so that the scan's partial sum, just before it adds the LAST dealer's point at bit b, is that point ('equal': the
    doubling inside the addition) or its opposite ('opposite': the partial sum returns to infinity there, is doubled as infinity
    and goes on), at the top bit, in the middle and at bit 0; lanes with inputs at infinity; and a random lane.  Needs bit b of
    the last weight set at the bits used, and the top bits of all weights at the same place (asserted)."""
    D, top = len(weights), weights[-1].bit_length() - 1
    assert D >= 2 and all(w.bit_length() - 1 == top for w in weights)
    mid = next(b for b in range(top // 2, top) if (weights[-1] >> b) & 1)
    low = next(b for b in range(0, top) if (weights[-1] >> b) & 1)
    mul = lambda k: O.g1_mul(M.G, k % R)
    lanes = []
    for b in (top, mid, low):
        for kind, sign in (("equal", 1), ("opposite", -1)):
            a = [rng.randrange(1, R) for _ in range(D - 1)]
            before = sum((w >> b) * ai for w, ai in zip(weights, a)) % R       # the other dealers, bit b's additions included
            den = (sign - 2 * (weights[-1] >> (b + 1))) % R                      # before + 2 (w_last >> (b + 1)) a_last = sign a_last
            a_last = before * pow(den, -1, R) % R
            assert a_last != 0 and (before + 2 * (weights[-1] >> (b + 1)) * a_last - sign * a_last) % R == 0
            lanes.append(("%s at bit %d" % (kind, b), [mul(ai) for ai in a] + [mul(a_last)]))
    P = mul(rng.randrange(1, R))
    lanes.append(("first input at infinity", [None] + [mul(rng.randrange(1, R)) for _ in range(D - 1)]))
    lanes.append(("only the last input a point", [None] * (D - 1) + [P]))
    lanes.append(("all infinity", [None] * D))
    lanes.append(("equal inputs", [P] * D))
    lanes.append(("opposite inputs", [P, O.g1_neg(P)] + [None] * (D - 2)))
    lanes.append(("random", [mul(rng.randrange(1, R)) for _ in range(D)]))
    return lanes


def crafted_weights(rng, dealers=3):
    """full-size weights with their top bits at the same place (bit 253, the first the scan reads), for crafted_lanes"""
    return [rng.randrange(1 << 253, R) for _ in range(dealers)]


def weight_vectors(rng):
    """dealers' weight lists from the special and window scalars of the sharing's tests, a 0 among them"""
    sp, ws = M.special_scalars(), M.window_scalars()
    vecs = [[s] for s in sp]                                              # one dealer, every special scalar (0: infinity)
    vecs += [[sp[i], sp[(i + 1) % len(sp)], sp[(i + 3) % len(sp)]] for i in range(len(sp))]
    vecs += [[ws[i], ws[-1 - i]] for i in range(0, len(ws), 6)]
    vecs += [[0, ws[5], rng.randrange(R)], [rng.randrange(R), 0, ws[-1]]]
    return vecs
