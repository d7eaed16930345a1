"""GPU: the committee's commitments and verifiable resharing -- spp_vss_combine_commitments, spp_vss_share_commitments,
spp_vss_reshare_receive -- against tests/reshare_model.py (Python integers), and end to end at the ring's size: a joint key, a
refresh round, the hand-over to a new committee, and the record that still opens."""
import ctypes
import random

import numpy as np
import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None

import reshare_model as RM
import vss_model as M
from oracle import bn254 as O

pytestmark = pytest.mark.gpu

R, Q = M.R, M.Q
BAD_POINT, BAD_SHARE, NOT_SHARE = RM.BAD_POINT, RM.BAD_SHARE, RM.NOT_SHARE
SPP_AUDIT_BAD_PARTIALS = 8
XS = (1, 2, 255, 4294967295)


@pytest.fixture(scope="module")
def ctx():
    import spp
    c = spp.Context(0)
    yield c
    c.close()


def _be(vals):
    return b"".join(int(v).to_bytes(32, "big") for v in vals)


def _random_points(ctx, rng, count):
    """count * 64 bytes of random curve points: the commitments of a dealing (tests/test_gpu_vss.py pins those to the model)"""
    from spp import witness
    return witness.vss_deal(ctx, [rng.randrange(R) for _ in range(count)], 1, 1)["commitments"]


# n crosses the wave edges of a one-lane-per-point launch; t' = 64 and 64 dealers once each
COMBINE_CASES = [(1, 1, 1), (63, 2, 2), (64, 3, 2), (65, 1, 3), (130, 2, 3), (3, 64, 2), (2, 2, 64)]


@pytest.mark.parametrize("n,t,dealers", COMBINE_CASES)
def test_combine_against_the_model(ctx, n, t, dealers):
    """weighted with the Lagrange weights of {1..dealers}; and weights = NULL on top of a base"""
    from spp import witness
    rng = random.Random(10000 * n + 100 * t + dealers)
    cms = [_random_points(ctx, rng, t * n) for _ in range(dealers)]
    base = _random_points(ctx, rng, t * n)
    lam = M.lagrange_at_zero(list(range(1, dealers + 1)))
    assert witness.lagrange_at_zero(range(1, dealers + 1)) == lam
    flags, bad, out = witness.vss_combine_commitments(ctx, t, cms, weights=lam)
    assert bad == 0 and flags == [[0] * (t * n)] * dealers
    assert out == RM.combine(cms, lam)[2]
    flags, bad, out = witness.vss_combine_commitments(ctx, t, cms, base=base)
    assert bad == 0 and flags == [[0] * (t * n)] * dealers
    assert out == RM.combine(cms, None, base)[2]


def test_crafted_values_in_one_launch(ctx):
    """the host test's crafted lanes at t' = 3, lane by lane under ONE weight vector, so the equal, opposite and infinity branches
    of the addition run on the device inside the shared scan; then the plain sums of equal, opposite and infinity inputs"""
    from spp import witness
    rng = random.Random(67)
    t = 3
    for dealers in (2, 3):
        weights = RM.crafted_weights(rng, dealers)
        lanes = [pts for _, pts in RM.crafted_lanes(weights, rng)]
        n = len(lanes)
        cms = [b"".join(O.g1_to_bytes(lanes[(v + k) % n][d]) for k in range(t) for v in range(n)) for d in range(dealers)]
        flags, bad, out = witness.vss_combine_commitments(ctx, t, cms, weights=weights)
        want = [O.g1_to_bytes(RM.lincomb_points(pts, weights)) for pts in lanes]
        assert bad == 0 and out == b"".join(want[(v + k) % n] for k in range(t) for v in range(n))
        assert bytes(64) in want
        flags, bad, out = witness.vss_combine_commitments(ctx, t, cms)
        plain = [O.g1_to_bytes(RM.lincomb_points(pts)) for pts in lanes]
        assert bad == 0 and out == b"".join(plain[(v + k) % n] for k in range(t) for v in range(n))
    # a weight of 0, every weight 0
    cms = [_random_points(ctx, rng, t * 5) for _ in range(2)]
    for w in ([0, 7], [R - 1, 0], [0, 0]):
        assert witness.vss_combine_commitments(ctx, t, cms, weights=w)[2] == RM.combine(cms, w)[2]


def test_combine_flags_every_input_that_is_no_point(ctx):
    from spp.lib import check
    rng = random.Random(3)
    n, t, dealers = 66, 2, 3
    cms = [bytearray(_random_points(ctx, rng, t * n)) for _ in range(dealers)]
    spots = [(0, 0, 0), (1, 1, 63), (2, 0, 64), (2, 1, 65)]
    for d, k, v in spots:
        at = (k * n + v) * 64
        px = int.from_bytes(cms[d][at:at + 32], "big")
        cms[d][at:at + 32] = (px + O.P).to_bytes(32, "big") if (d + v) % 2 else ((px + 1) % O.P).to_bytes(32, "big")
    for weights in (None, _be([3, 5, 7])):
        flags = (ctypes.c_uint32 * (dealers * t * n))(*([0xDEAD] * (dealers * t * n)))
        out = ctypes.create_string_buffer(b"\xa5" * (t * n * 64), t * n * 64)
        bad = ctypes.c_size_t(99)
        check(ctx.L.spp_vss_combine_commitments(ctx.h, t, dealers, n, b"".join(bytes(c) for c in cms), weights, None,
                                                ctypes.cast(out, ctypes.c_void_p), ctypes.cast(flags, ctypes.c_void_p), ctypes.byref(bad)))
        want = [0] * (dealers * t * n)
        for d, k, v in spots:
            want[(d * t + k) * n + v] = BAD_POINT
        assert list(flags) == want and bad.value == len(spots) and out.raw == b"\xa5" * (t * n * 64)


# ---- a committee of three at threshold 2 (by the device's dealings, pinned to the model elsewhere), its commitments by the model ----
CN, CT, CM = 65, 2, 3


@pytest.fixture(scope="module")
def committee(ctx):
    from spp import witness
    rng = random.Random(12)
    deals = [witness.vss_deal(ctx, [rng.randrange(R) for _ in range(CN)], CT, CM) for _ in range(CM)]
    D = RM.combine([d["commitments"] for d in deals])[2]
    shares = [M.share_sum([d["shares"][j]["y"] for d in deals]) for j in range(CM)]
    blinds = [M.share_sum([d["shares"][j]["y_blind"] for d in deals]) for j in range(CM)]
    return {"D": D, "shares": shares, "blinds": blinds, "deals": deals}


@pytest.mark.parametrize("t", [1, 2, 3])
def test_share_commitments_against_the_model(ctx, t):
    from spp import witness
    rng = random.Random(40 + t)
    n = 17                                                   # 4 * 17 lanes: more than one wave
    D = bytearray(_random_points(ctx, rng, t * n))
    if t > 1:                                                # crafted values: the Horner walk meets +-its next term, a middle term at infinity
        for v, kind in enumerate(("equal", "opposite", "infinity")):
            rows, rows_b = M.crafted_dealing(kind, t, XS[v + 1], rng)
            for k in range(t):
                D[(k * n + v) * 64:(k * n + v) * 64 + 64] = O.g1_to_bytes(M.commit(rows[k], rows_b[k]))
    D = bytes(D)
    got = witness.vss_share_commitments(ctx, t, D, XS)
    assert got == RM.share_commitments(t, n, D, XS)
    if t > 1:
        assert got[2][64:128] == bytes(64)                   # the opposite dealing at its x = 255


def test_a_member_checks_its_share_against_the_committee(ctx, committee):
    """spp_vss_receive with dealers = 1, commitments = D, x = x_j accepts each member's summed (share, blind), refuses it at another
    x, and the device's own sum of the dealings is the model's D"""
    from spp import witness
    c = committee
    flags, bad, D = witness.vss_combine_commitments(ctx, CT, [d["commitments"] for d in c["deals"]])
    assert bad == 0 and D == c["D"]
    for j in range(CM):
        flags, bad, share = witness.vss_receive(ctx, CT, j + 1, [D], [c["shares"][j]], [c["blinds"][j]])
        assert bad == 0 and flags == [[0] * CN] and share == c["shares"][j]
        flags, bad, share = witness.vss_receive(ctx, CT, (j + 1) % CM + 1, [D], [c["shares"][j]], [c["blinds"][j]])
        assert bad == CN and flags == [[BAD_SHARE] * CN] and share is None
    E = witness.vss_share_commitments(ctx, CT, D, [1, 2, 3])
    for j in range(CM):
        for v in (0, 63, 64):
            assert E[j][64 * v:64 * v + 64] == O.g1_to_bytes(M.commit(c["shares"][j][v], c["blinds"][j][v]))


# ---- reshare: S = {1, 3} of the committee above deal to (3, 5); the new member at x = 4 ----
ST, SM, SX = 3, 5, 4
S = (1, 3)


@pytest.fixture(scope="module")
def resharing(ctx, committee):
    from spp import witness
    c = committee
    deals = [witness.vss_deal(ctx, c["shares"][j - 1], ST, SM, blinds=c["blinds"][j - 1]) for j in S]
    view = {"cm": [d["commitments"] for d in deals], "ys": [d["shares"][SX - 1]["y"] for d in deals],
            "yb": [d["shares"][SX - 1]["y_blind"] for d in deals], "deals": deals}
    view["model"] = RM.reshare_receive(list(S), ST, SX, CN, c["D"], view["cm"], view["ys"], view["yb"])
    return view


def _reshare(ctx, D, cm, ys, yb, xs_old=S, t_new=ST, x_new=SX, n=CN):
    """(flags, bad, share_out, blind_out, committee_out) through the C call itself, the outputs pre-filled with 0xA5"""
    from spp.lib import check
    t_old = len(xs_old)
    flags = (ctypes.c_uint32 * (t_old * n))(*([0xDEAD] * (t_old * n)))
    share, blind = (ctypes.create_string_buffer(b"\xa5" * (n * 32), n * 32) for _ in range(2))
    out = ctypes.create_string_buffer(b"\xa5" * (t_new * n * 64), t_new * n * 64)
    bad = ctypes.c_size_t(99)
    p = lambda b: ctypes.cast(b, ctypes.c_void_p)
    check(ctx.L.spp_vss_reshare_receive(ctx.h, t_old, p((ctypes.c_uint32 * t_old)(*xs_old)), t_new, x_new, n, D, b"".join(cm),
                                        _be(v for row in ys for v in row), _be(v for row in yb for v in row), p(flags), p(share), p(blind),
                                        p(out), ctypes.byref(bad)))
    return [list(flags[j * n:(j + 1) * n]) for j in range(t_old)], bad.value, share.raw, blind.raw, out.raw


def _refused_with(ctx, D, cm, ys, yb, want):
    flags, bad, share, blind, out = _reshare(ctx, D, cm, ys, yb)
    assert flags == want and bad == sum(f != 0 for row in want for f in row)
    assert share == b"\xa5" * (CN * 32) and blind == share and out == b"\xa5" * (ST * CN * 64), "an output written although a check failed"


def test_reshare_receive_against_the_model(ctx, committee, resharing):
    r, D = resharing, committee["D"]
    mflags, mbad, mshare, mblind, mout = r["model"]
    assert mbad == 0
    flags, bad, share, blind, out = _reshare(ctx, D, r["cm"], r["ys"], r["yb"])
    assert bad == 0 and flags == mflags == [[0] * CN] * 2
    assert share == _be(mshare) and blind == _be(mblind) and out == mout
    assert out[:CN * 64] == D[:CN * 64]                                                  # D'_0 == D_0
    for v in (0, 64):                                                                    # share' G + blind' H == E'_x under D'
        assert O.g1_to_bytes(M.commit(mshare[v], mblind[v])) == O.g1_to_bytes(RM.share_commitment(ST, CN, out, SX, v))


@pytest.mark.parametrize("j,v", [(0, 0), (1, 63), (0, 64)])
def test_reshare_receive_refusals_by_flag(ctx, committee, resharing, j, v):
    from spp import witness
    r, c = resharing, committee
    D, cm, ys, yb = c["D"], r["cm"], r["ys"], r["yb"]
    one = lambda flag: [[flag if (jj, vv) == (j, v) else 0 for vv in range(CN)] for jj in range(2)]
    with_ = lambda rows, val: [[val if (jj, vv) == (j, v) else x for vv, x in enumerate(row)] for jj, row in enumerate(rows)]
    # one wrong sub-share, one wrong blind
    _refused_with(ctx, D, cm, with_(ys, (ys[j][v] + 1) % R), yb, one(BAD_SHARE))
    _refused_with(ctx, D, cm, ys, with_(yb, (yb[j][v] + 1) % R), one(BAD_SHARE))
    # the member deals share + 1 at value v, consistently: every sub-share checks, the constant term is not its share commitment
    secrets = list(c["shares"][S[j] - 1])
    secrets[v] = (secrets[v] + 1) % R
    d = witness.vss_deal(ctx, secrets, ST, SM, blinds=c["blinds"][S[j] - 1])
    sub = lambda rows, row: [row if jj == j else x for jj, x in enumerate(rows)]
    _refused_with(ctx, D, sub(cm, d["commitments"]), sub(ys, d["shares"][SX - 1]["y"]), sub(yb, d["shares"][SX - 1]["y_blind"]), one(NOT_SHARE))
    # the same with another blind: the share is right, the commitment still is not E_x
    d = witness.vss_deal(ctx, c["shares"][S[j] - 1], ST, SM, blinds=with_([c["blinds"][S[jj] - 1] for jj in range(2)], 5)[j])
    _refused_with(ctx, D, sub(cm, d["commitments"]), sub(ys, d["shares"][SX - 1]["y"]), sub(yb, d["shares"][SX - 1]["y_blind"]), one(NOT_SHARE))
    # what is no point: BAD_POINT alone, in the constant term and in the top coefficient
    for k in (0, ST - 1):
        at = (k * CN + v) * 64
        px = int.from_bytes(cm[j][at:at + 32], "big")
        raw = cm[j][:at] + (px + O.P).to_bytes(32, "big") + cm[j][at + 32:]
        _refused_with(ctx, D, sub(cm, raw), ys, yb, one(BAD_POINT))


def test_reshare_receive_with_another_set_or_receiver(ctx, committee, resharing):
    """the dealings of {1, 3} read as those of {1, 2}: member 3's constant terms are not E_2; the sub-shares of x = 4 at x = 5"""
    r, D = resharing, committee["D"]
    flags, bad, *_ = _reshare(ctx, D, r["cm"], r["ys"], r["yb"], xs_old=(1, 2))
    assert flags == [[0] * CN, [NOT_SHARE] * CN] and bad == CN
    flags, bad, *_ = _reshare(ctx, D, r["cm"], r["ys"], r["yb"], x_new=5)
    assert flags == [[BAD_SHARE] * CN] * 2 and bad == 2 * CN


def test_refusals(ctx):
    """every argument the header lists: SPP_ERR_BAD_INPUT, the index named, the outputs untouched; n == 0"""
    from spp.lib import SPP_ERR_BAD_INPUT, last_error
    L, h = ctx.L, ctx.h
    rng = random.Random(8)
    n, t, D_ = 4, 2, 2
    p = lambda b: ctypes.cast(b, ctypes.c_void_p)
    pts = _random_points(ctx, rng, D_ * t * n)
    notpt = pts[:64 * 5] + bytes(31) + b"\x01" + pts[64 * 5 + 32:]
    flags = (ctypes.c_uint32 * (D_ * t * n))(*([0xDEAD] * (D_ * t * n)))
    out = ctypes.create_string_buffer(b"\xa5" * (t * n * 64), t * n * 64)
    share, blind = (ctypes.create_string_buffer(b"\xa5" * (n * 32), n * 32) for _ in range(2))
    bad = ctypes.c_size_t(99)
    xs = lambda *v: p((ctypes.c_uint32 * len(v))(*v))

    def refused(rc, *words):
        assert rc == SPP_ERR_BAD_INPUT, rc
        msg = last_error()
        assert all(w in msg for w in words), msg
        assert list(flags) == [0xDEAD] * (D_ * t * n) and out.raw == b"\xa5" * (t * n * 64) and bad.value == 99
        assert share.raw == b"\xa5" * (n * 32) and blind.raw == share.raw

    def combine(t=t, dealers=D_, n=n, cm=pts, w=None, base=None, out_=p(out), flags_=p(flags), bad_=ctypes.byref(bad), h_=h):
        return L.spp_vss_combine_commitments(h_, t, dealers, n, cm, w, base, out_, flags_, bad_)

    refused(combine(h_=None), "NULL"); refused(combine(cm=None), "NULL"); refused(combine(out_=None), "NULL")
    refused(combine(flags_=None), "NULL"); refused(combine(bad_=None), "NULL")
    refused(combine(t=0), "threshold 0"); refused(combine(t=65), "threshold 65")
    refused(combine(dealers=0), "0 dealers"); refused(combine(dealers=256), "256 dealers")
    refused(combine(dealers=65, w=_be([1] * 65)), "65 dealers", "64")
    refused(combine(w=_be([1, R])), "weight 1"); refused(combine(n=(1 << 20) + 1), "2^20")
    refused(combine(base=notpt[:t * n * 64]), "base point 5")
    assert combine(n=0) == 0 and bad.value == 0
    bad.value = 99
    ms = ctypes.c_float(-1)
    assert L.spp_vss_combine_commitments_timed(h, 0, D_, n, pts, None, None, p(out), p(flags), ctypes.byref(bad), ctypes.byref(ms)) == SPP_ERR_BAD_INPUT

    D = pts[:t * n * 64]

    def commits(t=t, n=n, cm=D, count=2, xs_=xs(1, 2), out_=p(out), h_=h):
        return L.spp_vss_share_commitments(h_, t, n, cm, count, xs_, out_)

    refused(commits(h_=None), "NULL"); refused(commits(cm=None), "NULL"); refused(commits(xs_=None), "NULL"); refused(commits(out_=None), "NULL")
    refused(commits(t=0), "threshold 0"); refused(commits(t=65), "threshold 65")
    refused(commits(count=0), "0 indices"); refused(commits(count=256), "256 indices")
    refused(commits(xs_=xs(3, 0)), "xs[1] is 0"); refused(commits(xs_=xs(7, 7)), "xs[1] repeats xs[0]")
    refused(commits(n=(1 << 20) + 1), "2^20"); refused(commits(cm=notpt[:t * n * 64]), "committee commitment 5")
    assert commits(n=0) == 0 and out.raw == b"\xa5" * (t * n * 64)

    t_new = 1                                   # commitments t_old * t_new * n = the t * n points of D; committee_out fits in `out`
    y_in = _be([1] * (t * n))

    def receive(t_old=t, xs_=xs(1, 2), t_new=t_new, x_new=3, n=n, old=D, cm=D, ys=y_in, yb=y_in, flags_=p(flags), share_=p(share),
                blind_=p(blind), out_=p(out), bad_=ctypes.byref(bad), h_=h):
        return L.spp_vss_reshare_receive(h_, t_old, xs_, t_new, x_new, n, old, cm, ys, yb, flags_, share_, blind_, out_, bad_)

    for name in ("h_", "xs_", "old", "cm", "ys", "yb", "flags_", "share_", "blind_", "out_", "bad_"):
        refused(receive(**{name: None}), "NULL")
    refused(receive(t_old=0), "old threshold 0"); refused(receive(t_old=65), "old threshold 65")
    refused(receive(t_new=0), "new threshold 0"); refused(receive(t_new=65), "new threshold 65")
    refused(receive(x_new=0), "x_new is 0")
    refused(receive(xs_=xs(0, 2)), "xs_old[0] is 0"); refused(receive(xs_=xs(2, 2)), "xs_old[1] repeats xs_old[0]")
    refused(receive(n=(1 << 20) + 1), "2^20")
    refused(receive(ys=_be([1] * 6 + [R, 1])), "sub-share 6"); refused(receive(yb=_be([R] + [1] * 7)), "sub-share blind 0")
    refused(receive(old=notpt[:t * n * 64]), "committee commitment 5")
    assert receive(n=0) == 0 and bad.value == 0


# ---- end to end at the ring's size: a joint key of three, a refresh round, the hand-over to five, and back to three ----
def _reconstruct(ctx, shares):
    from spp.lib import check
    t, n = len(shares), len(shares[0]["y"])
    xs = (ctypes.c_uint32 * t)(*[s["x"] for s in shares])
    out = ctypes.create_string_buffer(n * 32)
    check(ctx.L.spp_shamir_reconstruct(ctx.h, t, ctypes.cast(xs, ctypes.c_void_p), _be(v for s in shares for v in s["y"]), n,
                                       ctypes.cast(out, ctypes.c_void_p), None))
    return [int.from_bytes(out.raw[32 * i:32 * i + 32], "big") for i in range(n)]


def _round(ctx, t, m, deals, old=None, D=None):
    """every member receives the dealings of a key round (old None) or of a refresh round on top of (shares, blinds, D); returns
    the members {"x", "y", "blind"} and the committee's commitments"""
    from spp import witness
    members = []
    for j in range(m):
        flags, bad, share = witness.vss_receive(ctx, t, j + 1, [d["commitments"] for d in deals], [d["shares"][j]["y"] for d in deals],
                                                [d["shares"][j]["y_blind"] for d in deals],
                                                zero_blinds=[d["blinds"] for d in deals] if old else None, base=old[j]["y"] if old else None)
        assert bad == 0
        blind = M.share_sum([d["shares"][j]["y_blind"] for d in deals], old[j]["blind"] if old else None)
        members.append({"x": j + 1, "y": share, "blind": blind})
    flags, bad, D = witness.vss_combine_commitments(ctx, t, [d["commitments"] for d in deals], base=D)
    assert bad == 0
    return members, D


def _hand_over(ctx, members, D, t_new, m_new):
    """the members given (as many as the old threshold) deal to a new committee; every new member receives and checks itself"""
    from spp import witness
    xs_old = [mem["x"] for mem in members]
    deals = [witness.vss_deal(ctx, mem["y"], t_new, m_new, blinds=mem["blind"]) for mem in members]
    new, D_new = [], None
    for k in range(m_new):
        flags, bad, share, blind, out = witness.vss_reshare_receive(ctx, xs_old, t_new, k + 1, D, [d["commitments"] for d in deals],
                                                                    [d["shares"][k]["y"] for d in deals],
                                                                    [d["shares"][k]["y_blind"] for d in deals])
        assert bad == 0
        assert D_new is None or out == D_new                       # every new member computes the same committee file
        D_new = out
        flags, bad, _ = witness.vss_receive(ctx, t_new, k + 1, [out], [share], [blind], want_share=False)
        assert bad == 0                                            # all 1 024 values of (share', blind') against D' on the device
        new.append({"x": k + 1, "y": share, "blind": blind})
    return new, D_new, deals


def _open(ctx, group, c0, c1):
    from spp import witness
    xs = [s["x"] for s in group]
    partials = [witness.rlwe_partial_decrypt(ctx, xs, me, s["y"], c0, c1) for me, s in enumerate(group)]
    _, msg, flags = witness.rlwe_combine_partials(ctx, partials, c0)
    return msg, flags


def test_end_to_end_hand_over(ctx):
    from spp import witness, lib
    L = lib.load_library()
    rng = np.random.default_rng(31)
    prng = random.Random(32)
    t, m = 2, 3
    a = witness.dkg_a_from_seed(L, bytes(range(32)))
    parts = [(rng.integers(-3, 4, 1024).astype(np.int8), rng.integers(-3, 4, 1024).astype(np.int8)) for _ in range(m)]
    pk_b = [int(v) for v in sum(np.array(witness.rlwe_keygen(ctx, s, a, e)[0][0], dtype=np.int64) for s, e in parts) % Q]
    key = [sum(int(s[v]) for s, _ in parts) % R for v in range(1024)]
    old, D = _round(ctx, t, m, [witness.vss_deal(ctx, [int(v) % R for v in s], t, m) for s, _ in parts])
    old, D = _round(ctx, t, m, [witness.vss_deal(ctx, [0] * 1024, t, m) for _ in range(m)], old, D)
    D0 = D[:1024 * 64]                                             # commits to the key; a refresh re-blinds it, a hand-over must not touch it
    # a record under the unchanged public key, opened by the old committee
    msg = rng.integers(0, 256, (2, 64)).astype(np.uint8)
    r, e1, e2 = (rng.integers(-3, 4, (2, k)).astype(np.int8) for k in (1024, 64, 1024))
    w = witness.rlwe_witness(ctx, a, pk_b, r, e1, e2, msg)
    c0, c1 = w["c0"], w["c1"]
    opened, flags = _open(ctx, [old[0], old[2]], c0, c1)
    assert flags == [0, 0] and np.array_equal(opened, msg)

    # ---- the hand-over: S = {1, 3} -> (3, 5) ----
    new, D_new, deals = _hand_over(ctx, [old[0], old[2]], D, 3, 5)
    assert D_new[:1024 * 64] == D0                                 # D'_0 == D_0 for all 1 024 values: the key is this key
    lam = M.lagrange_at_zero([1, 3])
    for v in prng.sample(range(1024), 16):                         # D' against the model on 16 values: a cap on the model's cost
        for k in range(3):
            at = (k * 1024 + v) * 64
            assert D_new[at:at + 64] == O.g1_to_bytes(RM.lincomb_points([O.g1_from_bytes(d["commitments"][at:at + 64]) for d in deals], lam)), (k, v)
    for pick in ((0, 1, 2), (4, 2, 1)):
        assert _reconstruct(ctx, [new[j] for j in pick]) == key
    skq = witness.reconstruct_sk(ctx, [new[j] for j in (0, 3, 4)])
    noise, skmax = witness.rlwe_key_check(ctx, a, pk_b, skq)[0]
    assert noise <= 9 and skmax <= 9
    got, flags = _open(ctx, [new[0], new[2], new[4]], c0, c1)
    assert flags == [0, 0] and got.tobytes() == opened.tobytes()
    got, flags = _open(ctx, [old[1], new[0], new[2]], c0, c1)     # one old and two new members
    assert flags == [SPP_AUDIT_BAD_PARTIALS] * 2
    assert _reconstruct(ctx, [old[1], new[0], new[2]]) != key

    # ---- a refresh among the five, then back to (2, 3) from S = {2, 4, 5} ----
    new, D_new = _round(ctx, 3, 5, [witness.vss_deal(ctx, [0] * 1024, 3, 5) for _ in range(5)], new, D_new)
    assert D_new[:1024 * 64] != D0
    back, D_back, _ = _hand_over(ctx, [new[1], new[3], new[4]], D_new, 2, 3)
    assert D_back[:1024 * 64] == D_new[:1024 * 64]
    assert _reconstruct(ctx, [back[2], back[0]]) == key
    got, flags = _open(ctx, [back[1], back[2]], c0, c1)
    assert flags == [0, 0] and got.tobytes() == opened.tobytes()
