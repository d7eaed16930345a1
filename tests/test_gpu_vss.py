"""GPU: the auditors' key without a dealer -- spp_vss_deal, spp_vss_receive, the joint key and a share refresh -- against
tests/vss_model.py (Python integers), spp_shamir_reconstruct, spp_rlwe_key_check and the threshold opening calls that read the
share files of a dealt key."""
import ctypes
import itertools
import random

import numpy as np
import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None

import vss_model as M
from oracle import bn254 as O

pytestmark = pytest.mark.gpu

R, Q = M.R, M.Q
BAD_POINT, BAD_SHARE, NOT_ZERO = M.BAD_POINT, M.BAD_SHARE, M.NOT_ZERO
SPP_AUDIT_BAD_PARTIALS = 8


@pytest.fixture(scope="module")
def ctx():
    import spp
    c = spp.Context(0)
    yield c
    c.close()


def _inputs(rng, n, t):
    row = lambda: [rng.randrange(R) for _ in range(n)]
    return row(), row(), [row() for _ in range(t - 1)], [row() for _ in range(t - 1)]


def _reconstruct(ctx, shares):
    """spp_shamir_reconstruct with the field elements themselves as output"""
    from spp.lib import check
    t, n = len(shares), len(shares[0]["y"])
    xs = (ctypes.c_uint32 * t)(*[s["x"] for s in shares])
    ys = b"".join(int(v).to_bytes(32, "big") for s in shares for v in s["y"])
    out = ctypes.create_string_buffer(n * 32)
    check(ctx.L.spp_shamir_reconstruct(ctx.h, t, ctypes.cast(xs, ctypes.c_void_p), ys, n, ctypes.cast(out, ctypes.c_void_p), None))
    return [int.from_bytes(out.raw[32 * i:32 * i + 32], "big") for i in range(n)]


def test_host_calls_match_the_model():
    from spp import witness, lib
    L = lib.load_library()
    assert witness.vss_generators(L) == (M.G, M.H)
    for seed in (bytes(32), bytes(range(32))):
        assert witness.dkg_a_from_seed(L, seed) == M.a_from_seed(seed)


# n crosses the wave and workgroup edges of a one-lane-per-commitment launch; t in {1, 2, 3} with m in {t, 5}; the share indices
# default and {255, 1, 4294967295}; one dealing at the largest threshold
DEAL_CASES = [(1, 1, 1, None), (1, 2, 5, None), (1, 3, 3, (255, 1, 4294967295)), (63, 2, 2, None), (64, 3, 5, None), (65, 1, 5, None),
              (65, 3, 3, (255, 1, 4294967295)), (130, 2, 5, None), (130, 3, 3, None), (64, 1, 1, None), (3, 64, 64, None)]


@pytest.mark.parametrize("n,t,m,xs", DEAL_CASES)
def test_deal_against_the_model(ctx, n, t, m, xs):
    from spp import witness
    rng = random.Random(1000 * n + 10 * t + m)
    secrets, blinds, coeffs, coeffs_blind = _inputs(rng, n, t)
    got = witness.vss_deal(ctx, secrets, t, m, xs=xs, blinds=blinds, coeffs=coeffs, coeffs_blind=coeffs_blind)
    xs = list(xs) if xs else list(range(1, m + 1))
    cm, ys, yb = M.deal(secrets, blinds, coeffs, coeffs_blind, xs)
    assert got["commitments"] == cm
    assert [s["x"] for s in got["shares"]] == xs
    assert [s["y"] for s in got["shares"]] == ys and [s["y_blind"] for s in got["shares"]] == yb
    assert got["blinds"] == blinds


def test_special_scalars_and_crafted_values_in_one_launch(ctx):
    """the host test's scalar pairs as constant terms (with (0, 0): 64 zero bytes) and its crafted dealings, lane by lane in one
    launch at t = 3; the receiver at x = 2 accepts every value, the crafted ones through the equal / opposite / infinity branches"""
    from spp import witness
    rng = random.Random(77)
    t, x = 3, 2
    pairs = M.scalar_pairs()
    rows = [[c, rng.randrange(R), rng.randrange(R)] for c, _ in pairs]
    rows_b = [[cb, rng.randrange(R), rng.randrange(R)] for _, cb in pairs]
    ws = M.window_scalars()
    for i, s in enumerate(ws):                      # the window scalars in the higher coefficients as well
        rows[i][1 + i % 2], rows_b[i][2 - i % 2] = s, ws[-1 - i]
    for kind in ("equal", "opposite", "infinity"):
        r_, b_ = M.crafted_dealing(kind, t, x, rng)
        at = rng.randrange(len(rows))
        rows.insert(at, r_)
        rows_b.insert(at, b_)
    n = len(rows)
    col = lambda rr, k: [r_[k] for r_ in rr]
    secrets, blinds = col(rows, 0), col(rows_b, 0)
    coeffs, coeffs_blind = [col(rows, 1), col(rows, 2)], [col(rows_b, 1), col(rows_b, 2)]
    got = witness.vss_deal(ctx, secrets, t, 3, blinds=blinds, coeffs=coeffs, coeffs_blind=coeffs_blind)
    cm, ys, yb = M.deal(secrets, blinds, coeffs, coeffs_blind, [1, 2, 3])
    assert got["commitments"] == cm
    zero = [v for v in range(n) if rows[v][0] == 0 and rows_b[v][0] == 0]
    assert zero and all(cm[64 * v:64 * v + 64] == bytes(64) for v in zero)
    assert [s["y"] for s in got["shares"]] == ys and [s["y_blind"] for s in got["shares"]] == yb
    flags, bad, share = witness.vss_receive(ctx, t, x, [cm], [ys[1]], [yb[1]])
    assert bad == 0 and flags == [[0] * n] and share == ys[1]


def test_deal_with_os_randomness(ctx):
    """nothing supplied but the secrets: every receiver accepts its view, any t shares reconstruct the secrets, the blinds that
    were used open the constant-term commitments, and two dealings of the same secrets differ"""
    from spp import witness
    rng = random.Random(5)
    n, t, m = 40, 3, 5
    secrets = [rng.randrange(R) for _ in range(n)]
    d = witness.vss_deal(ctx, secrets, t, m)
    for sh in d["shares"]:
        flags, bad, share = witness.vss_receive(ctx, t, sh["x"], [d["commitments"]], [sh["y"]], [sh["y_blind"]])
        assert bad == 0 and flags == [[0] * n] and share == sh["y"]
    for pick in ((0, 1, 2), (4, 2, 0), (1, 3, 4)):
        assert _reconstruct(ctx, [d["shares"][j] for j in pick]) == secrets
    assert all(0 <= b < R for b in d["blinds"]) and len(set(d["blinds"])) == n
    for v in (0, n - 1):
        assert d["commitments"][64 * v:64 * v + 64] == O.g1_to_bytes(M.commit(secrets[v], d["blinds"][v]))
    assert witness.vss_deal(ctx, secrets, t, m)["commitments"] != d["commitments"]


# ---- the receiver's decisions: a valid dealing of 3 dealers, n = 70, one thing changed at a time ----
DN, DT, DM, DX = 70, 2, 3, 2          # values, threshold, dealers = receivers, the receiver under test (share index 2)
SPOTS = [(d, v) for d in (0, DM - 1) for v in (0, 63, 64, 69)]


@pytest.fixture(scope="module")
def dealing():
    """three dealers' dealings by the model (commitments as bytes) and receiver DX's view of them"""
    rng = random.Random(9)
    inputs = [_inputs(rng, DN, DT) for _ in range(DM)]
    out = [M.deal(*inp, list(range(1, DM + 1))) for inp in inputs]
    return {"inputs": inputs, "cm": [o[0] for o in out], "ys": [o[1][DX - 1] for o in out], "yb": [o[2][DX - 1] for o in out],
            "ys_other": [o[1][DX] for o in out], "yb_other": [o[2][DX] for o in out]}


def _receive(ctx, cm, ys, yb, zero=None, base=None, x=DX):
    """(flags, bad, share_out bytes pre-filled with 0xA5) through the C call itself"""
    from spp.lib import check
    dealers, n = len(cm), len(ys[0])
    be = lambda rows: b"".join(int(v).to_bytes(32, "big") for row in rows for v in row)
    flags = (ctypes.c_uint32 * (dealers * n))(*([0xDEAD] * (dealers * n)))
    out = ctypes.create_string_buffer(b"\xa5" * (n * 32), n * 32)
    bad = ctypes.c_size_t(99)
    check(ctx.L.spp_vss_receive(ctx.h, DT, x, dealers, n, b"".join(cm), be(ys), be(yb), None if zero is None else be(zero),
                                None if base is None else be([base]), ctypes.cast(flags, ctypes.c_void_p), ctypes.cast(out, ctypes.c_void_p),
                                ctypes.byref(bad)))
    return [list(flags[d * n:(d + 1) * n]) for d in range(dealers)], bad.value, out.raw


def _expect_one(ctx, d, v, flag, cm, ys, yb, zero=None):
    flags, bad, out = _receive(ctx, cm, ys, yb, zero)
    want = [[0] * DN for _ in range(DM)]
    want[d][v] = flag
    assert flags == want and bad == 1, (d, v)
    assert out == b"\xa5" * (DN * 32), "share_out written although a check failed"


def _with(rows, d, v, value):
    rows = [list(r) for r in rows]
    rows[d][v] = value
    return rows


def _with_point(cm, d, k, v, raw):
    cm = list(cm)
    at = (k * DN + v) * 64
    cm[d] = cm[d][:at] + raw + cm[d][at + 64:]
    return cm


def test_receive_accepts_the_valid_dealing(ctx, dealing):
    flags, bad, out = _receive(ctx, dealing["cm"], dealing["ys"], dealing["yb"])
    assert bad == 0 and flags == [[0] * DN] * DM
    assert out == b"".join(v.to_bytes(32, "big") for v in M.share_sum(dealing["ys"]))


@pytest.mark.parametrize("d,v", SPOTS)
def test_receive_refuses_a_wrong_share(ctx, dealing, d, v):
    cm, ys, yb = dealing["cm"], dealing["ys"], dealing["yb"]
    _expect_one(ctx, d, v, BAD_SHARE, cm, _with(ys, d, v, (ys[d][v] + 1) % R), yb)                   # y + 1
    _expect_one(ctx, d, v, BAD_SHARE, cm, ys, _with(yb, d, v, yb[d][(v + 1) % DN]))                  # y' of another value
    for k in (0, DT - 1):                                                                           # a commitment with y negated
        at = (k * DN + v) * 64
        neg = O.g1_to_bytes(O.g1_neg(O.g1_from_bytes(cm[d][at:at + 64])))
        _expect_one(ctx, d, v, BAD_SHARE, _with_point(cm, d, k, v, neg), ys, yb)


@pytest.mark.parametrize("d,v", SPOTS)
def test_receive_refuses_what_is_no_point(ctx, dealing, d, v):
    cm, ys, yb = dealing["cm"], dealing["ys"], dealing["yb"]
    for k in (0, DT - 1):
        at = (k * DN + v) * 64
        px, py = O.g1_from_bytes(cm[d][at:at + 64])
        assert px + O.P < 1 << 256
        for raw in ((px + O.P).to_bytes(32, "big") + py.to_bytes(32, "big"),                         # a coordinate + p
                    px.to_bytes(32, "big") + (py + O.P).to_bytes(32, "big"),
                    px.to_bytes(32, "big") + ((py + 1) % O.P).to_bytes(32, "big"),                   # off the curve
                    bytes(32) + py.to_bytes(32, "big")):                                             # half of infinity's encoding
            _expect_one(ctx, d, v, BAD_POINT, _with_point(cm, d, k, v, raw), ys, yb)


def test_receive_with_the_wrong_receivers_x(ctx, dealing):
    """receiver 3's index against receiver 2's sub-shares, and receiver 3's own sub-shares at its own index"""
    flags, bad, out = _receive(ctx, dealing["cm"], dealing["ys"], dealing["yb"], x=DX + 1)
    assert flags == [[BAD_SHARE] * DN] * DM and bad == DM * DN and out == b"\xa5" * (DN * 32)
    flags, bad, out = _receive(ctx, dealing["cm"], dealing["ys_other"], dealing["yb_other"], x=DX + 1)
    assert bad == 0 and out == b"".join(v.to_bytes(32, "big") for v in M.share_sum(dealing["ys_other"]))


@pytest.fixture(scope="module")
def refresh_dealing(ctx):
    """three dealings of zero (by the device call, which the tests above pin to the model) and receiver DX's view"""
    from spp import witness
    rng = random.Random(10)
    inputs = [([0] * DN,) + _inputs(rng, DN, DT)[1:] for _ in range(DM)]
    deals = [witness.vss_deal(ctx, s, DT, DM, blinds=b, coeffs=c, coeffs_blind=cb) for s, b, c, cb in inputs]
    return {"inputs": inputs, "cm": [d["commitments"] for d in deals], "ys": [d["shares"][DX - 1]["y"] for d in deals],
            "yb": [d["shares"][DX - 1]["y_blind"] for d in deals], "zero": [d["blinds"] for d in deals]}


@pytest.mark.parametrize("d,v", SPOTS)
def test_refresh_refuses_what_is_not_a_dealing_of_zero(ctx, refresh_dealing, d, v):
    f = refresh_dealing
    cm, ys, yb, zero = f["cm"], f["ys"], f["yb"], f["zero"]
    if (d, v) == SPOTS[0]:
        flags, bad, out = _receive(ctx, cm, ys, yb, zero)
        assert bad == 0 and flags == [[0] * DN] * DM and out == b"".join(x.to_bytes(32, "big") for x in M.share_sum(ys))
    # a consistent dealing of the secret 1: the share check passes, the constant term is not s' H
    one = O.g1_to_bytes(M.commit(1, zero[d][v]))
    _expect_one(ctx, d, v, NOT_ZERO, _with_point(cm, d, 0, v, one), _with(ys, d, v, (ys[d][v] + 1) % R), yb, zero)
    # a wrong published blind
    _expect_one(ctx, d, v, NOT_ZERO, cm, ys, yb, _with(zero, d, v, (zero[d][v] + 1) % R))
    # both wrong: a share that does not match and a constant term that is not the blind's
    _expect_one(ctx, d, v, BAD_SHARE | NOT_ZERO, _with_point(cm, d, 0, v, one), ys, yb, zero)


def test_sum_with_and_without_base(ctx, dealing):
    """the sum of the sub-shares alone and on top of a base, with values that wrap past r: the base r - 1, and a value whose
    sub-shares alone already exceed r (three random field elements: most do; asserted)"""
    ys = dealing["ys"]
    assert any(sum(row[v] for row in ys) >= R for v in range(DN))
    rng = random.Random(11)
    base = [R - 1] + [rng.randrange(R) for _ in range(DN - 2)] + [0]
    flags, bad, out = _receive(ctx, dealing["cm"], ys, dealing["yb"], base=base)
    assert bad == 0 and out == b"".join(v.to_bytes(32, "big") for v in M.share_sum(ys, base))
    assert M.share_sum(ys, base)[0] == (M.share_sum(ys)[0] - 1) % R


def test_refusals(ctx, dealing):
    """every argument the header lists: SPP_ERR_BAD_INPUT, the index named, the outputs untouched"""
    from spp.lib import SppError, SPP_ERR_BAD_INPUT
    L, h = ctx.L, ctx.h
    n, t, m = 4, 2, 3
    be = lambda vals: b"".join(int(v).to_bytes(32, "big") for v in vals)
    good = be(range(1, n + 1))
    ys, yb = (ctypes.create_string_buffer(b"\xa5" * (m * n * 32), m * n * 32) for _ in range(2))
    cm = ctypes.create_string_buffer(b"\xa5" * (t * n * 64), t * n * 64)
    bo = ctypes.create_string_buffer(b"\xa5" * (n * 32), n * 32)
    p = lambda b: ctypes.cast(b, ctypes.c_void_p)
    xs = lambda *v: p((ctypes.c_uint32 * len(v))(*v))

    def deal(t=t, m=m, xs_=None, n=n, secrets=good, blinds=None, coeffs=None, coeffs_blind=None, ys_=p(ys), yb_=p(yb), cm_=p(cm), h_=h):
        return L.spp_vss_deal(h_, t, m, xs_, n, secrets, blinds, coeffs, coeffs_blind, ys_, yb_, cm_, p(bo))

    def refused(rc, *words):
        from spp.lib import last_error
        assert rc == SPP_ERR_BAD_INPUT, rc
        msg = last_error()
        assert all(w in msg for w in words), msg
        assert ys.raw == b"\xa5" * (m * n * 32) and yb.raw == ys.raw and cm.raw == b"\xa5" * (t * n * 64) and bo.raw == b"\xa5" * (n * 32)

    refused(deal(h_=None), "NULL"); refused(deal(secrets=None), "NULL"); refused(deal(ys_=None), "NULL")
    refused(deal(yb_=None), "NULL"); refused(deal(cm_=None), "NULL")
    refused(deal(t=0), "threshold 0"); refused(deal(t=65, m=70), "threshold 65")
    refused(deal(m=1), "1 shares"); refused(deal(m=256), "256 shares")
    refused(deal(xs_=xs(1, 0, 3)), "xs[1] is 0"); refused(deal(xs_=xs(7, 2, 7)), "xs[2] repeats xs[0]")
    refused(deal(secrets=be([1, 2, R, 4])), "secret 2"); refused(deal(blinds=be([1, 2, 3, R + 5])), "blind 3")
    refused(deal(coeffs=be([1, R, 3, 4])), "coefficient 1"); refused(deal(coeffs_blind=be([R, 2, 3, 4])), "blinding coefficient 0")
    refused(deal(n=(1 << 20) + 1), "2^20")
    assert deal(n=0) == 0
    assert ys.raw == b"\xa5" * (m * n * 32) and cm.raw == b"\xa5" * (t * n * 64)

    D = 2
    c_in, y_in = bytes(D * t * n * 64), be([1] * (D * n))
    flags = (ctypes.c_uint32 * (D * n))(*([0xDEAD] * (D * n)))
    out = ctypes.create_string_buffer(b"\xa5" * (n * 32), n * 32)
    bad = ctypes.c_size_t(99)

    def receive(t=t, x=1, dealers=D, n=n, cm_=c_in, ys_=y_in, yb_=y_in, zero=None, base=None, flags_=p(flags), bad_=ctypes.byref(bad), h_=h):
        return L.spp_vss_receive(h_, t, x, dealers, n, cm_, ys_, yb_, zero, base, flags_, p(out), bad_)

    def refused2(rc, *words):
        from spp.lib import last_error
        assert rc == SPP_ERR_BAD_INPUT, rc
        msg = last_error()
        assert all(w in msg for w in words), msg
        assert list(flags) == [0xDEAD] * (D * n) and out.raw == b"\xa5" * (n * 32) and bad.value == 99

    refused2(receive(h_=None), "NULL"); refused2(receive(cm_=None), "NULL"); refused2(receive(ys_=None), "NULL")
    refused2(receive(yb_=None), "NULL"); refused2(receive(flags_=None), "NULL"); refused2(receive(bad_=None), "NULL")
    refused2(receive(t=0), "threshold 0"); refused2(receive(t=65), "threshold 65"); refused2(receive(x=0), "x is 0")
    refused2(receive(dealers=0), "0 dealers"); refused2(receive(dealers=256), "256 dealers"); refused2(receive(n=(1 << 20) + 1), "2^20")
    refused2(receive(ys_=be([1] * 5 + [R] + [1] * 2)), "sub-share 5"); refused2(receive(yb_=be([1] * 7 + [R])), "sub-share blind 7")
    refused2(receive(zero=be([R] + [1] * 7)), "published blind 0"); refused2(receive(base=be([1, 2, 3, R])), "base share value 3")
    assert receive(n=0) == 0 and bad.value == 0
    assert SppError is not None


# ---- end to end at the ring's size: three auditors make a key, open records with it, refresh their shares ----
@pytest.fixture(scope="module")
def joint(ctx):
    from spp import witness, lib
    L = lib.load_library()
    rng = np.random.default_rng(21)
    t, m = 2, 3
    a = witness.dkg_a_from_seed(L, bytes(range(32)))
    parts = [(rng.integers(-3, 4, 1024).astype(np.int8), rng.integers(-3, 4, 1024).astype(np.int8)) for _ in range(m)]
    parts[0][0][:4] = (3, -3, 3, -3)                       # every auditor's extreme at the same coefficient: |sum| = 9
    parts[1][0][:4] = (3, -3, 3, -3)
    parts[2][0][:4] = (3, -3, 3, -3)
    bs = [witness.rlwe_keygen(ctx, s, a, e)[0][0].tolist() for s, e in parts]
    deals = [witness.vss_deal(ctx, [int(v) % R for v in s], t, m) for s, _ in parts]
    return {"t": t, "m": m, "a": a, "parts": parts, "bs": bs, "deals": deals}


def _receive_all(ctx, t, deals, zero=False, bases=None):
    from spp import witness
    shares = []
    for j in range(len(deals)):
        flags, bad, share = witness.vss_receive(ctx, t, j + 1, [d["commitments"] for d in deals], [d["shares"][j]["y"] for d in deals],
                                                [d["shares"][j]["y_blind"] for d in deals],
                                                zero_blinds=[d["blinds"] for d in deals] if zero else None,
                                                base=None if bases is None else bases[j]["y"])
        assert bad == 0 and all(f == 0 for row in flags for f in row)
        shares.append({"x": j + 1, "y": share})
    return shares


def test_joint_key(ctx, joint):
    """three deals, three receives: one public key, the model's; any two shares are the sum of the three secrets; the key checks"""
    from spp import witness
    t, m, a = joint["t"], joint["m"], joint["a"]
    pks = [[sum(b[v] for b in joint["bs"]) % Q for v in range(1024)] for _ in range(m)]       # every receiver sums the same public b_i
    want_b, want_s = M.joint_key(a, [(s.tolist(), e.tolist()) for s, e in joint["parts"]])
    assert pks[0] == pks[1] == pks[2] == want_b
    shares = _receive_all(ctx, t, joint["deals"])
    joint["shares"] = shares
    assert max(abs(v) for v in want_s) == 9
    for pick in itertools.combinations(range(m), t):
        assert _reconstruct(ctx, [shares[j] for j in pick]) == [v % R for v in want_s]
        skq = witness.reconstruct_sk(ctx, [shares[j] for j in pick])
        assert skq == [v % Q for v in want_s]
        noise, skmax = witness.rlwe_key_check(ctx, a, want_b, skq)[0]
        assert noise <= 9 and skmax <= 9 and skmax == 9


def _records():
    """four records: every byte 0 with noise +3 throughout, every byte 255 with noise -3, two random ones"""
    rng = np.random.default_rng(22)
    msg = rng.integers(0, 256, (4, 64)).astype(np.uint8)
    r, e1, e2 = (rng.integers(-3, 4, (4, k)).astype(np.int8) for k in (1024, 64, 1024))
    msg[0], msg[1] = 0, 255
    for arr in (r, e1, e2):
        arr[0], arr[1] = 3, -3
    return msg, r, e1, e2


def _open(ctx, pair, c0, c1):
    from spp import witness
    xs = [s["x"] for s in pair]
    partials = [witness.rlwe_partial_decrypt(ctx, xs, me, s["y"], c0, c1) for me, s in enumerate(pair)]
    _, msg, flags = witness.rlwe_combine_partials(ctx, partials, c0)
    return msg, flags


def test_opening_and_refresh(ctx, joint):
    """Records encrypted to the joint key open from any two aggregated shares through partial decryptions, before and after a
    refresh round.  An old share combined with a new one: the two differ by a full-size field element, so the combined slot is a
    random field element and not an integer below 2^104 -- the existing combine rule raises SPP_AUDIT_BAD_PARTIALS on every
    record (it does not merely give another message)."""
    from spp import witness
    t, m, a = joint["t"], joint["m"], joint["a"]
    shares = joint.get("shares") or _receive_all(ctx, t, joint["deals"])
    pk_b = [sum(b[v] for b in joint["bs"]) % Q for v in range(1024)]
    msg, r, e1, e2 = _records()
    w = witness.rlwe_witness(ctx, a, pk_b, r, e1, e2, msg)
    c0, c1 = w["c0"], w["c1"]
    for pick in itertools.combinations(range(m), t):
        got, flags = _open(ctx, [shares[j] for j in pick], c0, c1)
        assert flags == [0] * 4 and np.array_equal(got, msg), pick
    refresh = [witness.vss_deal(ctx, [0] * 1024, t, m) for _ in range(m)]
    new = _receive_all(ctx, t, refresh, zero=True, bases=shares)
    assert all(n_["y"] != o["y"] for n_, o in zip(new, shares))
    for pick in itertools.combinations(range(m), t):
        got, flags = _open(ctx, [new[j] for j in pick], c0, c1)
        assert flags == [0] * 4 and np.array_equal(got, msg), pick
    got, flags = _open(ctx, [shares[0], new[1]], c0, c1)
    assert flags == [SPP_AUDIT_BAD_PARTIALS] * 4
