"""The powers-of-tau transcript on the GPU: the per-point scalar multiplication through its unit entry points (G1 and G2) against
oracle/bn254.py big integers, a contribution byte for byte against tests/ptau_format.py, a chain of two, every refusal of the
verifier with its reason, and the command line over a chain."""
import hashlib
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

ENTROPY_1 = bytes(range(32))
ENTROPY_2 = bytes(range(100, 132))
LOG = 3


@pytest.fixture(scope="module")
def ctx():
    import spp
    c = spp.Context(0)
    yield c
    c.close()


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def special_scalars():
    from oracle.bn254 import R
    return [1, 2, 3, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, 1 << 253, (1 << 253) - 1, 15, 16, 17]


# --------------------------------------------------------------------------------------------------------------------------
# 1. a scalar per point, both groups
# --------------------------------------------------------------------------------------------------------------------------
N_MAX = 200


class Group:
    def __init__(self, name):
        from oracle import bn254 as O
        self.name = name
        g1 = name == "g1"
        self.gen, self.size = (O.G1_GEN, 64) if g1 else (O.G2_GEN, 128)
        self.add, self.mul, self.neg = (O.g1_add, O.g1_mul, O.g1_neg) if g1 else (O.g2_add, O.g2_mul, O.g2_neg)
        self.to_bytes = O.g1_to_bytes if g1 else O.g2_to_bytes

    def call(self, ctx):
        return ctx.g1_mul_each if self.name == "g1" else ctx.g2_mul_each


@pytest.fixture(scope="module", params=["g1", "g2"])
def each_case(request):
    """200 points of the progression P_0 + i Q with a scalar each: the special scalars at the even indices, random ones at the
    odd; an equal pair at (2, 3) whose scalars differ, an opposite pair at (4, 5), infinity at 7; the products, computed once.
    A list of n points is the first n of these, so every n of the test shares them."""
    from oracle import bn254 as O
    G = Group(request.param)
    rng = random.Random(78)
    p0, q = (G.mul(G.gen, rng.randrange(1, O.R)) for _ in range(2))
    pts = [p0]
    for _ in range(N_MAX - 1):
        pts.append(G.add(pts[-1], q))
    assert pts[9] == G.add(p0, G.mul(q, 9))                     # the progression against a direct product
    special = special_scalars()
    scalars = [special[(i // 2) % len(special)] if i % 2 == 0 else rng.randrange(1, O.R) for i in range(N_MAX)]
    pts[3] = pts[2]
    pts[5] = G.neg(pts[4])
    pts[7] = None
    assert scalars[2] != scalars[3]
    want = [None if p is None else G.mul(p, k) for p, k in zip(pts, scalars)]
    return G, pts, scalars, want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_mul_each_against_the_oracle(ctx, each_case, n):
    G, pts, scalars, want = each_case
    got = G.call(ctx)(b"".join(G.to_bytes(p) for p in pts[:n]), scalars[:n])
    for i in range(n):
        assert got[G.size * i:G.size * (i + 1)] == G.to_bytes(want[i]), "%s point %d of %d, scalar %x" % (G.name, i, n, scalars[i])


def test_mul_each_takes_every_special_scalar_on_one_point(ctx, each_case):
    """the same point in every lane, so that only the lanes' scalars differ inside the wave"""
    G, pts, _, _ = each_case
    ks = special_scalars()
    got = G.call(ctx)(G.to_bytes(pts[11]) * len(ks), ks)
    assert got == b"".join(G.to_bytes(G.mul(pts[11], k)) for k in ks)


def test_mul_each_refuses_zero_r_and_what_is_no_point(ctx, each_case):
    import spp
    from oracle import bn254 as O
    from spp import lib
    G = each_case[0]
    g = G.to_bytes(G.gen)
    call = G.call(ctx)
    for k in (0, O.R, O.R + 5, (1 << 256) - 1):
        with pytest.raises(spp.SppError) as e:
            call(g * 3, [5, k, 7])
        assert e.value.code == lib.SPP_ERR_BAD_INPUT, k
    last = int.from_bytes(g[-32:], "big")
    off_curve = g[:-32] + O.fe_be((last + 1) % O.P)                # the generator with its last coordinate + 1
    above_q = O.fe_be(int.from_bytes(g[:32], "big") + O.P) + g[32:]  # ... with its first coordinate + q
    for bad in (off_curve, above_q):
        with pytest.raises(spp.SppError) as e:
            call(g + bad, [5, 6])
        assert e.value.code == lib.SPP_ERR_BAD_INPUT
    assert call(b"", []) == b""                                    # n = 0


# --------------------------------------------------------------------------------------------------------------------------
# 3. a contribution, every byte; a chain of two
# --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain(ctx, tmp_path_factory):
    """t0 (new) -> (ENTROPY_1) t1 -> (ENTROPY_2) t2, and t0 -> (ENTROPY_2) tB"""
    tmp = tmp_path_factory.mktemp("ptau")
    t0, t1, t2, tB = (str(tmp / (name + ".ptau")) for name in ("t0", "t1", "t2", "tB"))
    ctx.ptau_new(LOG, t0)
    r1 = ctx.ptau_contribute(t0, t1, ENTROPY_1)
    r2 = ctx.ptau_contribute(t1, t2, ENTROPY_2)
    rB = ctx.ptau_contribute(t0, tB, ENTROPY_2)
    return dict(tmp=tmp, t0=t0, t1=t1, t2=t2, tB=tB, r1=r1, r2=r2, rB=rB)


def test_new_transcript_is_all_generators(chain):
    import ptau_format as F
    assert _read(chain["t0"]) == F.new(LOG)
    assert len(_read(chain["t0"])) == 12 + 64 * 15 + 128 * 8 + 64 * 8 + 64 * 8 + 128


def test_new_transcript_refuses_sizes_out_of_range(ctx, tmp_path):
    import spp
    from spp import lib
    for log in (0, 21):
        with pytest.raises(spp.SppError) as e:
            ctx.ptau_new(log, str(tmp_path / "bad.ptau"))
        assert e.value.code == lib.SPP_ERR_BAD_INPUT


def test_contribution_every_byte(ctx, chain):
    import ptau_format as F
    from spp import lib
    c = chain
    s = F.contribution_secrets(ENTROPY_1)
    want = F.contributed(_read(c["t0"]), *s[:3])
    assert _read(c["t1"]) == want
    assert want == F.transcript(LOG, *s[:3])                     # on the transcript of 1, 1, 1 a contribution IS the transcript of t, a, b
    assert c["r1"] == F.receipt(_read(c["t0"]), want, s)
    assert F.receipt_holds(_read(c["t0"]), want, c["r1"])
    again = str(c["tmp"] / "t1_again.ptau")                      # the same entropy again: the same bytes
    assert ctx.ptau_contribute(c["t0"], again, ENTROPY_1) == c["r1"] and _read(again) == want
    assert ctx.ptau_verify_contribution(c["t0"], c["t1"], c["r1"]) == (True, lib.SPP_PTAU_OK)


def test_chain_of_two_contributions(ctx, chain):
    import ptau_format as F
    from oracle import bn254 as O
    from spp import lib
    c = chain
    s1, s2 = F.contribution_secrets(ENTROPY_1), F.contribution_secrets(ENTROPY_2)
    assert _read(c["t2"]) == F.transcript(LOG, *(x * y % O.R for x, y in zip(s1[:3], s2[:3])))
    assert c["r2"] == F.receipt(_read(c["t1"]), _read(c["t2"]), s2)
    assert ctx.ptau_verify_contribution(c["t0"], c["t1"], c["r1"]) == (True, lib.SPP_PTAU_OK)
    assert ctx.ptau_verify_contribution(c["t1"], c["t2"], c["r2"]) == (True, lib.SPP_PTAU_OK)
    # link 2 presented against transcript 0: its proofs of knowledge are about other bases and another file
    assert ctx.ptau_verify_contribution(c["t0"], c["t2"], c["r2"]) == (False, lib.SPP_PTAU_RECEIPT)


# --------------------------------------------------------------------------------------------------------------------------
# 4. every refusal with its reason
# --------------------------------------------------------------------------------------------------------------------------
def _refusals():
    import ptau_format as F
    return F.REFUSALS


@pytest.mark.parametrize("case", _refusals())
def test_refusals_name_their_reason(ctx, chain, case):
    import ptau_format as F
    from spp import lib
    c = chain
    data, receipt, want = F.tampered(case, _read(c["t0"]), _read(c["t1"]), c["r1"], _read(c["tB"]))
    path = str(c["tmp"] / (case + ".ptau"))
    with open(path, "wb") as f:
        f.write(data)
    # a refusal is a result of the call, never a library error (which would raise)
    got = ctx.ptau_verify_contribution(c["t0"], path, receipt)
    assert got == (False, lib.PTAU_REASON_NAMES.index(want)), "%s: %s" % (case, lib.PTAU_REASON_NAMES[got[1]])


def test_untampered_files_pass_the_same_path(ctx, chain):
    """the rewrite through tests/ptau_format.py that the refusals use changes nothing by itself"""
    import ptau_format as F
    from spp import lib
    c = chain
    path = str(c["tmp"] / "rewritten.ptau")
    with open(path, "wb") as f:
        f.write(F.Ptau(_read(c["t1"])).to_bytes())
    assert _read(path) == _read(c["t1"])
    assert ctx.ptau_verify_contribution(c["t0"], path, c["r1"]) == (True, lib.SPP_PTAU_OK)


def test_contribution_refuses_a_transcript_that_holds_no_points(ctx, chain):
    """the contributor checks what it multiplies: an off-curve G1 point, a G2 point outside the subgroup, infinity"""
    import ptau_format as F
    import spp
    from spp import lib
    c = chain
    for case in ("t1_point_off_curve", "t2_point_off_subgroup", "truncated"):
        data, _, _ = F.tampered(case, _read(c["t0"]), _read(c["t1"]), c["r1"], _read(c["tB"]))
        path = str(c["tmp"] / ("in_" + case + ".ptau"))
        with open(path, "wb") as f:
            f.write(data)
        with pytest.raises(spp.SppError) as e:
            ctx.ptau_contribute(path, str(c["tmp"] / "never.ptau"), ENTROPY_2)
        assert e.value.code == lib.SPP_ERR_FORMAT, case
    assert not os.path.exists(str(c["tmp"] / "never.ptau"))


# --------------------------------------------------------------------------------------------------------------------------
# 8. the command line
# --------------------------------------------------------------------------------------------------------------------------
def test_command_line_chain_and_the_link_it_names(chain, capsys):
    """ptau-new, ptau-contribute twice and ptau-verify over the chain; then link 2 with an A1 point doubled: exit 1, the link and
    the reason"""
    import ptau_format as F
    from oracle import bn254 as O
    from spp import cli
    c = chain
    t0 = str(c["tmp"] / "cli" / "t.ptau")
    os.makedirs(os.path.dirname(t0))
    out1, out2 = str(c["tmp"] / "cli1"), str(c["tmp"] / "cli2")
    assert cli.main(["ptau-new", str(LOG), "--out", t0]) == 0
    assert _read(t0) == _read(c["t0"])
    capsys.readouterr()
    assert cli.main(["ptau-contribute", t0, "--out", out1, "--entropy", ENTROPY_1.hex()]) == 0
    first = capsys.readouterr().out
    k1 = [os.path.join(out1, "t" + e) for e in (".ptau", ".receipt")]
    assert _read(k1[0]) == _read(c["t1"]) and _read(k1[1]) == c["r1"]
    assert hashlib.sha256(c["r1"]).hexdigest() in first
    assert cli.main(["ptau-contribute", k1[0], "--out", out2, "--entropy", ENTROPY_2.hex()]) == 0
    k2 = [os.path.join(out2, "t" + e) for e in (".ptau", ".receipt")]
    capsys.readouterr()
    assert cli.main(["ptau-verify", t0] + k1 + k2) == 0
    assert "2 links verified" in capsys.readouterr().out
    p = F.Ptau(_read(k2[0]))
    p.A1[1] = O.g1_to_bytes(O.g1_mul(O.g1_from_bytes(p.A1[1]), 2))
    with open(k2[0], "wb") as f:
        f.write(p.to_bytes())
    assert cli.main(["ptau-verify", t0] + k1 + k2) == 1
    said = capsys.readouterr().out
    assert "link 1" in said and "link 2" in said and "REFUSED, ALPHA" in said and "links verified" not in said
    assert cli.main(["ptau-new", "0", "--out", t0]) == 2 and cli.main(["ptau-verify", t0, k1[0]]) == 2
