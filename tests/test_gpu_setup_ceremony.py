"""The setup ceremony on the GPU: the scaling kernel through its unit entry point, contributions on synthetic circuits byte for
byte against oracle/bn254.py big integers, a chain of two, the withdraw circuit proved under a contributed key, and every refusal
of the verifier with its reason.  Keys come from the oracle's CPU setup; tests/sppk_format.py restates the two file layouts."""
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


@pytest.fixture(scope="module")
def ctx():
    import spp
    c = spp.Context(0)
    yield c
    c.close()


def special_scalars():
    from oracle.bn254 import R
    return [1, 2, 3, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, 1 << 253, (1 << 253) - 1, 15, 16, 17]


# --------------------------------------------------------------------------------------------------------------------------
# 1. the unit entry point
# --------------------------------------------------------------------------------------------------------------------------
N_MAX = 200


@pytest.fixture(scope="module")
def progression():
    """200 distinct points P_i = P_0 + i Q, so that k P_i = k P_0 + i (k Q) costs one addition of big integers per point, and the
    products for every special scalar, computed once"""
    from oracle import bn254 as O
    rng = random.Random(77)
    p0, q = (O.g1_mul(O.G1_GEN, rng.randrange(1, O.R)) for _ in range(2))
    pts = [p0]
    for _ in range(N_MAX - 1):
        pts.append(O.g1_add(pts[-1], q))
    scaled = {}
    for k in special_scalars():
        kq, row = O.g1_mul(q, k), [O.g1_mul(p0, k)]
        for _ in range(N_MAX - 1):
            row.append(O.g1_add(row[-1], kq))
        scaled[k] = row
    assert scaled[3][7] == O.g1_mul(pts[7], 3)          # the progression against a direct product
    return pts, scaled


def _point_list(n, pts, scaled_row):
    """n points and their products: infinity at index 0 and at the last index, an equal pair at (2, 3), an opposite pair at (4, 5)"""
    from oracle import bn254 as O
    p, want = list(pts[:n]), list(scaled_row[:n])
    if n > 6:
        p[3], want[3] = p[2], want[2]
        p[5], want[5] = O.g1_neg(p[4]), O.g1_neg(want[4])
    p[0] = want[0] = None
    p[n - 1] = want[n - 1] = None
    return p, want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_scale_points_against_the_oracle(ctx, progression, n):
    from oracle import bn254 as O
    pts, scaled = progression
    for k in special_scalars():
        p, want = _point_list(n, pts, scaled[k])
        got = ctx.g1_scale_points(b"".join(O.g1_to_bytes(x) for x in p), k)
        assert got == b"".join(O.g1_to_bytes(x) for x in want), "n %d scalar %x" % (n, k)


def test_scale_points_refuses_zero_r_and_what_is_no_point(ctx):
    import spp
    from oracle import bn254 as O
    from spp import lib
    g = O.g1_to_bytes(O.G1_GEN)
    for k in (0, O.R, O.R + 5, (1 << 256) - 1):
        with pytest.raises(spp.SppError) as e:
            ctx.g1_scale_points(g * 3, k)
        assert e.value.code == lib.SPP_ERR_BAD_INPUT, k
    with pytest.raises(spp.SppError) as e:
        ctx.g1_scale_points(g + O.fe_be(1) + O.fe_be(3), 5)              # (1, 3) is not on the curve
    assert e.value.code == lib.SPP_ERR_BAD_INPUT
    with pytest.raises(spp.SppError) as e:
        ctx.g1_scale_points(O.fe_be(1 + O.P) + O.fe_be(2), 5)            # the generator with x + q
    assert e.value.code == lib.SPP_ERR_BAD_INPUT
    assert ctx.g1_scale_points(b"", 5) == b""                            # n = 0


# --------------------------------------------------------------------------------------------------------------------------
# 2., 3. one contribution, every byte
# --------------------------------------------------------------------------------------------------------------------------
def _synthetic_key(tmp, gen, seed):
    import synth_circuits as S
    from oracle import native
    sppc, pk, vk = (str(tmp / ("k0." + e)) for e in ("sppc", "pk", "vk"))
    S.write_sppc(gen.desc, sppc)
    native.setup(sppc, seed, pk, vk)
    return sppc, pk, vk


def _contribute(ctx, tmp, pk, vk, entropy, tag):
    pk_out, vk_out = str(tmp / (tag + ".pk")), str(tmp / (tag + ".vk"))
    receipt = ctx.setup_contribute(pk, vk, pk_out, vk_out, entropy)
    return pk_out, vk_out, receipt


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _check_contribution(ctx, tmp, pk, vk, want_kz):
    """contributes with ENTROPY_1 and compares pk_out, vk_out and the receipt with what big integers give"""
    import sppk_format as F
    from oracle import bn254 as O
    from spp import lib
    key = F.Sppk(_read(pk))
    assert len(key.points["K"]) + len(key.points["Z"]) == want_kz
    d, k = F.contribution_secrets(ENTROPY_1)
    want_pk, want_vk = F.contributed(_read(pk), _read(vk), d)
    pk1, vk1, receipt = _contribute(ctx, tmp, pk, vk, ENTROPY_1, "k1")
    assert _read(pk1) == want_pk
    assert _read(vk1) == want_vk
    # the receipt: delta1', T = k delta1, z = k + c d, and the equation the verifier checks
    delta1 = O.g1_from_bytes(key.delta1)
    T = O.g1_to_bytes(O.g1_mul(delta1, k))
    c, = O.hash_to_fr(hashlib.sha256(_read(pk)).digest() + key.delta1 + F.Sppk(want_pk).delta1 + T, b"spp-groth16-contribute-c1", 1)
    assert receipt == F.Sppk(want_pk).delta1 + T + ((k + c * d) % O.R).to_bytes(32, "big")
    assert F.receipt_holds(_read(pk), receipt)
    # the same entropy again: the same three outputs
    pk1b, vk1b, receipt_b = _contribute(ctx, tmp, pk, vk, ENTROPY_1, "k1_again")
    assert (_read(pk1b), _read(vk1b), receipt_b) == (want_pk, want_vk, receipt)
    assert ctx.setup_verify_contribution(pk, vk, pk1, vk1, receipt) == (True, lib.SPP_CONTRIB_OK)
    return pk1, vk1, receipt


def test_contribution_on_the_tiny_circuit(ctx, tmp_path):
    import synth_circuits as S
    g = S.gen_tiny()
    assert g.expect["domain_log"] == 3
    _, pk, vk = _synthetic_key(tmp_path, g, b"\x05" * 32)
    _check_contribution(ctx, tmp_path, pk, vk, 4 + 7)


def test_contribution_over_several_waves_and_a_ragged_tail(ctx, tmp_path):
    import synth_circuits as S
    _, pk, vk = _synthetic_key(tmp_path, S.gen_div(20), b"\x06" * 32)
    _check_contribution(ctx, tmp_path, pk, vk, 164)                      # 101 K + 63 Z points: two waves and 36 lanes


# --------------------------------------------------------------------------------------------------------------------------
# 4. a chain, and 6. the refusals
# --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_chain(ctx, tmp_path_factory):
    """pk0 -> (ENTROPY_1) pk1 -> (ENTROPY_2) pk2, and pk0 -> (ENTROPY_2) pkB"""
    import synth_circuits as S
    tmp = tmp_path_factory.mktemp("chain")
    _, pk0, vk0 = _synthetic_key(tmp, S.gen_tiny(), b"\x05" * 32)
    pk1, vk1, r1 = _contribute(ctx, tmp, pk0, vk0, ENTROPY_1, "k1")
    pk2, vk2, r2 = _contribute(ctx, tmp, pk1, vk1, ENTROPY_2, "k2")
    pkB, vkB, rB = _contribute(ctx, tmp, pk0, vk0, ENTROPY_2, "kB")
    return dict(tmp=tmp, pk0=pk0, vk0=vk0, pk1=pk1, vk1=vk1, r1=r1, pk2=pk2, vk2=vk2, r2=r2, pkB=pkB, vkB=vkB, rB=rB)


def test_chain_of_two_contributions(ctx, tiny_chain):
    import sppk_format as F
    from oracle import bn254 as O
    from spp import lib
    c = tiny_chain
    d1, _ = F.contribution_secrets(ENTROPY_1)
    d2, _ = F.contribution_secrets(ENTROPY_2)
    first, last = F.Sppk(_read(c["pk0"])), F.Sppk(_read(c["pk2"]))
    inv = pow(d1 * d2, -1, O.R)
    for name in ("K", "Z"):
        assert last.points[name] == [O.g1_to_bytes(O.g1_mul(O.g1_from_bytes(p), inv)) for p in first.points[name]]
    assert last.delta1 == O.g1_to_bytes(O.g1_mul(O.g1_from_bytes(first.delta1), d1 * d2))
    assert ctx.setup_verify_contribution(c["pk0"], c["vk0"], c["pk1"], c["vk1"], c["r1"]) == (True, lib.SPP_CONTRIB_OK)
    assert ctx.setup_verify_contribution(c["pk1"], c["vk1"], c["pk2"], c["vk2"], c["r2"]) == (True, lib.SPP_CONTRIB_OK)
    ok, reason = ctx.setup_verify_contribution(c["pk0"], c["vk0"], c["pk2"], c["vk2"], c["r2"])      # link 2 against the wrong key before
    assert not ok and reason in (lib.SPP_CONTRIB_SCALING, lib.SPP_CONTRIB_RECEIPT)


REFUSALS = ["k_point_replaced", "k_points_swapped", "z_point_other_scalar", "k_point_off_curve", "a_section_byte", "index_list", "delta2_of_another",
            "z_plus_one", "t_replaced", "vk_gamma2", "vk_delta2_old", "truncated"]


@pytest.mark.parametrize("case", REFUSALS)
def test_refusals_name_their_reason(ctx, tiny_chain, case):
    import sppk_format as F
    from oracle import bn254 as O
    from spp import lib
    c = tiny_chain
    pk, vk, receipt = F.Sppk(_read(c["pk1"])), F.Vk(_read(c["vk1"])), c["r1"]
    pk_bytes = None
    other = O.g1_to_bytes(O.g1_mul(O.G1_GEN, 12345))
    if case == "k_point_replaced":
        pk.points["K"][1], want = other, lib.SPP_CONTRIB_SCALING
    elif case == "k_points_swapped":
        pk.points["K"][0], pk.points["K"][2] = pk.points["K"][2], pk.points["K"][0]
        want = lib.SPP_CONTRIB_SCALING
    elif case == "z_point_other_scalar":
        pk.points["Z"][3], want = O.g1_to_bytes(O.g1_mul(O.g1_from_bytes(pk.points["Z"][3]), 2)), lib.SPP_CONTRIB_SCALING
    elif case == "k_point_off_curve":
        x, y = O.g1_from_bytes(pk.points["K"][3])
        pk.points["K"][3], want = O.g1_to_bytes((x, (y + 1) % O.P)), lib.SPP_CONTRIB_POINT_INVALID
    elif case == "a_section_byte":
        pk.points["A"][0], want = pk.points["A"][0][:-1] + bytes([pk.points["A"][0][-1] ^ 1]), lib.SPP_CONTRIB_NOT_A_DELTA_CHANGE
    elif case == "index_list":
        pk.wires["K"][0] += 1
        want = lib.SPP_CONTRIB_NOT_A_DELTA_CHANGE
    elif case == "delta2_of_another":
        pk.delta2, want = F.Sppk(_read(c["pkB"])).delta2, lib.SPP_CONTRIB_DELTA_PAIR
        vk.delta2 = pk.delta2
    elif case == "z_plus_one":
        z = (int.from_bytes(receipt[128:], "big") + 1) % O.R
        receipt, want = receipt[:128] + z.to_bytes(32, "big"), lib.SPP_CONTRIB_RECEIPT
    elif case == "t_replaced":
        receipt, want = receipt[:64] + other + receipt[128:], lib.SPP_CONTRIB_RECEIPT
    elif case == "vk_gamma2":
        vk.gamma2, want = O.g2_to_bytes(O.g2_mul(O.G2_GEN, 9)), lib.SPP_CONTRIB_VK
    elif case == "vk_delta2_old":
        vk.delta2, want = F.Vk(_read(c["vk0"])).delta2, lib.SPP_CONTRIB_VK
    else:
        pk_bytes, want = pk.to_bytes()[:-10], lib.SPP_CONTRIB_FORMAT
    pk_t, vk_t = str(c["tmp"] / (case + ".pk")), str(c["tmp"] / (case + ".vk"))
    with open(pk_t, "wb") as f:
        f.write(pk.to_bytes() if pk_bytes is None else pk_bytes)
    with open(vk_t, "wb") as f:
        f.write(vk.to_bytes())
    # a refusal is a result of the call, never a library error (which would raise)
    got = ctx.setup_verify_contribution(c["pk0"], c["vk0"], pk_t, vk_t, receipt)
    assert got == (False, want), "%s: %s" % (case, lib.CONTRIB_REASON_NAMES[got[1]])


def test_untampered_files_pass_the_same_path(ctx, tiny_chain):
    """the rewrite through tests/sppk_format.py that the refusals use changes nothing by itself"""
    import sppk_format as F
    from spp import lib
    c = tiny_chain
    assert F.Sppk(_read(c["pk1"])).to_bytes() == _read(c["pk1"]) and F.Vk(_read(c["vk1"])).to_bytes() == _read(c["vk1"])
    assert ctx.setup_verify_contribution(c["pk0"], c["vk0"], c["pk1"], c["vk1"], c["r1"]) == (True, lib.SPP_CONTRIB_OK)


def test_command_line_chain_and_the_link_it_names(tiny_chain, capsys):
    """setup-contribute twice and setup-verify over the chain; then link 2 with a Z point doubled: exit 1, the link and the reason"""
    import sppk_format as F
    from oracle import bn254 as O
    from spp import cli
    c = tiny_chain
    out1, out2 = str(c["tmp"] / "cli1"), str(c["tmp"] / "cli2")
    assert cli.main(["setup-contribute", c["pk0"], c["vk0"], "--out", out1, "--entropy", ENTROPY_1.hex()]) == 0
    first = capsys.readouterr().out
    k1 = [os.path.join(out1, "k0" + e) for e in (".pk", ".vk", ".receipt")]
    assert _read(k1[0]) == _read(c["pk1"]) and _read(k1[1]) == _read(c["vk1"]) and _read(k1[2]) == c["r1"]
    assert hashlib.sha256(c["r1"]).hexdigest() in first
    assert cli.main(["setup-contribute", k1[0], k1[1], "--out", out2, "--entropy", ENTROPY_2.hex()]) == 0
    k2 = [os.path.join(out2, "k0" + e) for e in (".pk", ".vk", ".receipt")]
    capsys.readouterr()
    assert cli.main(["setup-verify", c["pk0"], c["vk0"]] + k1 + k2) == 0
    assert "2 links verified" in capsys.readouterr().out
    key = F.Sppk(_read(k2[0]))
    key.points["Z"][0] = O.g1_to_bytes(O.g1_mul(O.g1_from_bytes(key.points["Z"][0]), 2))
    with open(k2[0], "wb") as f:
        f.write(key.to_bytes())
    assert cli.main(["setup-verify", c["pk0"], c["vk0"]] + k1 + k2) == 1
    said = capsys.readouterr().out
    assert "link 1" in said and "link 2" in said and "REFUSED, SCALING" in said and "links verified" not in said


# --------------------------------------------------------------------------------------------------------------------------
# 5. the withdraw circuit under a contributed key
# --------------------------------------------------------------------------------------------------------------------------
def _another_note(seed):
    """withdraw inputs of a note that is not the reference KAT (client/merkle.ts semantics from oracle/hashes.py)"""
    from oracle import hashes as H
    rng = random.Random(seed)
    tree = H.MerkleTree()
    sk, amount, rnd = rng.randrange(1, 1 << 128), rng.randrange(1, 1 << 40), rng.randrange(1 << 250)
    for _ in range(3):
        tree.insert(rng.randrange(1 << 250))
    owner = H.fixed_base_scalar_mul(sk)
    idx = tree.insert(H.poseidon_hash4(owner[0], owner[1], amount, rnd))
    tree.insert(rng.randrange(1 << 250))
    return [tree.root(), H.poseidon_hash2(sk, idx), rng.randrange(1, 1 << 240), amount, H.poseidon_hash2(owner[0], owner[1]),
            sk, owner[0], owner[1], rnd, idx] + tree.proof(idx)


def test_withdraw_circuit_under_a_contributed_key(ctx, withdraw_artifacts, withdraw_kat, tmp_path):
    import spp
    from oracle import native, circuit as C
    from spp import lib
    a = withdraw_artifacts
    pk1, vk1, receipt = _contribute(ctx, tmp_path, a["pk"], a["vk"], ENTROPY_1, "withdraw1")
    assert ctx.setup_verify_contribution(a["pk"], a["vk"], pk1, vk1, receipt) == (True, lib.SPP_CONTRIB_OK)
    rows, rs = [C.withdraw_inputs(withdraw_kat), _another_note(31)], [(3, 4), (5, 6)]
    h = ctx.load_circuit(a["sppc"], pk1, 6)                              # the contributed key through the existing loader
    try:
        proofs, pws, status = h.prove_batch(rows, rs)
    finally:
        h.close()
    assert status == [0, 0]
    orc = native.Prover(a["sppc"], pk1)
    vk_new, vk_old = _read(vk1), _read(a["vk"])
    for row, (r, s), proof, pw in zip(rows, rs, proofs, pws):
        rc, want_proof, want_pw = orc.prove(row, r, s)
        assert rc == 0 and proof == want_proof and pw == want_pw
        assert spp.verify(vk_new, proof, pw)
        assert not spp.verify(vk_old, proof, pw)
