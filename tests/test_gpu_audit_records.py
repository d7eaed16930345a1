"""GPU: audit records end to end on the device -- secrets -> (proof, public witness, ciphertext) -> verified, bound, decrypted
identity (spp_prove_audit_records(_device), spp_audit_open_batch) -- against the CPU oracle, over the reference's public key
(tests/golden/rlwe_pk.json) and its matching secret key (tests/golden/rlwe_decrypt.json)."""
import ctypes
import json
import os
import random

import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

B_ = 70
FIRST = 500
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
Q = 167772161
DELTA = Q // 256
BAD_PROOF, BAD_CT, BAD_ID = 1, 2, 4


@pytest.fixture(scope="module")
def ctx():
    import spp
    c = spp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def decrypt_fixture():
    return json.load(open(os.path.join(GOLDEN, "rlwe_decrypt.json")))


@pytest.fixture(scope="module")
def sk_mod_q(ctx, decrypt_fixture):
    """the auditors' key, reconstructed on the device from shares 1 + 2 of the fixture"""
    from spp import witness
    sk = witness.reconstruct_sk(ctx, decrypt_fixture["shares"])
    assert sk == decrypt_fixture["sk_mod_q"]
    return sk


def _oracle_row(rlwe_pk, i):
    from oracle import rlwe
    return rlwe.audit_inputs(rlwe_pk["a"], rlwe_pk["b"], 12345 + FIRST + i, random.Random(1000 + FIRST + i))


@pytest.fixture(scope="module")
def records(ctx, audit_artifacts, rlwe_pk):
    """70 records from workload.audit_noise: the device call twice (two calls in flight), the proofs-only call on the same inputs
    and blinding, and the host form."""
    import numpy as np
    from spp import workload
    dev = torch.device("cuda", 0)
    sks, r8, e18, e28 = workload.audit_noise(FIRST, B_)
    up = lambda raw: torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    d_a, d_b = up(np.asarray(rlwe_pk["a"], dtype=np.uint32).tobytes()), up(np.asarray(rlwe_pk["b"], dtype=np.uint32).tobytes())
    d_sk = up(b"".join(int(v).to_bytes(32, "big") for v in sks))
    d_r, d_e1, d_e2 = up(r8.tobytes()), up(e18.tobytes()), up(e28.tobytes())
    rs_vals = [(101 * i + 7, 103 * i + 9) for i in range(B_)]
    d_rs = up(b"".join(r.to_bytes(32, "big") + s.to_bytes(32, "big") for r, s in rs_vals))
    h = ctx.load_circuit(audit_artifacts["sppc"], audit_artifacts["pk"], 6)
    try:
        def outs(with_ct):
            o = [torch.zeros(388 * B_, dtype=torch.uint8, device=dev), torch.zeros(76 * B_, dtype=torch.uint8, device=dev),
                 torch.ones(B_, dtype=torch.int32, device=dev)]
            if with_ct:
                o += [torch.full((B_, 64), 0xFFFFFFFF, dtype=torch.int64, device=dev).to(torch.int32),
                      torch.full((B_, 1024), 0xFFFFFFFF, dtype=torch.int64, device=dev).to(torch.int32)]
            return o
        rec = [outs(True), outs(True)]
        plain = outs(False)
        ins = (d_a.data_ptr(), d_b.data_ptr(), d_sk.data_ptr(), d_r.data_ptr(), d_e1.data_ptr(), d_e2.data_ptr(), d_rs.data_ptr())
        for o in rec:                                                   # two calls in flight
            h.prove_audit_records_device(B_, *ins, *[t.data_ptr() for t in o])
        h.prove_audit_from_secrets_device(B_, *ins, *[t.data_ptr() for t in plain])
        h.sync()
        dl = lambda t: t.cpu().numpy()
        device = [dict(proofs=bytes(dl(o[0])), pws=bytes(dl(o[1])), status=dl(o[2]).tolist(),
                       c0=dl(o[3]).view(np.uint32), c1=dl(o[4]).view(np.uint32)) for o in rec]
        plain = dict(proofs=bytes(dl(plain[0])), pws=bytes(dl(plain[1])), status=dl(plain[2]).tolist())
        host = h.prove_audit_records(rlwe_pk["a"], rlwe_pk["b"], sks, r8, e18, e28, rs_vals)
        # one row with sk = 0 (no identity key: the circuit's fixed-base multiplication refuses it; every int8 noise value is
        # inside the circuit's range table, so the noise cannot be out of range through this interface): refused in place,
        # its ciphertext still returned
        sks_bad = list(sks[:6])
        sks_bad[2] = 0
        refused = h.prove_audit_records(rlwe_pk["a"], rlwe_pk["b"], sks_bad, r8[:6], e18[:6], e28[:6], rs_vals[:6])
    finally:
        h.close()
    return dict(device=device, plain=plain, host=host, refused=refused, refused_in=(sks_bad, r8[:6], e18[:6], e28[:6]), rs=rs_vals, sks=sks,
                vk=open(audit_artifacts["vk"], "rb").read())


def _split(buf, n):
    return [buf[n * i:n * (i + 1)] for i in range(len(buf) // n)]


def test_records_are_the_from_secrets_proofs_plus_the_oracles_ciphertext(records, audit_artifacts, rlwe_pk):
    from oracle import native
    a, b = records["device"]
    assert a["status"] == [0] * B_ == b["status"] == records["plain"]["status"]
    assert a["proofs"] == b["proofs"] and a["pws"] == b["pws"] and (a["c0"] == b["c0"]).all() and (a["c1"] == b["c1"]).all()
    # the existing call, same inputs and blinding: the same bytes
    assert a["proofs"] == records["plain"]["proofs"] and a["pws"] == records["plain"]["pws"]
    orc = native.Prover(audit_artifacts["sppc"], audit_artifacts["pk"])
    for i in (0, 33, 64, B_ - 1):
        d = _oracle_row(rlwe_pk, i)
        from oracle import rlwe
        rc, proof, pw = orc.prove(rlwe.audit_input_vector(d), *records["rs"][i])
        assert rc == 0 and a["proofs"][388 * i:388 * (i + 1)] == proof and a["pws"][76 * i:76 * (i + 1)] == pw, i
        assert a["c0"][i].tolist() == d["c0"] and a["c1"][i].tolist() == d["c1"], i
    assert int(a["c0"].max()) < Q and int(a["c1"].max()) < Q
    # the host form: the same bytes
    proofs, pws, status, c0, c1 = records["host"]
    assert status == [0] * B_ and b"".join(proofs) == a["proofs"] and b"".join(pws) == a["pws"]
    assert (c0 == a["c0"]).all() and (c1 == a["c1"]).all()


def test_refused_rows_keep_their_place_and_their_ciphertext(records, rlwe_pk):
    import numpy as np
    from oracle import rlwe, hashes as H
    proofs, pws, status, c0, c1 = records["refused"]
    assert [i for i in range(6) if status[i] != 0] == [2] and status[2] == -4
    assert proofs[2] == bytes(388)
    good = records["device"][0]
    for i in (0, 1, 3, 4, 5):
        assert proofs[i] == good["proofs"][388 * i:388 * (i + 1)] and pws[i] == good["pws"][76 * i:76 * (i + 1)]
        assert (c0[i] == good["c0"][i]).all() and (c1[i] == good["c1"][i]).all()
    # row 2 (sk = 0) has a ciphertext too: c1 does not depend on the message, c0 was written (coefficients below q, not all alike)
    sks, r8, e18, e28 = records["refused_in"]
    _, e1_2, _, _ = rlwe.rlwe_witness(rlwe_pk["a"], rlwe_pk["b"], r8[2].tolist(), e18[2].tolist(), e28[2].tolist(), [0] * 64)
    assert c1[2].tolist() == e1_2 and int(np.max(c0[2])) < Q and len(set(c0[2].tolist())) > 32


def test_round_trip_every_record_opens_to_its_owner(ctx, records, sk_mod_q):
    from oracle import hashes as H
    a = records["device"][0]
    owners, flags = ctx.audit_open(records["vk"], sk_mod_q, a["proofs"], a["pws"], a["c0"], a["c1"])
    print("flags:", flags)
    assert flags == [0] * B_                       # noise <= 3 -> about 2e4 against Delta / 2 = 3.3e5: no row may be left out
    assert owners == [H.fixed_base_scalar_mul(sk) for sk in records["sks"]]
    owners2, flags2 = ctx.audit_open(None, sk_mod_q, None, a["pws"], a["c0"], a["c1"])      # already verified elsewhere
    assert flags2 == [0] * B_ and owners2 == owners


def _oracle_flags(sk, pw, c0, c1):
    """bits 2 and 4 by the oracle's own computation"""
    from oracle import rlwe, hashes as H
    c0, c1 = [int(v) for v in c0], [int(v) for v in c1]
    wa, ct = int.from_bytes(pw[12:44], "big"), int.from_bytes(pw[44:76], "big")
    f = 0
    if max(c0 + c1) >= Q or H.poseidon2_sponge(rlwe.pack_values([v % Q for v in c0]) + rlwe.pack_values([v % Q for v in c1])) != ct:
        f |= BAD_CT
    ox, oy = rlwe.decode_owner(rlwe.rlwe_decrypt(sk, c0, c1))
    if ox >= R or oy >= R or (oy * oy - ox * ox * ox + 17) % R != 0 or H.poseidon_hash2(ox, oy) != wa:
        f |= BAD_ID
    return f, (ox, oy)


def _pw(wa, ct):
    return (2).to_bytes(4, "big") + (0).to_bytes(4, "big") + (2).to_bytes(4, "big") + wa.to_bytes(32, "big") + ct.to_bytes(32, "big")


def test_decisions_each_against_the_oracle(ctx, records, sk_mod_q):
    import numpy as np
    from oracle import hashes as H
    a = records["device"][0]
    proofs, pws = _split(a["proofs"], 388), _split(a["pws"], 76)
    c0, c1 = a["c0"].copy(), a["c1"].copy()
    expect = {}
    c0[3, 5] = (int(c0[3, 5]) + DELTA) % Q;                         expect[3] = BAD_CT | BAD_ID       # one message byte + 1
    c0[[10, 11]] = c0[[11, 10]]; c1[[10, 11]] = c1[[11, 10]];        expect[10] = expect[11] = BAD_CT | BAD_ID   # two records' ciphertexts swapped
    c1[20, 777] = Q;                                                 expect[20] = None                 # a coefficient = q: bit 2, bit 4 as the oracle has it
    proofs[30] = proofs[30][:100] + bytes([proofs[30][100] ^ 1]) + proofs[30][101:]; expect[30] = BAD_PROOF
    pws[40] = pws[40][:12] + pws[41][12:44] + pws[40][44:];          expect[40] = BAD_PROOF | BAD_ID   # wa_commitment of another record
    owners, flags = ctx.audit_open(records["vk"], sk_mod_q, proofs, pws, c0, c1)
    print("flags:", flags)
    ok = ctx.verify_batch(records["vk"], proofs, pws)
    assert [f & BAD_PROOF for f in flags] == [0 if v else 1 for v in ok]           # bit 1 is the batched verifier's decision, on all rows
    assert [i for i in range(B_) if not ok[i]] == [30, 40]
    true_owner = [H.fixed_base_scalar_mul(sk) for sk in records["sks"]]
    for i in range(B_):
        want, who = _oracle_flags(sk_mod_q, pws[i], c0[i], c1[i]) if i in expect else (0, true_owner[i])
        assert flags[i] & (BAD_CT | BAD_ID) == want and owners[i] == who, i
        if expect.get(i) is not None:
            assert flags[i] == expect[i], i
        elif i not in expect:
            assert flags[i] == 0, i
    assert flags[20] & BAD_CT and not flags[20] & BAD_PROOF
    assert owners[30] == true_owner[30] and owners[10] == true_owner[11] and owners[11] == true_owner[10]


def test_identity_checks_without_a_verifying_key(ctx, sk_mod_q, rlwe_pk):
    """An oracle-made encryption of 64 x 0xFF (owner_x >= r) and of the point (1, 1) (below r, off the curve), each with a public
    witness built from the oracle's sponge -- and, for (1, 1), from the oracle's H(1, 1), so that only the curve check can refuse
    it."""
    from oracle import rlwe, hashes as H
    rng = random.Random(77)
    cts, pws = [], []
    for msg, wa in (([255] * 64, 0), (rlwe.owner_msg(1, 1), H.poseidon_hash2(1, 1))):
        r, e1, e2 = ([rng.randint(-3, 3) for _ in range(n)] for n in (1024, 64, 1024))
        c0, c1, _, _ = rlwe.rlwe_witness(rlwe_pk["a"], rlwe_pk["b"], r, e1, e2, msg)
        cts.append((c0, c1))
        pws.append(_pw(wa, H.poseidon2_sponge(rlwe.pack_values(c0) + rlwe.pack_values(c1))))
    owners, flags = ctx.audit_open(None, sk_mod_q, None, pws, [c[0] for c in cts], [c[1] for c in cts])
    print("flags:", flags)
    assert flags == [BAD_ID, BAD_ID]
    assert owners[0] == ((1 << 256) - 1, (1 << 256) - 1) and owners[1] == (1, 1)


def test_random_ciphertexts_under_an_arbitrary_key(ctx):
    """the 33 random ciphertexts of test_auditor_side_reconstruct_and_decrypt: the owners are the oracle's decryption, decoded;
    no such ciphertext hashes to the zero commitment"""
    import numpy as np
    from oracle import rlwe
    rng = np.random.default_rng(11)
    c0 = rng.integers(0, rlwe.RLWE_Q, size=(33, 64), dtype=np.uint32)
    c1 = rng.integers(0, rlwe.RLWE_Q, size=(33, 1024), dtype=np.uint32)
    skr = rng.integers(0, rlwe.RLWE_Q, size=1024, dtype=np.uint32)
    owners, flags = ctx.audit_open(None, skr, None, [bytes(76)] * 33, c0, c1)
    for i in range(33):
        assert owners[i] == rlwe.decode_owner(rlwe.rlwe_decrypt(skr.tolist(), c0[i].tolist(), c1[i].tolist())), i
        assert flags[i] & BAD_CT and not flags[i] & BAD_PROOF, i


def test_refusals_and_the_empty_batch(ctx, records, sk_mod_q, withdraw_artifacts):
    import numpy as np
    import spp
    a = records["device"][0]
    L = ctx.L
    sk = np.asarray(sk_mod_q, dtype=np.uint32)
    c0, c1 = np.ascontiguousarray(a["c0"][:2]), np.ascontiguousarray(a["c1"][:2])
    owners, flags = np.zeros(128, dtype=np.uint8), np.zeros(2, dtype=np.uint32)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    vk = records["vk"]
    call = lambda **k: L.spp_audit_open_batch(*[{**dict(ctx=ctx.h, vk=vk, vk_len=len(vk), sk=p(sk), count=2, proofs=a["proofs"][:776], pws=a["pws"][:152],
                                                        c0=p(c0), c1=p(c1), owners=p(owners), flags=p(flags)), **k}[n]
                                                for n in ("ctx", "vk", "vk_len", "sk", "count", "proofs", "pws", "c0", "c1", "owners", "flags")])
    assert call() == 0 and flags.tolist() == [0, 0]
    for name in ("ctx", "sk", "proofs", "pws", "c0", "c1", "owners", "flags"):
        assert call(**{name: None}) == -1 and "NULL" in spp.last_error(), name
    assert call(vk=None) == -1 and call(vk_len=0) == -1                         # a key without its length, a length without a key
    assert call(vk=None, vk_len=0, proofs=None) == 0                             # no key: proofs may be NULL
    bad_sk = sk.copy(); bad_sk[1023] = Q
    assert call(sk=p(bad_sk)) == -1 and "[0, q)" in spp.last_error()
    wvk = open(withdraw_artifacts["vk"], "rb").read()                            # five public inputs
    assert call(vk=wvk, vk_len=len(wvk)) == -7 and "public inputs" in spp.last_error()
    assert call(vk=vk[:-1], vk_len=len(vk) - 1) == -7
    assert call(count=(1 << 24) + 1) == -1 and "2^24" in spp.last_error()        # refused before any buffer is read
    flags[:] = 9
    assert call(count=0) == 0 and flags.tolist() == [9, 9]
    assert ctx.audit_open(vk, sk_mod_q, [], [], np.zeros((0, 64)), np.zeros((0, 1024))) == ([], [])


def test_cli_audit_open(tmp_path, records, decrypt_fixture, capsys):
    from spp import cli, witness as W
    from oracle import hashes as H
    a = records["device"][0]
    i = 7
    shares = []
    for s in decrypt_fixture["shares"]:
        path = str(tmp_path / ("share_%d.json" % s["share_index"]))
        json.dump({"share_index": s["share_index"], "threshold": s["threshold"], "num_shares": 3,
                   "coefficients": [{"x": s["x"], "y": y} for y in s["y"]]}, open(path, "w"))
        shares.append(path)
    owner = H.fixed_base_scalar_mul(records["sks"][i])
    vk, proof, pw, ctj, bad = (str(tmp_path / n) for n in ("a.vk", "a.proof", "a.pw", "ciphertext.json", "tampered.json"))
    open(vk, "wb").write(records["vk"]); open(proof, "wb").write(a["proofs"][388 * i:388 * (i + 1)]); open(pw, "wb").write(a["pws"][76 * i:76 * (i + 1)])
    json.dump(W.ciphertext_json(a["c0"][i], a["c1"][i], owner), open(ctj, "w"))
    assert cli.main(["audit-open", vk, proof, pw, ctj, "--shares"] + shares) == 0
    out = capsys.readouterr().out
    assert "owner_x = 0x%064x" % owner[0] in out and "owner_y = 0x%064x" % owner[1] in out and "proof: verified" in out
    assert cli.main(["audit-open", "-", proof, pw, ctj, "--shares"] + shares) == 0
    assert "proof: not checked" in capsys.readouterr().out
    c0 = a["c0"][i].copy(); c0[5] = (int(c0[5]) + DELTA) % Q
    json.dump(W.ciphertext_json(c0, a["c1"][i], owner), open(bad, "w"))
    assert cli.main(["audit-open", vk, proof, pw, bad, "--shares"] + shares) == 1
    out = capsys.readouterr().out
    assert "proof: verified" in out and out.count("NOT the one the proof commits to") == 2
