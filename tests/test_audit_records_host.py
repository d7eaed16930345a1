"""Audit records, host side (no GPU): the C declarations of spp_prove_audit_records(_device) and spp_audit_open_batch, the header
the record-opening kernel is made of (csrc/audit_open.hpp) compiled for the host against the reference-derived fixtures, the
file formats the prover and the key holders leave for the auditor, and the argument errors of `spp audit-open`."""
import ctypes
import json
import os
import re
import subprocess

import pytest

from conftest import ROOT, GOLDEN

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
Q = 167772161
DELTA = Q // 256
CALLS = ("spp_prove_audit_records_device", "spp_prove_audit_records", "spp_audit_open_batch")


@pytest.fixture(scope="module")
def vectors():
    return json.load(open(os.path.join(GOLDEN, "rlwe_vectors.json")))


@pytest.fixture(scope="module")
def decrypt_fixture():
    return json.load(open(os.path.join(GOLDEN, "rlwe_decrypt.json")))


def test_header_declares_the_audit_record_calls_and_flags():
    hdr = open(os.path.join(ROOT, "include", "spp.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int spp_prove_audit_records_device(spp_circuit* c, size_t count, const void* d_pk_a, const void* d_pk_b, const void* d_sk, "
            "const void* d_r, const void* d_e1, const void* d_e2, const void* d_rs, void* d_proofs, void* d_pws, void* d_status, "
            "void* d_c0, void* d_c1);") in flat
    assert ("int spp_prove_audit_records(spp_circuit* c, const uint32_t* pk_a, const uint32_t* pk_b, size_t count, const uint8_t* sk, "
            "const int8_t* r, const int8_t* e1, const int8_t* e2, const uint8_t* rs, uint8_t* proofs, uint8_t* pws, int32_t* status, "
            "uint32_t* c0, uint32_t* c1);") in flat
    assert ("int spp_audit_open_batch(spp_ctx* ctx, const uint8_t* vk, size_t vk_len, const uint32_t* sk_mod_q, size_t count, "
            "const uint8_t* proofs, const uint8_t* pws, const uint32_t* c0, const uint32_t* c1, uint8_t* owners, uint32_t* flags);") in flat
    for name, val in (("SPP_AUDIT_BAD_PROOF", 1), ("SPP_AUDIT_BAD_CIPHERTEXT", 2), ("SPP_AUDIT_BAD_IDENTITY", 4)):
        assert re.search(r"#define %s %d\b" % (name, val), hdr), name
    # the reference interfaces the calls replace are named in the header's index
    assert "generate_audit.py:590-606" in hdr and "rlwe_decrypt.py:61-149" in hdr


def test_library_exports_the_calls_and_python_mirrors_the_flags():
    import spp
    from spp import lib
    L = spp.load_library()
    for name in CALLS:
        assert hasattr(L, name), name
    hdr = open(os.path.join(ROOT, "include", "spp.h")).read()
    for name in ("SPP_AUDIT_BAD_PROOF", "SPP_AUDIT_BAD_CIPHERTEXT", "SPP_AUDIT_BAD_IDENTITY"):
        assert getattr(lib, name) == int(re.search(r"#define %s (\d+)" % name, hdr).group(1))
    assert lib.AUDIT_PW_LEN == int(re.search(r"#define SPP_AUDIT_PW_LEN (\d+)", hdr).group(1)) == 76
    for m in ("prove_audit_records_device", "prove_audit_records"):
        assert callable(getattr(spp.prover.CircuitHandle, m))
    assert callable(spp.prover.Context.audit_open)


def test_calls_refuse_null_arguments_without_a_device():
    import spp
    L = spp.load_library()
    assert L.spp_prove_audit_records_device(None, 1, None, None, None, None, None, None, None, None, None, None, None, None) == -1
    assert "NULL" in spp.last_error()
    assert L.spp_prove_audit_records(None, None, None, 1, None, None, None, None, None, None, None, None, None, None) == -1
    assert L.spp_audit_open_batch(None, None, 0, None, 1, None, None, None, None, None, None) == -1
    assert "NULL" in spp.last_error()


def _ints(vals):
    return [int(x, 16) if isinstance(x, str) else int(x) for x in vals]


def _pw(wa, ct):
    return (2).to_bytes(4, "big") + (0).to_bytes(4, "big") + (2).to_bytes(4, "big") + wa.to_bytes(32, "big") + ct.to_bytes(32, "big")


def test_audit_open_header_on_the_host(tmp_path, vectors, decrypt_fixture):
    """csrc/audit_open.hpp under g++: the four reference vectors pack to c0_packed ++ c1_packed and decrypt to msg under the
    fixture key; 64 slots of 0xFF decode to an owner_x >= r; a coefficient equal to q raises the range flag (and decrypts as its
    residue); the decision compares both hashes with the public witness bytewise."""
    from oracle import rlwe, hashes as H
    exe = str(tmp_path / "audit_open_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "audit_open_check.cpp"), "-o", exe], check=True)
    sk = decrypt_fixture["sk_mod_q"]
    h64 = lambda v: "%064x" % v
    cases = []    # (c0, c1, ct_be computed, wa_be computed, pw, expected flags)
    for v in vectors:
        cases.append((v["c0"], v["c1"], 5, 6, _pw(6, 5), None))
    # vector 0 is the reference's own run: the key of sk = 12345; the true hashes, a pw that carries them -> 0
    v0 = vectors[0]
    owner = H.fixed_base_scalar_mul(12345)
    wa, ct = H.poseidon_hash2(*owner), H.poseidon2_sponge(_ints(v0["c0_packed"] + v0["c1_packed"]))
    cases.append((v0["c0"], v0["c1"], ct, wa, _pw(wa, ct), 0))
    cases.append((v0["c0"], v0["c1"], ct, wa, _pw(wa, ct ^ 1), 2))            # the pw commits to another ciphertext
    cases.append((v0["c0"], v0["c1"], ct, wa, _pw(wa ^ (1 << 255), ct), 4))   # ... to another identity (top byte differs)
    cases.append(([255 * DELTA] * 64, [0] * 1024, 5, 6, _pw(6, 5), 4))         # 64 x 0xFF: owner_x = 2^256 - 1 >= r
    c1q = list(v0["c1"]); c1q[1000] = Q                                        # a coefficient equal to q
    cases.append((v0["c0"], c1q, ct, wa, _pw(wa, ct), None))
    c0q = list(v0["c0"]); c0q[3] = Q
    cases.append((c0q, v0["c1"], ct, wa, _pw(wa, ct), None))
    # a point below r but off the curve: (1, 1) encrypted without noise
    msg_off = rlwe.owner_msg(1, 1)
    cases.append(([DELTA * m for m in msg_off], [0] * 1024, 5, 6, _pw(6, 5), 4))
    text = " ".join(str(x) for x in sk) + "\n%d\n" % len(cases)
    for c0, c1, ctb, wab, pw, _ in cases:
        text += " ".join(str(x) for x in list(c0) + list(c1)) + "\n%s %s %s\n" % (h64(ctb), h64(wab), pw.hex())
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-300:] + out.stderr
    lines = out.stdout.strip().split("\n")
    assert lines[-1] == "OK audit_open %d cases" % len(cases) and len(lines) == len(cases) + 1
    rows = [ln.split(" ") for ln in lines[:-1]]
    for i, v in enumerate(vectors):
        bad, point, flags, msg, owners, packed = rows[i]
        assert bad == "0" and list(bytes.fromhex(msg)) == v["msg"] == decrypt_fixture["decrypt"][i]["msg"], v["name"]
        assert [int(x, 16) for x in packed.split(",")] == _ints(v["c0_packed"] + v["c1_packed"]), v["name"]
        ox, oy = rlwe.decode_owner(v["msg"])
        assert bytes.fromhex(owners) == ox.to_bytes(32, "big") + oy.to_bytes(32, "big")
        on_curve = ox < R and oy < R and (oy * oy - ox * ox * ox + 17) % R == 0
        assert point == ("1" if on_curve else "0"), v["name"]
    assert rows[0][1] == "1" and bytes.fromhex(rows[0][4]) == owner[0].to_bytes(32, "big") + owner[1].to_bytes(32, "big")
    for i, case in enumerate(cases):
        if case[5] is not None:
            assert int(rows[i][2]) == case[5], i
    k = len(vectors)
    assert rows[k + 3][:2] == ["0", "0"] and rows[k + 3][3] == "ff" * 64 and int(rows[k + 3][4][:64], 16) == (1 << 256) - 1 >= R
    for j, (c0, c1) in ((k + 4, (v0["c0"], c1q)), (k + 5, (c0q, v0["c1"]))):
        assert rows[j][0] == "1" and int(rows[j][2]) & 2
        # the oracle reduces mod q too: same bytes, and the identity bit follows from them
        exp = rlwe.rlwe_decrypt(sk, c0, c1)
        assert list(bytes.fromhex(rows[j][3])) == exp
        assert (int(rows[j][2]) & 4 == 0) == (rlwe.decode_owner(exp) == owner)
    assert rows[k + 6][:3] == ["0", "0", "4"] and list(bytes.fromhex(rows[k + 6][3])) == msg_off


def test_fixture_key_decrypts_oracle_ciphertexts_on_the_cpu(decrypt_fixture, rlwe_pk):
    """The premise of the round trip, checked without the GPU: rlwe_decrypt.json's key is the secret of rlwe_pk.json, and 64 slots
    of 0xFF decode to an owner_x that is no field element."""
    import random
    from oracle import rlwe, hashes as H
    sk = decrypt_fixture["sk_mod_q"]
    for i in range(6):
        d = rlwe.audit_inputs(rlwe_pk["a"], rlwe_pk["b"], 12345 + 500 + i, random.Random(1000 + 500 + i))
        assert rlwe.decode_owner(rlwe.rlwe_decrypt(sk, d["c0"], d["c1"])) == H.fixed_base_scalar_mul(12345 + 500 + i) == (d["owner_x"], d["owner_y"])
    msg = rlwe.rlwe_decrypt(sk, [255 * DELTA] * 64, [0] * 1024)
    assert msg == [255] * 64 and rlwe.decode_owner(msg)[0] >= R


def test_ciphertext_json_round_trip_and_reference_keys(tmp_path, vectors):
    from spp import witness as W
    v = vectors[0]
    d = W.ciphertext_json(v["c0"], v["c1"], owner=(0x1234, 0x5678))
    # the key set and order of scripts/generate_audit.py:593-605
    assert list(d) == ["c0_sparse", "c1", "c0_packed", "c1_packed", "pack_width", "pack_bits", "msg_slots", "q", "delta",
                       "expected_owner_x", "expected_owner_y"]
    assert [int(x, 16) for x in d["c0_packed"]] == _ints(v["c0_packed"]) and [int(x, 16) for x in d["c1_packed"]] == _ints(v["c1_packed"])
    assert all(x == hex(int(x, 16)) for x in d["c0_packed"] + d["c1_packed"])
    assert (d["pack_width"], d["pack_bits"], d["msg_slots"], d["q"], d["delta"]) == (7, 32, 64, Q, DELTA)
    assert d["expected_owner_x"] == "0x1234" and d["expected_owner_y"] == "0x5678"
    path = str(tmp_path / "ciphertext.json")
    json.dump(d, open(path, "w"))
    assert W.load_ciphertext_json(path) == (v["c0"], v["c1"], (0x1234, 0x5678))
    json.dump(W.ciphertext_json(v["c0"], v["c1"]), open(path, "w"))
    assert W.load_ciphertext_json(path) == (v["c0"], v["c1"], None)
    for breakage in (lambda x: x.pop("c1"), lambda x: x.update(q=Q + 2), lambda x: x["c0_sparse"].pop(),
                     lambda x: x["c1_packed"].__setitem__(3, "0x1")):
        bad = W.ciphertext_json(v["c0"], v["c1"])
        breakage(bad)
        json.dump(bad, open(path, "w"))
        with pytest.raises(ValueError):
            W.load_ciphertext_json(path)
    with pytest.raises(ValueError):
        W.ciphertext_json(v["c0"][:-1] + [Q], v["c1"])


def _write_reference_shares(tmp_path, fixture):
    """the fixture's two shares in the file format of scripts/rlwe_keygen.py:157-171"""
    paths = []
    for s in fixture["shares"]:
        p = str(tmp_path / ("share_%d.json" % s["share_index"]))
        json.dump({"share_index": s["share_index"], "threshold": s["threshold"], "num_shares": 3,
                   "coefficients": [{"x": s["x"], "y": y} for y in s["y"]]}, open(p, "w"))
        paths.append(p)
    return paths


def test_load_share_json_feeds_the_reconstruction(tmp_path, decrypt_fixture):
    from spp import witness as W
    from oracle import rlwe
    shares = [W.load_share_json(p) for p in _write_reference_shares(tmp_path, decrypt_fixture)]
    assert [s["x"] for s in shares] == [1, 2] and all(s["threshold"] == 2 and len(s["y"]) == 1024 for s in shares)
    assert rlwe.reconstruct_sk([s["x"] for s in shares], [s["y"] for s in shares], 2) == decrypt_fixture["sk_mod_q"]
    bad = str(tmp_path / "bad.json")
    json.dump({"share_index": 1, "threshold": 2, "coefficients": [{"x": 1, "y": "0x1"}] * 3}, open(bad, "w"))
    with pytest.raises(ValueError):
        W.load_share_json(bad)
    json.dump({"threshold": 2}, open(bad, "w"))
    with pytest.raises(ValueError):
        W.load_share_json(bad)


def test_cli_audit_open_argument_errors_touch_no_device(tmp_path, vectors, decrypt_fixture, monkeypatch, capsys):
    from spp import cli, witness as W, prover
    def no_device(*a, **k):
        raise AssertionError("a device context was opened")
    monkeypatch.setattr(cli, "Context", no_device)
    monkeypatch.setattr(prover.Context, "__init__", no_device)
    shares = _write_reference_shares(tmp_path, decrypt_fixture)
    ctj, proof, pw = str(tmp_path / "ciphertext.json"), str(tmp_path / "a.proof"), str(tmp_path / "a.pw")
    json.dump(W.ciphertext_json(vectors[0]["c0"], vectors[0]["c1"]), open(ctj, "w"))
    open(proof, "wb").write(bytes(388)); open(pw, "wb").write(_pw(1, 2))
    with pytest.raises(SystemExit) as e:                                        # --shares is required
        cli.main(["audit-open", "-", proof, pw, ctj])
    assert e.value.code != 0
    with pytest.raises(SystemExit) as e:                                        # the ciphertext is missing
        cli.main(["audit-open", "-", proof, pw, "--shares"] + shares)
    assert e.value.code != 0
    assert cli.main(["audit-open", "-", proof, pw, ctj, "--shares", shares[0]]) != 0              # one share of a 2-of-3 key
    assert cli.main(["audit-open", "-", proof, pw, ctj, "--shares", shares[0], shares[0]]) != 0   # the same share twice
    assert cli.main(["audit-open", "-", proof, pw, str(tmp_path / "none.json"), "--shares"] + shares) != 0
    assert cli.main(["audit-open", str(tmp_path / "none.vk"), proof, pw, ctj, "--shares"] + shares) != 0
    open(proof, "wb").write(bytes(100))
    assert cli.main(["audit-open", "-", proof, pw, ctj, "--shares"] + shares) != 0                # a truncated proof
    open(proof, "wb").write(bytes(388))
    json.dump({"c0_sparse": [1]}, open(ctj, "w"))
    assert cli.main(["audit-open", "-", proof, pw, ctj, "--shares"] + shares) != 0                # not a ciphertext.json
    assert "audit-open" in capsys.readouterr().err
