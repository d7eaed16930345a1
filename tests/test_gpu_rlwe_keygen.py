"""GPU: auditor key generation on the device -- spp_rlwe_keygen_batch, spp_rlwe_key_check, spp_shamir_split and the two CLI
sub-commands -- against what the committed fixtures pin of the reference's scripts/rlwe_keygen.py (tests/rlwe_keygen_vectors.py),
a numpy int64 schoolbook product, Python integers, and the calls that already read these keys (spp_shamir_reconstruct,
spp_rlwe_witness_batch, spp_rlwe_decrypt_batch)."""
import ctypes
import itertools
import json
import os

import numpy as np
import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None

from conftest import GOLDEN
import rlwe_keygen_vectors as V

pytestmark = pytest.mark.gpu

Q, R = V.Q, V.R


@pytest.fixture(scope="module")
def ctx():
    import spp
    c = spp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def key():
    return V.fixture_key()


def _reconstruct(ctx, shares):
    """spp_shamir_reconstruct with the field elements themselves as output"""
    t, n = len(shares), len(shares[0]["y"])
    xs = (ctypes.c_uint32 * t)(*[s["x"] for s in shares])
    ys = b"".join(int(v).to_bytes(32, "big") for s in shares for v in s["y"])
    out = ctypes.create_string_buffer(n * 32)
    from spp.lib import check
    check(ctx.L.spp_shamir_reconstruct(ctx.h, t, ctypes.cast(xs, ctypes.c_void_p), ys, n, ctypes.cast(out, ctypes.c_void_p), None))
    return [int.from_bytes(out.raw[32 * i:32 * i + 32], "big") for i in range(n)]


def _shares_in_python(secrets, coeffs, xs):
    out = []
    for x in xs:
        ys = []
        for i, s in enumerate(secrets):
            v, xp = s, 1
            for row in coeffs:
                xp = xp * x % R
                v = (v + row[i] * xp) % R
            ys.append(v)
        out.append(ys)
    return out


def test_reference_pin(ctx, key):
    """sk, a, e derived from the fixtures -> b of rlwe_pk.json bit for bit, sk_mod_q of rlwe_decrypt.json"""
    from spp import witness
    b, skq = witness.rlwe_keygen(ctx, key["sk"], key["a"], key["e"])
    assert b.shape == skq.shape == (1, 1024)
    assert b[0].tolist() == key["b"]
    assert skq[0].tolist() == key["sk_mod_q"]


def test_edge_keys_against_the_schoolbook_product(ctx):
    """the host check's edge cases in one call of 6 keys, then 1 key and 67 keys (more keys than a wave has lanes)"""
    from spp import witness
    sk, a, e = V.edge_keys()
    b, skq = witness.rlwe_keygen(ctx, sk, a, e)
    for k in range(6):
        assert np.array_equal(b[k], V.public_b(sk[k], a[k], e[k])), k
        assert np.array_equal(skq[k], np.mod(sk[k].astype(np.int64), Q).astype(np.uint32)), k
    rng = np.random.default_rng(7)
    for count in (1, 67):
        sk = rng.integers(-3, 4, (count, 1024)).astype(np.int8)
        e = rng.integers(-3, 4, (count, 1024)).astype(np.int8)
        a = rng.integers(0, Q, (count, 1024)).astype(np.uint32)
        b, skq = witness.rlwe_keygen(ctx, sk, a, e)
        for k in range(count):
            assert np.array_equal(b[k], V.public_b(sk[k], a[k], e[k])), (count, k)
        assert np.array_equal(skq, np.mod(sk.astype(np.int64), Q).astype(np.uint32))
    # sk_mod_q is optional
    out = np.zeros(1024, dtype=np.uint32)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    assert ctx.L.spp_rlwe_keygen_batch(ctx.h, 1, p(sk[0]), p(a[0]), p(e[0]), p(out), None) == 0
    assert np.array_equal(out, b[0])


def test_key_check(ctx, key):
    from spp import witness
    a, b, skq = key["a"], key["b"], key["sk_mod_q"]
    noise, skmax = witness.rlwe_key_check(ctx, a, b, skq)[0]
    assert noise == max(abs(v) for v in key["e"]) <= 3 and skmax == max(abs(v) for v in key["sk"]) <= 3
    moved = list(b)
    moved[5] = (moved[5] + 1000) % Q
    sk9 = list(skq)
    sk9[0] = 9
    # three keys in one call: the good one, b[5] moved by 1000, sk[0] = 9
    got = witness.rlwe_key_check(ctx, [a, a, a], [b, moved, b], [skq, skq, sk9])
    assert got[0] == (noise, skmax)
    assert 997 <= got[1][0] <= 1003 and got[1][0] == abs(key["e"][5] + 1000) and got[1][1] == skmax
    assert got[2][1] == 9
    assert got[2][0] > 3        # and that key is no longer the secret of (a, b)


def test_shamir_pin(ctx, key):
    """the degree-1 coefficients derived from share 1 -> share 1, share 2 (all 1024 values) and the head of share 3"""
    from spp import witness
    shares = witness.shamir_split(ctx, [v % R for v in key["sk"]], 2, 3, coeffs=[key["c1"]])
    assert [s["x"] for s in shares] == [1, 2, 3]
    assert shares[0]["y"] == key["y1"]
    assert shares[1]["y"] == key["y2"]
    assert shares[2]["y"][:4] == key["share3_head"]


@pytest.mark.parametrize("n", [1, 257, 1024])
def test_shamir_shapes(ctx, n):
    from spp import witness
    special = [0, R - 1, 1, R - 2]
    val = lambda i, salt: special[i % 4] if i < 8 else (i * 0x9E3779B97F4A7C15F39CC0605CEDC835 + salt * 0x2545F4914F6CDD1D + 11) ** 3 % R
    secrets = [val(i, 1) for i in range(n)]
    # t = 1: every share is the secret
    shares = witness.shamir_split(ctx, secrets, 1, 3)
    assert [s["y"] for s in shares] == [secrets] * 3 and [s["x"] for s in shares] == [1, 2, 3]
    # t = 3, m = 5 at indices that are neither sorted nor small
    xs = [7, 2, 9, 4, 2 ** 32 - 1]
    coeffs = [[val(i + 3, 2) for i in range(n)], [val(i + 5, 3) for i in range(n)]]
    shares = witness.shamir_split(ctx, secrets, 3, 5, xs=xs, coeffs=coeffs)
    assert [s["x"] for s in shares] == xs
    assert [s["y"] for s in shares] == _shares_in_python(secrets, coeffs, xs)
    for subset in ((0, 1, 2), (4, 2, 0), (1, 3, 4)):
        assert _reconstruct(ctx, [shares[j] for j in subset]) == secrets, subset
    # the library's own coefficients: two sharings differ, both reconstruct
    one, two = witness.shamir_split(ctx, secrets, 3, 5, xs=xs), witness.shamir_split(ctx, secrets, 3, 5, xs=xs)
    assert all(s["y"] != t["y"] for s, t in zip(one, two))
    assert all(0 <= v < R for s in one + two for v in s["y"])
    assert _reconstruct(ctx, one[1:4]) == secrets and _reconstruct(ctx, [two[4], two[0], two[2]]) == secrets
    assert _reconstruct(ctx, one[:2] + two[2:3]) != secrets          # shares of two sharings do not combine


def test_round_trip_sample_keygen_encrypt_split_reconstruct_decrypt(ctx):
    """A sampled key through every consumer: encrypt 4 messages to it, share the secret 2-of-3, reconstruct from shares (1, 3),
    decrypt.  Worst-case noise |e*r + e1 + sk*e2| <= 1024*9 + 3 + 1024*9 = 18 435, far below Delta / 2 = 327 680."""
    from spp import witness
    sk, a, e = witness.rlwe_sample_key(ctx.L, 1, 3)
    b, skq = witness.rlwe_keygen(ctx, sk, a, e)
    assert witness.rlwe_key_check(ctx, a, b, skq)[0] == (int(np.abs(e).max()), int(np.abs(sk).max()))
    rng = np.random.default_rng(99)
    msg = rng.integers(0, 256, (4, 64)).astype(np.uint8)
    msg[0, :] = 255
    msg[1, :] = 0
    r, e2 = (rng.integers(-3, 4, (4, 1024)).astype(np.int8) for _ in range(2))
    e1 = rng.integers(-3, 4, (4, 64)).astype(np.int8)
    ct = witness.rlwe_witness(ctx, a[0], b[0], r, e1, e2, msg)
    shares = witness.shamir_split(ctx, [int(v) % R for v in sk[0]], 2, 3)
    back = witness.reconstruct_sk(ctx, [shares[0], shares[2]])
    assert back == skq[0].tolist()
    _, got = witness.rlwe_decrypt(ctx, back, ct["c0"], ct["c1"])
    assert np.array_equal(got, msg)


def test_cli_keygen_reproduces_the_fixture_and_key_check_decides(tmp_path, key, capsys):
    from spp import cli, witness
    out = str(tmp_path / "keys")
    assert cli.main(["rlwe-keygen", "--out", out, "--reference-seed", "42"]) == 0
    said = capsys.readouterr().out
    assert "max |b + a*sk| = 3" in said and "max |sk| = 3" in said
    pk_path = os.path.join(out, "rlwe_pk.json")
    assert witness.load_rlwe_pk_json(pk_path) == (key["a"], key["b"])
    golden = json.load(open(os.path.join(GOLDEN, "rlwe_pk.json")))
    mine = json.load(open(pk_path))
    assert [int(v, 16) for v in mine["a"]] == golden["a"] and [int(v, 16) for v in mine["b"]] == golden["b"]
    params = json.load(open(os.path.join(out, "rlwe_params.json")))
    assert (params["threshold"], params["num_shares"], params["noise_bound"], params["q"]) == (2, 3, 3, Q)
    share_paths = [os.path.join(out, "rlwe_sk_shares", "share_%d.json" % i) for i in (1, 2, 3)]
    files = [json.load(open(p)) for p in share_paths]
    for f, fx in zip(files, key["shares"]):
        assert (f["share_index"], f["threshold"], f["num_shares"]) == (fx["share_index"], 2, 3)
        assert [c["x"] for c in f["coefficients"]] == [fx["x"]] * 1024 and [c["y"] for c in f["coefficients"]] == fx["y"]
    assert [int(c["y"], 16) for c in files[2]["coefficients"][:4]] == key["share3_head"] and files[2]["coefficients"][0]["x"] == 3
    # every pair of shares is the key of this public key
    for pair in itertools.combinations(share_paths, 2):
        assert cli.main(["rlwe-key-check", pk_path, "--shares"] + list(pair)) == 0
    assert "max |b + a*sk| = 3" in capsys.readouterr().out
    # one coefficient of b altered: not a key pair any more
    mine["b"][700] = "0x%08x" % ((int(mine["b"][700], 16) + 12345) % Q)
    bad = str(tmp_path / "keys" / "altered_pk.json")
    json.dump(mine, open(bad, "w"))
    assert cli.main(["rlwe-key-check", bad, "--shares"] + share_paths[:2]) == 1
    assert "NOT a key pair" in capsys.readouterr().out
    # the default randomness: another key, which passes its own check
    fresh = str(tmp_path / "fresh")
    assert cli.main(["rlwe-keygen", "--out", fresh, "--threshold", "3", "--shares", "4"]) == 0
    assert witness.load_rlwe_pk_json(os.path.join(fresh, "rlwe_pk.json"))[1] != key["b"]
    fresh_shares = [os.path.join(fresh, "rlwe_sk_shares", "share_%d.json" % i) for i in (4, 1, 3)]
    assert cli.main(["rlwe-key-check", os.path.join(fresh, "rlwe_pk.json"), "--shares"] + fresh_shares) == 0
    assert cli.main(["rlwe-key-check", os.path.join(fresh, "rlwe_pk.json"), "--shares"] + fresh_shares[:2]) != 0   # 2 of a 3-of-4 key
