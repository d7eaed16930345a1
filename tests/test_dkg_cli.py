"""`spp.cli dkg-deal` / `dkg-receive`: three auditors make a key that no dealer held, the files load where an rlwe-keygen key
does, a refresh round renews the shares, and a swapped hash, a missing dealer and a changed sub-share are each refused by name
with nothing written.  What is wrong with the arguments is found before a device is opened (the two tests without the gpu mark)."""
import json
import os

import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None

SEED = "5a" * 32
T, M_ = 2, 3


def _main(argv, capsys):
    from spp import cli
    rc = cli.main(argv)
    return rc, capsys.readouterr()


def test_committee_size_is_refused_with_the_arithmetic(tmp_path, capsys):
    out = str(tmp_path / "d")
    rc, io = _main(["dkg-deal", "--index", "1", "--threshold", "2", "--shares", "11", "--a-seed", SEED, "--out", out], capsys)
    assert rc == 2 and "11 * 18432 + 3 = 202755" in io.err and "333827" in io.err and "327680" in io.err and "315395" in io.err
    assert not os.path.exists(out)
    rc, io = _main(["dkg-deal", "--index", "4", "--threshold", "2", "--shares", "3", "--a-seed", SEED, "--out", out], capsys)
    assert rc == 2 and "1..3" in io.err and not os.path.exists(out)
    rc, io = _main(["dkg-deal", "--index", "1", "--threshold", "4", "--shares", "3", "--a-seed", SEED, "--out", out], capsys)
    assert rc == 2 and "threshold" in io.err and not os.path.exists(out)


def test_seed_is_32_bytes(tmp_path, capsys):
    for bad in ("zz", "00" * 31, "00" * 33):
        rc, io = _main(["dkg-deal", "--index", "1", "--threshold", "2", "--shares", "3", "--a-seed", bad, "--out", str(tmp_path / "d")], capsys)
        assert rc == 2 and "spp dkg-deal" in io.err, bad


@pytest.fixture(scope="module")
def dealt(tmp_path_factory):
    """three dkg-deal runs into one directory per auditor"""
    from spp import cli
    root = tmp_path_factory.mktemp("dkg")
    dirs = [str(root / ("auditor_%d" % i)) for i in range(1, M_ + 1)]
    for i, d in enumerate(dirs, 1):
        assert cli.main(["dkg-deal", "--index", str(i), "--threshold", str(T), "--shares", str(M_), "--a-seed", SEED, "--out", d]) == 0
    return root, dirs


def _receive_args(dirs, j, out, deals=None, hashes=None, subs=None):
    order = range(1, M_ + 1)
    deals = deals or [os.path.join(dirs[i - 1], "deal_%d.json" % i) for i in order]
    hashes = hashes or [os.path.join(dirs[i - 1], "deal_%d.hash" % i) for i in order]
    subs = subs or [os.path.join(dirs[i - 1], "private", "subshare_%d_to_%d.json" % (i, j)) for i in order]
    return ["dkg-receive", "--index", str(j), "--deals"] + deals + ["--hashes"] + hashes + ["--subshares"] + subs + ["--out", out]


@pytest.fixture(scope="module")
def received(dealt):
    """three dkg-receive runs, one key directory per auditor; (directories, [(exit code, stdout)])"""
    import contextlib
    import io
    from spp import cli
    root, dirs = dealt
    outs = [str(root / ("key_%d" % j)) for j in range(1, M_ + 1)]
    results = []
    for j, out in enumerate(outs, 1):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            rc = cli.main(_receive_args(dirs, j, out))
        results.append((rc, buf.getvalue()))
    return outs, results


@pytest.mark.gpu
def test_round_trip(dealt, received, capsys):
    import hashlib
    from spp import witness
    root, dirs = dealt
    for i, d in enumerate(dirs, 1):
        body = open(os.path.join(d, "deal_%d.json" % i), "rb").read()
        deal = json.loads(body)
        assert open(os.path.join(d, "deal_%d.hash" % i)).read().strip() == hashlib.sha256(body).hexdigest()
        assert sorted(deal) == ["a_seed", "b", "commitments", "index", "kind", "num_shares", "threshold", "version"]
        assert (deal["kind"], deal["index"], deal["threshold"], deal["num_shares"], deal["a_seed"]) == ("key", i, T, M_, SEED)
        assert len(deal["commitments"]) == 2 * T * 1024 * 64 and len(deal["b"]) == 1024
        assert sorted(os.listdir(d)) == ["deal_%d.hash" % i, "deal_%d.json" % i, "private"]
        assert sorted(os.listdir(os.path.join(d, "private"))) == ["subshare_%d_to_%d.json" % (i, j) for j in range(1, M_ + 1)]
        sub = json.load(open(os.path.join(d, "private", "subshare_%d_to_2.json" % i)))
        assert sorted(sub) == ["from", "to", "y", "y_blind"] and (sub["from"], sub["to"]) == (i, 2)     # no s_i, no e_i anywhere
    outs, results = received
    for j, (out, (rc, text)) in enumerate(zip(outs, results), 1):
        assert rc == 0 and "share_%d.json" % j in text
        assert sorted(os.listdir(out)) == ["rlwe_params.json", "rlwe_pk.json", "rlwe_sk_shares"]
        assert os.listdir(os.path.join(out, "rlwe_sk_shares")) == ["share_%d.json" % j]
    pks = [open(os.path.join(out, "rlwe_pk.json")).read() for out in outs]
    assert pks[0] == pks[1] == pks[2]
    params = json.load(open(os.path.join(outs[0], "rlwe_params.json")))
    assert (params["noise_bound"], params["threshold"], params["num_shares"]) == (3 * M_, T, M_)
    share = lambda j, base=None: os.path.join(base or outs[j - 1], "rlwe_sk_shares", "share_%d.json" % j)
    # the files load where an rlwe-keygen key does
    for pick in ((1, 2), (3, 1)):
        rc, io = _main(["rlwe-key-check", os.path.join(outs[0], "rlwe_pk.json"), "--shares"] + [share(j) for j in pick], capsys)
        assert rc == 0 and "the shares hold the secret of this public key" in io.out, io.out + io.err
    # a is the seed's
    a, b = witness.load_rlwe_pk_json(os.path.join(outs[0], "rlwe_pk.json"))
    assert a == witness.dkg_a_from_seed(__import__("spp").lib.load_library(), bytes.fromhex(SEED))

    # ---- a refresh round: new shares at the same x, the same key ----
    rdirs = [str(root / ("refresh_%d" % i)) for i in range(1, M_ + 1)]
    for i, d in enumerate(rdirs, 1):
        rc, io = _main(["dkg-deal", "--index", str(i), "--threshold", str(T), "--shares", str(M_), "--a-seed", SEED, "--out", d, "--refresh"], capsys)
        assert rc == 0, io.err
        deal = json.load(open(os.path.join(d, "deal_%d.json" % i)))
        assert deal["kind"] == "refresh" and "b" not in deal and len(deal["zero_blinds"]) == 1024
    routs = [str(root / ("renewed_%d" % j)) for j in range(1, M_ + 1)]
    for j, out in enumerate(routs, 1):
        rc, io = _main(_receive_args(rdirs, j, out) + ["--refresh", share(j)], capsys)
        assert rc == 0, io.err
        assert os.listdir(out) == ["rlwe_sk_shares"] and os.listdir(os.path.join(out, "rlwe_sk_shares")) == ["share_%d.json" % j]
        old, new = witness.load_share_json(share(j)), witness.load_share_json(share(j, out))
        assert new["x"] == old["x"] == j and new["y"] != old["y"]
    rc, io = _main(["rlwe-key-check", os.path.join(outs[0], "rlwe_pk.json"), "--shares", share(1, routs[0]), share(3, routs[2])], capsys)
    assert rc == 0, io.out + io.err
    rc, io = _main(["rlwe-key-check", os.path.join(outs[0], "rlwe_pk.json"), "--shares", share(1), share(3, routs[2])], capsys)
    assert rc == 1, "an old share and a renewed one are not shares of one key"
    # key dealings are not refresh dealings
    rc, io = _main(_receive_args(dirs, 1, str(root / "mixed")) + ["--refresh", share(1)], capsys)
    assert rc == 2 and not os.path.exists(str(root / "mixed"))


@pytest.mark.gpu
def test_refusals_name_the_dealer_and_write_nothing(dealt, tmp_path, capsys):
    root, dirs = dealt
    out = str(tmp_path / "refused")
    path = lambda i, name: os.path.join(dirs[i - 1], name)
    # a swapped .hash: dealer 1's file against dealer 2's published hash
    hashes = [path(2, "deal_2.hash"), path(1, "deal_1.hash"), path(3, "deal_3.hash")]
    rc, io = _main(_receive_args(dirs, 2, out, hashes=hashes), capsys)
    assert rc == 1 and "dealer 1: hash check failed" in io.err and not os.path.exists(out)
    # a missing dealer
    rc, io = _main(_receive_args(dirs, 2, out, deals=[path(1, "deal_1.json"), path(3, "deal_3.json")],
                                 hashes=[path(1, "deal_1.hash"), path(3, "deal_3.hash")]), capsys)
    assert rc == 1 and "dealer 2: missing check failed" in io.err and not os.path.exists(out)
    # one flipped hex digit of dealer 3's sub-share to auditor 2, value 700 (the last digit: the value stays below r)
    sub = json.load(open(path(3, os.path.join("private", "subshare_3_to_2.json"))))
    y = sub["y"][700]
    sub["y"][700] = y[:-1] + "%x" % (int(y[-1], 16) ^ 1)
    changed = str(tmp_path / "subshare_3_to_2.json")
    json.dump(sub, open(changed, "w"))
    subs = [path(1, os.path.join("private", "subshare_1_to_2.json")), path(2, os.path.join("private", "subshare_2_to_2.json")), changed]
    rc, io = _main(_receive_args(dirs, 2, out, subs=subs), capsys)
    assert rc == 1 and "dealer 3: share check failed: value 700" in io.err and not os.path.exists(out)
    # a changed public file no longer has the published hash
    deal = open(path(2, "deal_2.json")).read()
    forged = str(tmp_path / "deal_2.json")
    open(forged, "w").write(deal.replace('"index": 2', '"index":  2'))
    rc, io = _main(_receive_args(dirs, 2, out, deals=[path(1, "deal_1.json"), forged, path(3, "deal_3.json")]), capsys)
    assert rc == 1 and "dealer 2: hash check failed" in io.err and not os.path.exists(out)


@pytest.mark.gpu
def test_dealt_key_opens_a_record_from_partials(received, tmp_path, capsys):
    """the files of a dealt key where an rlwe-keygen key's go: a record encrypted to the joint public key (the oracle's encryption,
    the public witness of its own commitments, `-`: verified elsewhere) is opened by audit-partial of auditors 1 and 3 and
    audit-open --partials, each auditor reading only its own directory's share"""
    import random
    from spp import cli, witness as W
    from oracle import rlwe, hashes as H
    outs, _ = received
    pk_a, pk_b = W.load_rlwe_pk_json(os.path.join(outs[1], "rlwe_pk.json"))
    owner = H.fixed_base_scalar_mul(777)
    rng = random.Random(6)
    r, e1, e2 = ([rng.randint(-3, 3) for _ in range(n)] for n in (1024, 64, 1024))
    c0, c1, _, _ = rlwe.rlwe_witness(pk_a, pk_b, r, e1, e2, rlwe.owner_msg(*owner))
    ct = H.poseidon2_sponge(rlwe.pack_values(c0) + rlwe.pack_values(c1))
    pw = (2).to_bytes(4, "big") + (0).to_bytes(4, "big") + (2).to_bytes(4, "big") + H.poseidon_hash2(*owner).to_bytes(32, "big") + ct.to_bytes(32, "big")
    proof, pwf, ctj = (str(tmp_path / n) for n in ("a.proof", "a.pw", "ciphertext.json"))
    open(proof, "wb").write(bytes(388)); open(pwf, "wb").write(pw)
    json.dump(W.ciphertext_json(c0, c1, owner), open(ctj, "w"))
    assert cli.main(["audit-pair-seeds", "--shares", str(M_), "--out", str(tmp_path)]) == 0
    share = lambda j: os.path.join(outs[j - 1], "rlwe_sk_shares", "share_%d.json" % j)
    seedf = lambda j: str(tmp_path / ("pair_seeds_%d.json" % j))
    part = lambda j: str(tmp_path / ("partial_%d.json" % j))
    assert cli.main(["audit-partial", share(1), "--with", "3", ctj, pwf, "--pair-seeds", seedf(1), "--out", part(1)]) == 0
    assert cli.main(["audit-partial", share(3), "--with", "1", ctj, pwf, "--pair-seeds", seedf(3), "--out", part(3)]) == 0
    capsys.readouterr()
    assert cli.main(["audit-open", "-", proof, pwf, ctj, "--partials", part(1), part(3)]) == 0
    out = capsys.readouterr().out
    assert "owner_x = 0x%064x" % owner[0] in out and "owner_y = 0x%064x" % owner[1] in out
    assert out.endswith("partials: combine to a decryption (2 auditors, no key rebuilt)\n")
