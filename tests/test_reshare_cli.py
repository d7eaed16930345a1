"""`spp.cli dkg-committee` / `dkg-reshare-deal` / `dkg-reshare-receive`: three auditors make a key and refresh it, two of them hand
it to a committee of five at threshold 3 through files, the new shares hold the secret of the unchanged public key, and a
forgotten refresh file, a stale share, a changed sub-share, a non-point, a missing dealer and a disagreeing set are each refused
by name with nothing written.  What is wrong with the arguments is found before a device is opened (the tests without the gpu
mark)."""
import json
import os

import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None

SEED = "5b" * 32
T, M_ = 2, 3
NT, NM = 3, 5
S = (1, 3)


def _main(argv, capsys):
    from spp import cli
    rc = cli.main([str(x) for x in argv])
    return rc, capsys.readouterr()


def _fake_files(tmp_path, kind="key"):
    """a deal file, a committee file and a sub-share file that parse (threshold 1 of 1, every point infinity): enough for the checks
    made before a device is opened"""
    deal = {"version": 1, "kind": kind, "index": 1, "threshold": 1, "num_shares": 1, "a_seed": SEED, "commitments": "00" * (1024 * 64)}
    if kind == "reshare":
        deal.update({"set": [1], "new_threshold": 1, "new_shares": 2})
    com = {"version": 1, "threshold": 1, "num_shares": 1, "xs": [1], "a_seed": SEED, "noise_bound": 3, "commitments": "00" * (1024 * 64)}
    sub = {"from": 1, "to": 1, "y": ["%064x" % 0] * 1024, "y_blind": ["%064x" % 0] * 1024}
    paths = [str(tmp_path / n) for n in ("deal_%s.json" % kind, "committee.json", "subshare_1_to_1.json")]
    for p, d in zip(paths, (deal, com, sub)):
        json.dump(d, open(p, "w"))
    return paths


def test_sizes_and_arguments_are_refused_before_any_file_is_read(tmp_path, capsys):
    out = str(tmp_path / "d")
    base = ["dkg-reshare-deal", "--share", "none.json", "--blind", "none.json", "--committee", "none.json", "--set", 1, 2, "--out", out]
    for t, m in ((0, 3), (65, 70), (4, 3), (3, 256)):
        rc, io = _main(base + ["--new-threshold", t, "--new-shares", m], capsys)
        assert rc == 2 and "1 <= threshold <= 64" in io.err and not os.path.exists(out), (t, m)
    rc, io = _main(["dkg-reshare-deal", "--share", "none.json", "--committee", "none.json", "--set", 1, 2, "--new-threshold", 2, "--new-shares", 12,
                    "--out", out], capsys)
    assert rc == 2 and "--blind" in io.err and "--subshares" in io.err and not os.path.exists(out)
    rc, io = _main(base + ["--new-threshold", 2, "--new-shares", 12], capsys)          # 12 members pass the size check: the files are read next
    assert rc == 2 and "none.json" in io.err and "threshold <= shares" not in io.err
    with pytest.raises(SystemExit):
        _main(["dkg-reshare-deal", "--help"], capsys)
    assert "noise" in capsys.readouterr().out


def test_committee_kinds_and_indices_are_refused_before_a_device_is_opened(tmp_path, capsys):
    out = str(tmp_path / "committee_out.json")
    key, com, sub = _fake_files(tmp_path, "key")
    rc, io = _main(["dkg-committee", "--deals", key, "--base", com, "--out", out], capsys)
    assert rc == 2 and "--base is for refresh dealings" in io.err
    refresh = _fake_files(tmp_path, "refresh")[0]
    rc, io = _main(["dkg-committee", "--deals", refresh, "--out", out], capsys)
    assert rc == 2 and "give --base" in io.err
    reshare = _fake_files(tmp_path, "reshare")[0]
    rc, io = _main(["dkg-committee", "--deals", reshare, "--out", out], capsys)
    assert rc == 2 and "dkg-reshare-receive" in io.err
    rc, io = _main(["dkg-committee", "--deals", com, "--out", out], capsys)
    assert rc == 2 and "not a deal file" in io.err
    rdir = str(tmp_path / "r")
    for k in (0, 3):
        rc, io = _main(["dkg-reshare-receive", "--index", k, "--committee", com, "--deals", reshare, "--subshares", sub, "--out", rdir], capsys)
        assert rc == 2 and ("addressed to auditor" in io.err or "1..2" in io.err)
    rc, io = _main(["dkg-reshare-receive", "--index", 1, "--committee", com, "--deals", key, "--subshares", sub, "--out", rdir], capsys)
    assert rc == 2 and "reshare_<j>.json" in io.err
    rc, io = _main(["dkg-reshare-receive", "--index", 1, "--committee", key, "--deals", reshare, "--subshares", sub, "--out", rdir], capsys)
    assert rc == 2 and "not a committee file" in io.err
    assert not os.path.exists(out) and not os.path.exists(rdir)


@pytest.fixture(scope="module")
def keyed(tmp_path_factory):
    """three auditors: a key round and a refresh round through dkg-deal / dkg-receive, and the committee file of each"""
    from spp import cli
    root = tmp_path_factory.mktemp("reshare")
    run = lambda argv: cli.main([str(x) for x in argv])
    order = range(1, M_ + 1)
    d = {"root": root, "deal": [str(root / ("deal_%d" % i)) for i in order], "key": [str(root / ("key_%d" % j)) for j in order],
         "rdeal": [str(root / ("refresh_%d" % i)) for i in order], "renewed": [str(root / ("renewed_%d" % j)) for j in order],
         "committee0": str(root / "committee_0.json"), "committee": str(root / "committee_1.json")}
    files = lambda dirs, ext: [os.path.join(dirs[i - 1], "deal_%d.%s" % (i, ext)) for i in order]
    subs = lambda dirs, j: [os.path.join(dirs[i - 1], "private", "subshare_%d_to_%d.json" % (i, j)) for i in order]
    for i in order:
        assert run(["dkg-deal", "--index", i, "--threshold", T, "--shares", M_, "--a-seed", SEED, "--out", d["deal"][i - 1]]) == 0
    for j in order:
        assert run(["dkg-receive", "--index", j, "--deals"] + files(d["deal"], "json") + ["--hashes"] + files(d["deal"], "hash")
                   + ["--subshares"] + subs(d["deal"], j) + ["--out", d["key"][j - 1]]) == 0
    assert run(["dkg-committee", "--deals"] + files(d["deal"], "json") + ["--out", d["committee0"]]) == 0
    for i in order:
        assert run(["dkg-deal", "--index", i, "--threshold", T, "--shares", M_, "--a-seed", SEED, "--out", d["rdeal"][i - 1], "--refresh"]) == 0
    for j in order:
        assert run(["dkg-receive", "--index", j, "--deals"] + files(d["rdeal"], "json") + ["--hashes"] + files(d["rdeal"], "hash")
                   + ["--subshares"] + subs(d["rdeal"], j) + ["--out", d["renewed"][j - 1], "--refresh",
                                                               os.path.join(d["key"][j - 1], "rlwe_sk_shares", "share_%d.json" % j)]) == 0
    assert run(["dkg-committee", "--deals"] + files(d["rdeal"], "json") + ["--base", d["committee0"], "--out", d["committee"]]) == 0
    d["subs"], d["files"] = subs, files
    d["share"] = lambda j: os.path.join(d["renewed"][j - 1], "rlwe_sk_shares", "share_%d.json" % j)
    d["old_share"] = lambda j: os.path.join(d["key"][j - 1], "rlwe_sk_shares", "share_%d.json" % j)
    return d


def _deal_args(d, j, out, t=NT, m=NM, subs=None, share=None, committee=None, sset=S):
    subs = d["subs"](d["deal"], j) + d["subs"](d["rdeal"], j) if subs is None else subs
    return (["dkg-reshare-deal", "--share", share or d["share"](j), "--subshares"] + subs + ["--committee", committee or d["committee"], "--set"]
            + list(sset) + ["--new-threshold", t, "--new-shares", m, "--out", out])


@pytest.fixture(scope="module")
def handed(keyed):
    """old members 1 and 3 deal to (3, 5); new members 1, 2 and 4 receive"""
    from spp import cli
    d = keyed
    d["hand"] = {j: str(d["root"] / ("hand_%d" % j)) for j in S}
    for j in S:
        assert cli.main([str(x) for x in _deal_args(d, j, d["hand"][j])]) == 0
    d["new"] = {k: str(d["root"] / ("new_%d" % k)) for k in (1, 2, 4)}
    for k, out in d["new"].items():
        assert cli.main([str(x) for x in _receive_args(d, k, out)]) == 0
    return d


def _receive_args(d, k, out, deals=None, subs=None, committee=None):
    deals = deals or [os.path.join(d["hand"][j], "reshare_%d.json" % j) for j in S]
    subs = subs or [os.path.join(d["hand"][j], "private", "subshare_%d_to_%d.json" % (j, k)) for j in S]
    return ["dkg-reshare-receive", "--index", k, "--committee", committee or d["committee"], "--deals"] + deals + ["--subshares"] + subs + ["--out", out]


@pytest.mark.gpu
def test_round_trip(handed, tmp_path, capsys):
    from spp import witness
    d = handed
    com0, com1 = json.load(open(d["committee0"])), json.load(open(d["committee"]))
    assert sorted(com0) == ["a_seed", "commitments", "noise_bound", "num_shares", "threshold", "version", "xs"]
    assert (com0["threshold"], com0["num_shares"], com0["xs"], com0["a_seed"], com0["noise_bound"]) == (T, M_, [1, 2, 3], SEED, 3 * M_)
    assert len(com0["commitments"]) == 2 * T * 1024 * 64
    assert (com1["threshold"], com1["num_shares"], com1["noise_bound"]) == (T, M_, 3 * M_) and com1["commitments"] != com0["commitments"]
    for j in S:
        assert sorted(os.listdir(d["hand"][j])) == ["private", "reshare_%d.json" % j]
        assert sorted(os.listdir(os.path.join(d["hand"][j], "private"))) == ["subshare_%d_to_%d.json" % (j, k) for k in range(1, NM + 1)]
        deal = json.load(open(os.path.join(d["hand"][j], "reshare_%d.json" % j)))
        assert sorted(deal) == ["a_seed", "commitments", "index", "kind", "new_shares", "new_threshold", "num_shares", "set", "threshold", "version"]
        assert (deal["kind"], deal["index"], deal["set"], deal["threshold"], deal["num_shares"], deal["new_threshold"], deal["new_shares"]) \
            == ("reshare", j, list(S), T, M_, NT, NM)
    pk = os.path.join(d["key"][0], "rlwe_pk.json")
    coms = []
    for k, out in d["new"].items():
        assert sorted(os.listdir(out)) == ["committee.json", "private", "rlwe_params.json", "rlwe_sk_shares"]   # no rlwe_pk.json: the key stays
        assert os.listdir(os.path.join(out, "private")) == ["blind_%d.json" % k]
        assert os.listdir(os.path.join(out, "rlwe_sk_shares")) == ["share_%d.json" % k]
        params = json.load(open(os.path.join(out, "rlwe_params.json")))
        assert (params["threshold"], params["num_shares"], params["noise_bound"]) == (NT, NM, 3 * M_)
        sh = witness.load_share_json(os.path.join(out, "rlwe_sk_shares", "share_%d.json" % k))
        assert (sh["x"], sh["threshold"]) == (k, NT)
        coms.append(open(os.path.join(out, "committee.json")).read())
    assert coms[0] == coms[1] == coms[2]
    new_com = json.loads(coms[0])
    assert (new_com["threshold"], new_com["num_shares"]) == (NT, NM) and len(new_com["commitments"]) == 2 * NT * 1024 * 64
    assert new_com["commitments"][:2 * 1024 * 64] == com1["commitments"][:2 * 1024 * 64]          # D'_0 == D_0: this key
    new_share = lambda k: os.path.join(d["new"][k], "rlwe_sk_shares", "share_%d.json" % k)
    rc, io = _main(["rlwe-key-check", pk, "--shares", new_share(1), new_share(2), new_share(4)], capsys)
    assert rc == 0 and "the shares hold the secret of this public key" in io.out, io.out + io.err
    rc, io = _main(["rlwe-key-check", pk, "--shares", d["share"](2), new_share(1), new_share(4)], capsys)
    assert rc == 1, "an old share and new ones are not shares of one key"
    # the blind file takes the place of the sub-share files at the next hand-over: new member 2 deals on, back to (2, 3)
    back = str(tmp_path / "back")
    rc, io = _main(["dkg-reshare-deal", "--share", new_share(2), "--blind", os.path.join(d["new"][2], "private", "blind_2.json"), "--committee",
                    os.path.join(d["new"][2], "committee.json"), "--set", 2, 4, 5, "--new-threshold", 2, "--new-shares", 3, "--out", back], capsys)
    assert rc == 0 and os.path.exists(os.path.join(back, "reshare_2.json")), io.err


@pytest.mark.gpu
def test_twelve_members_where_dkg_deal_refuses_them(keyed, tmp_path, capsys):
    d, out = keyed, str(tmp_path / "twelve")
    rc, io = _main(["dkg-deal", "--index", 1, "--threshold", 2, "--shares", 12, "--a-seed", SEED, "--out", out], capsys)
    assert rc == 2 and not os.path.exists(out)
    rc, io = _main(_deal_args(d, 1, out, t=7, m=12), capsys)
    assert rc == 0, io.err
    assert len(os.listdir(os.path.join(out, "private"))) == 12
    assert len(json.load(open(os.path.join(out, "reshare_1.json")))["commitments"]) == 2 * 7 * 1024 * 64


@pytest.mark.gpu
def test_share_mismatch_when_a_refresh_file_is_left_out(keyed, tmp_path, capsys):
    d, out = keyed, str(tmp_path / "mismatch")
    subs = d["subs"](d["deal"], 1) + d["subs"](d["rdeal"], 1)[:-1]                   # dealer 3's refresh sub-share forgotten
    rc, io = _main(_deal_args(d, 1, out, subs=subs), capsys)
    assert rc == 1 and "share-mismatch" in io.err and "refresh" in io.err and not os.path.exists(out)
    rc, io = _main(_deal_args(d, 1, out, share=d["old_share"](1)), capsys)           # the share from before the refresh
    assert rc == 1 and "share-mismatch" in io.err and not os.path.exists(out)
    rc, io = _main(_deal_args(d, 1, out, sset=(2, 3)), capsys)                       # not a member of the set
    assert rc == 2 and "--set" in io.err and not os.path.exists(out)
    rc, io = _main(_deal_args(d, 1, out, sset=(1, 2, 3)), capsys)                    # not exactly the threshold
    assert rc == 2 and "--set" in io.err and not os.path.exists(out)


@pytest.mark.gpu
def test_refusals_name_the_member_and_write_nothing(handed, tmp_path, capsys):
    d, out = handed, str(tmp_path / "refused")
    deal = lambda j: os.path.join(d["hand"][j], "reshare_%d.json" % j)
    sub = lambda j, k: os.path.join(d["hand"][j], "private", "subshare_%d_to_%d.json" % (j, k))

    def edited(path, name, change):
        obj = json.load(open(path))
        change(obj)
        new = str(tmp_path / name)
        json.dump(obj, open(new, "w"))
        return new

    # share: one flipped hex digit of member 3's sub-share to new member 2, value 700
    def flip(o):
        o["y"][700] = o["y"][700][:-1] + "%x" % (int(o["y"][700][-1], 16) ^ 1)
    rc, io = _main(_receive_args(d, 2, out, subs=[sub(1, 2), edited(sub(3, 2), "subshare_3_to_2.json", flip)]), capsys)
    assert rc == 1 and "old member 3: share check failed: value 700" in io.err and not os.path.exists(out)
    # point: the first commitment of member 1 is no point
    def unpoint(o):
        o["commitments"] = "ff" * 32 + o["commitments"][64:]
    rc, io = _main(_receive_args(d, 2, out, deals=[edited(deal(1), "reshare_1.json", unpoint), deal(3)]), capsys)
    assert rc == 1 and "old member 1: point check failed: value 0" in io.err and not os.path.exists(out)
    # missing: member 3's deal file, member 1's sub-share, a file twice
    rc, io = _main(_receive_args(d, 2, out, deals=[deal(1)]), capsys)
    assert rc == 1 and "old member 3: missing check failed" in io.err and not os.path.exists(out)
    rc, io = _main(_receive_args(d, 2, out, subs=[sub(3, 2)]), capsys)
    assert rc == 1 and "old member 1: missing check failed" in io.err and not os.path.exists(out)
    rc, io = _main(_receive_args(d, 2, out, deals=[deal(1), deal(3), deal(3)]), capsys)
    assert rc == 1 and "old member 3: missing check failed: dealt twice" in io.err and not os.path.exists(out)
    # set: the deals disagree on S; |S| is not the old threshold
    def other_set(o):
        o["set"] = [2, 3]
    rc, io = _main(_receive_args(d, 2, out, deals=[deal(1), edited(deal(3), "reshare_3.json", other_set)]), capsys)
    assert rc == 1 and "old member 3: set check failed" in io.err and not os.path.exists(out)
    def big_set(o):
        o["set"] = [1, 2, 3]
    rc, io = _main(_receive_args(d, 2, out, deals=[edited(deal(1), "r1.json", big_set), edited(deal(3), "r3.json", big_set)]), capsys)
    assert rc == 1 and "set check failed" in io.err and not os.path.exists(out)
    # agreement: another new threshold
    def other_t(o):
        o["new_threshold"] = 2
    rc, io = _main(_receive_args(d, 2, out, deals=[deal(1), edited(deal(3), "r3t.json", other_t)]), capsys)
    assert rc == 1 and "old member 3: agreement check failed" in io.err and not os.path.exists(out)
    # not-share: member 3 deals the share it held BEFORE the refresh (it checks against the committee file of that time); against
    # the current committee file its constant terms are not its share commitments, though every sub-share matches its own dealing
    stale = str(tmp_path / "stale")
    rc, io = _main(_deal_args(d, 3, stale, subs=d["subs"](d["deal"], 3), share=d["old_share"](3), committee=d["committee0"]), capsys)
    assert rc == 0, io.err
    rc, io = _main(_receive_args(d, 2, out, deals=[deal(1), os.path.join(stale, "reshare_3.json")],
                                 subs=[sub(1, 2), os.path.join(stale, "private", "subshare_3_to_2.json")]), capsys)
    assert rc == 1 and "old member 3: not-share check failed: value 0 (1024 values refused in all)" in io.err and not os.path.exists(out)


@pytest.mark.gpu
def test_committee_refusals(keyed, tmp_path, capsys):
    d, out = keyed, str(tmp_path / "committee.json")
    files = d["files"](d["deal"], "json")
    rc, io = _main(["dkg-committee", "--deals"] + files[:2] + ["--out", out], capsys)
    assert rc == 1 and "dealer 3: missing check failed" in io.err and not os.path.exists(out)
    rc, io = _main(["dkg-committee", "--deals"] + files[:2] + [d["files"](d["rdeal"], "json")[2], "--out", out], capsys)
    assert rc == 1 and "dealer 3: agreement check failed" in io.err and not os.path.exists(out)
    obj = json.load(open(files[1]))
    at = 2 * 64 * (1024 + 5)                                                         # coefficient 1 of value 5
    obj["commitments"] = obj["commitments"][:at] + "ff" * 32 + obj["commitments"][at + 64:]
    forged = str(tmp_path / "deal_2.json")
    json.dump(obj, open(forged, "w"))
    rc, io = _main(["dkg-committee", "--deals", files[0], forged, files[2], "--out", out], capsys)
    assert rc == 1 and "dealer 2: point check failed: value 5, coefficient 1" in io.err and not os.path.exists(out)
