"""Auditor key generation, host side (no GPU): csrc/rlwe_keygen.hpp compiled for the host and run lane by lane against the
schoolbook product (plain and under ASan + UBSan, stand-alone), the C declarations, exports and ctypes signatures of the four
calls, their refusals before any device work, the host-only sampler, the files of scripts/rlwe_keygen.py, and the argument errors
of `spp rlwe-keygen` / `spp rlwe-key-check`."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import rlwe_keygen_vectors as V

Q, R = V.Q, V.R
CSRC = os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd", "csrc")
CHECK = os.path.join(ROOT, "tests", "host", "rlwe_keygen_check.cpp")
CALLS = ("spp_rlwe_sample_key", "spp_rlwe_keygen_batch", "spp_rlwe_key_check", "spp_shamir_split")
BAD_INPUT = -1


@pytest.fixture(scope="module")
def key_file(tmp_path_factory):
    """the committed fixture key as the file of integers the host check reads: sk, a, e, and the reference's b"""
    k = V.fixture_key()
    path = str(tmp_path_factory.mktemp("rlwe_keygen") / "key.txt")
    with open(path, "w") as f:
        for part in ("sk", "a", "e", "b"):
            f.write(" ".join(str(v) for v in k[part]) + "\n")
    return path


def _run_check(tmp_path, key_file, flags, name):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-I", CSRC, CHECK, "-o", exe] + flags, check=True)
    out = subprocess.run([exe, key_file], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-600:] + out.stderr[-600:]
    lines = out.stdout.strip().split("\n")
    assert lines[-1].startswith("OK rlwe_keygen: 10 keys"), lines[-1]
    for case in ("random key", "sk = 0", "sk = +3, a = q - 1", "sk = -3", "a = 0", "sk = X^1023, e = -3", "the reference's key"):
        assert any(re.fullmatch(re.escape(case) + r"\s+ok", ln) for ln in lines), case
    m = re.search(r"largest \|intermediate\| met: (\d+) ", out.stdout)
    assert m and 0 < int(m.group(1)) < 2 ** 31
    return int(m.group(1))


def test_keygen_header_on_the_host_against_the_schoolbook_product(tmp_path, key_file):
    """The phases k_rlwe_keygen and k_rlwe_key_noise run, lane by lane under g++: random keys, sk = 0, sk = +3 with a = q - 1,
    sk = -3, a = 0, sk = X^1023 with e = -3, and the committed fixture key, whose b must be tests/golden/rlwe_pk.json's."""
    _run_check(tmp_path, key_file, ["-O2"], "rlwe_keygen_check")


def test_keygen_header_under_asan_ubsan(tmp_path, key_file):
    """the same program, stand-alone, with -fsanitize=address,undefined: a signed overflow anywhere in the chain aborts it"""
    _run_check(tmp_path, key_file, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"],
               "rlwe_keygen_check_san")


def test_header_declares_the_four_calls():
    hdr = open(os.path.join(ROOT, "include", "spp.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert "int spp_rlwe_sample_key(size_t count, uint32_t bound, int8_t* sk, uint32_t* a, int8_t* e);" in flat
    assert ("int spp_rlwe_keygen_batch(spp_ctx* ctx, size_t count, const int8_t* sk, const uint32_t* a, const int8_t* e, uint32_t* pk_b, "
            "uint32_t* sk_mod_q);") in flat
    assert ("int spp_rlwe_key_check(spp_ctx* ctx, size_t count, const uint32_t* pk_a, const uint32_t* pk_b, const uint32_t* sk_mod_q, "
            "uint32_t* max_abs);") in flat
    assert ("int spp_shamir_split(spp_ctx* ctx, uint32_t t, uint32_t m, const uint32_t* xs, size_t n, const uint8_t* secrets_be, "
            "const uint8_t* coeffs_be, uint8_t* ys);") in flat
    # the reference interfaces the calls replace are named in the header's index
    assert "rlwe_keygen.py:98-182" in hdr and ":51-65" in hdr


def test_library_exports_the_calls_and_lib_py_sets_their_argtypes():
    import spp
    from spp import witness
    L = spp.load_library()
    for name, nargs in zip(CALLS, (5, 7, 6, 8)):
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == nargs, name
    for name in ("rlwe_keygen", "rlwe_key_check", "shamir_split", "write_rlwe_pk_json", "write_rlwe_params_json", "write_share_json"):
        assert callable(getattr(witness, name)), name


def _fake_ctx():
    """something that is not NULL where a context goes: every refusal below is made before the context is touched"""
    return ctypes.create_string_buffer(4096)


def test_calls_refuse_null_arguments_without_a_device():
    import spp
    L = spp.load_library()
    buf = ctypes.create_string_buffer(8192)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.spp_rlwe_sample_key(1, 3, None, p, p) == BAD_INPUT and "NULL" in spp.last_error()
    assert L.spp_rlwe_sample_key(1, 3, p, None, p) == BAD_INPUT
    assert L.spp_rlwe_sample_key(1, 3, p, p, None) == BAD_INPUT
    assert L.spp_rlwe_keygen_batch(None, 1, p, p, p, p, None) == BAD_INPUT and "NULL" in spp.last_error()
    fake = _fake_ctx()
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert L.spp_rlwe_keygen_batch(fake, 1, *args, None) == BAD_INPUT and "NULL" in spp.last_error()
    assert L.spp_rlwe_key_check(None, 1, p, p, p, p) == BAD_INPUT and "NULL" in spp.last_error()
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert L.spp_rlwe_key_check(fake, 1, *args) == BAD_INPUT and "NULL" in spp.last_error()
    assert L.spp_shamir_split(None, 2, 3, None, 1, buf.raw[:32], None, p) == BAD_INPUT and "NULL" in spp.last_error()
    assert L.spp_shamir_split(fake, 2, 3, None, 1, None, None, p) == BAD_INPUT and "NULL" in spp.last_error()
    assert L.spp_shamir_split(fake, 2, 3, None, 1, buf.raw[:32], None, None) == BAD_INPUT and "NULL" in spp.last_error()


def test_range_and_shape_errors_are_refused_before_the_context_is_touched():
    import spp
    L = spp.load_library()
    fake = _fake_ctx()
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    sk = np.zeros(2048, dtype=np.int8)
    e = np.zeros(2048, dtype=np.int8)
    a = np.zeros(2048, dtype=np.uint32)
    out = np.zeros(2048, dtype=np.uint32)
    mx = np.zeros(4, dtype=np.uint32)
    # sampler: bound outside [1, 127], count > 2^16
    for bound in (0, 128, 1 << 31):
        assert L.spp_rlwe_sample_key(1, bound, p(sk), p(a), p(e)) == BAD_INPUT and "bound" in spp.last_error()
    assert L.spp_rlwe_sample_key((1 << 16) + 1, 3, p(sk), p(a), p(e)) == BAD_INPUT and "2^16" in spp.last_error()
    # keygen: a value >= q, named by its index; count > 2^16
    a[1500] = Q
    assert L.spp_rlwe_keygen_batch(fake, 2, p(sk), p(a), p(e), p(out), None) == BAD_INPUT
    assert "a[1500]" in spp.last_error()
    assert L.spp_rlwe_keygen_batch(fake, (1 << 16) + 1, p(sk), p(a), p(e), p(out), None) == BAD_INPUT and "2^16" in spp.last_error()
    a[1500] = 0
    # key check: each of the three polynomials
    for k, name in enumerate(("pk_a", "pk_b", "sk_mod_q")):
        polys = [np.zeros(2048, dtype=np.uint32) for _ in range(3)]
        polys[k][1029] = 0xffffffff
        assert L.spp_rlwe_key_check(fake, 2, p(polys[0]), p(polys[1]), p(polys[2]), p(mx)) == BAD_INPUT
        assert "%s[1029]" % name in spp.last_error()
    assert L.spp_rlwe_key_check(fake, (1 << 16) + 1, p(a), p(a), p(a), p(mx)) == BAD_INPUT and "2^16" in spp.last_error()
    # sharing: thresholds, share counts, indices, sizes, field elements
    be = lambda vals: b"".join(int(v).to_bytes(32, "big") for v in vals)
    ys = ctypes.create_string_buffer(255 * 4 * 32)
    split = lambda t, m, xs, n, sec, co: L.spp_shamir_split(fake, t, m, None if xs is None else (ctypes.c_uint32 * len(xs))(*xs), n, sec, co,
                                                            ctypes.cast(ys, ctypes.c_void_p))
    sec = be([1, 2, 3, R - 1])
    for t, m in ((0, 3), (65, 70), (3, 2), (2, 256)):
        assert split(t, m, None, 4, sec, None) == BAD_INPUT, (t, m)
    assert split(2, 3, [1, 0, 3], 4, sec, None) == BAD_INPUT and "xs[1]" in spp.last_error()
    assert split(2, 3, [5, 7, 5], 4, sec, None) == BAD_INPUT and "xs[2]" in spp.last_error()
    assert split(2, 3, None, (1 << 20) + 1, sec, None) == BAD_INPUT and "2^20" in spp.last_error()
    assert split(2, 3, None, 4, be([1, 2, R, 3]), None) == BAD_INPUT and "secret 2" in spp.last_error()
    assert split(3, 3, None, 4, sec, be([0, 1, 2, 3, 4, R + 5, 6, 7])) == BAD_INPUT and "coefficient 5" in spp.last_error()
    # nothing to do is SPP_OK, still without a device
    assert L.spp_rlwe_keygen_batch(fake, 0, p(sk), p(a), p(e), p(out), None) == 0
    assert L.spp_rlwe_key_check(fake, 0, p(a), p(a), p(a), p(mx)) == 0
    assert split(2, 3, None, 0, sec, None) == 0
    assert L.spp_rlwe_sample_key(0, 3, p(sk), p(a), p(e)) == 0


@pytest.mark.parametrize("bound", [1, 3, 127])
def test_sample_key_ranges(bound):
    import spp
    from spp import witness
    sk, a, e = witness.rlwe_sample_key(spp.load_library(), 2, bound)
    assert sk.shape == a.shape == e.shape == (2, 1024)
    for s in (sk, e):
        assert int(s.min()) >= -bound and int(s.max()) <= bound
    assert int(a.max()) < Q
    assert int(a.max()) > Q // 2          # 2048 uniform draws all in the lower half: probability 2^-2048


def test_sample_key_draws_differ_and_cover_the_range():
    import spp
    from spp import witness
    L = spp.load_library()
    one, two = witness.rlwe_sample_key(L, 1, 3), witness.rlwe_sample_key(L, 1, 3)
    for x, y in zip(one, two):
        assert not np.array_equal(x, y)
    # every value of [-3, 3] in 1024 draws: a value is missed with probability 7 * (6/7)^1024 < 2^-224
    for s in (one[0], one[2]):
        assert sorted(set(int(v) for v in s[0])) == [-3, -2, -1, 0, 1, 2, 3]


def test_share_json_round_trip(tmp_path):
    from spp import witness as W
    ys = [0, 1, R - 1] + [(i * 0x9E3779B97F4A7C15 + 12345) % R for i in range(3, 1024)]
    path = str(tmp_path / "share_2.json")
    W.write_share_json(path, 2, 2, 3, 2, ys)
    d = json.load(open(path))
    assert list(d) == ["share_index", "threshold", "num_shares", "coefficients"]
    assert (d["share_index"], d["threshold"], d["num_shares"]) == (2, 2, 3)
    assert d["coefficients"][0] == {"x": 2, "y": "0x0"}                         # to_hex_bn254: zero is "0x0"
    assert d["coefficients"][1] == {"x": 2, "y": "0x" + "0" * 63 + "1"}
    assert all(len(c["y"]) == 66 for c in d["coefficients"][1:])
    back = W.load_share_json(path)
    assert back == {"x": 2, "y": ys, "share_index": 2, "threshold": 2}
    with pytest.raises(ValueError):
        W.write_share_json(path, 1, 2, 3, 1, [R])
    with pytest.raises(ValueError):
        W.write_share_json(path, 1, 2, 3, 0, [1])


def test_pk_json_is_read_by_the_reader_of_cli_compile(tmp_path):
    """write_rlwe_pk_json -> the expression `spp compile audit --rlwe-pk` builds its aux vector with"""
    from spp import cli, witness as W
    k = V.fixture_key()
    path = str(tmp_path / "rlwe_pk.json")
    W.write_rlwe_pk_json(path, k["a"], k["b"])
    pk = json.load(open(path))
    assert list(pk) == ["a", "b"] and all(re.fullmatch(r"0x[0-9a-f]{8}", v) for v in pk["a"] + pk["b"])
    assert [cli._num(str(x)) for x in pk["a"]] + [cli._num(str(x)) for x in pk["b"]] == k["a"] + k["b"]
    assert W.load_rlwe_pk_json(path) == (k["a"], k["b"])
    assert W.load_rlwe_pk_json(os.path.join(ROOT, "tests", "golden", "rlwe_pk.json")) == (k["a"], k["b"])
    with pytest.raises(ValueError):
        W.write_rlwe_pk_json(path, k["a"][:-1] + [Q], k["b"])
    params = str(tmp_path / "rlwe_params.json")
    W.write_rlwe_params_json(params, 2, 3)
    assert json.load(open(params)) == {"N": 1024, "q": Q, "noise_bound": 3, "plaintext_modulus": 256, "delta": Q // 256, "threshold": 2,
                                       "num_shares": 3, "field": "BN254"}
    assert open(params).read().startswith('{\n  "N": 1024,')                     # indent=2, the reference's key order


def test_fixture_shares_serialise_to_the_reference_field_names(tmp_path):
    """the shares rebuilt from the fixture (share 1 + the derived degree-1 coefficients, in Python integers) are the fixture's, and
    share_json gives them the reference's field names and hex form"""
    from spp import witness as W
    k = V.fixture_key()
    shares = [[(s + c * x) % R for s, c in zip(k["sk"], k["c1"])] for x in (1, 2, 3)]
    assert shares[0] == k["y1"] and shares[1] == k["y2"] and shares[2][:4] == k["share3_head"]
    for idx, fx in zip((1, 2), k["shares"]):
        d = W.share_json(idx, 2, 3, idx, shares[idx - 1])
        assert set(d) == {"share_index", "threshold", "num_shares", "coefficients"} and d["num_shares"] == 3
        assert (d["share_index"], d["threshold"]) == (fx["share_index"], fx["threshold"])
        assert [c["x"] for c in d["coefficients"]] == [fx["x"]] * 1024
        assert [c["y"] for c in d["coefficients"]] == fx["y"]                      # the same strings the reference wrote
    # random.Random(42) in the reference's order gives this very key
    sk, a, e, coeffs = W.reference_key_draws(42)
    assert (sk, a, e, coeffs) == (k["sk"], k["a"], k["e"], [k["c1"]])


def test_cli_argument_errors_touch_no_device(tmp_path, monkeypatch, capsys):
    from spp import cli, witness as W, prover
    def no_device(*a, **k):
        raise AssertionError("a device context was opened")
    monkeypatch.setattr(cli, "Context", no_device)
    monkeypatch.setattr(prover.Context, "__init__", no_device)
    k = V.fixture_key()
    out = str(tmp_path / "keys")
    for argv in (["rlwe-keygen"], ["rlwe-keygen", "--out", out, "--threshold", "x"], ["rlwe-key-check", "pk.json"],
                 ["rlwe-key-check", "--shares", "s.json"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code != 0
    for t, m in ((0, 3), (3, 2), (65, 70), (2, 256)):
        assert cli.main(["rlwe-keygen", "--out", out, "--threshold", str(t), "--shares", str(m)]) != 0
    assert not os.path.exists(out)                                                # refused before anything is written
    blocker = str(tmp_path / "file")
    open(blocker, "w").write("x")
    assert cli.main(["rlwe-keygen", "--out", os.path.join(blocker, "keys")]) != 0   # DIR cannot be made
    assert "rlwe-keygen" in capsys.readouterr().err
    pk = str(tmp_path / "rlwe_pk.json")
    W.write_rlwe_pk_json(pk, k["a"], k["b"])
    sh = []
    for idx, ys in ((1, k["y1"]), (2, k["y2"])):
        sh.append(str(tmp_path / ("share_%d.json" % idx)))
        W.write_share_json(sh[-1], idx, 2, 3, idx, ys)
    assert cli.main(["rlwe-key-check", pk, "--shares", sh[0]]) != 0                # one share of a 2-of-3 key
    assert cli.main(["rlwe-key-check", pk, "--shares", sh[0], sh[0]]) != 0         # the same share twice
    assert cli.main(["rlwe-key-check", str(tmp_path / "none.json"), "--shares"] + sh) != 0
    assert cli.main(["rlwe-key-check", pk, "--shares", sh[0], str(tmp_path / "none.json")]) != 0
    assert cli.main(["rlwe-key-check", pk, "--params", str(tmp_path / "none.json"), "--shares"] + sh) != 0
    bad = str(tmp_path / "bad_pk.json")
    json.dump({"a": [1, 2, 3]}, open(bad, "w"))
    assert cli.main(["rlwe-key-check", bad, "--shares"] + sh) != 0                 # not an rlwe_pk.json
    json.dump({"a": k["a"], "b": k["b"][:-1] + [Q]}, open(bad, "w"))
    assert cli.main(["rlwe-key-check", bad, "--shares"] + sh) != 0                 # a coefficient equal to q
    assert "rlwe-key-check" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        cli.main(["rlwe-keygen", "--help"])
    text = re.sub(r"\s+", " ", capsys.readouterr().out)
    assert e.value.code == 0 and "--reference-seed" in text and "fixtures only" in text and "NEVER a key to use" in text
