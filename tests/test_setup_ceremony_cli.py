"""`spp.cli setup-contribute` / `setup-verify`: what is wrong with the arguments or the files is found before a device is opened
(exit 2, a message on stderr), so none of this needs a GPU."""
import os

import pytest


def _main(argv, capsys):
    from spp import cli
    rc = cli.main(argv)
    return rc, capsys.readouterr()


@pytest.fixture()
def files(tmp_path):
    paths = {}
    for name in ("k0.pk", "k0.vk", "k1.pk", "k1.vk", "k1.receipt", "k2.pk", "k2.vk", "k2.receipt"):
        paths[name] = str(tmp_path / name)
        with open(paths[name], "wb") as f:
            f.write(b"\0" * 8)
    return paths


def test_chain_arguments_are_grouped_by_link():
    from spp import cli
    assert cli.parse_ceremony_chain(["pk0", "vk0", "pk1", "vk1", "r1"]) == [("pk0", "vk0", "pk1", "vk1", "r1")]
    assert cli.parse_ceremony_chain(["pk0", "vk0", "pk1", "vk1", "r1", "pk2", "vk2", "r2"]) == [("pk0", "vk0", "pk1", "vk1", "r1"),
                                                                                              ("pk1", "vk1", "pk2", "vk2", "r2")]
    for n in (1, 2, 3, 4, 6, 7, 9, 10):
        with pytest.raises(ValueError):
            cli.parse_ceremony_chain(["f%d" % i for i in range(n)])


@pytest.mark.parametrize("n", [2, 4, 6, 7])
def test_setup_verify_refuses_a_chain_that_is_no_chain(files, capsys, n):
    order = ["k0.pk", "k0.vk", "k1.pk", "k1.vk", "k1.receipt", "k2.pk", "k2.vk", "k2.receipt"]
    rc, io = _main(["setup-verify"] + [files[k] for k in order[:n]], capsys)
    assert rc == 2 and "triples" in io.err and io.out == ""


def test_setup_verify_names_a_missing_file(files, capsys):
    missing = files["k1.vk"] + ".nowhere"
    rc, io = _main(["setup-verify", files["k0.pk"], files["k0.vk"], files["k1.pk"], missing, files["k1.receipt"]], capsys)
    assert rc == 2 and missing in io.err and io.out == ""


def test_setup_contribute_checks_its_arguments_first(files, tmp_path, capsys):
    out = str(tmp_path / "out")
    rc, io = _main(["setup-contribute", files["k0.pk"] + ".nowhere", files["k0.vk"], "--out", out], capsys)
    assert rc == 2 and ".nowhere" in io.err
    rc, io = _main(["setup-contribute", files["k0.pk"], files["k0.vk"] + ".nowhere", "--out", out], capsys)
    assert rc == 2 and ".nowhere" in io.err
    for bad in ("zz", "00" * 31, "00" * 33):
        rc, io = _main(["setup-contribute", files["k0.pk"], files["k0.vk"], "--out", out, "--entropy", bad], capsys)
        assert rc == 2 and "spp setup-contribute" in io.err, bad
    # the key's own directory as --out would overwrite the key the verifier needs
    rc, io = _main(["setup-contribute", files["k0.pk"], files["k0.vk"], "--out", os.path.dirname(files["k0.pk"])], capsys)
    assert rc == 2 and "key before" in io.err
    with open(files["k0.pk"], "rb") as f:
        assert f.read() == b"\0" * 8
    with pytest.raises(SystemExit):                                      # --out is required
        _main(["setup-contribute", files["k0.pk"], files["k0.vk"]], capsys)
