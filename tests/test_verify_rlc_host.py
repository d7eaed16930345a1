"""CPU: the random-linear-combination batch verifier (csrc/verify_rlc.hpp, csrc/f12_coop.hpp) as a g++ build,
tests/host/verify_rlc_check.cpp: the wave-cooperative Fq12 routines run lane by lane against their one-lane counterparts, and the
whole pipeline (terms, fold, the serial and the emulated cooperative tail, the fallback through verify_one) on the cases of
tests/verify_vectors.py, whose verdicts are known by construction.  tests/test_gpu_verify_rlc.py puts the same batches through the
gfx950 build."""
import ctypes
import os
import random
import re
import subprocess

import pytest

from conftest import ROOT
import verify_vectors as V
import verify_rlc_vectors as RV

CSRC = os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "verify_rlc_check.cpp")
SEEDS = {"withdraw": b"\x07" * 32, "audit": b"\x09" * 32}               # conftest.py: withdraw_artifacts / audit_artifacts
NPUB = {"withdraw": 5, "audit": 2}
SERIAL_TAIL, NO_FALLBACK = 1, 2
RLC_SEEDS = (bytes(range(32)), b"\xa5" * 32)


@pytest.fixture(scope="module")
def key_paths(withdraw_artifacts, audit_artifacts):
    return {"withdraw": withdraw_artifacts["vk"], "audit": audit_artifacts["vk"]}


@pytest.fixture(scope="module")
def keys(key_paths):
    return {k: open(p, "rb").read() for k, p in key_paths.items()}


@pytest.fixture(scope="module")
def case_lists(keys):
    return {k: V.cases(keys[k], V.trapdoor(SEEDS[k]), NPUB[k], random.Random(4048 + NPUB[k])) for k in keys}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("verify_rlc") / "verify_rlc_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", CSRC, SRC, "-o", out], check=True)
    return out


def run_pipeline(exe, tmp, vk_path, batch, seed, group, flags=0, env=None):
    """(verdicts, stats, tails agree) of one run of the stand-alone program on [(proof, pw)]"""
    path = os.path.join(str(tmp), "batch.bin")
    with open(path, "wb") as f:
        for proof, pw in batch:
            f.write(proof + pw)
    p = subprocess.run([exe, vk_path, path, seed.hex(), str(group), str(flags)], capture_output=True, text=True, env=env)
    assert p.returncode == 0, (p.stdout, p.stderr[-2000:])
    lines = dict(l.split(" ", 1) for l in p.stdout.strip().splitlines())
    assert set(lines) == {"VERDICTS", "STATS", "TAILS"}, p.stdout
    verdicts = [c == "1" for c in lines["VERDICTS"]]
    assert len(verdicts) == len(batch)
    return verdicts, tuple(int(v) for v in lines["STATS"].split()), lines["TAILS"] == "agree"


def test_cooperative_routines_equal_their_one_lane_counterparts(exe):
    """f12_mul, f12_mul_line, f12_frob, f12_conj6, f12_pow_x, the five-table Miller loop and final_exp_is_one, 64 lanes emulated"""
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert out.strip().splitlines()[-1].startswith("OK "), out


@pytest.mark.parametrize("key", ["withdraw", "audit"])
def test_all_cases_in_one_batch(exe, tmp_path, key_paths, case_lists, key):
    cs = case_lists[key]
    assert len(cs) == V.N_CASES
    got, stats, agree = run_pipeline(exe, tmp_path, key_paths[key], [(c[1], c[2]) for c in cs], RLC_SEEDS[0], 64)
    wrong = ["%s (%s): expected %s, got %s" % (c[0], c[4], c[3], g) for c, g in zip(cs, got) if g != c[3]]
    assert not wrong, "\n".join(wrong)
    assert stats == (1, 1, 39, 16)                                       # dropped: 12 format + 4 subgroup; 55 - 16 re-verified
    assert agree


@pytest.mark.parametrize("seed", RLC_SEEDS)
def test_all_valid_batch_refuses_no_group_and_re_verifies_nothing(exe, tmp_path, key_paths, case_lists, seed):
    """the fallback must not hide a tail that wrongly refuses: on valid proofs only, no group is refused"""
    batch = RV.cycled(RV.accepts(case_lists["withdraw"]), 130)
    assert len(RV.accepts(case_lists["withdraw"])) == 24
    for flags in (0, SERIAL_TAIL):
        got, stats, agree = run_pipeline(exe, tmp_path, key_paths["withdraw"], [(c[1], c[2]) for c in batch], seed, 64, flags)
        assert got == [True] * 130 and stats == (3, 0, 0, 0) and agree, (flags, stats, agree)


@pytest.fixture(scope="module")
def pairs(keys):
    return RV.cancelling_pairs(keys["withdraw"], V.trapdoor(SEEDS["withdraw"]), NPUB["withdraw"], random.Random(77))


@pytest.mark.parametrize("kind", RV.KINDS)
def test_cancelling_pairs_are_refused(exe, tmp_path, key_paths, keys, pairs, kind):
    """each proof alone is invalid and the product of the two equations with all scalars equal is one (the oracle's pairing says so):
    a combination without distinct scalars accepts this pair"""
    assert RV.unweighted_product_is_one(keys["withdraw"], pairs, kind)
    for flags in (0, NO_FALLBACK, SERIAL_TAIL):
        got, stats, agree = run_pipeline(exe, tmp_path, key_paths["withdraw"], pairs[kind], RLC_SEEDS[1], 64, flags)
        assert got == [False, False] and agree, (kind, flags, got)
        assert stats == (1, 1, 0 if flags & NO_FALLBACK else 2, 0)


def test_stand_alone_program_under_asan_ubsan(tmp_path, key_paths, case_lists):
    """the same program, instrumented: the routines, then the 55 audit-key cases through the pipeline"""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    out = str(tmp_path / "san_verify_rlc_check")
    subprocess.run(["g++", "-O1", "-std=c++17"] + san + ["-I", CSRC, SRC, "-o", out], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([out], capture_output=True, text=True, env=env)
    text = p.stdout + p.stderr
    assert p.returncode == 0 and "runtime error" not in text and "AddressSanitizer" not in text, text[-3000:]
    assert p.stdout.strip().splitlines()[-1].startswith("OK ")
    cs = case_lists["audit"]
    got, stats, agree = run_pipeline(out, tmp_path, key_paths["audit"], [(c[1], c[2]) for c in cs], RLC_SEEDS[0], 64, env=env)
    assert got == [c[3] for c in cs] and stats == (1, 1, 39, 16) and agree


def test_c_abi_of_the_rlc_verifier():
    import spp
    hdr = open(os.path.join(ROOT, "include", "spp.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert ("int spp_verify_batch_rlc(spp_ctx* ctx, const uint8_t* vk, size_t vk_len, size_t count, const uint8_t* proofs, "
            "const uint8_t* pws, size_t pw_len, const uint8_t* seed32 , uint32_t group , uint32_t flags, int32_t* ok, uint32_t stats[4] , "
            "float* kernel_ms);") in flat
    assert re.search(r"#define SPP_RLC_SERIAL_TAIL 1\b", hdr) and re.search(r"#define SPP_RLC_NO_FALLBACK 2\b", hdr)
    from spp import lib as L_
    assert (L_.SPP_RLC_SERIAL_TAIL, L_.SPP_RLC_NO_FALLBACK) == (1, 2)
    L = spp.load_library()
    ok = (ctypes.c_int32 * 4)()
    okp = ctypes.cast(ok, ctypes.c_void_p)
    ctx = ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p)          # never dereferenced: every call below is refused first
    vk = bytes(64)
    BAD_INPUT = -1
    assert L.spp_verify_batch_rlc(None, vk, len(vk), 0, None, None, 12, None, 0, 0, okp, None, None) == BAD_INPUT
    assert L.spp_verify_batch_rlc(ctx, None, 0, 0, None, None, 12, None, 0, 0, okp, None, None) == BAD_INPUT
    assert L.spp_verify_batch_rlc(ctx, vk, len(vk), 0, None, None, 12, None, 0, 0, None, None, None) == BAD_INPUT
    assert L.spp_verify_batch_rlc(ctx, vk, len(vk), 1, None, None, 12, None, 0, 0, okp, None, None) == BAD_INPUT
    for group in (63, 96, 8192):
        assert L.spp_verify_batch_rlc(ctx, vk, len(vk), 0, None, None, 12, None, group, 0, okp, None, None) == BAD_INPUT, group
        assert b"group" in L.spp_last_error()
    assert L.spp_verify_batch_rlc(ctx, vk, len(vk), 0, None, None, 12, None, 64, 4, okp, None, None) == BAD_INPUT   # an unknown flag
    for group in (0, 64, 4096):                                          # an empty batch with a group that is allowed: nothing to do
        assert L.spp_verify_batch_rlc(ctx, vk, len(vk), 0, None, None, 12, None, group, 0, okp, None, None) == 0, group


def test_cli_verify_batch_refuses_bad_arguments_before_opening_a_device(tmp_path, keys, case_lists, capsys):
    from spp import cli
    c = case_lists["audit"][0]
    vk, proof, pw = tmp_path / "a.vk", tmp_path / "a.proof", tmp_path / "a.pw"
    vk.write_bytes(keys["audit"]); proof.write_bytes(c[1]); pw.write_bytes(c[2])
    assert cli.main(["verify-batch", str(vk), str(proof)]) == 2                       # a proof without its public witness
    assert cli.main(["verify-batch", str(vk), str(pw), str(proof)]) == 2              # the pair the wrong way round: not 388 bytes
    assert cli.main(["verify-batch", str(vk), str(proof), str(tmp_path / "missing.pw")]) == 2
    assert capsys.readouterr().err.count("spp verify-batch:") == 3
