"""CPU: the index arithmetic of the random-linear-combination verifier over a compacted list (csrc/verify_rlc_list.hpp) as a g++
build, tests/host/verify_rlc_list_check.cpp: the functions k_verify_rlc_terms_list / k_verify_rlc_group_list and their launcher are
made of, run lane after lane on a list that is a permutation with gaps, at the lengths 0, 1, 63, 64, 65 and 129 with group 64 --
block coverage exact and disjoint, a verdict for position j at list[j] and nowhere else, exactly the live members of a refused group
on the fallback list as instruction indices, slices of two groups equal to one slice -- and the C ABI and Python surface of the
pool's verifier mode and of spp_audit_open_batch_rlc as far as they go without a device.  tests/test_gpu_pool_rlc.py runs the
kernels."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "verify_rlc_list_check.cpp")
LENGTHS = (0, 1, 63, 64, 65, 129)


def _cases(out):
    """{(length, slice length): (ok digits, fallback indices, stats)}"""
    got = {}
    for line in out.splitlines():
        m = re.fullmatch(r"CASE (\d+) (\d+) OK=([01]*) FALLBACK=([\d,]*) STATS=(\d+),(\d+),(\d+),(\d+)", line)
        if m:
            got[(int(m[1]), int(m[2]))] = (m[3], [int(v) for v in m[4].split(",") if v], tuple(int(m[k]) for k in range(5, 9)))
    return got


def _check_output(out):
    assert out.strip().splitlines()[-1].startswith("OK "), out
    cases = _cases(out)
    assert sorted(cases) == sorted((n, s) for n in LENGTHS for s in (128, 1 << 18))
    for n in LENGTHS:
        one, two = cases[(n, 1 << 18)], cases[(n, 128)]
        assert one == two, n                                             # slices of two groups each: the same result as one slice
        ok, fallback, stats = one
        assert len(ok) == 200 and ok.count("1") <= n
        assert stats[0] == (n + 63) // 64 and stats[2] == len(fallback) and stats[1] <= stats[0]
        assert all(ok[i] == "1" for i in fallback if i % 37 != 5)        # a re-verified valid proof is accepted after all
    assert cases[(0, 128)] == ("0" * 200, [], (0, 0, 0, 0))
    assert cases[(129, 128)][2][1] >= 1 and cases[(129, 128)][2][3] >= 1   # the cases reach a refused group and dropped proofs


def test_list_index_arithmetic_lane_after_lane(tmp_path):
    exe = str(tmp_path / "verify_rlc_list_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", exe], check=True)
    _check_output(subprocess.run([exe], capture_output=True, text=True).stdout)


def test_stand_alone_program_under_asan_ubsan(tmp_path):
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    exe = str(tmp_path / "san_verify_rlc_list_check")
    subprocess.run(["g++", "-O1", "-std=c++17"] + san + ["-I", CSRC, SRC, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env)
    text = p.stdout + p.stderr
    assert p.returncode == 0 and "runtime error" not in text and "AddressSanitizer" not in text, text[-3000:]
    _check_output(p.stdout)


def test_c_abi_of_the_pool_verifier_and_the_rlc_audit_open():
    import spp
    from spp import lib as L_
    hdr = open(os.path.join(ROOT, "include", "spp.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))
    assert "int spp_pool_set_verifier(spp_pool*, int mode, uint32_t group );" in flat
    assert "int spp_pool_verify_stats(spp_pool*, uint32_t stats[8]);" in flat
    assert ("int spp_audit_open_batch_rlc(spp_ctx* ctx, const uint8_t* vk, size_t vk_len, const uint32_t* sk_mod_q, size_t count, "
            "const uint8_t* proofs, const uint8_t* pws, const uint32_t* c0, const uint32_t* c1, uint32_t group, uint8_t* owners, "
            "uint32_t* flags, uint32_t stats[4] );") in flat
    assert re.search(r"#define SPP_POOL_VERIFY_EACH\s+0\b", hdr) and re.search(r"#define SPP_POOL_VERIFY_RLC\s+1\b", hdr)
    assert (L_.SPP_POOL_VERIFY_EACH, L_.SPP_POOL_VERIFY_RLC) == (0, 1)
    L = spp.load_library()
    BAD_INPUT = -1
    stats8 = (ctypes.c_uint32 * 8)()
    assert L.spp_pool_set_verifier(None, 1, 64) == BAD_INPUT and b"NULL" in L.spp_last_error()
    assert L.spp_pool_verify_stats(None, stats8) == BAD_INPUT
    # spp_audit_open_batch_rlc: the group is looked at first, then the checks of spp_audit_open_batch (every call here is refused
    # before the context is touched)
    ctx = ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p)
    sk = (ctypes.c_uint32 * 1024)()
    skp = ctypes.cast(sk, ctypes.c_void_p)
    stats = (ctypes.c_uint32 * 4)(9, 9, 9, 9)
    for group in (63, 96, 8192):
        assert L.spp_audit_open_batch_rlc(ctx, None, 0, skp, 0, None, None, None, None, group, None, None, stats) == BAD_INPUT, group
        assert b"group" in L.spp_last_error()
    assert list(stats) == [0, 0, 0, 0]
    assert L.spp_audit_open_batch_rlc(None, None, 0, skp, 0, None, None, None, None, 64, None, None, None) == BAD_INPUT
    assert L.spp_audit_open_batch_rlc(ctx, None, 0, None, 0, None, None, None, None, 64, None, None, None) == BAD_INPUT
    assert L.spp_audit_open_batch_rlc(ctx, b"\x00" * 8, 0, skp, 0, None, None, None, None, 64, None, None, None) == BAD_INPUT   # a key without its length
    sk[1023] = 167772161
    assert L.spp_audit_open_batch_rlc(ctx, None, 0, skp, 0, None, None, None, None, 0, None, None, None) == BAD_INPUT and b"[0, q)" in L.spp_last_error()
    sk[1023] = 0
    for group in (0, 64, 4096):                                          # an empty batch without a key: nothing to do
        assert L.spp_audit_open_batch_rlc(ctx, None, 0, skp, 0, None, None, None, None, group, None, None, None) == 0, group


def test_python_surface_refuses_before_a_device_is_opened(tmp_path, capsys):
    from spp import cli, witness
    with pytest.raises(ValueError):
        witness.Pool(None, b"", b"", 1, verifier="fast")                 # refused before the context is looked at
    wvk, avk, log = (str(tmp_path / n) for n in ("w.vk", "a.vk", "log.jsonl"))
    open(wvk, "wb").write(b"x"); open(avk, "wb").write(b"y"); open(log, "w").write("{\"deposit\": {\"root\": \"00\"}}\n")
    assert cli.main(["pool-replay", wvk, avk, log, "--verifier", "rlc", "--group", "64"]) == 2      # the log's root is not 32 bytes
    assert "spp pool-replay:" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["pool-replay", wvk, avk, log, "--verifier", "both"])
