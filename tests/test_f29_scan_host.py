"""csrc/f29.hpp on the host: the product-scanning Montgomery products (one, two and four products, squaring) against
clear / mac / reduce limb for limb on both parameter sets, the accumulators in both forms, and the one-multiplication filter of
is_zero_mod_p against the compares it replaced (tests/host/f29_scan_check.cpp) -- a plain build and one under AddressSanitizer +
UBSan of the same stand-alone program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "f29_scan_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_scanning_products_equal_mac_reduce(tmp_path, flags):
    """Random limbs and limbs at the bounds of every call site (1 x 1, 2 x 1, 2 x 3, 1x3 + 2x1, the G2 sums of two and four products),
    Fr and Fq; chains of additions in both forms; 0, p .. (KMAX + 2) p and their neighbours through both zero tests."""
    exe = str(tmp_path / "f29_scan_check")
    subprocess.run(["g++", "-std=c++17"] + flags + ["-I", CSRC, SRC, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    proc = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert "runtime error" not in proc.stderr and "AddressSanitizer" not in proc.stderr, proc.stderr[-3000:]
    assert proc.returncode == 0 and proc.stdout.strip().splitlines()[-1].startswith("OK "), proc.stdout + proc.stderr


def test_gen_consts_emits_the_committed_header():
    """bn254_consts.hpp (with PINV29, the constant of the filter) is what gen_consts.py prints."""
    out = subprocess.run(["python3", os.path.join(CSRC, "gen_consts.py")], capture_output=True, text=True, check=True).stdout
    assert out == open(os.path.join(CSRC, "bn254_consts.hpp")).read()
