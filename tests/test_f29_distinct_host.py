"""csrc/f29.hpp on the host: madd_distinct, the mixed addition of the flat table walk that refuses the same-x case, against madd
(tests/host/f29_distinct_check.cpp) -- a plain build and one under AddressSanitizer + UBSan of the same stand-alone program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "f29_distinct_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_madd_distinct_equals_madd_or_refuses(tmp_path, flags):
    """Both accumulators (G1 and G2), random chains, extremal limbs and the first addition from infinity: where the x coordinates
    differ every limb equals madd's; where the entry is the accumulated point or its negative the result is false and no limb
    changed."""
    exe = str(tmp_path / "f29_distinct_check")
    subprocess.run(["g++", "-std=c++17"] + flags + ["-I", CSRC, SRC, "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    proc = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert "runtime error" not in proc.stderr and "AddressSanitizer" not in proc.stderr, proc.stderr[-3000:]
    assert proc.returncode == 0 and proc.stdout.strip().splitlines()[-1].startswith("OK "), proc.stdout + proc.stderr
