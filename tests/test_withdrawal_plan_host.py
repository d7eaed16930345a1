"""The withdrawal plan, host side (no GPU): csrc/withdrawal_plan.hpp compiled for the host (tests/host/withdrawal_plan_check.cpp runs
the per-lane and per-tile pieces of the kernels as sequential loops, launch by launch) against the model below, the constants of
include/spp.h against the Python mirror, the NULL refusals of spp_withdrawal_audit_plan and spp_prove_withdrawals without a device,
and the check program once more under AddressSanitizer and UBSan, as a stand-alone binary.

plan_model is the reference for this file and for the two GPU files: a set for the resident keys and a dict of first occurrences."""
import os
import random
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

RESIDENT = 0xFFFFFFFF
TILE = 1024
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
CSRC = os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "withdrawal_plan_check.cpp")
COUNTS = [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]


def plan_model(keys, resident=()):
    """(audit_of, audit_note) for 32-byte keys and the keys the pool's audit-record set holds"""
    resident, first = set(resident), {}
    for i, k in enumerate(keys):
        if k not in resident:
            first.setdefault(k, i)
    audit_note = sorted(first.values())
    slot = {i: s for s, i in enumerate(audit_note)}
    return [RESIDENT if k in resident else slot[first[k]] for k in keys], audit_note


def key_families(rng, count, kind):
    """`count` keys of one of the families the plan has to get right"""
    word = lambda: rng.getrandbits(256).to_bytes(32, "big")
    if kind == "equal":
        return [word()] * count
    if kind == "distinct":
        return [i.to_bytes(4, "big") + word()[4:] for i in range(count)]
    if kind == "repeated":                                            # about 30 % of the keys are copies of an earlier one
        keys = []
        for _ in range(count):
            keys.append(rng.choice(keys) if keys and rng.random() < 0.3 else word())
        return keys
    if kind == "low64":                                               # one home slot under any salt: the slot function reads bytes 24..31
        low = word()[24:]
        pool = [rng.getrandbits(192).to_bytes(24, "big") + low for _ in range(max(1, count // 3))]
        return [rng.choice(pool) for _ in range(count)]
    if kind == "plus_r":                                              # v and v + r are two identities
        vs = [rng.randrange(1 << 253) for _ in range(max(1, count // 4))]
        pool = [v.to_bytes(32, "big") for v in vs] + [(v + R).to_bytes(32, "big") for v in vs]
        return [rng.choice(pool) for _ in range(count)]
    raise ValueError(kind)


FAMILIES = ("equal", "distinct", "repeated", "low64", "plus_r")


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wplan") / "withdrawal_plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", CSRC, SRC, "-o", exe], check=True)
    return exe


def run_plan(exe, keys, resident=(), capacity=0, salt=0x5EED5EED5EED5EED, order=0):
    text = "plan %x %d %d %d %d\n%s\n" % (salt, order, capacity, len(resident), len(keys), "\n".join(k.hex() for k in list(resident) + list(keys)))
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout[-300:], out.stderr[-2000:])
    lines = out.stdout.split("\n")
    n = int(lines[0].split()[1])
    audit_of, audit_note = [int(v) for v in lines[1].split()], [int(v) for v in lines[2].split()]
    assert lines[0].startswith("n_audits ") and len(audit_note) == n
    return audit_of, audit_note


def test_constants_of_the_header_the_library_and_the_python_mirror(check_exe):
    from spp import lib
    hdr = open(os.path.join(ROOT, "include", "spp.h")).read()
    assert re.search(r"#define SPP_AUDIT_RESIDENT 0xFFFFFFFFu\b", hdr) and lib.SPP_AUDIT_RESIDENT == RESIDENT
    assert int(re.search(r"#define SPP_WITHDRAWALS_MAX (\d+)", hdr).group(1)) == lib.SPP_WITHDRAWALS_MAX == 1 << 20
    out = subprocess.run([check_exe], input="constants\n", capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [TILE, 64, lib.SPP_WITHDRAWALS_MAX, RESIDENT]
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int spp_withdrawal_audit_plan(spp_ctx* ctx, spp_pool* pool /* optional */, size_t count, const uint8_t* wa /* count * 32 B */, "
            "uint32_t* audit_of /* count */, uint32_t* audit_note /* count */, uint32_t* n_audits);") in flat
    assert ("int spp_prove_withdrawals(spp_circuit* withdraw, spp_circuit* audit, spp_merkle_tree* t, spp_pool* pool /* optional */, uint64_t size, "
            "const uint32_t* pk_a, const uint32_t* pk_b, size_t count, const uint8_t* notes /* count * SPP_NOTE_LEN */,") in flat
    for ref in ("route.ts:129-287", "submit_audit.rs:65-73", "generate_audit.py:469-506"):
        assert ref in hdr, ref
    assert "chosen by identity alone" in hdr


def test_python_mirror_declares_both_calls():
    import spp
    from spp import prover
    L = spp.load_library()
    assert hasattr(L, "spp_withdrawal_audit_plan") and hasattr(L, "spp_prove_withdrawals")
    assert callable(prover.Context.withdrawal_audit_plan) and callable(spp.prove_withdrawals) and callable(spp.WithdrawalBundle.log)
    b = spp.WithdrawalBundle([b"p0", b"p1", b"p2"], [b"w0", b"w1", b"w2"], [0, 0, 0], [0, RESIDENT, 0], [0], [b"ap"], [b"aw"], [0], None, None)
    assert b.n_audits == 1
    assert b.log([b"A" * 32, b"B" * 32, b"C" * 32]) == [("submit_audit", b"ap", b"aw"), ("withdraw", b"p0", b"w0", b"A" * 32),
                                                        ("withdraw", b"p1", b"w1", b"B" * 32), ("withdraw", b"p2", b"w2", b"C" * 32)]
    with pytest.raises(ValueError):
        b.log([b"A" * 32])


def test_both_calls_refuse_null_without_a_device():
    import ctypes
    import spp
    L = spp.load_library()
    buf = ctypes.create_string_buffer(4096)
    vp = ctypes.cast(buf, ctypes.c_void_p)
    n = ctypes.c_uint32(7)
    pw = lambda *a: L.spp_prove_withdrawals(*a)
    calls = (lambda: L.spp_withdrawal_audit_plan(None, None, 1, bytes(32), vp, vp, ctypes.byref(n)),
             lambda: L.spp_withdrawal_audit_plan(None, None, 0, None, None, None, None),
             lambda: pw(None, None, None, None, 0, vp, vp, 1, bytes(160), None, None, None, None, None, vp, vp, None, vp, vp, ctypes.byref(n),
                        1, vp, vp, None, vp, vp),
             lambda: pw(None, None, None, None, 0, None, None, 0, None, None, None, None, None, None, None, None, None, None, None, None,
                        0, None, None, None, None, None))
    for k, call in enumerate(calls):
        L.spp_verify(None, 0, None, 0, None, 0, None)     # leaves another message behind
        assert call() == -1 and "NULL" in spp.last_error(), k
    assert n.value == 7                                    # a refused call writes nothing


@pytest.mark.parametrize("count", COUNTS)
def test_every_key_family_at_the_wave_and_tile_edges(check_exe, count):
    rng = random.Random(4000 + count)
    for kind in FAMILIES:
        keys = key_families(rng, count, kind)
        want = plan_model(keys)
        assert run_plan(check_exe, keys) == want, kind
        of, note = want
        assert note == sorted(note) and all(keys[note[s]] == keys[i] and note[s] <= i for i, s in enumerate(of))
        if kind == "equal":
            assert note == [0] and of == [0] * count
        if kind == "distinct":
            assert note == list(range(count)) == of


@pytest.mark.parametrize("count", [65, TILE + 1, 2 * TILE + 1])
def test_plan_depends_neither_on_the_lane_order_nor_on_the_salt(check_exe, count):
    rng = random.Random(5000 + count)
    for kind in ("repeated", "low64", "plus_r"):
        keys = key_families(rng, count, kind)
        distinct = list(dict.fromkeys(keys))
        resident = rng.sample(distinct, len(distinct) // 3)
        want = plan_model(keys, resident)
        for salt in (0x0123456789ABCDEF, 0xFEDCBA9876543210):
            for order in (0, 77, 78):
                assert run_plan(check_exe, keys, resident, len(resident) + 5, salt, order) == want, (kind, hex(salt), order)


@pytest.mark.parametrize("count", [64, TILE, 2 * TILE + 1])
def test_resident_keys_get_no_record(check_exe, count):
    """a resident subset, among it a key that occurs five times; a resident key that is no key of the batch; all resident"""
    rng = random.Random(6000 + count)
    keys = key_families(rng, count, "repeated")
    five = rng.getrandbits(256).to_bytes(32, "big")
    for p in rng.sample(range(count), 5):
        keys[p] = five
    distinct = list(dict.fromkeys(keys))
    resident = [five] + rng.sample([k for k in distinct if k != five], len(distinct) // 4) + [rng.getrandbits(256).to_bytes(32, "big")]
    of, note = run_plan(check_exe, keys, resident, 2 * len(resident))
    assert (of, note) == plan_model(keys, resident)
    assert [of[i] for i, k in enumerate(keys) if k == five] == [RESIDENT] * 5 and all(keys[i] not in resident for i in note)
    # the twin of a resident key (+ r, or the same low 64 bits) is not resident
    v = rng.randrange(1 << 253)
    a, b = v.to_bytes(32, "big"), (v + R).to_bytes(32, "big")
    c = bytes([a[0] ^ 0x40]) + a[1:]
    assert run_plan(check_exe, [a, b, c, b, a], [a], 4) == ([RESIDENT, 0, 1, 0, RESIDENT], [1, 2])
    assert run_plan(check_exe, keys, distinct, len(distinct)) == ([RESIDENT] * count, [])
    # a pool that holds nothing is no pool
    assert run_plan(check_exe, keys, [], 8) == plan_model(keys)


def test_check_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the same program built with -fsanitize=address,undefined and run directly: every array of the plan is a std::vector of
    exactly the size the device buffers have, so an index out of range in the header is reported"""
    exe = str(tmp_path / "withdrawal_plan_check_san")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, SRC, "-o", exe],
                           capture_output=True, text=True)
    if build.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", build.stderr):
        pytest.skip("the sanitizer runtime is not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    rng = random.Random(7)
    for count, kind in ((1, "equal"), (65, "low64"), (TILE + 1, "repeated"), (2 * TILE + 1, "plus_r")):
        keys = key_families(rng, count, kind)
        distinct = list(dict.fromkeys(keys))
        resident = rng.sample(distinct, len(distinct) // 3)
        assert run_plan(exe, keys, resident, len(resident) + 1, order=5) == plan_model(keys, resident)
