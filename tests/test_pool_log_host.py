"""spp_pool_settle_log, host side (no GPU): the declaration, the export, the Python mirror and the NULL refusal, and the log pieces of
csrc/pool_table.hpp compiled for the host (tests/host/pool_log_check.cpp) -- the ring at a position inside a batch and the whole
rule of a log in which deposits, submit_audits and withdraws alternate -- against PoolModel of tests/test_pool_host.py fed the log
ONE instruction at a time.  PoolModel calls nothing under test."""
import os
import random
import re
import subprocess

import pytest

from conftest import ROOT
from test_pool_host import (PoolModel, keys_homed_at, home_slot, slots_for, OK, AUDIT_EXISTS, NO_AUDIT_RECORD, BAD_ROOT, NULLIFIER_USED,
                            BAD_RECIPIENT, BAD_PROOF)

VALID, INVALID = b"\x01", b"\x00"                      # the "proof" of the host log: its own validity bit


def test_header_declares_settle_log_and_cites_the_program():
    hdr = open(os.path.join(ROOT, "include", "spp.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int spp_pool_settle_log(spp_pool*, size_t count, const uint8_t* kinds, size_t n_deposits, const uint8_t* roots, "
            "size_t n_audits, const uint8_t* audit_proofs, const uint8_t* audit_pws, "
            "size_t n_withdraws, const uint8_t* withdraw_proofs, const uint8_t* withdraw_pws, const uint8_t* recipients, "
            "int32_t* result, uint64_t* amounts);") in flat
    for name, val in (("SPP_INSTR_DEPOSIT", 0), ("SPP_INSTR_SUBMIT_AUDIT", 1), ("SPP_INSTR_WITHDRAW", 2)):
        assert re.search(r"#define %s %d\b" % (name, val), hdr), name
    refs = ("state.rs:28-46", "instructions/deposit.rs:21-37", "submit_audit.rs:41-87", "withdraw.rs:94-175")
    index = hdr[:hdr.index("#ifndef SPP_H")]
    entry = index[index.index("spp_pool_settle_log"):]
    comment = hdr[hdr.rindex("/*", 0, hdr.index("#define SPP_INSTR_DEPOSIT")):hdr.index("#define SPP_INSTR_DEPOSIT")]
    for ref in refs:
        assert ref in entry, ref
        assert ref in comment, ref
    # the kinds are not SPP_POOL_* macros: the ten numeric ones are what they were
    assert len(re.findall(r"#define (SPP_POOL_\w+) (\d+)", hdr)) == 10


def test_library_exports_settle_log_and_python_mirrors_the_kinds():
    import spp
    from spp import lib, witness
    L = spp.load_library()
    assert hasattr(L, "spp_pool_settle_log")
    hdr = open(os.path.join(ROOT, "include", "spp.h")).read()
    kinds = re.findall(r"#define (SPP_INSTR_\w+) (\d+)", hdr)
    assert len(kinds) == 3
    for name, val in kinds:
        assert getattr(lib, name) == int(val), name
    assert callable(witness.Pool.settle_log)


def test_settle_log_refuses_null_without_a_device():
    import spp
    L = spp.load_library()
    k = bytes([0])
    calls = (lambda: L.spp_pool_settle_log(None, 1, k, 1, bytes(32), 0, None, None, 0, None, None, None, None, None),
             lambda: L.spp_pool_settle_log(None, 0, None, 0, None, 0, None, None, 0, None, None, None, None, None))
    for n, call in enumerate(calls):
        L.spp_verify(None, 0, None, 0, None, 0, None)     # leaves another message behind
        assert call() == -1 and "NULL" in spp.last_error(), n


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pool_log") / "pool_log_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "pool_log_check.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, text):
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-300:] + out.stderr
    return out.stdout.split("\n")


@pytest.mark.parametrize("t0", [0, 5, 32, 40])
@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 70])
def test_ring_at_every_position_of_a_batch_on_the_host(check_exe, t0, n):
    """t0 roots pushed before the call, n by the batch's deposits; at every position d = 0..n the root check is check_root of the
    program after exactly t0 + d pushes -- for every root ever pushed, the zero root and an unknown one"""
    rng = random.Random(1000 * t0 + n)
    pushed = [rng.getrandbits(254).to_bytes(32, "big") for _ in range(t0 + n)]
    queries = pushed + [bytes(32), rng.getrandbits(254).to_bytes(32, "big")]
    lines = _run(check_exe, "ringat %d %d %d\n%s\n" % (t0, n, len(queries), "\n".join(k.hex() for k in pushed + queries)))
    m = PoolModel()
    for r in pushed[:t0]:
        m.add_root(r)
    for d in range(n + 1):
        if d:
            m.add_root(pushed[t0 + d - 1])
        total = t0 + d
        assert lines[1 + d] == "".join("1" if m.check_root(q) else "0" for q in queries), d
        # the window, spelled out: root i (pushed as the i+1st) is known from its own push through the 32 pushes that follow it
        # -- while fewer than i + 33 roots have been pushed -- and the zero root only while fewer than 32 have been pushed at all
        want = "".join("1" if i < total < i + 33 else "0" for i in range(t0 + n)) + ("1" if total < 32 else "0") + "0"
        assert lines[1 + d] == want, d
    assert bytes.fromhex(lines[0]) == m.state()


def _withdraw_pw(root, nullifier, address, amount, wa):
    return bytes(12) + root + nullifier + bytes(2) + address[:30] + amount.to_bytes(32, "big") + wa


def _audit_pw(wa, tag):
    return bytes(12) + wa + tag.to_bytes(32, "big")


def _random_log(rng, n, preloaded):
    """n instructions over 10 random identities and 2 crafted ones: (kind, ...) tuples for PoolModel, whose verifier reads the
    validity bit out of the one-byte proof.  Returns (pre, log, identities)."""
    kinds = ["d", "w", "a", "w", "a", "w"]                  # identity 0: see the prefix below
    kinds += rng.choices("daw", [45, 120, 235], k=n - len(kinds))
    n_audits = kinds.count("a")
    # two identities whose wa keys share a home slot of the audit resolve table (>= 2 x n_audits slots), one pair of identities whose
    # wa keys share their low 64 bits (same home, other bytes)
    salt = 0x0F1E2D3C4B5A6978
    rslots = slots_for(n_audits)
    was = [rng.getrandbits(256).to_bytes(32, "big") for _ in range(9)]
    was.append(bytes([was[3][0] ^ 1]) + was[3][1:])
    was += keys_homed_at(home_slot(was[5], salt, rslots), salt, rslots, 2, rng)
    assert home_slot(was[10], salt, rslots) == home_slot(was[11], salt, rslots) and was[9][24:] == was[3][24:] and len(set(was)) == 12
    ids = [dict(wa=was[i], address=rng.getrandbits(256).to_bytes(32, "big"),
                notes=[(rng.getrandbits(254).to_bytes(32, "big"), rng.randrange(1, 1 << 64)) for _ in range(3)]) for i in range(12)]
    pre = []
    if preloaded:                                           # a pool that has lived: 40 roots, a record, a spent note
        pre = [("R", rng.getrandbits(254).to_bytes(32, "big")) for _ in range(40)]
        pre += [("A", ids[8]["wa"]), ("A", ids[11]["wa"]), ("N", ids[8]["notes"][0][0]), ("N", ids[2]["notes"][1][0])]
    roots = [r for k, r in pre if k == "R"]
    unknown = rng.getrandbits(254).to_bytes(32, "big")
    log = []
    for pos, k in enumerate(kinds):
        i = 0 if pos < 6 else rng.randrange(12)
        me = ids[i]
        if k == "d":
            roots.append(rng.getrandbits(254).to_bytes(32, "big"))
            log.append(("deposit", roots[-1]))
        elif k == "a":
            valid = pos == 4 if pos < 6 else rng.random() < 0.45
            log.append(("submit_audit", VALID if valid else INVALID, _audit_pw(me["wa"], pos)))
        else:
            how = "good" if pos < 6 else rng.choices(["good", "bad", "recipient", "stale", "unknown", "zero"], [50, 15, 12, 12, 6, 5])[0]
            root = {"stale": rng.choice(roots), "unknown": unknown, "zero": bytes(32)}.get(how, roots[-1] if rng.random() < 0.5 else rng.choice(roots[-32:]))
            nullifier, amount = rng.choice(me["notes"])
            address = ids[(i + 1) % 12]["address"] if how == "recipient" else me["address"]
            log.append(("withdraw", INVALID if how == "bad" else VALID, _withdraw_pw(root, nullifier, me["address"], amount, me["wa"]), address))
    return salt, pre, log, ids


@pytest.mark.parametrize("preloaded", [False, True])
def test_whole_log_rule_on_the_host(check_exe, preloaded):
    """400 instructions of the three kinds interleaved, the claims made in descending order by the check: every code, every
    amount, the ring bytes and both sets are those of taking the log one instruction at a time"""
    rng = random.Random(4242 + preloaded)
    salt, pre, log, ids = _random_log(rng, 400, preloaded)
    assert len(log) == 400 and 35 <= sum(ins[0] == "deposit" for ins in log) <= 55
    m = PoolModel(lambda proof, pw: proof == VALID, lambda proof, pw: proof == VALID)
    for k, v in pre:
        if k == "R":
            m.add_root(v)
        else:
            (m.audits if k == "A" else m.nullifiers)[v] = True
    want, want_amounts, text = [], [], []
    for ins in log:                                         # one at a time
        if ins[0] == "deposit":
            m.add_root(ins[1])
            want.append(OK); want_amounts.append(0)
            text.append("d " + ins[1].hex())
        elif ins[0] == "submit_audit":
            want.append(m.submit_audit(ins[1], ins[2])); want_amounts.append(0)
            text.append("a %s %d" % (ins[2].hex(), ins[1] == VALID))
        else:
            c, a = m.withdraw(ins[1], ins[2], ins[3])
            want.append(c); want_amounts.append(a)
            text.append("w %s %s %d" % (ins[2].hex(), ins[3].hex(), ins[1] == VALID))
    head = "log %x %d %d %d\n" % (salt, 512, len(pre), len(log))
    lines = _run(check_exe, head + "".join("%s %s\n" % (k, v.hex()) for k, v in pre) + "\n".join(text) + "\n")
    got = [int(x) for x in lines[0].split()]
    assert got == want                                      # every instruction of the log
    assert [int(x) for x in lines[1].split()] == want_amounts
    assert bytes.fromhex(lines[2]) == m.state()
    keys = lambda line: sorted(bytes.fromhex(x) for x in line.split() if x != "-")
    assert keys(lines[3]) == sorted(m.nullifiers) and keys(lines[4]) == sorted(m.audits)
    assert set(got) == {OK, AUDIT_EXISTS, NO_AUDIT_RECORD, BAD_ROOT, NULLIFIER_USED, BAD_RECIPIENT, BAD_PROOF}
    # the three cross-kind cases, each on at least one identity that had no record at the call
    resident = {v for k, v in pre if k == "A"}
    seen = {"before": 0, "after_invalid_only": 0, "after_valid": 0}
    for me in ids:
        if me["wa"] in resident:
            continue
        audits_so_far, has_record = 0, False
        for ins, code in zip(log, got):
            if ins[0] == "submit_audit" and ins[2][12:44] == me["wa"]:
                audits_so_far += 1
                has_record = has_record or code == OK
            elif ins[0] == "withdraw" and ins[2][140:172] == me["wa"]:
                if not has_record:
                    assert code == NO_AUDIT_RECORD
                    seen["before" if audits_so_far == 0 else "after_invalid_only"] += 1
                else:
                    assert code != NO_AUDIT_RECORD
                    seen["after_valid"] += code == OK
    assert all(seen.values()), seen
    assert got[:6] == [OK, NO_AUDIT_RECORD, BAD_PROOF, NO_AUDIT_RECORD, OK, OK]


def test_an_empty_log_settles_to_nothing_on_the_host(check_exe):
    lines = _run(check_exe, "log 1 8 0 0\n")
    assert lines[0] == "" and lines[1] == "" and bytes.fromhex(lines[2]) == PoolModel().state() and lines[3] == "-" == lines[4]
