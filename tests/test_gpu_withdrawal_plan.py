"""GPU: the withdrawal plan (spp_withdrawal_audit_plan) against the model of tests/test_withdrawal_plan_host.py -- a set for the
resident keys, a dict of first occurrences.  No circuit is loaded: the pools take the golden verifying keys and their audit-record
sets are filled by import_keys.  Sizes 1, 63, 64, 65 (a wave), 1024, 1025 (a tile) and 2^17 + 1 (129 tile counts: past two waves of
the second scan level); keys are random 256-bit words, some >= r, plus the families of the host file."""
import ctypes
import os
import random

import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None

from conftest import GOLDEN
from test_withdrawal_plan_host import plan_model, key_families, FAMILIES, RESIDENT, R

pytestmark = pytest.mark.gpu

NULLIFIERS, AUDITS = 0, 1
SIZES = [1, 63, 64, 65, 1024, 1025, (1 << 17) + 1]


@pytest.fixture(scope="module")
def ctx():
    import spp
    c = spp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def vks():
    return tuple(open(os.path.join(GOLDEN, n), "rb").read() for n in ("reference_withdraw.vk", "reference_audit.vk"))


def mixed_keys(rng, count):
    """random words (a quarter of them >= r) with every family of the host file mixed in"""
    keys = [rng.getrandbits(256).to_bytes(32, "big") for _ in range(count)]
    assert count < 8 or any(int.from_bytes(k, "big") >= R for k in keys)
    for kind in FAMILIES[2:]:
        part = key_families(rng, max(1, count // 8), kind)
        for k in part:
            keys[rng.randrange(count)] = k
    for _ in range(count // 5):                                         # and plain repeats
        keys[rng.randrange(count)] = keys[rng.randrange(count)]
    return keys


@pytest.mark.parametrize("count", SIZES)
def test_plan_without_a_pool(ctx, count):
    rng = random.Random(100 + count)
    keys = mixed_keys(rng, count)
    got = ctx.withdrawal_audit_plan(keys)
    assert got == plan_model(keys)
    assert ctx.withdrawal_audit_plan(keys) == got                       # another salt from the operating system: the same plan
    if count <= 1025:
        for kind in FAMILIES:
            fam = key_families(rng, count, kind)
            assert ctx.withdrawal_audit_plan(fam) == plan_model(fam), kind


@pytest.mark.parametrize("count", SIZES)
def test_plan_with_a_pool_marks_resident_keys_and_leaves_the_pool_alone(ctx, vks, count):
    from spp import witness as W_
    rng = random.Random(200 + count)
    keys = mixed_keys(rng, count)
    five = rng.getrandbits(256).to_bytes(32, "big")
    for p in rng.sample(range(count), min(5, count)):
        keys[p] = five
    distinct = list(dict.fromkeys(keys))
    capacity = 64 if count <= 1025 else 1 << 17
    resident = [five] + rng.sample([k for k in distinct if k != five], min(len(distinct) - 1, capacity // 2 - 2))
    resident.append(rng.getrandbits(256).to_bytes(32, "big"))           # a record of nobody in the batch
    with W_.Pool(ctx, vks[0], vks[1], capacity) as pool:
        pool.import_keys(AUDITS, resident)
        pool.import_keys(NULLIFIERS, keys[:min(count, capacity // 2)])  # the other set is not the one consulted
        before = (pool.counts(), pool.state(), pool.contains(AUDITS, distinct[:64]))
        of, note = ctx.withdrawal_audit_plan(keys, pool)
        assert (of, note) == plan_model(keys, resident)
        assert [of[i] for i, k in enumerate(keys) if k == five] == [RESIDENT] * min(5, count)
        assert ctx.withdrawal_audit_plan(keys, pool) == (of, note)
        assert (pool.counts(), pool.state(), pool.contains(AUDITS, distinct[:64])) == before
        assert pool.counts() == (len(set(keys[:min(count, capacity // 2)])), len(resident))
    # v + r and a key with the same low 64 bits are not the resident key
    v = rng.randrange(1 << 253)
    a, b = v.to_bytes(32, "big"), (v + R).to_bytes(32, "big")
    c = bytes([a[0] ^ 0x40]) + a[1:]
    with W_.Pool(ctx, vks[0], vks[1], 8) as pool:
        pool.import_keys(AUDITS, [a])
        assert ctx.withdrawal_audit_plan([a, b, c, b, a], pool) == ([RESIDENT, 0, 1, 0, RESIDENT], [1, 2])


def test_resident_exactly_when_wallet_sync_reports_audited(ctx, vks):
    from spp import lib, witness as W_
    rng = random.Random(16)
    sks = [rng.randrange(1, 1 << 200) for _ in range(6)]
    deposits = [(sks[rng.randrange(6)], rng.randrange(1, 1 << 40), rng.randrange(1 << 250)) for _ in range(16)]
    with W_.ShieldedPoolMerkleTree(ctx, 16) as tree, W_.Pool(ctx, vks[0], vks[1], 64) as pool:
        tree.deposit(deposits)
        was = [rec[4] for rec in tree.sync(deposits)]
        pool.import_keys(AUDITS, list(dict.fromkeys(was))[::2])
        records = tree.sync(deposits, pool)
        audited = [bool(rec[1] & lib.SPP_WALLET_AUDITED) for rec in records]
        of, note = ctx.withdrawal_audit_plan([rec[4] for rec in records], pool)
        assert [s == RESIDENT for s in of] == audited and True in audited and False in audited
        assert (of, note) == plan_model([w.to_bytes(32, "big") for w in was], [w.to_bytes(32, "big") for w in list(dict.fromkeys(was))[::2]])


def test_refusals(ctx, vks):
    import spp
    from spp import lib, witness as W_
    L = ctx.L
    n = ctypes.c_uint32(9)
    out = (ctypes.c_uint32 * 4)()
    vp = ctypes.cast(out, ctypes.c_void_p)
    # count > 2^20: refused before anything is read (the key buffer is one key long)
    assert L.spp_withdrawal_audit_plan(ctx.h, None, lib.SPP_WITHDRAWALS_MAX + 1, bytes(32), vp, vp, ctypes.byref(n)) == -1
    assert "2^20" in spp.last_error() and n.value == 9
    other = spp.Context(0)
    try:
        with W_.Pool(other, vks[0], vks[1], 8) as pool:
            with pytest.raises(spp.SppError) as e:
                ctx.withdrawal_audit_plan([bytes(32)], pool)
            assert e.value.code == -1 and "another spp_ctx" in str(e.value)
            assert other.withdrawal_audit_plan([bytes(32)], pool) == ([0], [0])
    finally:
        other.close()
    assert ctx.withdrawal_audit_plan([]) == ([], [])
    for args in ((None, vp, vp, ctypes.byref(n)), (bytes(32), None, vp, ctypes.byref(n)), (bytes(32), vp, None, ctypes.byref(n)),
                 (bytes(32), vp, vp, None)):
        assert L.spp_withdrawal_audit_plan(ctx.h, None, 1, *args) == -1 and "NULL" in spp.last_error()
