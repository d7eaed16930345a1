"""Deposits into the resident tree, host side: the 72-byte deposit instruction body (deposit.rs:21-37), the packing of deposits
for spp_merkle_tree_deposit, and the per-deposit root rule of k_deposit_roots restated over the oracle's hashes."""
import random

import pytest

from oracle import hashes as H
from oracle.bn254 import R

KAT_COMMITMENT = 0x1d0a5a67676a2de671f28d445d2bab498ca1a6b0dccccbbe665039e9d3bf517f


def test_deposit_instruction_data_of_the_kat(withdraw_kat):
    """amount u64 LE | commitment | new_root (deposit.rs:22-36), written out by hand for the KAT's one deposit."""
    from spp.witness import deposit_instruction_data
    root = int(withdraw_kat["root"], 16)
    data = deposit_instruction_data(withdraw_kat["amount"], KAT_COMMITMENT, root)
    assert data == bytes.fromhex(
        "8096980000000000"                                                     # 10 000 000 = 0x989680, little-endian
        "1d0a5a67676a2de671f28d445d2bab498ca1a6b0dccccbbe665039e9d3bf517f"     # commitment, big-endian
        "0b5396cd78e7d0fb124fded66bf0acfb027d4d6817003874a9f05bd43049f5af")    # new_root, big-endian
    assert len(data) == 72
    assert deposit_instruction_data((1 << 64) - 1, 0, R - 1)[:8] == b"\xff" * 8
    for bad in ((1 << 64, 1, 1), (-1, 1, 1), (1, R, 1), (1, 1, R)):
        with pytest.raises(ValueError):
            deposit_instruction_data(*bad)


def test_pack_deposits_layout_and_range():
    from spp.witness import pack_deposits
    buf = pack_deposits([(1, 2, 3), (R, (1 << 64) - 1, (1 << 256) - 1)])
    assert len(buf) == 2 * 96
    assert buf[:96] == b"".join(v.to_bytes(32, "big") for v in (1, 2, 3))
    # values >= r still pack: the library refuses them and names the deposit
    assert buf[96:] == R.to_bytes(32, "big") + ((1 << 64) - 1).to_bytes(32, "big") + b"\xff" * 32
    assert pack_deposits([]) == b""
    for bad in ((1 << 256, 1, 1), (1, 1 << 256, 1), (1, 1, 1 << 256), (-1, 1, 1)):
        with pytest.raises(ValueError):
            pack_deposits([(5, 6, 7), bad])
    with pytest.raises(ValueError):
        pack_deposits([(1, 2)])


def _levels(leaves, depth, defaults):
    levels = [list(leaves)]
    for lv in range(depth):
        cur = levels[-1]
        levels.append([H.poseidon_hash2(cur[j], cur[j + 1] if j + 1 < len(cur) else defaults[lv]) for j in range(0, len(cur), 2)])
    return levels


def _deposit_root(levels, i, depth, defaults):
    """k_deposit_roots: the root after leaves 0..i, read from the tree after the whole call (levels) -- a left sibling covers only
    leaves < i (final), a right sibling only leaves > i (empty in the prefix tree: the level default)."""
    v = levels[0][i]
    for lv in range(depth):
        p = i >> lv
        v = H.poseidon_hash2(levels[lv][p - 1], v) if p & 1 else H.poseidon_hash2(v, defaults[lv])
    return v


@pytest.mark.parametrize("start", [0, 1, 7, 16])
def test_per_deposit_root_rule_equals_the_tree_after_every_insert(start):
    depth = 5
    defaults = H.default_hashes(depth)
    rng = random.Random(start)
    leaves = [rng.randrange(R) for _ in range(1 << depth)]
    prefix_roots = []
    orc = H.MerkleTree(depth)
    for leaf in leaves:
        orc.insert(leaf)
        prefix_roots.append(orc.root())
    # one call from `start` up to a full tree, and one that ends part way
    for end in (1 << depth, start + 5):
        levels = _levels(leaves[:end], depth, defaults)
        got = [_deposit_root(levels, i, depth, defaults) for i in range(start, end)]
        assert got == prefix_roots[start:end], (start, end)
