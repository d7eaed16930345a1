"""The resident tree through the N-API addon and the CommonJS twin of proof.helper.ts: deposit from secrets, then withdraw from
notes against the same tree (ShieldedPoolMerkleTree.deposit, generateProofsFromTree).  Skipped when node or its headers are
absent."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

NODE_DIR = os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd", "node")
pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"),
                                 reason="node toolchain not present")]


@pytest.fixture(scope="module")
def helper():
    subprocess.run(["make", "-C", NODE_DIR, "-s"], check=True)
    return os.path.join(NODE_DIR, "proof.helper.js")


def test_deposit_then_withdraw_through_node(helper, withdraw_artifacts, withdraw_kat, tmp_path):
    from spp.witness import deposit_instruction_data
    cdir = tmp_path / "noir_circuit"
    os.makedirs(cdir / "target")
    shutil.copy(withdraw_artifacts["sppc"], cdir / "target" / "shielded_pool_verifier.sppc")
    shutil.copy(withdraw_artifacts["pk"], cdir / "target" / "shielded_pool_verifier.pk")
    k = withdraw_kat
    script = """
      const h = require(%s);
      const fs = require('fs');
      const k = %s;
      const hex = (v) => '0x' + v.toString(16).padStart(64, '0');
      const tree = new h.ShieldedPoolMerkleTree(16);
      const [d] = tree.deposit([{secret_key: k.secret_key, amount: k.amount, randomness: k.randomness}]);
      const cfg = {circuitDir: %s, circuitName: 'shielded_pool_verifier'};
      const [p] = h.generateProofsFromTree(cfg, tree, [{recipient: k.recipient, amount: k.amount, secret_key: k.secret_key,
                                                        randomness: k.randomness, index: d.index}]);
      const vk = fs.readFileSync(%s);
      let threw = '';
      try { tree.deposit([{secret_key: k.secret_key, amount: (1n << 64n).toString(), randomness: k.randomness}]); }
      catch (e) { threw = e.message; }
      process.stdout.write(JSON.stringify({
        index: d.index, commitment: hex(d.commitment), root: hex(d.root), getRoot: hex(tree.getRoot()), size: tree.size,
        proof0: tree.getProof(0).map(hex), ix: d.instructionData.toString('hex'),
        ok: h.addon.verify(vk, p.proof, p.publicWitness), pwRoot: p.publicWitness.slice(12, 44).toString('hex'),
        threw, sizeAfter: tree.size }));
    """ % (json.dumps(helper), json.dumps(k), json.dumps(str(cdir)), json.dumps(withdraw_artifacts["vk"]))
    r = subprocess.run(["node", "-e", script], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    root = int(k["root"], 16)
    assert out["index"] == 0 and int(out["root"], 16) == root == int(out["getRoot"], 16) and out["size"] == 1
    assert out["commitment"].startswith("0x1d0a5a67")
    assert [int(s, 16) for s in out["proof0"]] == [int(s, 16) for s in k["siblings"]]
    assert bytes.fromhex(out["ix"]) == deposit_instruction_data(k["amount"], int(out["commitment"], 16), root)
    assert out["ok"] is True and int(out["pwRoot"], 16) == root
    assert out["threw"].startswith("libspp error -1") and "amount" in out["threw"] and out["sizeAfter"] == 1
