"""Deposit proofs from records against the resident tree (spp_prove_deposits_device) against the same proofs from rows built
beforehand (spp_prove_batch_device), one GPU, throughput tables (window 0 = auto); the withdraw-notes rate from the same process as
context.

A full depth-16 tree: 61 440 random leaves, then 4 096 deposits (spp_merkle_tree_deposit), so the batch is leaves 61 440 .. 65 535.
The rows leg proves the rows spp_deposit_rows_from_tree wrote (resident in HBM), which leaves k_deposit_rows out; the tree leg
proves the records (resident in HBM): k_deposit_rows runs in front of each batch on the tree's stream.  Legs of K pipelined steps,
ended by a device synchronise, alternate for R rounds; proofs/s = median over the rounds, and the spread of a leg = max - min of
its rounds.  The proofs of the two legs' last steps (same blinding) are compared byte for byte.  k_deposit_rows alone: the median
host time of a synchronous spp_deposit_rows_from_tree call for the batch (upload and download of 96 B / 768 B per deposit included)
-- the kernel's own duration needs a profiler run.
Prints one JSON line and writes it to --out (default profiles/deposit_proofs_probe.json)."""
import argparse, ctypes, json, os, random, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd"))
import torch  # noqa: E402  (before libspp: one HIP runtime)
import spp  # noqa: E402
from spp import witness as W  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--rows-calls", type=int, default=11, help="synchronous rows calls for the k_deposit_rows figure")
ap.add_argument("--no-withdraw", action="store_true", help="skip the withdraw-notes context leg")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deposit_proofs_probe.json"))
args = ap.parse_args()
B, K = args.batch, args.steps
assert 1 <= B <= 1 << 16
dev = torch.device("cuda", 0)
tmp = tempfile.mkdtemp()
ctx = spp.Context(0)
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def keys(cid, name):
    sppc, pkp, vkp = (os.path.join(tmp, name + "." + e) for e in ("sppc", "pk", "vk"))
    spp.build_circuit(cid, sppc)
    ctx.setup(sppc, b"\x2a" * 32, pkp, vkp)
    return sppc, pkp, vkp


up = lambda raw: torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
rng = random.Random(6)
first = (1 << 16) - B
tree = W.ShieldedPoolMerkleTree(ctx, 16)
if first:
    tree.insert_many([rng.randrange(R) for _ in range(first)])
records = [(rng.randrange(1, 1 << 128), rng.randrange(1, 1 << 40), rng.randrange(1 << 250)) for _ in range(B)]
assert tree.deposit(records)[0] == first and len(tree) == 1 << 16
rec_b = W.pack_deposits(records)
rows_buf = ctypes.create_string_buffer(B * 24 * 32)
rows_ms = []
for _ in range(args.rows_calls + 1):
    t0 = time.perf_counter()
    spp.lib.check(ctx.L.spp_deposit_rows_from_tree(tree.h, first, B, rec_b, ctypes.cast(rows_buf, ctypes.c_void_p)))
    rows_ms.append((time.perf_counter() - t0) * 1e3)
rows_ms = rows_ms[1:]

sppc, pkp, vkp = keys(6, "deposit")
t0 = time.time()
h = ctx.load_circuit(sppc, pkp, 0)
load_s = time.time() - t0
inp, d_rec = up(rows_buf.raw), up(rec_b)
rs = up(b"".join((1000003 * i + 17).to_bytes(32, "big") + (998244353 * i + 29).to_bytes(32, "big") for i in range(B)))
mk = lambda pw_len: [(torch.zeros(B * 388, dtype=torch.uint8, device=dev), torch.zeros(B * pw_len, dtype=torch.uint8, device=dev),
                      torch.ones(B, dtype=torch.int32, device=dev)) for _ in range(2)]
outs = {"rows": mk(h.pw_len), "tree": mk(h.pw_len)}
nstep = {"rows": 0, "tree": 0, "withdraw_notes": 0}


def step(path):
    k = nstep[path] & 1
    nstep[path] += 1
    pr, pw, st = (t.data_ptr() for t in outs[path][k])
    if path == "rows":
        h.prove_batch_device(B, inp.data_ptr(), rs.data_ptr(), pr, pw, st)
    elif path == "tree":
        h.prove_deposits_device(tree, first, B, d_rec.data_ptr(), rs.data_ptr(), pr, pw, st)
    else:
        hw.prove_withdraw_notes_device(tree, B, d_notes.data_ptr(), rs.data_ptr(), pr, pw, st)
    return k


def legs(paths, handle):
    for path in paths:
        for _ in range(args.warmup):
            step(path)
        handle.sync(); torch.cuda.synchronize()
    rate, last = {p: [] for p in paths}, {}
    for _ in range(args.rounds):
        for path in paths:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(K):
                last[path] = step(path)
            handle.sync(); torch.cuda.synchronize()
            rate[path].append(B * K / (time.perf_counter() - t0))
    return rate, last


rate, last = legs(("rows", "tree"), h)
status_ok = all(int(outs[p][last[p]][2].abs().sum().item()) == 0 for p in ("rows", "tree"))
proofs_equal = all(torch.equal(outs["rows"][last["rows"]][i], outs["tree"][last["tree"]][i]) for i in (0, 1))
vk = open(vkp, "rb").read()
pr, pw = (bytes(outs["tree"][last["tree"]][i].cpu().numpy()) for i in (0, 1))
t0 = time.perf_counter()
codes, end_root, end_index = W.verify_deposit_chain(ctx, vk, pr, pw, tree.root_at(first), first, lamports=[r[1] for r in records])
chain_ms = (time.perf_counter() - t0) * 1e3
chain_ok = codes == [0] * B and end_root == tree.getRoot() and end_index == 1 << 16
h.close()

withdraw = None
if not args.no_withdraw:
    wsppc, wpkp, _ = keys(1, "withdraw")
    hw = ctx.load_circuit(wsppc, wpkp, 0)
    recipients = [rng.randrange(1, 1 << 240) for _ in range(B)]
    d_notes = up(W.pack_withdraw_notes([(recipients[i], records[i][1], records[i][0], records[i][2], first + i) for i in range(B)]))
    outs["withdraw_notes"] = mk(hw.pw_len)
    wrate, wlast = legs(("withdraw_notes",), hw)
    withdraw = {"proofs_per_s": round(statistics.median(wrate["withdraw_notes"]), 1), "rounds": [round(v, 1) for v in wrate["withdraw_notes"]],
                "all_status_zero": int(outs["withdraw_notes"][wlast["withdraw_notes"]][2].abs().sum().item()) == 0}
    hw.close()
tree.close()
ctx.close()

med = {p: statistics.median(v) for p, v in rate.items()}
spread = {p: max(v) - min(v) for p, v in rate.items()}
res = {
    "probe": "deposit_proofs_probe",
    "circuit": "deposit (depth 16; 11 093 constraints, domain 2^14)",
    "batch": B, "first_index": first, "steps_per_leg": K, "rounds": args.rounds, "warmup": args.warmup, "window_bits": "auto (0)",
    "load_s": round(load_s, 2),
    "from_rows_proofs_per_s": round(med["rows"], 1),
    "from_tree_proofs_per_s": round(med["tree"], 1),
    "tree_over_rows": round(med["tree"] / med["rows"], 4),
    "from_rows_rounds": [round(v, 1) for v in rate["rows"]],
    "from_tree_rounds": [round(v, 1) for v in rate["tree"]],
    "from_rows_spread": round(spread["rows"], 1),
    "difference_within_from_rows_spread": abs(med["tree"] - med["rows"]) <= spread["rows"],
    "deposit_rows_call_ms": {"median": round(statistics.median(rows_ms), 3), "min": round(min(rows_ms), 3), "max": round(max(rows_ms), 3),
                             "calls": len(rows_ms), "what": "host time of spp_deposit_rows_from_tree, copies included"},
    "verify_deposit_chain_ms": round(chain_ms, 2), "chain_all_ok_and_ends_in_the_tree_root": chain_ok,
    "proofs_and_pws_byte_equal_last_step": proofs_equal,
    "all_status_zero": status_ok,
    "withdraw_notes_same_process": withdraw,
}
line = json.dumps(res)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
