"""Withdraw proofs from notes (spp_prove_withdraw_notes_device) against withdraw proofs from rows (spp_prove_batch_device), one GPU,
hand-written withdraw circuit, throughput tables (window 0 = auto).

4 096 distinct notes in ONE depth-16 resident tree (the draws of spp.workload.withdraw_rows, seed 2).  The rows path proves the rows
that workload.withdraw_rows assembles with six library calls (resident in HBM); the notes path proves the notes (resident in HBM)
against the resident tree: k_withdraw_rows runs in front of each batch.  Legs of K pipelined steps, ended by a device synchronise,
alternate for R rounds; proofs/s = median over the rounds.  The proofs of the two paths' last steps (same blinding) are compared
byte for byte.  Single-proof latency both ways with 8-bit tables (median of alternating calls).
Prints one JSON line and writes it to --out (default profiles/withdraw_notes_probe.json)."""
import argparse, ctypes, json, os, random, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd"))
import torch  # noqa: E402  (before libspp: one HIP runtime)
import spp  # noqa: E402
from spp import workload, witness as W  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--single", type=int, default=20, help="single-proof calls per path")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "withdraw_notes_probe.json"))
args = ap.parse_args()
B, K = args.batch, args.steps
assert K >= 5
dev = torch.device("cuda", 0)
tmp = tempfile.mkdtemp()
sppc, pkp, vkp = (os.path.join(tmp, "w." + e) for e in ("sppc", "pk", "vk"))
spp.build_circuit(1, sppc)
ctx = spp.Context(0)
ctx.setup(sppc, b"\x2a" * 32, pkp, vkp)
t0 = time.time()
h = ctx.load_circuit(sppc, pkp, 0)
load_s = time.time() - t0

# ---- the same 4 096 notes as workload.withdraw_rows(ctx, B, seed=2): same draws, same tree ----
rng = random.Random(2)
sks = [rng.randrange(1, 1 << 128) for _ in range(B)]
amounts = [rng.randrange(1, 1 << 40) for _ in range(B)]
rnds = [rng.randrange(1 << 250) for _ in range(B)]
recipients = [rng.randrange(1, 1 << 240) for _ in range(B)]
owners = W.identity_public_keys(ctx, sks)
tree = W.ShieldedPoolMerkleTree(ctx, 16)
tree.insert_many(W.poseidon_hash_batch(ctx, [[o[0], o[1], a, r] for o, a, r in zip(owners, amounts, rnds)]))
notes = [(recipients[i], amounts[i], sks[i], rnds[i], i) for i in range(B)]
notes_b = W.pack_withdraw_notes(notes)
rows_b = workload.withdraw_rows(ctx, B, seed=2)
rows_tree = ctypes.create_string_buffer(len(rows_b))
spp.lib.check(ctx.L.spp_withdraw_rows_from_tree(tree.h, B, notes_b, ctypes.cast(rows_tree, ctypes.c_void_p)))
rows_equal = rows_tree.raw == rows_b

up = lambda raw: torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
inp, d_notes = up(rows_b), up(notes_b)
rs = up(b"".join((1000003 * i + 17).to_bytes(32, "big") + (998244353 * i + 29).to_bytes(32, "big") for i in range(B)))
outs = {p: [(torch.zeros(B * 388, dtype=torch.uint8, device=dev), torch.zeros(B * h.pw_len, dtype=torch.uint8, device=dev),
             torch.ones(B, dtype=torch.int32, device=dev)) for _ in range(2)] for p in ("rows", "notes")}
nstep = {"rows": 0, "notes": 0}


def step(path):
    k = nstep[path] & 1
    nstep[path] += 1
    pr, pw, st = (t.data_ptr() for t in outs[path][k])
    if path == "rows":
        h.prove_batch_device(B, inp.data_ptr(), rs.data_ptr(), pr, pw, st)
    else:
        h.prove_withdraw_notes_device(tree, B, d_notes.data_ptr(), rs.data_ptr(), pr, pw, st)
    return k


for path in ("rows", "notes"):
    for _ in range(args.warmup):
        step(path)
    h.sync(); torch.cuda.synchronize()
rate = {"rows": [], "notes": []}
last = {}
for _ in range(args.rounds):
    for path in ("rows", "notes"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(K):
            last[path] = step(path)
        h.sync(); torch.cuda.synchronize()
        rate[path].append(B * K / (time.perf_counter() - t0))
status_ok = all(int(outs[p][last[p]][2].abs().sum().item()) == 0 for p in ("rows", "notes"))
proofs_equal = all(torch.equal(outs["rows"][last["rows"]][i], outs["notes"][last["notes"]][i]) for i in (0, 1))
h.close()

# ---- single proof, 8-bit tables ----
h8 = ctx.load_circuit(sppc, pkp, 8)
one = {p: (torch.zeros(388, dtype=torch.uint8, device=dev), torch.zeros(h8.pw_len, dtype=torch.uint8, device=dev),
           torch.ones(1, dtype=torch.int32, device=dev)) for p in ("rows", "notes")}
lat = {"rows": [], "notes": []}
for it in range(args.single + 2):
    for path in ("rows", "notes"):
        pr, pw, st = (t.data_ptr() for t in one[path])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if path == "rows":
            h8.prove_batch_device(1, inp.data_ptr(), rs.data_ptr(), pr, pw, st)
        else:
            h8.prove_withdraw_notes_device(tree, 1, d_notes.data_ptr(), rs.data_ptr(), pr, pw, st)
        h8.sync()
        if it >= 2:
            lat[path].append((time.perf_counter() - t0) * 1e3)
single_ok = all(int(one[p][2].item()) == 0 for p in one) and torch.equal(one["rows"][0], one["notes"][0])
h8.close()
tree.close()
ctx.close()

med = {p: statistics.median(v) for p, v in rate.items()}
res = {
    "probe": "withdraw_notes_probe",
    "circuit": "withdraw (hand-written, depth 16)",
    "batch": B, "steps_per_leg": K, "rounds": args.rounds, "warmup": args.warmup, "window_bits": "auto (0)", "load_s": round(load_s, 2),
    "rows_path_proofs_per_s": round(med["rows"], 1),
    "notes_path_proofs_per_s": round(med["notes"], 1),
    "notes_over_rows": round(med["notes"] / med["rows"], 4),
    "rows_path_rounds": [round(v, 1) for v in rate["rows"]],
    "notes_path_rounds": [round(v, 1) for v in rate["notes"]],
    "single_proof_ms_8bit": {"rows_path": round(statistics.median(lat["rows"]), 3), "notes_path": round(statistics.median(lat["notes"]), 3),
                             "calls": args.single},
    "rows_from_tree_equal_workload_rows": rows_equal,
    "proofs_and_pws_byte_equal_last_step": proofs_equal,
    "single_proof_byte_equal": single_ok,
    "all_status_zero": status_ok,
}
line = json.dumps(res)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
