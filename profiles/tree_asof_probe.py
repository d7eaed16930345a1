"""The resident tree as of an earlier size: what the as-of calls cost beside the calls on the tree as it stands, one GPU.

A FULL depth-16 tree (65 536 leaves; the first 4 096 are the commitments of 4 096 notes, the draws of withdraw_notes_probe.py, the rest
random field elements) and those 4 096 notes, all of them leaves of the prefix of 32 768.
  rows      spp_withdraw_rows_from_tree_at(size = 32 768) against (a) spp_withdraw_rows_from_tree on the same tree and (b) the only way
            without the as-of calls: a second tree built from the first 32 768 leaves, then its rows.  Host calls, transfers included,
            median of --calls; the rows of the as-of call and of (b) are compared byte for byte.
  proofs    spp_prove_withdraw_notes_at_device(size = 32 768) against spp_prove_withdraw_notes_device, legs of K pipelined steps
            alternating for R rounds as in withdraw_notes_probe.py, throughput tables (window 0); the public roots are checked.
  find      spp_merkle_tree_find_roots for the 2^16 roots of sizes 1 .. 65 536: the first call (walks all 65 537 prefix roots, builds the
            index) and the second.
  sizes     one spp_pool_root_sizes call (40 roots pushed), median of --calls.
Prints one JSON line and writes it to --out (default profiles/tree_asof_probe.json)."""
import argparse, ctypes, json, os, random, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd"))
import torch  # noqa: E402  (before libspp: one HIP runtime)
import spp  # noqa: E402
from spp import witness as W  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--size", type=int, default=32768)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--calls", type=int, default=11)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_asof_probe.json"))
args = ap.parse_args()
B, K, SIZE, DEPTH = args.batch, args.steps, args.size, 16
FULL = 1 << DEPTH
R_MOD = W.FR_MODULUS
dev = torch.device("cuda", 0)
tmp = tempfile.mkdtemp()
sppc, pkp, vkp = (os.path.join(tmp, "w." + e) for e in ("sppc", "pk", "vk"))
spp.build_circuit(1, sppc)
ctx = spp.Context(0)
ctx.setup(sppc, b"\x2a" * 32, pkp, vkp)
h = ctx.load_circuit(sppc, pkp, 0)
L = ctx.L

rng = random.Random(2)
sks = [rng.randrange(1, 1 << 128) for _ in range(B)]
amounts = [rng.randrange(1, 1 << 40) for _ in range(B)]
rnds = [rng.randrange(1 << 250) for _ in range(B)]
recipients = [rng.randrange(1, 1 << 240) for _ in range(B)]
owners = W.identity_public_keys(ctx, sks)
leaves = W.poseidon_hash_batch(ctx, [[o[0], o[1], a, r] for o, a, r in zip(owners, amounts, rnds)])
leaves += [rng.randrange(1, R_MOD) for _ in range(FULL - B)]
tree = W.ShieldedPoolMerkleTree(ctx, DEPTH)
tree.insert_many(leaves)
notes_b = W.pack_withdraw_notes([(recipients[i], amounts[i], sks[i], rnds[i], i) for i in range(B)])
row_bytes = (10 + DEPTH) * 32
vp = lambda b: ctypes.cast(b, ctypes.c_void_p)


def timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


# ---- rows ----
rows_now, rows_at, rows_second = (ctypes.create_string_buffer(B * row_bytes) for _ in range(3))
ms = {"now": [], "at": [], "second_tree": []}
for it in range(args.calls + 1):
    a = timed(lambda: spp.lib.check(L.spp_withdraw_rows_from_tree(tree.h, B, notes_b, vp(rows_now))))
    b = timed(lambda: spp.lib.check(L.spp_withdraw_rows_from_tree_at(tree.h, SIZE, B, notes_b, vp(rows_at))))
    if it:
        ms["now"].append(a); ms["at"].append(b)
leaves_b = b"".join(v.to_bytes(32, "big") for v in leaves[:SIZE])


def second_tree():
    t = ctypes.c_void_p()
    spp.lib.check(L.spp_merkle_tree_new(ctx.h, DEPTH, ctypes.byref(t)))
    spp.lib.check(L.spp_merkle_tree_insert(t, SIZE, leaves_b, None))
    spp.lib.check(L.spp_withdraw_rows_from_tree(t, B, notes_b, vp(rows_second)))
    L.spp_merkle_tree_free(t)


for it in range(4):
    c = timed(second_tree)
    if it:
        ms["second_tree"].append(c)
rows_equal = rows_at.raw == rows_second.raw
root_at = tree.root_at(SIZE)

# ---- proofs ----
up = lambda raw: torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
d_notes = up(notes_b)
rs = up(b"".join((1000003 * i + 17).to_bytes(32, "big") + (998244353 * i + 29).to_bytes(32, "big") for i in range(B)))
outs = {p: [(torch.zeros(B * 388, dtype=torch.uint8, device=dev), torch.zeros(B * h.pw_len, dtype=torch.uint8, device=dev),
             torch.ones(B, dtype=torch.int32, device=dev)) for _ in range(2)] for p in ("now", "at")}
nstep = {"now": 0, "at": 0}


def step(path):
    k = nstep[path] & 1
    nstep[path] += 1
    pr, pw, st = (t.data_ptr() for t in outs[path][k])
    h.prove_withdraw_notes_device(tree, B, d_notes.data_ptr(), rs.data_ptr(), pr, pw, st, size=None if path == "now" else SIZE)
    return k


for path in ("now", "at"):
    for _ in range(args.warmup):
        step(path)
    h.sync(); torch.cuda.synchronize()
rate = {"now": [], "at": []}
last = {}
for _ in range(args.rounds):
    for path in ("now", "at"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(K):
            last[path] = step(path)
        h.sync(); torch.cuda.synchronize()
        rate[path].append(B * K / (time.perf_counter() - t0))
status_ok = all(int(outs[p][last[p]][2].abs().sum().item()) == 0 for p in ("now", "at"))
pw_at = bytes(outs["at"][last["at"]][1].cpu().numpy())
pw_now = bytes(outs["now"][last["now"]][1].cpu().numpy())
roots_ok = all(int.from_bytes(pw_at[h.pw_len * i + 12:h.pw_len * i + 44], "big") == root_at for i in range(B)) and \
    all(int.from_bytes(pw_now[h.pw_len * i + 12:h.pw_len * i + 44], "big") == tree.getRoot() for i in range(B))
h.close()

# ---- find_roots: this tree has not built its prefix roots or its root index yet ----
golden = os.path.join(ROOT, "tests", "golden")
wvk, avk = (open(os.path.join(golden, n), "rb").read() for n in ("reference_withdraw.vk", "reference_audit.vk"))
with W.ShieldedPoolMerkleTree(ctx, DEPTH) as t2:
    t2.insert_many(leaves)
    want = t2.prefix_roots(1, FULL)
    keys = b"".join(v.to_bytes(32, "big") for v in want)
with W.ShieldedPoolMerkleTree(ctx, DEPTH) as t3, W.Pool(ctx, wvk, avk, 64) as pool:
    t3.insert_many(leaves)
    sizes = (ctypes.c_uint64 * FULL)()
    find_first = timed(lambda: spp.lib.check(L.spp_merkle_tree_find_roots(t3.h, FULL, keys, vp(sizes), None)))
    find_ok = list(sizes) == list(range(1, FULL + 1))
    find_second = [timed(lambda: spp.lib.check(L.spp_merkle_tree_find_roots(t3.h, FULL, keys, vp(sizes), None))) for _ in range(5)]
    pool.add_roots(want[SIZE - 40:SIZE])
    rs_ms = []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        got = pool.root_sizes(t3)
        rs_ms.append((time.perf_counter() - t0) * 1e3)
    sizes_ok = got[1] == SIZE and got[0][0] == SIZE
tree.close()
ctx.close()

med = {p: statistics.median(v) for p, v in rate.items()}
mm = {p: statistics.median(v) for p, v in ms.items()}
res = {
    "probe": "tree_asof_probe", "circuit": "withdraw (hand-written, depth 16)", "tree_leaves": FULL, "notes": B, "size": SIZE,
    "rows_ms": {"current_size": round(mm["now"], 3), "as_of": round(mm["at"], 3), "second_tree_then_rows": round(mm["second_tree"], 3),
                "calls": args.calls},
    "rows_as_of_over_current": round(mm["at"] / mm["now"], 4),
    "rows_second_tree_over_as_of": round(mm["second_tree"] / mm["at"], 2),
    "steps_per_leg": K, "rounds": args.rounds, "warmup": args.warmup, "window_bits": "auto (0)",
    "proofs_per_s": {"current_size": round(med["now"], 1), "as_of": round(med["at"], 1)},
    "proofs_as_of_over_current": round(med["at"] / med["now"], 4),
    "current_size_rounds": [round(v, 1) for v in rate["now"]], "as_of_rounds": [round(v, 1) for v in rate["at"]],
    "find_roots_ms": {"roots": FULL, "first_call": round(find_first, 3), "second_call": round(statistics.median(find_second), 3)},
    "root_sizes_ms": round(statistics.median(rs_ms), 3),
    "rows_as_of_equal_second_tree": rows_equal, "public_roots_ok": roots_ok, "all_status_zero": status_ok,
    "find_roots_ok": find_ok, "root_sizes_ok": sizes_ok,
}
line = json.dumps(res)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
