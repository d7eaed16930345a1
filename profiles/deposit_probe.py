"""Deposits into the resident tree (spp_merkle_tree_deposit) against the reference-shaped loop, one GPU.

(a) one call depositing 65 536 notes into an empty depth-16 tree (filling it);
(b) one call depositing 4 096 notes into an empty depth-16 tree;
(c) the loop client/payroll-demo.ts / test-shielded-pool.ts runs per deposit, for the same 4 096 deposits: insert(1) then
    getRoot() (spp_merkle_tree_insert + spp_merkle_tree_root).  Its commitments are precomputed on the device
    (spp_grumpkin_keygen_batch + spp_poseidon_hash_batch), so only the tree path is compared.
Every timing is host wall time around calls that end in a device synchronise, on a fresh tree (created outside the clock),
packing done beforehand; median over --trees trees after one warm-up tree per leg.  The roots of (b) and (c) are compared, and
(a)'s last root against a tree fed with insert_many of its commitments.
Prints one JSON line and writes it to --out (default profiles/deposit_probe.json)."""
import argparse, ctypes, json, os, random, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd"))
import torch  # noqa: E402,F401  (before libspp: one HIP runtime)
import spp  # noqa: E402
from spp import witness as W  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--full", type=int, default=1 << 16)
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--trees", type=int, default=5, help="timed fresh trees per leg (median)")
ap.add_argument("--loop-trees", type=int, default=3, help="timed fresh trees for the per-deposit loop (c)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deposit_probe.json"))
args = ap.parse_args()
DEPTH = 16
assert args.full <= 1 << DEPTH and args.batch <= args.full

ctx = spp.Context(0)
L = ctx.L
rng = random.Random(3)
deps = [(rng.randrange(1, 1 << 128), rng.randrange(1, 1 << 63), rng.randrange(1 << 253)) for _ in range(args.full)]
buf = W.pack_deposits(deps)
vp = lambda b: ctypes.cast(b, ctypes.c_void_p)


def deposit_call(n):
    """one spp_merkle_tree_deposit of the first n deposits into a fresh tree: (seconds, commitments, roots, tree)"""
    tree = W.ShieldedPoolMerkleTree(ctx, DEPTH)
    first = ctypes.c_uint64(0)
    com, roots = ctypes.create_string_buffer(32 * n), ctypes.create_string_buffer(32 * n)
    b = buf[:96 * n]
    t0 = time.perf_counter()
    spp.lib.check(L.spp_merkle_tree_deposit(tree.h, n, b, ctypes.byref(first), vp(com), vp(roots)))
    dt = time.perf_counter() - t0
    return dt, com.raw, roots.raw, tree


def loop_call(leaves_be, n):
    """the reference-shaped loop: insert(1) + getRoot() per deposit, on a fresh tree"""
    tree = W.ShieldedPoolMerkleTree(ctx, DEPTH)
    root = ctypes.create_string_buffer(32)
    roots = bytearray()
    first = ctypes.c_uint64(0)
    t0 = time.perf_counter()
    for k in range(n):
        spp.lib.check(L.spp_merkle_tree_insert(tree.h, 1, leaves_be[32 * k:32 * k + 32], ctypes.byref(first)))
        spp.lib.check(L.spp_merkle_tree_root(tree.h, vp(root)))
        roots += root.raw
    dt = time.perf_counter() - t0
    tree.close()
    return dt, bytes(roots)


res = {"probe": "deposit_probe", "depth": DEPTH, "full": args.full, "batch": args.batch, "trees": args.trees,
       "loop_trees": args.loop_trees}
# (a) and (b): one warm-up tree each, then the timed fresh trees
legs = {}
for name, n in (("a_full", args.full), ("b_batch", args.batch)):
    deposit_call(n)[3].close()
    times = []
    for r in range(args.trees):
        dt, com, roots, t = deposit_call(n)
        times.append(dt)
        if r < args.trees - 1:
            t.close()
    legs[name] = (com, roots, t)                           # the last tree's outputs, checked below
    res[name + "_ms"] = round(statistics.median(times) * 1e3, 3)
    res[name + "_runs_ms"] = [round(x * 1e3, 3) for x in times]
    res[name + "_deposits_per_s"] = round(n / statistics.median(times), 1)

# (a): the final root against a tree fed with insert_many of the returned commitments
com_a, roots_a, tree_a = legs["a_full"]
commitments_a = [int.from_bytes(com_a[32 * i:32 * i + 32], "big") for i in range(args.full)]
with W.ShieldedPoolMerkleTree(ctx, DEPTH) as twin:
    twin.insert_many(commitments_a)
    res["a_final_root_equals_insert_many"] = twin.getRoot() == int.from_bytes(roots_a[-32:], "big") == tree_a.getRoot()
tree_a.close()
legs["b_batch"][2].close()

# (c): commitments of the same first `batch` deposits through the two batch calls, then the loop
owners = W.identity_public_keys(ctx, [d[0] for d in deps[:args.batch]])
leaves = W.poseidon_hash_batch(ctx, [[o[0], o[1], d[1], d[2]] for o, d in zip(owners, deps[:args.batch])])
leaves_be = b"".join(v.to_bytes(32, "big") for v in leaves)
res["b_commitments_equal_keygen_plus_poseidon"] = legs["b_batch"][0] == leaves_be
loop_call(leaves_be, 64)                                   # warm-up
loop_times, loop_roots = [], None
for _ in range(args.loop_trees):
    dt, loop_roots = loop_call(leaves_be, args.batch)
    loop_times.append(dt)
res["c_loop_ms"] = round(statistics.median(loop_times) * 1e3, 3)
res["c_loop_runs_ms"] = [round(x * 1e3, 3) for x in loop_times]
res["c_loop_deposits_per_s"] = round(args.batch / statistics.median(loop_times), 1)
res["b_roots_equal_c_loop_roots"] = legs["b_batch"][1] == loop_roots
res["a_over_c_time"] = round(res["a_full_ms"] / res["c_loop_ms"], 4)
res["b_over_c_speedup"] = round(res["c_loop_ms"] / res["b_batch_ms"], 1)
ctx.close()

line = json.dumps(res)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
