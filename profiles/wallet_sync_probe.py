"""Wallet sync (spp_wallet_sync) against the same answers composed from the calls that existed before it, one GPU.

A depth-16 tree filled with 65 536 deposits, the same 65 536 secrets shuffled, a pool holding the nullifiers of half of them.
(a) one spp_wallet_sync call on a tree that has no leaf index yet (it builds it: one insert launch over all leaves);
(b) the same call again on that tree (the index is reused);
(c) the composition: spp_grumpkin_keygen_batch, spp_poseidon_hash_batch twice (commitment, wa_commitment), a host dictionary
    over the leaf list (built inside the clock: it is the composition's index) and its lookups, spp_poseidon_hash_batch for the
    nullifiers, spp_pool_contains twice.  Its buffers are put together with numpy, not per element.
All three in one run; every timing is host wall time around calls that end in a device synchronise, inputs packed beforehand;
one warm-up, then the median of --runs runs, each of (a) on a fresh tree (made outside the clock by spp_merkle_tree_insert of
the same leaves).  The outputs of (b) and (c) are compared.  Prints one JSON line and writes it to --out."""
import argparse, ctypes, json, os, random, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before libspp: one HIP runtime)
import spp  # noqa: E402
from spp import witness as W  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--count", type=int, default=1 << 16)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wallet_sync_probe.json"))
args = ap.parse_args()
DEPTH, N = 16, args.count
assert 2 <= N <= 1 << DEPTH and args.runs >= 1

ctx = spp.Context(0)
L, check = ctx.L, spp.lib.check
npp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
inp = lambda a: ctypes.c_char_p(a.ctypes.data)             # the input arguments are declared char pointers
rng = random.Random(5)
deps = [(rng.randrange(1, 1 << 128), rng.randrange(1, 1 << 63), rng.randrange(1 << 253)) for _ in range(N)]
order = list(range(N))
rng.shuffle(order)
secrets = np.frombuffer(W.pack_deposits([deps[k] for k in order]), dtype=np.uint8).reshape(N, 3, 32).copy()
sks = np.ascontiguousarray(secrets[:, 0])
golden = os.path.join(ROOT, "tests", "golden")
wvk, avk = (open(os.path.join(golden, n), "rb").read() for n in ("reference_withdraw.vk", "reference_audit.vk"))

with W.ShieldedPoolMerkleTree(ctx, DEPTH) as t0_:
    _, leaves, _ = t0_.deposit(deps)
leaves_be = b"".join(v.to_bytes(32, "big") for v in leaves)


def fresh_tree():
    t = W.ShieldedPoolMerkleTree(ctx, DEPTH)
    check(L.spp_merkle_tree_insert(t.h, N, leaves_be, None))
    return t


def sync_call(tree, pool):
    idx, flags, rec = np.zeros(N, np.uint64), np.zeros(N, np.uint32), np.zeros((N, 5, 32), np.uint8)
    t0 = time.perf_counter()
    check(L.spp_wallet_sync(tree.h, pool.h if pool else None, N, inp(secrets), None, npp(idx), npp(flags), npp(rec), None))
    return time.perf_counter() - t0, idx, flags, rec


def composed(pool):
    t0 = time.perf_counter()
    xy = np.zeros((N, 2, 32), np.uint8)
    check(L.spp_grumpkin_keygen_batch(ctx.h, N, inp(sks), npp(xy)))
    h4 = np.ascontiguousarray(np.concatenate([xy, secrets[:, 1:3]], axis=1))
    com, wa, nf = (np.zeros((N, 32), np.uint8) for _ in range(3))
    check(L.spp_poseidon_hash_batch(ctx.h, N, 4, inp(h4), npp(com)))
    check(L.spp_poseidon_hash_batch(ctx.h, N, 2, inp(xy), npp(wa)))
    t1 = time.perf_counter()
    where = {}
    for i in range(N - 1, -1, -1):                          # descending: the lowest index of a repeated value stays
        where[leaves_be[32 * i:32 * i + 32]] = i
    cb = com.tobytes()
    idx = np.array([where.get(cb[32 * i:32 * i + 32], W.WALLET_ABSENT) for i in range(N)], dtype=np.uint64)
    t2 = time.perf_counter()
    h2 = np.zeros((N, 2, 32), np.uint8)
    h2[:, 0] = secrets[:, 0]
    h2[:, 1, 24:] = idx.astype(">u8").view(np.uint8).reshape(N, 8)
    check(L.spp_poseidon_hash_batch(ctx.h, N, 2, inp(h2), npp(nf)))
    spent, audited = np.zeros(N, np.uint8), np.zeros(N, np.uint8)
    check(L.spp_pool_contains(pool.h, 0, N, inp(nf), npp(spent)))
    check(L.spp_pool_contains(pool.h, 1, N, inp(wa), npp(audited)))
    flags = (1 + 2 * spent.astype(np.uint32) + 4 * audited.astype(np.uint32))
    rec = np.stack([com, nf, wa, xy[:, 0], xy[:, 1]], axis=1)
    t3 = time.perf_counter()
    return t3 - t0, t2 - t1, idx, flags, rec


res = {"probe": "wallet_sync_probe", "depth": DEPTH, "count": N, "runs": args.runs}
with W.Pool(ctx, wvk, avk, N) as pool:
    with fresh_tree() as tree:
        _, _, _, rec = sync_call(tree, None)                # the nullifiers, for the pool
    pool.import_keys(0, [rec[i, 1].tobytes() for i in range(0, N, 2)])
    first, second, comp, comp_dict = [], [], [], []
    for run in range(args.runs + 1):                        # run 0 is the warm-up of all three
        with fresh_tree() as tree:
            a = sync_call(tree, pool)
            b = sync_call(tree, pool)
        c = composed(pool)
        if run:
            first.append(a[0]); second.append(b[0]); comp.append(c[0]); comp_dict.append(c[1])
    res["outputs_equal"] = bool((b[1] == c[2]).all() and (b[2] == c[3]).all() and (b[3] == c[4]).all() and (a[1] == b[1]).all()
                                and (a[2] == b[2]).all())
    res["spent"] = int(((b[2] & 2) != 0).sum())
    res["found"] = int((b[1] != W.WALLET_ABSENT).sum())
ms = lambda xs: round(statistics.median(xs) * 1e3, 3)
res["a_first_call_builds_index_ms"] = ms(first)
res["b_second_call_ms"] = ms(second)
res["c_composed_ms"] = ms(comp)
res["c_host_dictionary_ms"] = ms(comp_dict)
for k, xs in (("a", first), ("b", second), ("c", comp)):
    res[k + "_runs_ms"] = [round(x * 1e3, 3) for x in xs]
res["c_over_b"] = round(res["c_composed_ms"] / res["b_second_call_ms"], 2)
res["c_over_a"] = round(res["c_composed_ms"] / res["a_first_call_builds_index_ms"], 2)
ctx.close()

line = json.dumps(res)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
