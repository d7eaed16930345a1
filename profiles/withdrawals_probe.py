"""Withdrawals from notes (spp_prove_withdrawals) against the same work composed from the calls that existed before it, one GPU.

4 096 notes against a full depth-16 tree (65 536 deposits), both circuits resident with throughput tables planned under one budget.
  bundle     one spp.prove_withdrawals call: rows, plan, the withdraw proof of every note, one audit record per identity the pool
             does not hold, everything back on the host
  composed   what a caller did before: spp_prove_withdraw_notes_device for every note and spp_prove_audit_records_device for EVERY
             note, both enqueued before either is waited for (the two handles of bench.py's pair leg), then all outputs copied to
             the host.  Its inputs are resident on the device before the clock starts; the bundle's are host buffers.
The two paths alternate call by call in one run on one box (boxes of a pool differ by several percent); one warm-up pair, then the
median of --runs.  Three workloads: every identity distinct, each identity on four notes, every identity resident in the pool.
Also the plan alone (spp_withdrawal_audit_plan, host buffers in and out) at 2^16 and 2^20 keys, a third of them repeats.
Prints one JSON line and writes it to --out."""
import argparse, json, os, random, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before libspp: one HIP runtime)
import spp  # noqa: E402
from spp import witness as W, workload  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--notes", type=int, default=4096)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--budget", type=float, default=228e9, help="bytes of table memory for both circuits together")
ap.add_argument("--window", type=int, default=0, help="fixed window bits instead of the planned tables (quick runs)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "withdrawals_probe.json"))
args = ap.parse_args()
DEPTH, B = 16, args.notes
LEAVES = 1 << DEPTH
assert 4 <= B <= LEAVES and B % 4 == 0 and args.runs >= 1

dev = torch.device("cuda:0")
ctx = spp.Context(0)
rlwe_pk = json.load(open(os.path.join(ROOT, "tests", "golden", "rlwe_pk.json")))
tmp = tempfile.mkdtemp(prefix="spp_withdrawals_probe_")
paths = {}
for name, cid in (("audit", 2), ("withdraw", 1)):
    sppc, pkp, vkp = (os.path.join(tmp, name + "." + e) for e in ("sppc", "pk", "vk"))
    spp.build_circuit(cid, sppc, aux=(list(rlwe_pk["a"]) + list(rlwe_pk["b"])) if cid == 2 else None)
    ctx.setup(sppc, b"\x2a" * 32, pkp, vkp)
    paths[name] = (sppc, pkp, vkp)
if args.window:
    ha, hw = (ctx.load_circuit(paths[k][0], paths[k][1], args.window) for k in ("audit", "withdraw"))
else:
    plans = ctx.plan_windows([paths["audit"][1], paths["withdraw"][1]], args.budget)
    ha = ctx.load_circuit(paths["audit"][0], paths["audit"][1], bits=plans[0])
    hw = ctx.load_circuit(paths["withdraw"][0], paths["withdraw"][1], bits=plans[1])
wvk, avk = (open(paths[k][2], "rb").read() for k in ("withdraw", "audit"))

rng = random.Random(11)
ids = [rng.randrange(1, 1 << 128) for _ in range(B)]
_, r8, e18, e28 = workload.audit_noise(0, B)
pk_a, pk_b = (np.ascontiguousarray(rlwe_pk[k], dtype=np.uint32) for k in ("a", "b"))
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
d_pk = (up(pk_a), up(pk_b))
d_noise = (up(r8), up(e18), up(e28))
rs_pairs = [(1000003 * i + 17, 998244353 * i + 29) for i in range(B)]
d_rs = up(np.frombuffer(b"".join(x.to_bytes(32, "big") + y.to_bytes(32, "big") for x, y in rs_pairs), dtype=np.uint8))


def world(per_identity):
    """a full tree whose first B leaves are the notes, `per_identity` notes on each secret key"""
    sks = [ids[i // per_identity] for i in range(B)] + [rng.randrange(1, 1 << 128) for _ in range(LEAVES - B)]
    deps = [(sk, rng.randrange(1, 1 << 63), rng.randrange(1 << 253)) for sk in sks]
    tree = W.ShieldedPoolMerkleTree(ctx, DEPTH)
    tree.deposit(deps)
    notes = [(rng.randrange(1, 1 << 239), deps[i][1], deps[i][0], deps[i][2], i) for i in range(B)]
    return tree, notes


def composed(tree, d_notes, d_sk, outs):
    t0 = time.perf_counter()
    pr, pw, st, apr, apw, ast, c0, c1 = outs
    ha.prove_audit_records_device(B, d_pk[0].data_ptr(), d_pk[1].data_ptr(), d_sk.data_ptr(), d_noise[0].data_ptr(), d_noise[1].data_ptr(),
                                  d_noise[2].data_ptr(), d_rs.data_ptr(), apr.data_ptr(), apw.data_ptr(), ast.data_ptr(), c0.data_ptr(), c1.data_ptr())
    hw.prove_withdraw_notes_device(tree, B, d_notes.data_ptr(), d_rs.data_ptr(), pr.data_ptr(), pw.data_ptr(), st.data_ptr())
    ha.sync(); hw.sync()
    host = [t.cpu() for t in outs]
    dt = time.perf_counter() - t0
    assert int(host[2].abs().sum()) == 0 and int(host[5].abs().sum()) == 0
    return dt


def bundle(tree, notes, pool):
    t0 = time.perf_counter()
    b = spp.prove_withdrawals(hw, ha, tree, notes, pk_a, pk_b, r8, e18, e28, pool=pool, rs_withdraw=rs_pairs, rs_audit=rs_pairs)
    dt = time.perf_counter() - t0
    assert not any(b.status) and not any(b.audit_status)
    return dt, b


res = {"probe": "withdrawals_probe", "notes": B, "depth": DEPTH, "runs": args.runs, "tables": "window %d" % args.window if args.window else
       "planned under %.0f GB" % (args.budget / 1e9), "table_bytes": ha.table_bytes + hw.table_bytes}
z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)
outs = (z(388 * B, torch.uint8), z(hw.pw_len * B, torch.uint8), z(B, torch.int32), z(388 * B, torch.uint8), z(ha.pw_len * B, torch.uint8),
        z(B, torch.int32), z(64 * B, torch.int32), z(1024 * B, torch.int32))
ms = lambda xs: round(statistics.median(xs) * 1e3, 2)
for name, per_identity, resident in (("distinct", 1, False), ("four_notes_per_identity", 4, False), ("all_resident", 1, True)):
    tree, notes = world(per_identity)
    d_notes = up(np.frombuffer(W.pack_withdraw_notes(notes), dtype=np.uint8))
    d_sk = up(np.frombuffer(b"".join(n[2].to_bytes(32, "big") for n in notes), dtype=np.uint8))
    with W.Pool(ctx, wvk, avk, 2 * B) as pool:
        if resident:
            pool.import_keys(1, [rec[4] for rec in tree.sync([(n[2], n[1], n[3]) for n in notes])])
        tb, tc = [], []
        for run in range(args.runs + 1):                    # run 0 warms both paths up
            dt, b = bundle(tree, notes, pool)
            dc = composed(tree, d_notes, d_sk, outs)
            if run:
                tb.append(dt); tc.append(dc)
    tree.close()
    res[name] = {"n_audits": b.n_audits, "bundle_ms": ms(tb), "composed_ms": ms(tc), "bundle_pairs_per_s": round(B / statistics.median(tb), 1),
                 "composed_pairs_per_s": round(B / statistics.median(tc), 1), "bundle_runs_ms": [round(x * 1e3, 2) for x in tb],
                 "composed_runs_ms": [round(x * 1e3, 2) for x in tc]}
for logn in (16, 20):
    n = 1 << logn
    words = np.frombuffer(random.Random(logn).randbytes(32 * n), dtype=np.uint8).reshape(n, 32).copy()
    words[n // 3:2 * n // 3] = words[:2 * n // 3 - n // 3]              # a third of the keys repeat an earlier one
    keys = words.tobytes()
    ts = []
    for run in range(args.runs + 1):
        t0 = time.perf_counter()
        of, note = ctx.withdrawal_audit_plan([keys])                    # one buffer: no per-key packing inside the clock
        if run:
            ts.append(time.perf_counter() - t0)
    res["plan_2^%d_keys" % logn] = {"ms": ms(ts), "n_audits": len(note), "includes": "upload, five launches, download, and the Python lists of the result"}
ha.close(); hw.close(); ctx.close()

line = json.dumps(res)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
