"""The pool ledger on one GPU: what settling costs on top of verifying, and what the compacted verify list saves on a replay log.

(a) all valid: --n distinct valid withdrawals (default 2^15) settled by spp_pool_withdraw_batch on a fresh pool (audit records
    imported, the deposits' roots pushed), against spp_verify_batch on the same proofs and public witnesses -- the call that
    existed before, the yardstick.  The two take turns, --runs timed runs each after one warm-up; host wall time around calls
    that end in a device synchronise, all buffers and pools made beforehand.  The ledger's overhead is the difference.  Beside it:
    the duplicate rule alone, taken one instruction at a time by the Python model on the host (validity given, no verification).
(b) replay: a batch of 4 x --n instructions (2^17) -- the same withdrawals four times over -- on a pool in which the nullifiers of
    half of them are already spent, so half the instructions are replays the screen settles without their proof; with the
    compacted verify list (default) and without it (env SPP_POOL_COMPACT=0: every proof verified), taking turns.  Both must decide
    the same, and as the model does.
Kernel durations come from a separate run of this script under `rocprofv3 --kernel-trace --stats` (profiles/README.md).
Prints one JSON line and writes it to --out (default profiles/pool_probe.json)."""
import argparse, ctypes, json, os, random, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before libspp: one HIP runtime)
import spp  # noqa: E402
from spp import witness as W  # noqa: E402
from spp.lib import check, SPP_POOL_NULLIFIERS, SPP_POOL_AUDIT_RECORDS, POOL_RESULT_NAMES  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1 << 15)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--window", type=int, default=8, help="window of the prover's tables (the proofs are only the workload here)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_probe.json"))
args = ap.parse_args()
N, REP = args.n, 4
os.environ.setdefault("SPP_POOL_SALT", "5eed5eed5eed5eed")
res = {"probe": "pool_probe", "n": N, "replay_batch": REP * N, "runs": args.runs}

# ---- the workload: N deposits, N withdraw proofs from notes against the resident tree ----
tmp = tempfile.mkdtemp(prefix="spp_pool_")
sppc, pkp, vkp = (os.path.join(tmp, "w." + e) for e in ("sppc", "pk", "vk"))
spp.build_circuit(1, sppc)
ctx = spp.Context(0)
L = ctx.L
ctx.setup(sppc, b"\x2b" * 32, pkp, vkp)
wvk = open(vkp, "rb").read()
avk = open(os.path.join(ROOT, "tests", "golden", "reference_audit.vk"), "rb").read()   # no audit proof is verified here
rng = random.Random(99)
sks = [1000 + i for i in range(N)]
amounts = [rng.randrange(1, 1 << 40) for _ in range(N)]
rnds = [rng.randrange(1 << 250) for _ in range(N)]
addresses = [rng.getrandbits(256).to_bytes(32, "big") for _ in range(N)]
h = ctx.load_circuit(sppc, pkp, args.window)
with W.ShieldedPoolMerkleTree(ctx, 16) as tree:
    _, _, roots = tree.deposit([(sks[i], amounts[i], rnds[i]) for i in range(N)])
    t0 = time.perf_counter()
    proofs, pws, status = h.prove_withdraw_notes(tree, [(W.recipient_word(addresses[i]), amounts[i], sks[i], rnds[i], i) for i in range(N)])
    res["workload_prove_s"] = round(time.perf_counter() - t0, 2)
h.close()
assert status == [0] * N
proofs_b, pws_b, addr_b = b"".join(proofs), b"".join(pws), b"".join(addresses)
was = [w[140:172] for w in pws]
nullifiers = [w[44:76] for w in pws]
last_roots = roots[-33:]                                   # what the ring still holds after N deposits
p = lambda x: x.ctypes.data_as(ctypes.c_void_p)


def fresh_pool(compact=True, spent=()):
    os.environ["SPP_POOL_COMPACT"] = "1" if compact else "0"
    pool = W.Pool(ctx, wvk, avk, 8 * N)
    pool.import_keys(SPP_POOL_AUDIT_RECORDS, was)
    pool.add_roots(last_roots)
    if spent:
        pool.import_keys(SPP_POOL_NULLIFIERS, spent)
    return pool


def settle(pool, count, pb, wb, rb):
    out, amt = np.zeros(count, dtype=np.int32), np.zeros(count, dtype=np.uint64)
    t0 = time.perf_counter()
    check(L.spp_pool_withdraw_batch(pool.h, count, pb, wb, rb, p(out), p(amt)))
    return time.perf_counter() - t0, out, amt


def verify_alone(count, pb, wb):
    ok, ms = np.zeros(count, dtype=np.int32), ctypes.c_float(0)
    t0 = time.perf_counter()
    check(L.spp_verify_batch(ctx.h, wvk, len(wvk), count, pb, wb, 172, p(ok), ctypes.byref(ms)))
    return time.perf_counter() - t0, ok, ms.value


def model(keys, spent):
    """the duplicate rule one instruction at a time, every proof valid and every other check passed: 0 = OK, 4 = NULLIFIER_USED"""
    t0 = time.perf_counter()
    seen, out = set(spent), []
    for k in keys:
        if k in seen:
            out.append(4)
        else:
            seen.add(k)
            out.append(0)
    return time.perf_counter() - t0, out


# ---- (a) all valid ----
pools = [fresh_pool() for _ in range(args.runs + 1)]
ta, tv, tk = [], [], []
for k, pool in enumerate(pools):
    dv, ok, kms = verify_alone(N, proofs_b, pws_b)
    da, codes, amt = settle(pool, N, proofs_b, pws_b, addr_b)
    assert ok.all() and not codes.any() and amt.tolist() == amounts and pool.counts() == (N, N)
    pool.close()
    if k:                                                  # the first round is the warm-up
        tv.append(dv); ta.append(da); tk.append(kms)
tm, want = model(nullifiers, ())
assert want == codes.tolist()
a, v = statistics.median(ta), statistics.median(tv)
res.update({"a_withdraw_batch_ms": round(a * 1e3, 2), "a_withdraw_batch_runs_ms": [round(x * 1e3, 2) for x in ta],
            "a_verify_batch_ms": round(v * 1e3, 2), "a_verify_batch_runs_ms": [round(x * 1e3, 2) for x in tv],
            "a_k_verify_ms": round(statistics.median(tk), 2), "a_ledger_overhead_ms": round((a - v) * 1e3, 2),
            "a_ledger_overhead_over_verify": round((a - v) / v, 4), "a_withdrawals_per_s": round(N / a, 1),
            "a_python_model_duplicate_rule_ms": round(tm * 1e3, 2)})

# ---- (b) replay: 4 x N instructions, the nullifiers of the first half of the withdrawals already spent ----
M = REP * N
pb, wb, rb = proofs_b * REP, pws_b * REP, addr_b * REP
spent = nullifiers[:N // 2]
tm, want = model(nullifiers * REP, spent)
legs = {True: [], False: []}
for k in range(args.runs + 1):
    got = {}
    for compact in (True, False):
        pool = fresh_pool(compact, spent)
        dt, codes, _ = settle(pool, M, pb, wb, rb)
        got[compact] = codes
        assert pool.counts() == (N, N)
        pool.close()
        if k:
            legs[compact].append(dt)
    assert (got[True] == got[False]).all() and got[True].tolist() == want
c, f = statistics.median(legs[True]), statistics.median(legs[False])
res.update({"b_replays_settled_by_the_screen": int(M // 2), "b_compacted_ms": round(c * 1e3, 2), "b_compacted_runs_ms": [round(x * 1e3, 2) for x in legs[True]],
            "b_every_proof_ms": round(f * 1e3, 2), "b_every_proof_runs_ms": [round(x * 1e3, 2) for x in legs[False]],
            "b_compacted_over_every_proof": round(c / f, 4), "b_instructions_per_s_compacted": round(M / c, 1),
            "b_python_model_duplicate_rule_ms": round(tm * 1e3, 2),
            "b_codes": {POOL_RESULT_NAMES[x]: int((got[True] == x).sum()) for x in sorted(set(got[True].tolist()))}})
ctx.close()

line = json.dumps(res)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as fo:
        fo.write(line + "\n")
