"""The pool ledger on one GPU: one alternating log (deposit, submit_audit, withdraw, deposit, ...) settled by spp_pool_settle_log in ONE
call, against the same log cut at every change of kind and settled run by run through spp_pool_add_roots /
spp_pool_submit_audit_batch / spp_pool_withdraw_batch -- what `pool-replay` did before, the yardstick.  Both on identical fresh
pools; the decisions, the ring bytes and the counts must be equal.

The log is built from --k distinct identities (withdraw proofs from notes and audit records from the same keys).  The first half
of the identities get their audit record at the head of the log.  Every other submit_audit is for an identity of the second half
under the proof of its neighbour: no record is ever created, so the verifier is asked every time.  Every withdraw is for an identity
of the first half under the proof of its neighbour: the record exists, the root is in the ring, the nullifier stays free, so the
verifier is asked every time.  Every run of the cut log is therefore one instruction that really launches the verifier -- the case
a relayer's log is, each transaction carrying a proof of its own.  The proofs swapped in are well-formed, so the verifier does all
its work before it says no.  Times are host wall time around Pool.settle_log / Pool.add_roots / submit_audit / withdraw, the
marshalling of the Python lists included on both sides.

(a) --triples deposit/submit_audit/withdraw triples (default 100: 300 instructions, 300 runs) through both methods, taking turns,
    --runs timed rounds after one warm-up round, host wall time around calls that end in a device synchronise.
(b) settle_log alone on the same pattern continued to --n instructions (default 2^15), --runs timed rounds after one warm-up.
Prints one JSON line and writes it to --out (default profiles/pool_log_probe.json)."""
import argparse, json, os, random, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd"))
import torch  # noqa: E402,F401  (before libspp: one HIP runtime)
import spp  # noqa: E402
from spp import witness as W, workload  # noqa: E402
from spp.lib import POOL_RESULT_NAMES  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--k", type=int, default=8, help="distinct identities (even)")
ap.add_argument("--triples", type=int, default=100)
ap.add_argument("--n", type=int, default=1 << 15)
ap.add_argument("--runs", type=int, default=2)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_log_probe.json"))
args = ap.parse_args()
K, H = args.k, args.k // 2
assert K >= 4 and K % 2 == 0
os.environ.setdefault("SPP_POOL_SALT", "5eed5eed5eed5eed")
res = {"probe": "pool_log_probe", "identities": K, "runs_timed": args.runs}

# ---- the workload: K deposits, K withdraw proofs from notes, K audit records from the same secret keys ----
tmp = tempfile.mkdtemp(prefix="spp_pool_log_")
rlwe = json.load(open(os.path.join(ROOT, "tests", "golden", "rlwe_pk.json")))
paths = {n: tuple(os.path.join(tmp, n + "." + e) for e in ("sppc", "pk", "vk")) for n in ("withdraw", "audit")}
spp.build_circuit(1, paths["withdraw"][0])
spp.build_circuit(2, paths["audit"][0], aux=list(rlwe["a"]) + list(rlwe["b"]))
ctx = spp.Context(0)
ctx.setup(paths["withdraw"][0], b"\x2b" * 32, paths["withdraw"][1], paths["withdraw"][2])
ctx.setup(paths["audit"][0], b"\x2c" * 32, paths["audit"][1], paths["audit"][2])
wvk, avk = open(paths["withdraw"][2], "rb").read(), open(paths["audit"][2], "rb").read()
rng = random.Random(98)
sks, r8, e18, e28 = workload.audit_noise(900, K)
amounts = [rng.randrange(1, 1 << 40) for _ in range(K)]
rnds = [rng.randrange(1 << 250) for _ in range(K)]
addresses = [rng.getrandbits(256).to_bytes(32, "big") for _ in range(K)]
with W.ShieldedPoolMerkleTree(ctx, 16) as tree:
    _, _, roots = tree.deposit([(sks[i], amounts[i], rnds[i]) for i in range(K)])
    h = ctx.load_circuit(paths["withdraw"][0], paths["withdraw"][1], 6)
    wp, ww, st = h.prove_withdraw_notes(tree, [(W.recipient_word(addresses[i]), amounts[i], sks[i], rnds[i], i) for i in range(K)])
    h.close()
assert st == [0] * K
h = ctx.load_circuit(paths["audit"][0], paths["audit"][1], 6)
apf, aw, st, _, _ = h.prove_audit_records(rlwe["a"], rlwe["b"], sks, r8, e18, e28)
h.close()
assert st == [0] * K
true_root = int(roots[-1]).to_bytes(32, "big")
assert all(ww[i][12:44] == true_root and ww[i][140:172] == aw[i][12:44] for i in range(K))


def make_log(triples):
    """[(kind, ...)] and the codes the program gives (by the argument in the docstring)"""
    r, log, want = random.Random(97), [], []
    for j in range(triples):
        log.append(("deposit", true_root if j % 8 == 0 else r.getrandbits(250).to_bytes(32, "big")))
        w, w2 = j % H, (j + 1) % H                             # a withdraw of w under the proof of w2: looked at, never lands
        if j < H:                                              # the head: the records of the first half
            log += [("submit_audit", apf[j], aw[j]), ("withdraw", wp[w2], ww[w], addresses[w])]
            want += [0, 0, 6]
        else:                                                  # an audit of a under the proof of a2: looked at, never lands
            a, a2 = H + j % H, H + (j + 1) % H
            log += [("submit_audit", apf[a2], aw[a]), ("withdraw", wp[w2], ww[w], addresses[w])]
            want += [0, 6, 6]
    return log, want


def cut_into_runs(pool, log):
    codes, runs, i = [], 0, 0
    while i < len(log):
        j = i
        while j < len(log) and log[j][0] == log[i][0]:
            j += 1
        cols = list(zip(*(ins[1:] for ins in log[i:j])))
        if log[i][0] == "deposit":
            pool.add_roots(cols[0]); codes += [0] * (j - i)
        elif log[i][0] == "submit_audit":
            codes += pool.submit_audit(cols[0], cols[1])
        else:
            codes += pool.withdraw(cols[0], cols[1], cols[2])[0]
        runs += 1
        i = j
    return codes, runs


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


# ---- (a) one call against run cutting ----
log, want = make_log(args.triples)
t_one, t_cut = [], []
for k in range(args.runs + 1):
    with W.Pool(ctx, wvk, avk, len(log)) as one, W.Pool(ctx, wvk, avk, len(log)) as cut:
        dc, (by_runs, n_runs) = timed(lambda: cut_into_runs(cut, log))
        do, (codes, _) = timed(lambda: one.settle_log(log))
        assert codes == by_runs == want, "the two methods decide differently"
        assert one.state() == cut.state() and one.counts() == cut.counts() == (0, H)
    if k:                                                      # the first round is the warm-up
        t_one.append(do); t_cut.append(dc)
o, c = statistics.median(t_one), statistics.median(t_cut)
res.update({"a_instructions": len(log), "a_runs": n_runs, "a_run_cutting_s": round(c, 3), "a_run_cutting_runs_s": [round(x, 3) for x in t_cut],
            "a_ms_per_run": round(c / n_runs * 1e3, 2), "a_settle_log_ms": round(o * 1e3, 2), "a_settle_log_runs_ms": [round(x * 1e3, 2) for x in t_one],
            "a_run_cutting_over_settle_log": round(c / o, 1),
            "a_codes": {POOL_RESULT_NAMES[x]: codes.count(x) for x in sorted(set(codes))}})

# ---- (b) settle_log alone at --n instructions ----
big, want = make_log((args.n + 2) // 3)
big, want = big[:args.n], want[:args.n]
t_big = []
for k in range(args.runs + 1):
    with W.Pool(ctx, wvk, avk, len(big)) as pool:
        d, (codes, _) = timed(lambda: pool.settle_log(big))
        assert codes == want and pool.counts() == (0, H)
    if k:
        t_big.append(d)
b = statistics.median(t_big)
res.update({"b_instructions": len(big), "b_settle_log_ms": round(b * 1e3, 2), "b_settle_log_runs_ms": [round(x * 1e3, 2) for x in t_big],
            "b_instructions_per_s": round(len(big) / b, 1)})
ctx.close()

line = json.dumps(res)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as fo:
        fo.write(line + "\n")
