"""The pool ledger and the audit opening on the random-linear-combination verifier, one GPU: mode SPP_POOL_VERIFY_RLC against mode
SPP_POOL_VERIFY_EACH (k_verify_list, the default and the baseline: the path the ledger had before the mode existed), and
spp_audit_open_batch_rlc against spp_audit_open_batch.  One process, one build of the workload (the generator of
profiles/pool_probe.py: --n deposits, --n withdraw proofs from notes against the resident tree).

(a) all valid: --n distinct valid withdrawals (default 2^15) through spp_pool_withdraw_batch on a fresh pool, mode EACH then mode
    RLC on an identical fresh pool, taking turns.
(b) replay: the 4 x --n batch of profiles/pool_probe.py (2^17; the nullifiers of half the withdrawals already spent, so the screen
    settles half the instructions and the verify list holds 2^16 proofs, in-batch duplicates included), the same way.
(c) audit opening: --n records (2048 distinct ones repeated, as profiles/audit_open_probe.py makes them), spp_audit_open_batch then
    spp_audit_open_batch_rlc, all records valid -- and once more with that probe's tampering (one record in 30 with a proof byte
    flipped, one in 30 under another record's wa_commitment), where every group of 256 holds a proof that does not verify and the
    combined check can only lose.
Host wall time around calls that end in a device synchronise, pools and buffers made beforehand; medians of --runs timed calls
(default 5) per leg after one warm-up each.  Both modes must decide the same.  Prints one JSON line and writes it to --out (default
profiles/pool_rlc_probe.json)."""
import argparse, ctypes, json, os, random, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before libspp: one HIP runtime)
import spp  # noqa: E402
from spp import witness as W, workload  # noqa: E402
from spp.lib import check, SPP_POOL_NULLIFIERS, SPP_POOL_AUDIT_RECORDS, POOL_RESULT_NAMES  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1 << 15)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--group", type=int, default=0, help="proofs per combined equation (0: the default, 256)")
ap.add_argument("--audit-batch", type=int, default=2048, help="distinct audit records, repeated up to --n")
ap.add_argument("--window", type=int, default=8, help="window of the prover's tables (the proofs are only the workload here)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_rlc_probe.json"))
args = ap.parse_args()
N, REP = args.n, 4
os.environ.setdefault("SPP_POOL_SALT", "5eed5eed5eed5eed")
os.environ["SPP_POOL_COMPACT"] = "1"
res = {"probe": "pool_rlc_probe", "n": N, "replay_batch": REP * N, "runs": args.runs, "group": args.group or 256, "baseline": "mode EACH (k_verify_list / k_verify)"}
p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
med = statistics.median
ms = lambda xs: [round(x * 1e3, 2) for x in xs]

# ---- the workload: N deposits, N withdraw proofs from notes against the resident tree ----
tmp = tempfile.mkdtemp(prefix="spp_pool_rlc_")
sppc, pkp, vkp = (os.path.join(tmp, "w." + e) for e in ("sppc", "pk", "vk"))
spp.build_circuit(1, sppc)
ctx = spp.Context(0)
L = ctx.L
ctx.setup(sppc, b"\x2b" * 32, pkp, vkp)
wvk = open(vkp, "rb").read()
rng = random.Random(99)
sks = [1000 + i for i in range(N)]
amounts = [rng.randrange(1, 1 << 40) for _ in range(N)]
rnds = [rng.randrange(1 << 250) for _ in range(N)]
addresses = [rng.getrandbits(256).to_bytes(32, "big") for _ in range(N)]
h = ctx.load_circuit(sppc, pkp, args.window)
with W.ShieldedPoolMerkleTree(ctx, 16) as tree:
    _, _, roots = tree.deposit([(sks[i], amounts[i], rnds[i]) for i in range(N)])
    proofs, pws, status = h.prove_withdraw_notes(tree, [(W.recipient_word(addresses[i]), amounts[i], sks[i], rnds[i], i) for i in range(N)])
h.close()
assert status == [0] * N
proofs_b, pws_b, addr_b = b"".join(proofs), b"".join(pws), b"".join(addresses)
was = [w[140:172] for w in pws]
nullifiers = [w[44:76] for w in pws]
last_roots = roots[-33:]                                   # what the ring still holds after N deposits
avk = open(os.path.join(ROOT, "tests", "golden", "reference_audit.vk"), "rb").read()   # no audit proof is verified by the pools


def fresh_pool(verifier, spent=()):
    pool = W.Pool(ctx, wvk, avk, 8 * N, verifier=verifier, group=args.group)
    pool.import_keys(SPP_POOL_AUDIT_RECORDS, was)
    pool.add_roots(last_roots)
    if spent:
        pool.import_keys(SPP_POOL_NULLIFIERS, spent)
    return pool


def settle(pool, count, pb, wb, rb):
    out, amt = np.zeros(count, dtype=np.int32), np.zeros(count, dtype=np.uint64)
    t0 = time.perf_counter()
    check(L.spp_pool_withdraw_batch(pool.h, count, pb, wb, rb, p(out), p(amt)))
    return time.perf_counter() - t0, out


def pool_legs(tag, count, pb, wb, rb, spent, want):
    """mode EACH then mode RLC on identical fresh pools, runs + 1 times (the first is the warm-up)"""
    t, stats = {"each": [], "rlc": []}, None
    for k in range(args.runs + 1):
        got = {}
        for verifier in ("each", "rlc"):
            pool = fresh_pool(verifier, spent)
            dt, got[verifier] = settle(pool, count, pb, wb, rb)
            if verifier == "rlc":
                stats = pool.verify_stats()[0]
            else:
                assert pool.verify_stats() == ((0, 0, 0, 0), (0, 0, 0, 0))
            pool.close()
            if k:
                t[verifier].append(dt)
        assert (got["each"] == got["rlc"]).all() and got["each"].tolist() == want
    e, r = med(t["each"]), med(t["rlc"])
    res.update({tag + "_each_ms": round(e * 1e3, 2), tag + "_each_runs_ms": ms(t["each"]), tag + "_rlc_ms": round(r * 1e3, 2),
                tag + "_rlc_runs_ms": ms(t["rlc"]), tag + "_each_over_rlc_time": round(e / r, 3), tag + "_rlc_stats": list(stats),
                tag + "_rlc_faster": bool(r < e),
                tag + "_codes": {POOL_RESULT_NAMES[x]: int((got["rlc"] == x).sum()) for x in sorted(set(got["rlc"].tolist()))}})


def model(keys, spent):
    """the duplicate rule one instruction at a time, every proof valid and every other check passed: 0 = OK, 4 = NULLIFIER_USED"""
    seen, out = set(spent), []
    for k in keys:
        out.append(4 if k in seen else 0)
        seen.add(k)
    return out


# ---- (a) all valid, (b) replay ----
pool_legs("a", N, proofs_b, pws_b, addr_b, (), [0] * N)
spent = nullifiers[:N // 2]
pool_legs("b", REP * N, proofs_b * REP, pws_b * REP, addr_b * REP, spent, model(nullifiers * REP, spent))
del proofs, pws, proofs_b, pws_b

# ---- (c) audit opening ----
B = min(args.audit_batch, N)
Q = 167772161
golden = os.path.join(ROOT, "tests", "golden")
rlwe_pk = json.load(open(os.path.join(golden, "rlwe_pk.json")))
sk_mod_q = np.asarray(json.load(open(os.path.join(golden, "rlwe_decrypt.json")))["sk_mod_q"], dtype=np.uint32)
asppc, apk, avkp = (os.path.join(tmp, "a." + e) for e in ("sppc", "pk", "vk"))
spp.build_circuit(2, asppc, aux=list(rlwe_pk["a"]) + list(rlwe_pk["b"]))
ctx.setup(asppc, b"\x2a" * 32, apk, avkp)
vk = open(avkp, "rb").read()
h = ctx.load_circuit(asppc, apk, 0)
a_sks, r8, e18, e28 = workload.audit_noise(0, B)
ap_, aw_, st, c0_1, c1_1 = h.prove_audit_records(rlwe_pk["a"], rlwe_pk["b"], a_sks, r8, e18, e28, [(1000003 * i + 17, 998244353 * i + 29) for i in range(B)])
h.close()
assert st == [0] * B
rep = -(-N // B)
proofs1 = np.frombuffer(b"".join(ap_), dtype=np.uint8).reshape(B, 388)
pws1 = np.frombuffer(b"".join(aw_), dtype=np.uint8).reshape(B, 76)
tile = lambda x: np.ascontiguousarray(np.tile(np.asarray(x), (rep, 1))[:N])
proofs, pws, c0, c1 = tile(proofs1), tile(pws1), tile(np.asarray(c0_1, dtype=np.uint32)), tile(np.asarray(c1_1, dtype=np.uint32))


def open_legs(tag, proofs_b, pws_b):
    t, out, stats = {False: [], True: []}, {}, (ctypes.c_uint32 * 4)()
    for k in range(args.runs + 1):
        for rlc in (False, True):
            owners, flags = np.zeros((N, 64), dtype=np.uint8), np.zeros(N, dtype=np.uint32)
            t0 = time.perf_counter()
            if rlc:
                check(L.spp_audit_open_batch_rlc(ctx.h, vk, len(vk), p(sk_mod_q), N, proofs_b, pws_b, p(c0), p(c1), args.group, p(owners), p(flags), stats))
            else:
                check(L.spp_audit_open_batch(ctx.h, vk, len(vk), p(sk_mod_q), N, proofs_b, pws_b, p(c0), p(c1), p(owners), p(flags)))
            if k:
                t[rlc].append(time.perf_counter() - t0)
            out[rlc] = (owners, flags)
        assert (out[False][0] == out[True][0]).all() and (out[False][1] == out[True][1]).all()
    e, r = med(t[False]), med(t[True])
    flags = out[True][1]
    res.update({tag + "_audit_open_ms": round(e * 1e3, 2), tag + "_audit_open_runs_ms": ms(t[False]), tag + "_audit_open_rlc_ms": round(r * 1e3, 2),
                tag + "_audit_open_rlc_runs_ms": ms(t[True]), tag + "_each_over_rlc_time": round(e / r, 3), tag + "_rlc_stats": list(stats),
                tag + "_rlc_faster": bool(r < e), tag + "_flag_counts": {str(f): int((flags == f).sum()) for f in sorted(set(flags.tolist()))}})


open_legs("c_valid", proofs.tobytes(), pws.tobytes())
assert res["c_valid_flag_counts"] == {"0": N} and res["c_valid_rlc_stats"][1:] == [0, 0, 0]
idx = np.arange(N)
proofs[idx % 30 == 2, 100] ^= 1                                   # bit 1: off the twist, dropped by the term kernel
pws[idx % 30 == 3, 12:44] = pws[(idx[idx % 30 == 3] + 1) % N, 12:44]   # another record's wa_commitment: bits 1 and 4, refuses its group
open_legs("c_tampered", proofs.tobytes(), pws.tobytes())
ctx.close()

line = json.dumps(res)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as fo:
        fo.write(line + "\n")
