"""Auditor key generation on one GPU: spp_rlwe_keygen_batch, spp_rlwe_key_check and spp_shamir_split at --count keys.

(a) spp_rlwe_keygen_batch for `count` sampled keys (sk, e in [-3, 3], a uniform), sk_mod_q asked for;
(b) spp_rlwe_key_check on their output;
(c) spp_shamir_split 2-of-3 of one key's 1024 coefficients, sharing coefficients from the library, through the Python mirror
    (its conversions of 4 096 field elements to and from Python integers are inside the clock).
Every timing is host wall time around one synchronous call (uploads and downloads of the call included: that is what a caller
gets), sampling and packing done beforehand; two warm-up calls, then the median of --runs.  The reference figure is
scripts/rlwe_keygen.py's single schoolbook product, 0.23 s, which (a) does `count` times per call.
Keys 0 and count - 1 of (a) are compared with a numpy int64 schoolbook product, and (b) must report the maxima of e and sk.
Prints one JSON line and writes it to --out (default profiles/rlwe_keygen_probe.json)."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before libspp: one HIP runtime)
import spp  # noqa: E402
from spp import witness as W  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--count", type=int, default=4096)
ap.add_argument("--runs", type=int, default=9)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rlwe_keygen_probe.json"))
args = ap.parse_args()
Q, N = W.RLWE_Q, W.RLWE_N

ctx = spp.Context(0)
sk, a, e = W.rlwe_sample_key(ctx.L, args.count, 3)


def timed(call):
    for _ in range(2):
        out = call()
    times = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        out = call()
        times.append(time.perf_counter() - t0)
    return out, times


def schoolbook_b(k):
    full = np.convolve(a[k].astype(np.int64), sk[k].astype(np.int64))
    prod = full[:N].copy()
    prod[:N - 1] -= full[N:]
    return np.mod(e[k].astype(np.int64) - prod, Q).astype(np.uint32)


res = {"probe": "rlwe_keygen_probe", "count": args.count, "runs": args.runs, "reference_s_per_product": 0.23}
(b, skq), times = timed(lambda: W.rlwe_keygen(ctx, sk, a, e))
res["a_keygen_ms"] = round(statistics.median(times) * 1e3, 3)
res["a_keygen_runs_ms"] = [round(x * 1e3, 3) for x in times]
res["a_keys_per_s"] = round(args.count / statistics.median(times), 1)
res["a_equals_schoolbook"] = all(np.array_equal(b[k], schoolbook_b(k)) for k in (0, args.count - 1))
maxima, times = timed(lambda: W.rlwe_key_check(ctx, a, b, skq))
res["b_key_check_ms"] = round(statistics.median(times) * 1e3, 3)
res["b_key_check_runs_ms"] = [round(x * 1e3, 3) for x in times]
res["b_maxima_are_those_of_e_and_sk"] = maxima == [(int(np.abs(e[k]).max()), int(np.abs(sk[k]).max())) for k in range(args.count)]
secrets = [int(v) % W.FR_MODULUS for v in sk[0]]
shares, times = timed(lambda: W.shamir_split(ctx, secrets, 2, 3))
res["c_split_2_of_3_ms"] = round(statistics.median(times) * 1e3, 3)
res["c_split_runs_ms"] = [round(x * 1e3, 3) for x in times]
res["c_reconstructs"] = W.reconstruct_sk(ctx, [shares[2], shares[0]]) == skq[0].tolist()
ctx.close()

line = json.dumps(res)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
