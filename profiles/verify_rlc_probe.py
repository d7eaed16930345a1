"""Batch verification by random linear combination against the per-proof verifier, on one GPU.

Inputs: --batch (default 2048) distinct audit proofs from the GPU prover (workload.audit_noise), tiled to each count.  Timed on the
same host buffers, at the counts of --counts (default 2^12, 2^15, 2^17), in alternating rounds, medians over --rounds:
    base    spp_verify_batch                          (k_verify, one lane per proof: unchanged by this feature, the baseline)
    coop    spp_verify_batch_rlc                      (cooperative tail)
    serial  spp_verify_batch_rlc, SPP_RLC_SERIAL_TAIL (one-lane tail)
then, at 2^15: a sweep of `group` over 64, 256, 1024 (cooperative tail), and one run with a single forged proof (the cost of a
fallback: its group is settled proof by proof).  kernel_ms is the event time around all launches of a call, wall_ms the host time
around the call (uploads, key preparation and download included).  Every timed call runs under a time limit (SIGALRM with its
default action: a call that hangs ends the process).  --quick: one untimed-style pass at 2^15 only, for a kernel trace
(rocprofv3 --kernel-trace --stats -- python profiles/verify_rlc_probe.py --quick --out "").
Prints one JSON line and writes it to --out (default profiles/verify_rlc_probe.json)."""
import argparse, ctypes, json, os, signal, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before libspp: one HIP runtime)
import spp  # noqa: E402
from spp import workload, lib as L_  # noqa: E402
from spp.lib import check  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--counts", type=int, nargs="+", default=[1 << 12, 1 << 15, 1 << 17])
ap.add_argument("--batch", type=int, default=2048)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--limit", type=int, default=60, help="seconds a timed call may take")
ap.add_argument("--quick", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_rlc_probe.json"))
args = ap.parse_args()
B = args.batch
golden = os.path.join(ROOT, "tests", "golden")
rlwe_pk = json.load(open(os.path.join(golden, "rlwe_pk.json")))

tmp = tempfile.mkdtemp(prefix="spp_verify_rlc_")
sppc, pkp, vkp = (os.path.join(tmp, "c." + e) for e in ("sppc", "pk", "vk"))
spp.build_circuit(2, sppc, aux=list(rlwe_pk["a"]) + list(rlwe_pk["b"]))
ctx = spp.Context(0)
L = ctx.L
ctx.setup(sppc, b"\x2a" * 32, pkp, vkp)
vk = open(vkp, "rb").read()
h = ctx.load_circuit(sppc, pkp, 0)
dev = torch.device("cuda", 0)
up = lambda raw: torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
p = lambda x: x.ctypes.data_as(ctypes.c_void_p)

# ---- B distinct proofs from the GPU prover ----
sks, r8, e18, e28 = workload.audit_noise(0, B)
d_a, d_b = up(np.asarray(rlwe_pk["a"], dtype=np.uint32).tobytes()), up(np.asarray(rlwe_pk["b"], dtype=np.uint32).tobytes())
d_sk = up(b"".join(int(v).to_bytes(32, "big") for v in sks))
d_r, d_e1, d_e2 = up(r8.tobytes()), up(e18.tobytes()), up(e28.tobytes())
d_rs = up(b"".join((1000003 * i + 17).to_bytes(32, "big") + (998244353 * i + 29).to_bytes(32, "big") for i in range(B)))
o = [torch.zeros(B * 388, dtype=torch.uint8, device=dev), torch.zeros(B * 76, dtype=torch.uint8, device=dev),
     torch.zeros(B, dtype=torch.int32, device=dev)]
h.prove_audit_from_secrets_device(B, *[t.data_ptr() for t in (d_a, d_b, d_sk, d_r, d_e1, d_e2, d_rs)], *[t.data_ptr() for t in o])
h.sync()
assert int(o[2].abs().sum().item()) == 0
proofs1, pws1 = o[0].cpu().numpy().reshape(B, 388), o[1].cpu().numpy().reshape(B, 76)
h.close()
SEED = bytes(range(7, 39))      # fixed after the proofs exist; a run is reproducible


def tiled(n):
    rep = -(-n // B)
    return np.ascontiguousarray(np.tile(proofs1, (rep, 1))[:n]), np.ascontiguousarray(np.tile(pws1, (rep, 1))[:n])


def call(kind, n, pb, wb, group=0):
    """(wall ms, kernel ms, verdicts, stats) of one call, under the time limit"""
    ok, stats, ms = np.zeros(n, dtype=np.int32), (ctypes.c_uint32 * 4)(), ctypes.c_float(0)
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    signal.alarm(args.limit)
    t0 = time.perf_counter()
    if kind == "base":
        check(L.spp_verify_batch(ctx.h, vk, len(vk), n, pb, wb, 76, p(ok), ctypes.byref(ms)))
    else:
        check(L.spp_verify_batch_rlc(ctx.h, vk, len(vk), n, pb, wb, 76, SEED, group, L_.SPP_RLC_SERIAL_TAIL if kind == "serial" else 0, p(ok),
                                     stats, ctypes.byref(ms)))
    wall = time.perf_counter() - t0
    signal.alarm(0)
    return wall * 1e3, ms.value, ok, tuple(stats)


def timed(kinds, n, pb, wb, rounds, groups=None):
    """alternating rounds after one warm-up each; {kind: {...medians...}}"""
    t = {k: ([], []) for k in kinds}
    for r in range(rounds + 1):
        for k in kinds:
            wall, ms, ok, stats = call(k if groups is None else "coop", n, pb, wb, 0 if groups is None else groups[k])
            assert ok.all(), "%s refused a valid proof at count %d" % (k, n)
            assert k == "base" or stats[1:] == (0, 0, 0), (k, stats)
            if r:
                t[k][0].append(wall); t[k][1].append(ms)
    return {str(k): {"kernel_ms": round(statistics.median(t[k][1]), 2), "wall_ms": round(statistics.median(t[k][0]), 2),
                     "kernel_runs_ms": [round(x, 2) for x in t[k][1]]} for k in kinds}


res = {"probe": "verify_rlc_probe", "batch_distinct": B, "rounds": args.rounds, "default_group": 256, "counts": {}}
if args.quick:
    pb, wb = (x.tobytes() for x in tiled(1 << 15))
    for k in ("base", "coop", "serial"):
        wall, ms, ok, stats = call(k, 1 << 15, pb, wb)
        assert ok.all()
        res["counts"].setdefault(str(1 << 15), {})[k] = {"kernel_ms": round(ms, 2), "wall_ms": round(wall, 2)}
else:
    for n in args.counts:
        pb, wb = (x.tobytes() for x in tiled(n))
        r = timed(("base", "coop", "serial"), n, pb, wb, args.rounds)
        r["coop_over_base_kernel_speedup"] = round(r["base"]["kernel_ms"] / r["coop"]["kernel_ms"], 3)
        r["serial_over_base_kernel_speedup"] = round(r["base"]["kernel_ms"] / r["serial"]["kernel_ms"], 3)
        res["counts"][str(n)] = r
    n = 1 << 15
    pa, wa = tiled(n)
    pb, wb = pa.tobytes(), wa.tobytes()
    res["group_sweep_2p15"] = timed((64, 256, 1024), n, pb, wb, args.rounds, groups={64: 64, 256: 256, 1024: 1024})
    # one forged proof (the Krs of its neighbour) in the middle: one group of 256 goes through the per-proof verifier
    pa[n // 2, 192:256] = pa[n // 2 + 1, 192:256]
    fb = pa.tobytes()
    runs = []
    for r in range(args.rounds + 1):
        wall, ms, ok, stats = call("coop", n, fb, wb)
        assert stats == (n // 256, 1, 256, 0) and int(ok.sum()) == n - 1 and ok[n // 2] == 0, stats
        if r:
            runs.append(ms)
    res["one_forged_2p15"] = {"kernel_ms": round(statistics.median(runs), 2), "kernel_runs_ms": [round(x, 2) for x in runs], "stats": list(stats)}
ctx.close()

line = json.dumps(res)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
