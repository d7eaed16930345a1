"""The setup ceremony on the audit key (about 62 K points in K | Z): one contribution, its verification, and the scaling kernel
alone against one host thread.

(a) spp_setup_contribute on the audit circuit's key (made by spp_setup here): files read and written, K | Z scaled on the device,
    delta1', delta2' and the receipt on the host;
(b) spp_setup_verify_contribution of that link: both keys read, every point decoded and checked on the device, the receipt, the two
    pairing products on the host, two 62 K-point Pippenger sums on the device;
(c) spp_g1_scale_points_timed over the key's K | Z points with the contribution's 1/d: the kernel between two events, and one host
    thread running scalar_mul + to_affine (csrc/bn254.hpp) over the first --host-points points, scaled to all of them.  The call
    compares the two results byte for byte.
(a) and (b) are host wall time around one synchronous call, two warm-up calls, then the median of --runs.
Prints one JSON line and writes it to --out (default profiles/setup_ceremony_probe.json)."""
import argparse, json, os, statistics, struct, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd"))
import torch  # noqa: E402,F401  (before libspp: one HIP runtime)
import spp  # noqa: E402
from oracle import bn254 as O  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--host-points", type=int, default=512)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "setup_ceremony_probe.json"))
args = ap.parse_args()
ENTROPY = bytes(range(32))


def kz_points(pk):
    """the K points and the Z points of an SPPK container, concatenated"""
    at = 28 + 3 * 64 + 2 * 128
    out = b""
    for name, size, wires in (("A", 64, 1), ("B1", 64, 1), ("B2", 128, 1), ("K", 64, 1), ("Z", 64, 0)):
        n, = struct.unpack_from("<I", pk, at)
        at += 4 + 4 * n * wires
        if name in ("K", "Z"):
            out += pk[at:at + size * n]
        at += size * n
    return out


def timed(call):
    for _ in range(2):
        out = call()
    times = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        out = call()
        times.append(time.perf_counter() - t0)
    return out, times


rlwe = json.load(open(os.path.join(ROOT, "tests", "golden", "rlwe_pk.json")))
res = {"probe": "setup_ceremony_probe", "runs": args.runs}
with tempfile.TemporaryDirectory() as d:
    sppc, pk0, vk0, pk1, vk1 = (os.path.join(d, n) for n in ("audit.sppc", "k0.pk", "k0.vk", "k1.pk", "k1.vk"))
    spp.build_circuit(2, sppc, aux=list(rlwe["a"]) + list(rlwe["b"]))
    ctx = spp.Context(0)
    ctx.setup(sppc, b"\x09" * 32, pk0, vk0)
    points = kz_points(open(pk0, "rb").read())
    res["points"] = len(points) // 64
    res["pk_bytes"] = os.path.getsize(pk0)
    receipt, times = timed(lambda: ctx.setup_contribute(pk0, vk0, pk1, vk1, ENTROPY))
    res["a_contribute_ms"] = round(statistics.median(times) * 1e3, 2)
    res["a_contribute_runs_ms"] = [round(x * 1e3, 2) for x in times]
    verdict, times = timed(lambda: ctx.setup_verify_contribution(pk0, vk0, pk1, vk1, receipt))
    res["b_verify_ms"] = round(statistics.median(times) * 1e3, 2)
    res["b_verify_runs_ms"] = [round(x * 1e3, 2) for x in times]
    res["b_accepted"] = verdict == (True, 0)
    dinv = pow(O.hash_to_fr(ENTROPY, b"spp-groth16-contribute-v1", 2)[0], -1, O.R)
    kernel, host = [], []
    for _ in range(2 + args.runs):
        out, kms, hms = ctx.g1_scale_points_timed(points, dinv, args.host_points)
        kernel.append(kms)
        host.append(hms)
    res["c_kernel_ms"] = round(statistics.median(kernel[2:]), 3)
    res["c_kernel_runs_ms"] = [round(x, 3) for x in kernel[2:]]
    res["c_host_points"] = min(args.host_points, res["points"])
    res["c_host_thread_ms_for_host_points"] = round(statistics.median(host[2:]), 2)
    res["c_host_thread_ms_all_points_scaled"] = round(statistics.median(host[2:]) * res["points"] / max(res["c_host_points"], 1), 1)
    res["c_kernel_equals_contribution"] = out == kz_points(open(pk1, "rb").read())
    ctx.close()

line = json.dumps(res)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
