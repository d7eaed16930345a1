"""The ceremony's first phase at the audit circuit's size (domain_log 15): a transcript contribution, its verification, the derivation
of the audit key from the transcript, and the group inverse NTT alone against one host thread.

(a) spp_ptau_contribute on a transcript of L = 15 that already holds one contribution: 131 071 G1 and 32 768 G2 points decoded and
    checked, the G2 subgroup on the host, the per-point products on the device, beta2 and the receipt on the host;
(b) spp_ptau_verify_contribution of that link: both files read, every point checked, the receipt, eight Pippenger sums on the
    device (two of them in G2), the Miller loops on the host;
(c) spp_setup_from_ptau for the audit circuit: three G1 transforms and one G2 transform of 2^15 points, the column gathers, Z;
(d) spp_ec_intt_timed, G1 and G2, over the transcript's T1[0 .. n) and T2: the stages and the scaling between events, and one host
    thread over the first --host-butterflies butterflies of stage 0 (the text the lanes run), scaled to the n / 2 * (L - 1) butterflies
    of a transform that carry a product.
(a) - (c) are host wall time around one synchronous call, one warm-up call, then the median of --runs.
Prints one JSON line and writes it to --out (default profiles/ptau_probe.json)."""
import argparse, json, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd"))
import torch  # noqa: E402,F401  (before libspp: one HIP runtime)
import spp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log", type=int, default=15)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--host-butterflies", type=int, default=512)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ptau_probe.json"))
args = ap.parse_args()
L, n = args.log, 1 << args.log


def timed(call):
    out = call()
    times = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        out = call()
        times.append(time.perf_counter() - t0)
    return out, round(1e3 * statistics.median(times), 2)


rlwe = json.load(open(os.path.join(ROOT, "tests", "golden", "rlwe_pk.json")))
res = {"probe": "ptau_probe", "domain_log": L, "runs": args.runs}
with tempfile.TemporaryDirectory() as d:
    p = lambda name: os.path.join(d, name)
    spp.build_circuit(2, p("audit.sppc"), aux=list(rlwe["a"]) + list(rlwe["b"]))
    ctx = spp.Context(0)
    ctx.ptau_new(L, p("t0.ptau"))
    ctx.ptau_contribute(p("t0.ptau"), p("t1.ptau"), bytes(range(32)))
    receipt, res["contribute_ms"] = timed(lambda: ctx.ptau_contribute(p("t1.ptau"), p("t2.ptau"), bytes(range(100, 132))))
    verdict, res["verify_ms"] = timed(lambda: ctx.ptau_verify_contribution(p("t1.ptau"), p("t2.ptau"), receipt))
    assert verdict == (True, 0), verdict
    _, res["derive_ms"] = timed(lambda: ctx.setup_from_ptau(p("audit.sppc"), p("t2.ptau"), p("audit.pk"), p("audit.vk")))
    data = open(p("t2.ptau"), "rb").read()
    t2_at = 12 + 64 * (2 * n - 1)
    for group, name, raw in ((1, "g1", data[12:12 + 64 * n]), (2, "g2", data[t2_at:t2_at + 128 * n])):
        _, stages, finish, host = ctx.ec_intt_timed(group, raw, L, args.host_butterflies)
        products = (n // 2) * (L - 1)
        res["intt_" + name] = {"stages_ms": round(stages, 2), "scale_ms": round(finish, 2), "host_butterflies": min(args.host_butterflies, n // 2),
                               "host_ms": round(host, 2), "host_thread_scaled_ms": round(host / min(args.host_butterflies, n // 2) * products, 1)}
    ctx.close()
print(json.dumps(res))
with open(args.out, "w") as f:
    f.write(json.dumps(res) + "\n")
