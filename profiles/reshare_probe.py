"""Handing the auditors' key to a new committee on one GPU: the new committee's commitments D'_k[v] = sum_j lambda_j C'_{j,k}[v]
at n = 1024 for (dealers, t') in --shapes, with the Lagrange weights of the set {1..dealers}.

(a) spp_vss_combine_commitments_timed through ctypes on packed buffers: the whole synchronous call as host wall time (upload,
    decoding the points, the shared-scan kernel, download) and inside it the device time of the kernels (events around them);
(b) for comparison the same result composed from what existed before: one spp_g1_mul_each call per dealer, its t' * n points
    against that dealer's weight repeated (host wall time of the calls, uploads, point checks and downloads included).  The
    (dealers - 1) * t' * n affine additions that would follow on the host are NOT in the figure; 16 sampled outputs are added with
    Python integers and must equal (a)'s bytes;
(c) one full spp_vss_reshare_receive of the same dealings (the sub-share checks, the constant terms against the old committee,
    the two weighted sums and (a)'s kernels), host wall time of the whole call.
The dealings are real ones: one dealer's sharing at threshold `dealers` makes the old committee, each of its members deals its
share at threshold t'.  (a) and (b) alternate in one process; two warm-up rounds, then the median of --runs.  Prints one JSON
line and writes it to --out (default profiles/reshare_probe.json)."""
import argparse, ctypes, json, os, random, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd"))
import torch  # noqa: E402,F401  (before libspp: one HIP runtime)
import spp  # noqa: E402
from spp import witness as W  # noqa: E402
from spp.lib import check  # noqa: E402
from oracle import bn254 as O  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", type=int, nargs="+", default=[2, 2, 8, 8, 64, 64], help="dealers t' pairs")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reshare_probe.json"))
args = ap.parse_args()
N, R = W.RLWE_N, W.FR_MODULUS

ctx = spp.Context(0)
L, h = ctx.L, ctx.h
rng = random.Random(1)
be = lambda vals: b"".join(int(v).to_bytes(32, "big") for v in vals)
vp = lambda b: ctypes.cast(b, ctypes.c_void_p)
med = lambda xs: round(statistics.median(xs), 3)


def one_shape(dealers, t):
    xs = list(range(1, dealers + 1))
    lam = W.lagrange_at_zero(xs)
    old = W.vss_deal(ctx, [rng.randrange(1, R) for _ in range(N)], dealers, dealers)           # the old committee: D, shares, blinds
    deals = [W.vss_deal(ctx, sh["y"], t, t, blinds=sh["y_blind"]) for sh in old["shares"]]    # each member deals on at threshold t'
    cms = b"".join(d["commitments"] for d in deals)
    count = t * N
    weights = be(lam)
    out = ctypes.create_string_buffer(count * 64)
    flags = (ctypes.c_uint32 * (dealers * count))()
    bad = ctypes.c_size_t(0)
    ms = ctypes.c_float(0)
    prods = [ctypes.create_string_buffer(count * 64) for _ in range(dealers)]
    scalars = [be([l]) * count for l in lam]

    def combine():
        t0 = time.perf_counter()
        check(L.spp_vss_combine_commitments_timed(h, t, dealers, N, cms, weights, None, vp(out), vp(flags), ctypes.byref(bad), ctypes.byref(ms)))
        return (time.perf_counter() - t0) * 1e3, float(ms.value)

    def composed():
        t0 = time.perf_counter()
        for d in range(dealers):
            check(L.spp_g1_mul_each(h, deals[d]["commitments"], count, scalars[d], vp(prods[d])))
        return (time.perf_counter() - t0) * 1e3

    for _ in range(2):
        combine(); composed()
    rows, comp = [], []
    for _ in range(args.runs):
        rows.append(combine())
        comp.append(composed())
    assert bad.value == 0

    def host_sum(i):
        acc = None
        for d in range(dealers):
            acc = O.g1_add(acc, O.g1_from_bytes(prods[d].raw[64 * i:64 * i + 64]))
        return O.g1_to_bytes(acc)
    same = all(host_sum(i) == out.raw[64 * i:64 * i + 64] for i in [0, count - 1] + [rng.randrange(count) for _ in range(14)])
    # the new member at x = 1 receives the same dealings
    ys, yb = be(v for d in deals for v in d["shares"][0]["y"]), be(v for d in deals for v in d["shares"][0]["y_blind"])
    cx = (ctypes.c_uint32 * dealers)(*xs)
    rflags = (ctypes.c_uint32 * (dealers * N))()
    share, blind = ctypes.create_string_buffer(N * 32), ctypes.create_string_buffer(N * 32)
    com = ctypes.create_string_buffer(count * 64)

    def receive():
        t0 = time.perf_counter()
        check(L.spp_vss_reshare_receive(h, dealers, vp(cx), t, 1, N, old["commitments"], cms, ys, yb, vp(rflags), vp(share), vp(blind), vp(com),
                                        ctypes.byref(bad)))
        return (time.perf_counter() - t0) * 1e3

    receive()
    recv = [receive() for _ in range(args.runs)]
    return {"dealers": dealers, "t_new": t, "outputs": count, "combine_call_ms": med([r[0] for r in rows]),
            "combine_kernels_ms": med([r[1] for r in rows]), "combine_kernels_runs_ms": [round(r[1], 3) for r in rows],
            "composed_mul_each_calls_ms": med(comp), "composed_runs_ms": [round(x, 3) for x in comp], "composed_equals_combine": same,
            "reshare_receive_call_ms": med(recv), "reshare_receive_runs_ms": [round(x, 3) for x in recv],
            "reshare_receive_accepts": bad.value == 0, "reshare_committee_equals_combine": com.raw == out.raw,
            "key_commitments_unchanged": com.raw[:N * 64] == old["commitments"][:N * 64]}


shapes = list(zip(args.shapes[0::2], args.shapes[1::2]))
res = {"probe": "reshare_probe", "n": N, "runs": args.runs, "by_shape": [one_shape(d, t) for d, t in shapes]}
ctx.close()
line = json.dumps(res)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
