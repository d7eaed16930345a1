"""The auditors' key without a dealer on one GPU: one dealing and one receive at n = 1024 for t in --thresholds, m = t + 1.

(a) spp_vss_deal_timed with every scalar supplied (nothing drawn inside the clock), through ctypes on packed buffers: the whole
    synchronous call as host wall time (uploads, the two evaluations, the commitment kernel, downloads), and inside it the device
    times of the two evaluations together and of the commitment kernel (events around the launches);
(b) spp_vss_receive of receiver m's view of m such dealings, host wall time of the whole call;
(c) for comparison the same t * n commitments composed from what existed before: spp_g1_mul_each twice, over G repeated and over
    H repeated (host wall time of the two calls, uploads, point checks and downloads included).  The t * n affine additions that
    would follow on the host are NOT in the figure; 16 sampled points are added with Python integers and must equal (a)'s bytes.
(a) and (c) alternate in one process; two warm-up rounds, then the median of --runs.  A scalar 0 is no input of (c), so the
scalars are drawn from [1, r).  Prints one JSON line and writes it to --out (default profiles/dkg_probe.json)."""
import argparse, ctypes, json, os, random, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd"))
import torch  # noqa: E402,F401  (before libspp: one HIP runtime)
import spp  # noqa: E402
from spp import witness as W  # noqa: E402
from spp.lib import check  # noqa: E402
from oracle import bn254 as O  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--thresholds", type=int, nargs="+", default=[2, 8, 64])
ap.add_argument("--runs", type=int, default=9)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dkg_probe.json"))
args = ap.parse_args()
N, R = W.RLWE_N, W.FR_MODULUS

ctx = spp.Context(0)
L, h = ctx.L, ctx.h
G, H = W.vss_generators(L)
rng = random.Random(1)
be = lambda vals: b"".join(int(v).to_bytes(32, "big") for v in vals)
vp = lambda b: ctypes.cast(b, ctypes.c_void_p)
med = lambda xs: round(statistics.median(xs), 3)


def one_threshold(t):
    m = t + 1
    scal = lambda k: be(rng.randrange(1, R) for _ in range(k))
    secrets, blinds, coeffs, coeffs_blind = scal(N), scal(N), scal((t - 1) * N), scal((t - 1) * N)
    ys, yb = (ctypes.create_string_buffer(m * N * 32) for _ in range(2))
    cm = ctypes.create_string_buffer(t * N * 64)
    ms = (ctypes.c_float * 2)()
    g_pts, h_pts = O.g1_to_bytes(G) * (t * N), O.g1_to_bytes(H) * (t * N)
    cg, ch = (ctypes.create_string_buffer(t * N * 64) for _ in range(2))

    def deal(sec=secrets, bl=blinds, co=coeffs, cb=coeffs_blind):
        t0 = time.perf_counter()
        check(L.spp_vss_deal_timed(h, t, m, None, N, sec, bl, co, cb, vp(ys), vp(yb), vp(cm), None, ms))
        return (time.perf_counter() - t0) * 1e3, ms[0], ms[1]

    def composed():
        t0 = time.perf_counter()
        check(L.spp_g1_mul_each(h, g_pts, t * N, secrets + coeffs, vp(cg)))
        check(L.spp_g1_mul_each(h, h_pts, t * N, blinds + coeffs_blind, vp(ch)))
        return (time.perf_counter() - t0) * 1e3

    for _ in range(2):
        deal(); composed()
    rows, comp = [], []
    for _ in range(args.runs):
        rows.append(deal())
        comp.append(composed())
    same = all(O.g1_to_bytes(O.g1_add(O.g1_from_bytes(cg.raw[64 * i:64 * i + 64]), O.g1_from_bytes(ch.raw[64 * i:64 * i + 64])))
               == cm.raw[64 * i:64 * i + 64] for i in [0, t * N - 1] + [rng.randrange(t * N) for _ in range(14)])
    # receiver m's view of m dealings (the first is the one above)
    cms, yv, ybv = [cm.raw], [ys.raw[(m - 1) * N * 32:]], [yb.raw[(m - 1) * N * 32:]]
    for _ in range(m - 1):
        deal(scal(N), scal(N), scal((t - 1) * N), scal((t - 1) * N))
        cms.append(cm.raw); yv.append(ys.raw[(m - 1) * N * 32:]); ybv.append(yb.raw[(m - 1) * N * 32:])
    c_all, y_all, yb_all = b"".join(cms), b"".join(yv), b"".join(ybv)
    flags = (ctypes.c_uint32 * (m * N))()
    share = ctypes.create_string_buffer(N * 32)
    bad = ctypes.c_size_t(0)

    def receive():
        t0 = time.perf_counter()
        check(L.spp_vss_receive(h, t, m, m, N, c_all, y_all, yb_all, None, None, vp(flags), vp(share), ctypes.byref(bad)))
        return (time.perf_counter() - t0) * 1e3

    for _ in range(2):
        receive()
    recv = [receive() for _ in range(args.runs)]
    return {"t": t, "m": m, "commitments": t * N, "deal_call_ms": med([r[0] for r in rows]), "evaluations_ms": med([r[1] for r in rows]),
            "commit_kernel_ms": med([r[2] for r in rows]), "commit_kernel_runs_ms": [round(r[2], 3) for r in rows],
            "composed_two_mul_each_calls_ms": med(comp), "composed_runs_ms": [round(x, 3) for x in comp],
            "composed_equals_commitments": same, "receive_call_ms": med(recv), "receive_runs_ms": [round(x, 3) for x in recv],
            "receive_accepts": bad.value == 0}


res = {"probe": "dkg_probe", "n": N, "runs": args.runs, "window_bits": 8, "table_points": 16320,
       "by_threshold": [one_threshold(t) for t in args.thresholds]}
ctx.close()
line = json.dumps(res)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
