"""The reference's own R1CS (tests/golden/reference_withdraw.ccs with its solver, spp/ccs.py to_sppc_solved) proved from resident
inputs at B = 1, 16, 64, 256, 1024, 4096 -- by this tree's libspp.so and by another build of it (--parent: the parent commit's
library), alternating, each run in a fresh process: parent, new, parent, new, parent.

Per run and batch size: warm-up calls, then the median host wall time of one spp_prove_batch_device call followed by spp_sync
(inputs, blinding and outputs stay on the device; every proof is the reference KAT row under its own blinding -- the solver's work
does not depend on the values), and the proofs per second that gives.  B = 1 also records spp_last_timings: [0] is the solver with
the commitment.  One handle, 8-bit windows (the layout of the one-proof latency path), for every batch size: the two libraries
differ in the solver only, so the layout of the MSM tables is the same on both sides.  Status words must all be 0, and the proof
bytes of row 0 must be the same in every run.
The parent's spread at a batch size = (largest - smallest) / smallest of its runs' medians.  Prints one JSON document and writes it
to --out (default profiles/generic_coop_probe.json)."""
import argparse, hashlib, json, os, statistics, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd"))
SIZES = (1, 16, 64, 256, 1024, 4096)
WARMUP = {1: 5, 16: 3, 64: 3, 256: 2, 1024: 2, 4096: 1}
ITERS = {1: 25, 16: 15, 64: 11, 256: 7, 1024: 5, 4096: 5}

ap = argparse.ArgumentParser()
ap.add_argument("--parent", help="libspp.so of the parent commit")
ap.add_argument("--child", help="(internal) measure with this library and print one JSON line")
ap.add_argument("--dir", help="(internal) directory with the container and the key")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generic_coop_probe.json"))
args = ap.parse_args()


def child():
    import torch
    import spp.lib
    spp.lib.LIB_PATH = args.child
    import spp
    from spp import acir, ccs
    from oracle import circuit as C
    golden = os.path.join(ROOT, "tests", "golden")
    sppc, pk, vk = (os.path.join(args.dir, "solved." + e) for e in ("sppc", "pk", "vk"))
    ctx = spp.Context(0)
    if not os.path.exists(pk):
        program = acir.load_program(os.path.join(golden, "reference_withdraw_acir.json"))
        c = ccs.load_ccs(os.path.join(golden, "reference_withdraw.ccs"))
        ccs.to_sppc_solved(ccs.decode_system(c), c, program, sppc)
        ctx.setup(sppc, b"\x0b" * 32, pk, vk)
    h = ctx.load_circuit(sppc, pk, 8)
    row = C.withdraw_inputs(json.load(open(os.path.join(golden, "withdraw_kat.json"))))
    row_b = b"".join(int(v).to_bytes(32, "big") for v in row)
    out = {"lib": args.child, "plan": h.plan_stats(), "sizes": {}}
    for B in SIZES:
        rs = b"".join((3 * i + 1).to_bytes(32, "big") + (5 * i + 2).to_bytes(32, "big") for i in range(B))
        dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
        d_in, d_rs = dev(row_b * B), dev(rs)
        d_proofs = torch.zeros(388 * B, dtype=torch.uint8, device="cuda")
        d_pws = torch.zeros(h.pw_len * B, dtype=torch.uint8, device="cuda")
        d_st = torch.ones(B, dtype=torch.int32, device="cuda")

        def call():
            h.prove_batch_device(B, d_in.data_ptr(), d_rs.data_ptr(), d_proofs.data_ptr(), d_pws.data_ptr(), d_st.data_ptr())
            h.sync()
        for _ in range(WARMUP[B]):
            call()
        times = []
        for _ in range(ITERS[B]):
            t0 = time.perf_counter()
            call()
            times.append(time.perf_counter() - t0)
        assert int(d_st.abs().sum().item()) == 0, "a proof was refused"
        med = statistics.median(times)
        rec = {"median_ms": med * 1e3, "min_ms": min(times) * 1e3, "max_ms": max(times) * 1e3, "proofs_per_s": B / med,
               "proof0_sha256": hashlib.sha256(bytes(d_proofs[:388].cpu().numpy())).hexdigest()}
        if B == 1:
            rec["last_timings_ms"] = h.last_timings()
        out["sizes"][str(B)] = rec
    h.close()
    ctx.close()
    print("PROBE " + json.dumps(out))


def main():
    new_lib = os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd", "libspp.so")
    runs = {"parent": [], "new": []}
    with tempfile.TemporaryDirectory() as d:
        for which in ("parent", "new", "parent", "new", "parent"):
            lib = args.parent if which == "parent" else new_lib
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, "--dir", d], capture_output=True, text=True,
                               timeout=420)
            line = [l for l in p.stdout.splitlines() if l.startswith("PROBE ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit("the %s run failed (exit %d)" % (which, p.returncode))
            runs[which].append(json.loads(line[0][6:]))
            sys.stderr.write("%s run done\n" % which)
            sys.stderr.flush()
    doc = {"what": "reference R1CS with its solver, resident inputs, 8-bit windows; host wall time per call (ms), median of the timed calls",
           "warmup": WARMUP, "iters": ITERS, "order": "parent, new, parent, new, parent (a fresh process each)",
           "plan_parent": runs["parent"][0]["plan"], "plan_new": runs["new"][0]["plan"], "sizes": {}}
    same_bytes = True
    for B in map(str, SIZES):
        par = [r["sizes"][B]["median_ms"] for r in runs["parent"]]
        new = [r["sizes"][B]["median_ms"] for r in runs["new"]]
        spread = (max(par) - min(par)) / min(par)
        ratio = statistics.median(par) / statistics.median(new)
        same_bytes = same_bytes and len({r["sizes"][B]["proof0_sha256"] for rr in runs.values() for r in rr}) == 1
        doc["sizes"][B] = {"parent_median_ms": par, "new_median_ms": new, "parent_spread": spread, "parent_over_new": ratio,
                           "new_faster_beyond_spread": max(new) < min(par) and ratio - 1 > spread,
                           "new_within_spread": abs(ratio - 1) <= spread,
                           "parent_proofs_per_s": int(B) / (statistics.median(par) / 1e3), "new_proofs_per_s": int(B) / (statistics.median(new) / 1e3)}
    doc["same_proof_bytes_in_every_run"] = same_bytes
    doc["b1_last_timings_ms"] = {"parent": runs["parent"][0]["sizes"]["1"]["last_timings_ms"], "new": runs["new"][0]["sizes"]["1"]["last_timings_ms"]}
    faster = [int(B) for B in doc["sizes"] if doc["sizes"][B]["new_faster_beyond_spread"]]
    doc["largest_size_where_new_is_faster"] = max(faster) if faster else 0
    text = json.dumps(doc, indent=1)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    child() if args.child else main()
