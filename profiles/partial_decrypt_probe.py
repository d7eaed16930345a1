"""Threshold opening on one GPU: what an auditor's partial decryptions cost, and what opening from partials costs against opening
with the rebuilt key.

(a) spp_rlwe_partial_decrypt_batch for one auditor of a 2-of-3 set on --records records (default 2^15), masks and smudging
    noise on: host wall time around the synchronous call, uploads (share, ciphertexts, noise) and the download of the partials
    included.  The kernels alone (k_partial_scale, k_rlwe_partial) are read from a `rocprofv3 --kernel-trace --stats` run of this
    script (profiles/partial_decrypt_kernel_stats.csv): the call has no device-pointer form to put a clock around.
(b) spp_audit_open_batch_partials on the two auditors' partials against spp_audit_open_batch with the reconstructed key, same
    records, same verifying key, alternating runs.
The records are --batch distinct ones (workload.audit_noise) proved here and repeated up to --records; a tenth of them is
tampered with (ciphertext byte, proof byte, wa_commitment) so that flags occur -- no coefficient >= q: the partial call refuses
such a ciphertext, an auditor has nothing to compute on it.  Before any time is reported the outputs are checked against each
other: owners and flags of both paths equal, the commitments the partial call keyed its masks by equal to the public witnesses'
of the untampered records.  Median of --runs after one warm-up each.
Prints one JSON line and writes it to --out (default profiles/partial_decrypt_probe.json)."""
import argparse, ctypes, json, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before libspp: one HIP runtime)
import spp  # noqa: E402
from spp import workload, witness as W  # noqa: E402
from spp.lib import check  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--records", type=int, default=1 << 15)
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "partial_decrypt_probe.json"))
args = ap.parse_args()
B, N = args.batch, args.records
Q = W.RLWE_Q
golden = os.path.join(ROOT, "tests", "golden")
rlwe_pk = json.load(open(os.path.join(golden, "rlwe_pk.json")))
fixture = json.load(open(os.path.join(golden, "rlwe_decrypt.json")))
shares = fixture["shares"][:2]
xs = np.asarray([int(s["x"]) for s in shares], dtype=np.uint32)
ys = [b"".join((int(v, 16) if isinstance(v, str) else int(v)).to_bytes(32, "big") for v in s["y"]) for s in shares]

tmp = tempfile.mkdtemp(prefix="spp_partial_")
sppc, pkp, vkp = (os.path.join(tmp, "c." + e) for e in ("sppc", "pk", "vk"))
spp.build_circuit(2, sppc, aux=list(rlwe_pk["a"]) + list(rlwe_pk["b"]))
ctx = spp.Context(0)
L = ctx.L
ctx.setup(sppc, b"\x2a" * 32, pkp, vkp)
vk = open(vkp, "rb").read()
p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
res = {"probe": "partial_decrypt_probe", "records": N, "batch": B, "runs": args.runs, "threshold": 2}

sk_mod_q = np.asarray(W.reconstruct_sk(ctx, shares), dtype=np.uint32)
h = ctx.load_circuit(sppc, pkp, 0)
sks, r8, e18, e28 = workload.audit_noise(0, B)
proofs1, pws1, status, c0_1, c1_1 = h.prove_audit_records(rlwe_pk["a"], rlwe_pk["b"], sks, r8, e18, e28,
                                                         [(1000003 * i + 17, 998244353 * i + 29) for i in range(B)])
h.close()
assert status == [0] * B
rep = -(-N // B)
as_rows = lambda blobs, n: np.frombuffer(b"".join(blobs), dtype=np.uint8).reshape(B, n)
proofs = np.ascontiguousarray(np.tile(as_rows(proofs1, 388), (rep, 1))[:N])
pws = np.ascontiguousarray(np.tile(as_rows(pws1, 76), (rep, 1))[:N])
c0 = np.ascontiguousarray(np.tile(np.asarray(c0_1, dtype=np.uint32), (rep, 1))[:N])
c1 = np.ascontiguousarray(np.tile(np.asarray(c1_1, dtype=np.uint32), (rep, 1))[:N])
idx = np.arange(N)
c0[idx % 30 == 1, 5] = (c0[idx % 30 == 1, 5] + Q // 256) % Q      # one message byte + 1: bits 2 and 4
proofs[idx % 30 == 2, 100] ^= 1                                   # bit 1
pws[idx % 30 == 3, 12:44] = pws[(idx[idx % 30 == 3] + 1) % N, 12:44]   # another record's wa_commitment: bits 1 and 4
proofs_b, pws_b = proofs.tobytes(), pws.tobytes()
seed = os.urandom(32)                                             # the pair's seed, the same at both ends
seeds = seed + seed
e, rho = W.rlwe_sample_smudge(L, N * 64, 1024)
e2, rho2 = W.rlwe_sample_smudge(L, N * 64, 1024)
parts = np.zeros((2, N, 64, 32), dtype=np.uint8)
cts = np.zeros((N, 32), dtype=np.uint8)


def leg_partial(me, ee, rr):
    t0 = time.perf_counter()
    check(L.spp_rlwe_partial_decrypt_batch(ctx.h, 2, p(xs), me, ys[me], N, p(c0), p(c1), p(ee), p(rr), seeds, p(parts[me]), p(cts)))
    return time.perf_counter() - t0


def leg_open(threshold):
    owners, flags = np.zeros((N, 64), dtype=np.uint8), np.zeros(N, dtype=np.uint32)
    t0 = time.perf_counter()
    if threshold:
        check(L.spp_audit_open_batch_partials(ctx.h, vk, len(vk), 2, ctypes.cast(parts.ctypes.data, ctypes.c_char_p), N, proofs_b, pws_b, p(c0),
                                              p(c1), p(owners), p(flags)))
    else:
        check(L.spp_audit_open_batch(ctx.h, vk, len(vk), p(sk_mod_q), N, proofs_b, pws_b, p(c0), p(c1), p(owners), p(flags)))
    return time.perf_counter() - t0, owners, flags


leg_partial(1, e2, rho2)                                          # the other auditor (and the warm-up)
tp = [leg_partial(0, e, rho) for _ in range(args.runs)]
untouched = idx % 30 != 1
res["a_commitments_equal_the_public_witnesses"] = bool((cts[untouched] == pws[untouched][:, 44:76]).all())
leg_open(True); leg_open(False)                                   # warm-up
tt, tk = [], []
for _ in range(args.runs):
    dt, owners_t, flags_t = leg_open(True); tt.append(dt)
    dt, owners_k, flags_k = leg_open(False); tk.append(dt)
ctx.close()
res["b_flags_equal"] = bool((flags_t == flags_k).all())
res["b_owners_equal"] = bool((owners_t == owners_k).all())
res["flag_counts"] = {str(f): int((flags_t == f).sum()) for f in sorted(set(flags_t.tolist()))}
failed = [k for k in ("a_commitments_equal_the_public_witnesses", "b_flags_equal", "b_owners_equal") if not res[k]]
if failed:
    sys.exit("partial_decrypt_probe: " + ", ".join(failed) + " is false; no time reported")
res.update({"a_partial_decrypt_ms": round(statistics.median(tp) * 1e3, 2), "a_runs_ms": [round(x * 1e3, 2) for x in tp],
            "a_records_per_s": round(N / statistics.median(tp), 1),
            "b_open_partials_ms": round(statistics.median(tt) * 1e3, 2), "b_open_partials_runs_ms": [round(x * 1e3, 2) for x in tt],
            "b_open_key_ms": round(statistics.median(tk) * 1e3, 2), "b_open_key_runs_ms": [round(x * 1e3, 2) for x in tk],
            "b_partials_over_key_time": round(statistics.median(tt) / statistics.median(tk), 4)})

line = json.dumps(res)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
