"""Audit records on one GPU: opening them in one pass against the composed path, and what the ciphertext costs the prover.

(a) spp_audit_open_batch on --records records (default 2^15): one upload, k_verify + k_audit_open, one download;
(b) the same decisions over the calls that existed before it: spp_verify_batch, packing on the host (numpy) +
    spp_poseidon2_sponge_batch, spp_rlwe_decrypt_batch, spp_poseidon_hash_batch, and the range check and comparisons in numpy
    (no curve check: H(x, y) == wa_commitment implies it for an honest commitment, and Python big ints would only slow (b) down);
(c) spp_prove_audit_records_device against spp_prove_audit_from_secrets_device at --batch (default 2048, the bench batch): rounds
    of --steps pipelined calls each, the two legs taking turns; proofs/s per round, the median over the rounds, and the spread
    (max - min) / median of the baseline leg's own rounds.
The records are --batch distinct ones (workload.audit_noise) proved here, repeated up to --records; a tenth of them is tampered
with (ciphertext byte, proof byte, wa_commitment) so that every flag occurs.  (a) and (b) are host wall time around calls that
end in a device synchronise, all buffers made beforehand, median of --runs after one warm-up each; their flags are compared.
Prints one JSON line and writes it to --out (default profiles/audit_open_probe.json)."""
import argparse, ctypes, json, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before libspp: one HIP runtime)
import spp  # noqa: E402
from spp import workload  # noqa: E402
from spp.lib import check  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--records", type=int, default=1 << 15)
ap.add_argument("--batch", type=int, default=2048)
ap.add_argument("--runs", type=int, default=3, help="timed runs of (a) and of (b)")
ap.add_argument("--rounds", type=int, default=5, help="timed rounds per leg of (c)")
ap.add_argument("--steps", type=int, default=6, help="pipelined calls per round of (c)")
ap.add_argument("--window", type=int, default=0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audit_open_probe.json"))
args = ap.parse_args()
B, N = args.batch, args.records
Q = 167772161
golden = os.path.join(ROOT, "tests", "golden")
rlwe_pk = json.load(open(os.path.join(golden, "rlwe_pk.json")))
sk_mod_q = np.asarray(json.load(open(os.path.join(golden, "rlwe_decrypt.json")))["sk_mod_q"], dtype=np.uint32)   # the key's secret half

tmp = tempfile.mkdtemp(prefix="spp_audit_open_")
sppc, pkp, vkp = (os.path.join(tmp, "c." + e) for e in ("sppc", "pk", "vk"))
spp.build_circuit(2, sppc, aux=list(rlwe_pk["a"]) + list(rlwe_pk["b"]))
ctx = spp.Context(0)
L = ctx.L
ctx.setup(sppc, b"\x2a" * 32, pkp, vkp)
vk = open(vkp, "rb").read()
h = ctx.load_circuit(sppc, pkp, args.window)
dev = torch.device("cuda", 0)
up = lambda raw: torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
cp = lambda x: ctypes.cast(x.ctypes.data, ctypes.c_char_p)    # a numpy buffer where the binding takes bytes: no copy
res = {"probe": "audit_open_probe", "records": N, "batch": B, "runs": args.runs, "rounds": args.rounds, "steps_per_round": args.steps}

# ---- (c) the prover: records against proofs only ----
sks, r8, e18, e28 = workload.audit_noise(0, B)
d_a, d_b = up(np.asarray(rlwe_pk["a"], dtype=np.uint32).tobytes()), up(np.asarray(rlwe_pk["b"], dtype=np.uint32).tobytes())
d_sk = up(b"".join(int(v).to_bytes(32, "big") for v in sks))
d_r, d_e1, d_e2 = up(r8.tobytes()), up(e18.tobytes()), up(e28.tobytes())
d_rs = up(b"".join((1000003 * i + 17).to_bytes(32, "big") + (998244353 * i + 29).to_bytes(32, "big") for i in range(B)))
ins = [t.data_ptr() for t in (d_a, d_b, d_sk, d_r, d_e1, d_e2, d_rs)]
outs = [[torch.zeros(B * 388, dtype=torch.uint8, device=dev), torch.zeros(B * 76, dtype=torch.uint8, device=dev),
         torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B * 64, dtype=torch.int32, device=dev),
         torch.zeros(B * 1024, dtype=torch.int32, device=dev)] for _ in range(2)]   # two sets: consecutive calls are pipelined


def round_of(records):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(args.steps):
        o = [t.data_ptr() for t in outs[k & 1]]
        if records:
            h.prove_audit_records_device(B, *ins, *o)
        else:
            h.prove_audit_from_secrets_device(B, *ins, *o[:3])
    h.sync()
    return args.steps * B / (time.perf_counter() - t0)


round_of(True); round_of(False)                                   # warm-up (workspaces, scratch)
rates = {True: [], False: []}
for _ in range(args.rounds):
    for leg in (False, True):
        rates[leg].append(round_of(leg))
base, rec = statistics.median(rates[False]), statistics.median(rates[True])
res.update({"c_from_secrets_proofs_per_s": round(base, 1), "c_records_proofs_per_s": round(rec, 1),
            "c_from_secrets_rounds": [round(x, 1) for x in rates[False]], "c_records_rounds": [round(x, 1) for x in rates[True]],
            "c_records_over_from_secrets": round(rec / base, 4),
            "c_from_secrets_spread": round((max(rates[False]) - min(rates[False])) / base, 4)})
assert int(outs[(args.steps - 1) & 1][2].abs().sum().item()) == 0
o = outs[(args.steps - 1) & 1]                                    # the last call was a records call
dl = lambda t: t.cpu().numpy()
proofs1, pws1 = dl(o[0]).reshape(B, 388), dl(o[1]).reshape(B, 76)
c0_1, c1_1 = dl(o[3]).view(np.uint32).reshape(B, 64), dl(o[4]).view(np.uint32).reshape(B, 1024)
h.close()

# ---- the records of (a) and (b): B distinct ones repeated, a tenth tampered with ----
rep = -(-N // B)
proofs = np.ascontiguousarray(np.tile(proofs1, (rep, 1))[:N])
pws = np.ascontiguousarray(np.tile(pws1, (rep, 1))[:N])
c0 = np.ascontiguousarray(np.tile(c0_1, (rep, 1))[:N])
c1 = np.ascontiguousarray(np.tile(c1_1, (rep, 1))[:N])
idx = np.arange(N)
c0[idx % 30 == 1, 5] = (c0[idx % 30 == 1, 5] + Q // 256) % Q      # one message byte + 1: bits 2 and 4
proofs[idx % 30 == 2, 100] ^= 1                                   # bit 1
pws[idx % 30 == 3, 12:44] = pws[(idx[idx % 30 == 3] + 1) % N, 12:44]   # another record's wa_commitment: bits 1 and 4
c1[idx % 300 == 4, 777] = Q                                       # a coefficient = q: bit 2 (and whatever it decrypts to)
proofs_b, pws_b = proofs.tobytes(), pws.tobytes()


def leg_a():
    owners, flags = np.zeros((N, 64), dtype=np.uint8), np.zeros(N, dtype=np.uint32)
    t0 = time.perf_counter()
    check(L.spp_audit_open_batch(ctx.h, vk, len(vk), p(sk_mod_q), N, proofs_b, pws_b, p(c0), p(c1), p(owners), p(flags)))
    return time.perf_counter() - t0, owners, flags


def pack_be(c):
    """pack_values (7 coefficients x 32 bits per field) as 32-byte big-endian fields, vectorised"""
    n, m = c.shape
    nf = -(-m // 7)
    padded = np.zeros((n, nf * 7), dtype=np.uint32)
    padded[:, :m] = c
    out = np.zeros((n, nf, 8), dtype=">u4")
    out[:, :, 1:] = padded.reshape(n, nf, 7)[:, :, ::-1]
    return out.view(np.uint8).reshape(n, nf * 32)


def leg_b():
    t0 = time.perf_counter()
    ok = np.zeros(N, dtype=np.int32)
    check(L.spp_verify_batch(ctx.h, vk, len(vk), N, proofs_b, pws_b, 76, p(ok), None))
    in_range = (c0 < Q).all(axis=1) & (c1 < Q).all(axis=1)
    packed = np.ascontiguousarray(np.concatenate([pack_be(c0), pack_be(c1)], axis=1))
    ct = np.zeros((N, 32), dtype=np.uint8)
    check(L.spp_poseidon2_sponge_batch(ctx.h, N, 157, cp(packed), p(ct)))
    msg = np.zeros((N, 64), dtype=np.uint8)
    check(L.spp_rlwe_decrypt_batch(ctx.h, p(sk_mod_q), N, p(np.ascontiguousarray(c0 % Q)), p(np.ascontiguousarray(c1 % Q)), p(msg)))
    owners = np.ascontiguousarray(np.concatenate([msg[:, 31::-1], msg[:, :31:-1]], axis=1))
    wa = np.zeros((N, 32), dtype=np.uint8)
    check(L.spp_poseidon_hash_batch(ctx.h, N, 2, cp(owners), p(wa)))
    flags = (ok == 0).astype(np.uint32) | (2 * (~in_range | (ct != pws[:, 44:76]).any(axis=1))).astype(np.uint32) \
        | (4 * (wa != pws[:, 12:44]).any(axis=1)).astype(np.uint32)
    return time.perf_counter() - t0, owners, flags


leg_a(); leg_b()                                                  # warm-up
ta, tb = [], []
for _ in range(args.runs):
    dt, owners_a, flags_a = leg_a(); ta.append(dt)
    dt, owners_b, flags_b = leg_b(); tb.append(dt)
ctx.close()
res.update({"a_audit_open_ms": round(statistics.median(ta) * 1e3, 2), "a_runs_ms": [round(x * 1e3, 2) for x in ta],
            "b_composed_ms": round(statistics.median(tb) * 1e3, 2), "b_runs_ms": [round(x * 1e3, 2) for x in tb],
            "a_over_b_time": round(statistics.median(ta) / statistics.median(tb), 4),
            "a_records_per_s": round(N / statistics.median(ta), 1),
            "a_flags_equal_b_flags": bool((flags_a == flags_b).all()), "a_owners_equal_b_owners": bool((owners_a == owners_b).all()),
            "flag_counts": {str(f): int((flags_a == f).sum()) for f in sorted(set(flags_a.tolist()))},
            "a_not_slower_than_b": bool(statistics.median(ta) <= statistics.median(tb))})

line = json.dumps(res)
print(line, flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
# the one pass moves a third of the bytes and synchronises once instead of four times: it must decide the same and not be slower
failed = [k for k in ("a_flags_equal_b_flags", "a_owners_equal_b_owners", "a_not_slower_than_b") if not res[k]]
if failed:
    sys.exit("audit_open_probe: " + ", ".join(failed) + " is false")
