"""GPU: threshold opening -- spp_rlwe_partial_decrypt_batch, spp_rlwe_combine_partials, spp_audit_open_batch_partials and the
three sub-commands around them -- against tests/partial_vectors.py (Python integers; shares from a Python Shamir split) and
against the path that rebuilds the key (spp_audit_open_batch, `audit-open --shares`)."""
import ctypes
import json
import os
import random

import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None

from conftest import GOLDEN
import auditor_vectors as V
import partial_vectors as P

pytestmark = pytest.mark.gpu

R, Q = P.R, P.Q
BAD_PROOF, BAD_CT, BAD_ID, BAD_PARTIALS = 1, 2, 4, 8
NREC = 65


@pytest.fixture(scope="module")
def ctx():
    import spp
    c = spp.Context(0)
    yield c
    c.close()


def device_partial(ctx, share, xs, me, cts, seeds=None, e=None, rho=None, want_commitments=False):
    from spp import witness
    return witness.rlwe_partial_decrypt(ctx, xs, me, share, [c[0] for c in cts], [c[1] for c in cts], e, rho,
                                        None if seeds is None else seeds[me], want_commitments)


def as_ints(part):
    """uint8 [count, 64, 32] -> [count][64] ints"""
    return [P.unbe(part[i].tobytes()) for i in range(part.shape[0])]


# ---------------------------------------------------------------------------------------------------------- (a) the partials
@pytest.mark.parametrize("name,count,blinded", [("1of1", 1, True), ("1of1", 2, False), ("1of1", 65, True),
                                                ("2of3", 1, False), ("2of3", 2, True), ("2of3", 65, True),
                                                ("3of5", 1, True), ("3of5", 2, False), ("3of5", 65, False)])
def test_every_partial_equals_the_restatement(ctx, name, count, blinded):
    t, xs, _ = P.SETS[name]
    shares = P.shares_of(name)
    cts = P.records(count)
    seeds = P.pair_seeds(xs) if blinded else None
    want_ct = [P.ct_commitment(c0, c1) for c0, c1 in cts]
    for me in range(t):
        e, rho = P.smudge(count, 100 * t + me) if blinded else (None, None)
        got, got_ct = device_partial(ctx, shares[me], xs, me, cts, seeds, e, rho, want_commitments=True)
        assert got_ct == want_ct                                   # the masks are keyed by the recomputed commitment
        for i, (c0, c1) in enumerate(cts):
            want = P.partial(shares[me], xs, me, c0, c1, None if seeds is None else seeds[me], e and e[i], rho and rho[i], want_ct[i])
            assert as_ints(got[i:i + 1])[0] == want, (name, me, i)


def test_the_batch_size_at_which_the_commitments_get_a_kernel_of_their_own(ctx):
    """Up to 2 048 records (RP_COOP_SPONGE_MAX) the wave that computes a record's partial hashes its ciphertext too; from 2 049 on
    the commitments come from a kernel with one lane per record.  2 049 distinct records through the second path: records 0, 63,
    64, 2 047 and 2 048 (alone in the last block of that kernel) against the restatement, all commitments and all partials of
    the first 2 048 against the first path's, which the tests above hold against the restatement."""
    import numpy as np
    count = 2049
    rng = np.random.default_rng(20491)
    c0 = rng.integers(0, Q, size=(count, 64), dtype=np.uint32)
    c1 = rng.integers(0, Q, size=(count, 1024), dtype=np.uint32)
    cts = list(zip(c0, c1))
    t, xs, _ = P.SETS["2of3"]
    share, seeds = P.shares_of("2of3")[1], P.pair_seeds(xs)
    e, rho = P.smudge(count, 2049)
    big, big_ct = device_partial(ctx, share, xs, 1, cts, seeds, e, rho, want_commitments=True)
    small, small_ct = device_partial(ctx, share, xs, 1, cts[:2048], seeds, e[:2048], rho[:2048], want_commitments=True)
    assert big_ct[:2048] == small_ct and (big[:2048] == small).all()
    for i in (0, 63, 64, 2047, 2048):
        ct = P.ct_commitment(c0[i].tolist(), c1[i].tolist())
        assert big_ct[i] == ct, i
        assert as_ints(big[i:i + 1])[0] == P.partial(share, xs, 1, c0[i].tolist(), c1[i].tolist(), seeds[1], e[i], rho[i], ct), i


def test_sixty_four_auditors(ctx):
    """t = 64 at one record: two of the 64 partials against the restatement (63 masks per slot each), and all 64 combined"""
    from spp import witness
    xs = V.share_xs(64)
    shares = P.split(list(P.small_key()), 64, xs, random.Random(64))
    seeds = P.pair_seeds(xs)
    cts = P.records(1)
    c0, c1 = cts[0]
    parts = [device_partial(ctx, shares[m], xs, m, cts, seeds) for m in range(64)]
    for m in (0, xs.index((1 << 32) - 1)):
        assert as_ints(parts[m])[0] == P.partial(shares[m], xs, m, c0, c1, seeds[m]), m
    owners, msg, flags = witness.rlwe_combine_partials(ctx, parts, [c0])
    key = [v if v < R // 2 else v - R for v in P.small_key()]
    assert flags == [0] and msg[0].tolist() == V.decrypt(key, c0, c1)
    assert owners[0] == V.decode_owner(msg[0].tolist())


def test_extremes_of_the_accumulator_and_the_blinding(ctx):
    """t = 1 at x = 1: lambda = 1, so the share is the scaled share.  All r - 1 against all q - 1 (slot 0: one added term, 1 023
    subtracted; slot 63: 64 added), the share of limbs 0x2fffffff, 0xffffffff x 7, a single non-zero c1[j] at j = 0, 63, 64,
    1023; e = +-2^20 and rho = 2^64 - 1 on the slots."""
    e = [[P.EXTREME_SMUDGE[k % 4][0] for k in range(64)]]
    rho = [[P.EXTREME_SMUDGE[k % 4][1] for k in range(64)]]
    assert {(1 << 20, (1 << 64) - 1), (-(1 << 20), (1 << 64) - 1)} <= set(zip(e[0], rho[0]))
    c0 = P.records(1)[0][0]
    for name, u, c1 in P.extreme_dots():
        if max(c1) >= Q:
            continue                                                # the header's bound, not the call's: refused by the API
        got = as_ints(device_partial(ctx, u, [1], 0, [(c0, c1)], None, e, rho))[0]
        assert got == P.partial(u, [1], 0, c0, c1, None, e[0], rho[0]), name
        plain = as_ints(device_partial(ctx, u, [1], 0, [(c0, c1)]))[0]
        assert plain == P.dot(u, c1), name


# ------------------------------------------------------------------------------------------------------- (b) the combination
def test_combined_partials_decrypt_like_the_key_on_every_rounding_decision(ctx):
    """e = rho = 0: spp_rlwe_combine_partials gives exactly V.decrypt on the dialled ciphertexts (every tie, both sides of the
    centring, byte 128 from both sides), the accumulator extremes and 65 ciphertexts of the pool.  The keys, given mod q, are
    shared as their centred Fr values."""
    from spp import witness
    vectors = V.dialled_vectors() + V.extreme_vectors() + V.dialled_pool()[:65]
    seen = 0
    for n, (sk, group) in enumerate(V.by_key(vectors)):
        name = ("2of3", "3of5")[n % 2]
        t, xs, _ = P.SETS[name]
        shares = P.split(P.centred_key(sk), t, xs, random.Random(1234 + n))
        seeds = P.pair_seeds(xs, n)
        cts = [(v["c0"], v["c1"]) for v in group]
        parts = [device_partial(ctx, shares[m], xs, m, cts, seeds) for m in range(t)]
        owners, msg, flags = witness.rlwe_combine_partials(ctx, parts, [c[0] for c in cts])
        assert flags == [0] * len(group)
        for i, v in enumerate(group):
            assert msg[i].tolist() == v["msg"], v["name"]
            seen += 1
    assert seen == 10 + 6 + 65                                      # pool #0 is dialled_vectors' -X^63 ciphertext: by_key keeps both


# ---------------------------------------------------------------------------------------------- (c) whole records, both paths
@pytest.fixture(scope="module")
def decrypt_fixture():
    return json.load(open(os.path.join(GOLDEN, "rlwe_decrypt.json")))


@pytest.fixture(scope="module")
def records(ctx, audit_artifacts, rlwe_pk):
    """65 audit records made the way tests/test_gpu_audit_records.py makes them (host form)"""
    from spp import workload
    sks, r8, e18, e28 = workload.audit_noise(900, NREC)
    rs_vals = [(107 * i + 3, 109 * i + 5) for i in range(NREC)]
    h = ctx.load_circuit(audit_artifacts["sppc"], audit_artifacts["pk"], 6)
    try:
        proofs, pws, status, c0, c1 = h.prove_audit_records(rlwe_pk["a"], rlwe_pk["b"], sks, r8, e18, e28, rs_vals)
    finally:
        h.close()
    assert status == [0] * NREC
    return dict(proofs=list(proofs), pws=list(pws), c0=c0, c1=c1, sks=sks, vk=open(audit_artifacts["vk"], "rb").read())


def test_records_open_from_partials_as_from_the_key(ctx, records, decrypt_fixture):
    from spp import witness
    from oracle import hashes as H
    shares = decrypt_fixture["shares"]
    xs = [int(s["x"]) for s in shares]
    ys = [[int(v, 16) if isinstance(v, str) else int(v) for v in s["y"]] for s in shares]
    sk = witness.reconstruct_sk(ctx, shares)
    proofs, pws = list(records["proofs"]), list(records["pws"])
    c0, c1 = records["c0"].copy(), records["c1"].copy()
    proofs[30] = proofs[30][:100] + bytes([proofs[30][100] ^ 1]) + proofs[30][101:]            # a forged proof
    c0[[10, 11]] = c0[[11, 10]]; c1[[10, 11]] = c1[[11, 10]]                                   # two ciphertexts swapped
    pws[40] = pws[40][:12] + pws[41][12:44] + pws[40][44:]                                     # the identity of another record
    seeds = P.pair_seeds(xs, 77)
    parts = []
    for m in range(len(xs)):                                                                   # each auditor on what it was handed
        e, rho = witness.rlwe_sample_smudge(ctx.L, NREC * 64, 1024)
        assert int(abs(e).max()) <= 1024 and len(set(rho.tolist())) > NREC * 63
        parts.append(witness.rlwe_partial_decrypt(ctx, xs, m, ys[m], c0, c1, e, rho, seeds[m]))
    for vk, pr in ((records["vk"], proofs), (None, None)):
        owners, flags = ctx.audit_open(vk, sk, pr, pws, c0, c1)
        owners_t, flags_t = ctx.audit_open(vk, None, pr, pws, c0, c1, partials=parts)
        print("flags:", flags_t)
        assert owners_t == owners and flags_t == flags
        want = {10: BAD_CT | BAD_ID, 11: BAD_CT | BAD_ID, 40: BAD_ID | (BAD_PROOF if vk else 0), 30: BAD_PROOF if vk else 0}
        assert flags_t == [want.get(i, 0) for i in range(NREC)]
    true_owner = [H.fixed_base_scalar_mul(s) for s in records["sks"]]
    assert [owners_t[i] for i in range(NREC) if i not in (10, 11)] == [true_owner[i] for i in range(NREC) if i not in (10, 11)]


# ------------------------------------------------------------------------------------------------------------------ (d) bit 8
def test_partials_that_do_not_belong_together_are_flagged(ctx):
    import numpy as np
    from spp import witness
    count = 5
    cts = P.records(count)
    c0 = [c[0] for c in cts]
    shares = P.split(list(P.small_key()), 2, [1, 2, 3], random.Random(88))       # 2 of 3: shares[j] belongs to x = j + 1
    a12 = device_partial(ctx, shares[0], [1, 2], 0, cts)
    b12 = device_partial(ctx, shares[1], [1, 2], 1, cts)
    a13 = device_partial(ctx, shares[0], [1, 3], 0, cts)
    pws = [bytes(76)] * count
    owners, msg, flags = witness.rlwe_combine_partials(ctx, [a12, b12], c0)
    key = [v if v < R // 2 else v - R for v in P.small_key()]
    assert flags == [0] * count and [m.tolist() for m in msg] == [V.decrypt(key, *c) for c in cts]
    # auditor 1 computed for the set {1, 3}, auditor 2 for {1, 2}: every record
    _, _, flags = witness.rlwe_combine_partials(ctx, [a13, b12], c0)
    assert flags == [BAD_PARTIALS] * count
    assert [f & BAD_PARTIALS for f in ctx.audit_open(None, None, None, pws, c0, [c[1] for c in cts], partials=[a13, b12])[1]] == [BAD_PARTIALS] * count

    def bump(part, rec, slot, by):
        out = part.copy()
        v = (int.from_bytes(out[rec, slot].tobytes(), "big") + by) % R
        out[rec, slot] = np.frombuffer(v.to_bytes(32, "big"), dtype=np.uint8)
        return out
    # one slot of one partial raised by 2^110: exactly that record, through both calls
    for rec, slot in ((0, 0), (3, 63)):
        bad = bump(a12, rec, slot, 1 << 110)
        want = [BAD_PARTIALS if i == rec else 0 for i in range(count)]
        _, msg2, flags = witness.rlwe_combine_partials(ctx, [bad, b12], c0)
        assert flags == want and [i for i in range(count) if msg2[i].tolist() != msg[i].tolist()] in ([], [rec])
        got = ctx.audit_open(None, None, None, pws, c0, [c[1] for c in cts], partials=[bad, b12])[1]
        assert [f & BAD_PARTIALS for f in got] == want
        want_msg, want_flag = P.combine([as_ints(bad)[rec], as_ints(b12)[rec]], c0[rec])
        assert msg2[rec].tolist() == want_msg and want_flag == BAD_PARTIALS
    # the edge itself: +-(2^104 - 1) accepted, +-2^104 flagged (record 1, slot 7 set to the value minus the other partial)
    other = as_ints(b12)[1][7]
    for value, flagged in ((P.SMALL - 1, 0), (-(P.SMALL - 1), 0), (P.SMALL, BAD_PARTIALS), (-P.SMALL, BAD_PARTIALS)):
        edge = bump(a12, 1, 7, (value - other - as_ints(a12)[1][7]) % R)
        _, _, flags = witness.rlwe_combine_partials(ctx, [edge, b12], c0)
        assert flags == [0, flagged, 0, 0, 0], value
    # q added to a slot: nothing flagged, no byte changed
    plus_q = bump(a12, 2, 31, Q)
    _, msg3, flags = witness.rlwe_combine_partials(ctx, [plus_q, b12], c0)
    assert flags == [0] * count and (msg3 == msg).all()
    base = ctx.audit_open(None, None, None, pws, c0, [c[1] for c in cts], partials=[a12, b12])
    assert ctx.audit_open(None, None, None, pws, c0, [c[1] for c in cts], partials=[plus_q, b12]) == base


# -------------------------------------------------------------------------------------------------------------- (e) refusals
def test_refusals_leave_the_outputs_untouched_and_name_the_index(ctx):
    import numpy as np
    import spp
    L = ctx.L
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    t, xs, _ = P.SETS["2of3"]
    share = P.be(P.shares_of("2of3")[0])
    cts = P.records(2)
    c0 = np.asarray([c[0] for c in cts], dtype=np.uint32)
    c1 = np.asarray([c[1] for c in cts], dtype=np.uint32)
    cx = np.asarray(xs, dtype=np.uint32)
    out = np.full(2 * 64 * 32, 0xAB, dtype=np.uint8)
    ctc = np.full(64, 0xAB, dtype=np.uint8)
    base = dict(ctx=ctx.h, t=t, xs=p(cx), self=0, share=share, count=2, c0=p(c0), c1=p(c1), e=None, rho=None, seeds=None, out=p(out), ct=p(ctc))
    order = ("ctx", "t", "xs", "self", "share", "count", "c0", "c1", "e", "rho", "seeds", "out", "ct")

    def partial(**k):
        rc = L.spp_rlwe_partial_decrypt_batch(*[{**base, **k}[n] for n in order])
        if rc != 0:
            assert (out == 0xAB).all() and (ctc == 0xAB).all()
        return rc, spp.last_error()
    for name in ("ctx", "xs", "share", "c0", "c1", "out"):
        assert partial(**{name: None}) == (-1, "NULL argument"), name
    assert partial(t=0)[0] == -1 and partial(t=65)[0] == -1 and "[1, 64]" in spp.last_error()
    rc, err = partial(self=2)
    assert rc == -1 and "self 2" in err
    for bad_xs, word in (([3, 0], "xs[1] is 0"), ([3, 3], "xs[1] repeats xs[0]")):
        rc, err = partial(xs=p(np.asarray(bad_xs, dtype=np.uint32)))
        assert rc == -1 and word in err, err
    for i in (0, 1023):
        bad = share[:32 * i] + R.to_bytes(32, "big") + share[32 * (i + 1):]
        rc, err = partial(share=bad)
        assert rc == -1 and "share value %d " % i in err, err
    for arr, key, rec, idx in ((c0, "c0", 1, 63), (c1, "c1", 0, 0), (c1, "c1", 1, 1023)):
        bad = arr.copy()
        bad[rec, idx] = Q
        rc, err = partial(**{key: p(bad)})
        assert rc == -1 and "ciphertext %d: %s[%d]" % (rec, key, idx) in err, err
    assert partial(count=(1 << 24) + 1)[0] == -1 and "2^24" in spp.last_error()
    assert partial(count=0, c0=None, c1=None, out=None, ct=None)[0] == 0 and (out == 0xAB).all()
    assert partial()[0] == 0 and not (out == 0xAB).all()
    good = out.copy()

    # the combiner
    parts = np.concatenate([good, good])
    msg = np.full(128, 0xCD, dtype=np.uint8)
    flags = np.full(2, 0xEE, dtype=np.uint32)
    cbase = dict(ctx=ctx.h, t=2, count=2, parts=parts.tobytes(), c0=p(c0), msg=p(msg), flags=p(flags))

    def combine(**k):
        rc = L.spp_rlwe_combine_partials(*[{**cbase, **k}[n] for n in ("ctx", "t", "count", "parts", "c0", "msg", "flags")])
        if rc != 0:
            assert (msg == 0xCD).all() and (flags == 0xEE).all()
        return rc, spp.last_error()
    for name in ("ctx", "parts", "c0", "msg"):
        assert combine(**{name: None}) == (-1, "NULL argument"), name
    assert combine(t=0)[0] == -1 and combine(t=65)[0] == -1
    i = 2 * 64 + 64 + 5                                              # auditor 1, record 1, slot 5
    bad = parts.copy()
    bad[32 * i:32 * i + 32] = np.frombuffer(R.to_bytes(32, "big"), dtype=np.uint8)
    rc, err = combine(parts=bad.tobytes())
    assert rc == -1 and "partial %d (auditor 1, record 1, slot 5)" % i in err, err
    badc = c0.copy()
    badc[1, 2] = Q + 1
    rc, err = combine(c0=p(badc))
    assert rc == -1 and "ciphertext 1: c0[2]" in err, err
    assert combine(count=(1 << 24) + 1)[0] == -1 and "2^24" in spp.last_error()
    assert combine(count=0)[0] == 0 and (msg == 0xCD).all()
    assert combine(flags=None)[0] == 0 and not (msg == 0xCD).all() and (flags == 0xEE).all()

    # the open call: the argument checks of spp_audit_open_batch, and the partials'
    owners = np.full(128, 0xCD, dtype=np.uint8)
    pws = bytes(152)
    obase = dict(ctx=ctx.h, vk=None, vk_len=0, t=2, parts=parts.tobytes(), count=2, proofs=None, pws=pws, c0=p(c0), c1=p(c1), owners=p(owners),
                 flags=p(flags))

    def opn(**k):
        rc = L.spp_audit_open_batch_partials(*[{**obase, **k}[n] for n in ("ctx", "vk", "vk_len", "t", "parts", "count", "proofs", "pws", "c0", "c1",
                                                                           "owners", "flags")])
        if rc != 0:
            assert (owners == 0xCD).all() and (flags == 0xEE).all()
        return rc, spp.last_error()
    for name in ("ctx", "parts", "pws", "c0", "c1", "owners", "flags"):
        rc, err = opn(**{name: None})
        assert rc == -1 and "NULL" in err, name
    assert opn(t=0)[0] == -1 and opn(t=65)[0] == -1 and opn(vk_len=5)[0] == -1
    rc, err = opn(parts=bad.tobytes())
    assert rc == -1 and "(auditor 1, record 1, slot 5)" in err
    assert opn(count=(1 << 24) + 1)[0] == -1 and "2^24" in spp.last_error()
    assert opn(count=0)[0] == 0 and (owners == 0xCD).all()
    rc, _ = opn(c1=p(np.where(np.arange(2048).reshape(2, 1024) == 1024 + 9, Q, c1).astype(np.uint32)))      # a coefficient >= q: bit 2, no refusal
    assert rc == 0 and flags[1] & BAD_CT and not (owners == 0xCD).all()
    # the wrappers refuse what cannot be a set of partials
    with pytest.raises(ValueError):
        ctx.audit_open(None, None, None, [pws[:76]] * 2, c0, c1)
    with pytest.raises(ValueError):
        ctx.audit_open(None, [0] * 1024, None, [pws[:76]] * 2, c0, c1, partials=[good.reshape(2, 64, 32)])
    e, rho = np.zeros(4, dtype=np.int32), np.zeros(4, dtype=np.uint64)
    assert L.spp_rlwe_sample_smudge(4, (1 << 20) + 1, p(e), p(rho)) == -1 and "2^20" in spp.last_error()
    assert L.spp_rlwe_sample_smudge(4, 0, p(e), p(rho)) == 0 and e.tolist() == [0] * 4 and len(set(rho.tolist())) == 4
    assert L.spp_rlwe_sample_smudge(4, 5, None, p(rho)) == -1


# -------------------------------------------------------------------------------------------------------------------- (f) CLI
def test_cli_round_trip(tmp_path, capsys):
    """rlwe-keygen, audit-pair-seeds, two audit-partial runs, audit-open --partials on one record under the fresh key: the same
    lines as audit-open --shares.  The record is the oracle's encryption under that key with the public witness of its own
    commitments (`-`: verified elsewhere); audit-partial refuses a ciphertext that is not the public witness's."""
    from spp import cli, witness as W
    from oracle import rlwe, hashes as H
    keys = str(tmp_path / "keys")
    assert cli.main(["rlwe-keygen", "--out", keys, "--threshold", "2", "--shares", "3"]) == 0
    assert cli.main(["audit-pair-seeds", "--shares", "3", "--out", keys]) == 0
    s13 = [W.load_pair_seeds_json(os.path.join(keys, "pair_seeds_%d.json" % i)) for i in (1, 3)]
    assert s13[0][1][3] == s13[1][1][1] and s13[0][1][2] != s13[0][1][3] and sorted(s13[0][1]) == [2, 3]
    pk_a, pk_b = W.load_rlwe_pk_json(os.path.join(keys, "rlwe_pk.json"))
    owner = H.fixed_base_scalar_mul(4242)
    rng = random.Random(5)
    r, e1, e2 = ([rng.randint(-3, 3) for _ in range(n)] for n in (1024, 64, 1024))
    c0, c1, _, _ = rlwe.rlwe_witness(pk_a, pk_b, r, e1, e2, rlwe.owner_msg(*owner))
    ct = H.poseidon2_sponge(rlwe.pack_values(c0) + rlwe.pack_values(c1))
    pw = (2).to_bytes(4, "big") + (0).to_bytes(4, "big") + (2).to_bytes(4, "big") + H.poseidon_hash2(*owner).to_bytes(32, "big") + ct.to_bytes(32, "big")
    proof, pwf, ctj, other = (str(tmp_path / n) for n in ("a.proof", "a.pw", "ciphertext.json", "other.json"))
    open(proof, "wb").write(bytes(388)); open(pwf, "wb").write(pw)
    json.dump(W.ciphertext_json(c0, c1, owner), open(ctj, "w"))
    c0b = list(c0); c0b[5] = (c0b[5] + 1) % Q
    json.dump(W.ciphertext_json(c0b, c1, owner), open(other, "w"))
    share = lambda i: os.path.join(keys, "rlwe_sk_shares", "share_%d.json" % i)
    seedf = lambda i: os.path.join(keys, "pair_seeds_%d.json" % i)
    part = lambda i: str(tmp_path / ("partial_%d.json" % i))
    capsys.readouterr()
    assert cli.main(["audit-partial", share(1), "--with", "3", ctj, pwf, "--pair-seeds", seedf(1), "--out", part(1)]) == 0
    assert cli.main(["audit-partial", share(3), ctj, pwf, "--with", "1", "--pair-seeds", seedf(3), "--smudge", "2048", "--out", part(3)]) == 0
    assert cli.main(["audit-partial", share(2), "--with", "1", other, pwf, "--pair-seeds", seedf(2), "--out", part(2)]) == 1
    assert "REFUSED" in capsys.readouterr().err and not os.path.exists(part(2))
    assert cli.main(["audit-partial", share(2), "--with", "1", ctj, pwf, "--smudge", "65537", "--out", part(2)]) == 2       # 2 * 65 537 > 2^17
    assert "2^17" in capsys.readouterr().err and not os.path.exists(part(2))
    assert cli.main(["audit-open", "-", proof, pwf, ctj, "--shares", share(1), share(3)]) == 0
    by_key = capsys.readouterr().out
    assert "owner_x = 0x%064x" % owner[0] in by_key and "owner_y = 0x%064x" % owner[1] in by_key
    assert cli.main(["audit-open", "-", proof, pwf, ctj, "--partials", part(3), part(1)]) == 0
    by_partials = capsys.readouterr().out
    assert by_partials.startswith(by_key) and by_partials[len(by_key):] == "partials: combine to a decryption (2 auditors, no key rebuilt)\n"
    # one of the two made for another set; both options at once; neither
    assert cli.main(["audit-partial", share(1), "--with", "2", ctj, pwf, "--pair-seeds", seedf(1), "--out", part(2)]) == 0
    assert cli.main(["audit-open", "-", proof, pwf, ctj, "--partials", part(3), part(2)]) == 2
    assert "one set" in capsys.readouterr().err
    for argv in (["--partials", part(3), "--shares", share(1)], []):
        with pytest.raises(SystemExit) as ex:
            cli.main(["audit-open", "-", proof, pwf, ctj] + argv)
        assert ex.value.code != 0
