"""GPU: the auditor-side kernels on inputs an adversary would send -- k_rlwe_decrypt (spp_rlwe_decrypt_batch), phase 1 of
k_audit_open (spp_audit_open_batch: range flag, LDS ciphertext, decryption, record tail) and both outputs of k_shamir_combine
(spp_shamir_reconstruct) -- bit-exact against the big-integer expectations of tests/auditor_vectors.py.  The same vectors are
held against the oracle and the g++ build of csrc/audit_open.hpp in tests/test_auditor_vectors_host.py."""
import ctypes

import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None

import auditor_vectors as V

pytestmark = pytest.mark.gpu

BAD_PROOF, BAD_CT, BAD_ID = 1, 2, 4
ZERO_PW = bytes(76)


@pytest.fixture(scope="module")
def ctx():
    import spp
    c = spp.Context(0)
    yield c
    c.close()


def _decrypt(ctx, sk, vectors):
    from spp import witness
    _, msg = witness.rlwe_decrypt(ctx, sk, [v["c0"] for v in vectors], [v["c1"] for v in vectors])
    return [m.tolist() for m in msg]


def _pw(wa, ct):
    return (2).to_bytes(4, "big") + (0).to_bytes(4, "big") + (2).to_bytes(4, "big") + wa.to_bytes(32, "big") + ct.to_bytes(32, "big")


# ------------------------------------------------------------------------------------------------------------ k_rlwe_decrypt
def test_decrypt_dialled_and_extreme_ciphertexts_in_one_call_per_key(ctx):
    """every slot on a rounding decision, and the largest sums the 64-bit accumulator is sized for: one call per key"""
    seen = 0
    for sk, group in V.by_key(V.dialled_vectors() + V.extreme_vectors()):
        got = _decrypt(ctx, sk, group)
        for v, m in zip(group, got):
            print(v["name"], "slots that differ:", [t for t in range(64) if m[t] != v["msg"][t]])
            assert m == v["msg"], v["name"]
            seen += 1
    assert seen == 16
    pool = V.dialled_pool()                                         # 129 blocks of the kernel under one key
    assert _decrypt(ctx, pool[0]["sk"], pool) == [v["msg"] for v in pool]


def test_decrypt_dialled_ciphertexts_one_per_call(ctx):
    for v in V.dialled_vectors():
        assert _decrypt(ctx, v["sk"], [v]) == [v["msg"]], v["name"]


def test_decrypt_refuses_a_coefficient_not_below_q(ctx):
    """spp_rlwe_decrypt_batch takes no coefficient >= q (k_rlwe_decrypt would load it raw into sums sized for 28 bits): refused
    before any device work, ciphertext and coefficient named, msg untouched.  spp_audit_open_batch is the call for such records."""
    import numpy as np
    import spp
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    sk = np.asarray(V.range_key(), dtype=np.uint32)
    recs = [V.clean_record(i) for i in range(3)]
    c0 = np.asarray([r[0] for r in recs], dtype=np.uint32)
    c1 = np.asarray([r[1] for r in recs], dtype=np.uint32)
    msg = np.full((3, 64), 0xAB, dtype=np.uint8)
    assert ctx.L.spp_rlwe_decrypt_batch(ctx.h, p(sk), 3, p(c0), p(c1), p(msg)) == 0
    assert msg.tolist() == [V.decrypt(V.range_key(), r[0], r[1]) for r in recs]
    for value in (V.Q, (1 << 32) - 1):
        for rec in (0, 2):
            for where, index in (("c0", 0), ("c0", 63), ("c1", 0), ("c1", 1023)):
                b0, b1 = c0.copy(), c1.copy()
                (b0 if where == "c0" else b1)[rec, index] = value
                msg[:] = 0xAB
                assert ctx.L.spp_rlwe_decrypt_batch(ctx.h, p(sk), 3, p(b0), p(b1), p(msg)) == -1, (value, rec, where, index)
                err = spp.last_error()
                assert "ciphertext %d:" % rec in err and "%s[%d] " % (where, index) in err and "[0, q)" in err, err
                assert (msg == 0xAB).all()
    b1 = c1.copy(); b1[1, 5] = V.Q; b1[2, 0] = V.Q                  # the first one in the order of the buffers is named
    assert ctx.L.spp_rlwe_decrypt_batch(ctx.h, p(sk), 3, p(c0), p(b1), p(msg)) == -1 and "ciphertext 1: c1[5] " in spp.last_error()
    assert ctx.L.spp_rlwe_decrypt_batch(ctx.h, p(sk), 0, p(c0), p(b1), p(msg)) == 0      # an empty batch reads nothing


# -------------------------------------------------------------------------------------------------------------- k_audit_open
def _open(ctx, sk, vectors, pws=None):
    return ctx.audit_open(None, sk, None, pws if pws is not None else [ZERO_PW] * len(vectors), [v["c0"] for v in vectors],
                          [v["c1"] for v in vectors])


def test_audit_open_on_the_same_vectors(ctx):
    """no verifying key, the zero public witness: the owners are the expected bytes decoded; bit 2 on every record (nothing
    hashes to the zero commitment), bit 4 with it (no owner hashes to zero either), bit 1 never"""
    for sk, group in V.by_key(V.dialled_vectors() + V.extreme_vectors()):
        owners, flags = _open(ctx, sk, group)
        for v, who, f in zip(group, owners, flags):
            assert who == V.decode_owner(v["msg"]), v["name"]
            assert f & BAD_CT and not f & BAD_PROOF and f == BAD_CT | BAD_ID, (v["name"], f)


@pytest.mark.parametrize("count,first", [(1, 7), (63, 1), (64, 64), (65, 30), (129, 0)])
def test_audit_open_batch_shapes(ctx, count, first):
    """The record tail of a block, lanes >= nrec, and the LDS ciphertext that one record after the other passes through: `count`
    distinct dialled ciphertexts (the pool from `first` on, cyclically), so a record that read its neighbour's would show."""
    pool = V.dialled_pool()
    batch = [pool[(first + i) % len(pool)] for i in range(count)]
    owners, flags = _open(ctx, batch[0]["sk"], batch)
    assert len(owners) == count == len(flags)
    want = [V.decode_owner(v["msg"]) for v in batch]
    assert len(set(want)) == count
    print("records that differ:", [i for i in range(count) if owners[i] != want[i]])
    assert owners == want
    assert all(f & BAD_CT and not f & BAD_PROOF for f in flags) and flags == [BAD_CT | BAD_ID] * count


@pytest.fixture(scope="module")
def range_batch():
    """the out-of-range batch and its twin without the injections, each record with the public witness of its residues: the
    oracle's sponge as ct_commitment and a zero wa_commitment, so bit 2 hangs on the range flag alone"""
    from oracle import rlwe, hashes as H
    clean, injected, bad = V.out_of_range_batch()
    sponge = lambda c0, c1: H.poseidon2_sponge(rlwe.pack_values([x % V.Q for x in c0]) + rlwe.pack_values([x % V.Q for x in c1]))
    pw_clean = [_pw(0, sponge(c0, c1)) for c0, c1, _ in clean]
    pw_inj = [_pw(0, sponge(*injected[i][:2])) if i in bad else pw_clean[i] for i in range(len(clean))]
    assert all(pw_inj[i] != pw_clean[i] for i in bad)
    return dict(clean=clean, injected=injected, bad=bad, pw_clean=pw_clean, pw_inj=pw_inj)


def test_out_of_range_coefficients_flag_their_own_record(ctx, range_batch):
    """One coefficient >= q at c0[0], c0[63], each component of the first and of the last uint4 of c1, and the last word of the
    wave's first round of loads and the first of its second (c1[255], c1[256]), in records of both blocks: the flag finds it
    wherever it is, stays with its record, and the record is decrypted as its residues."""
    rb = range_batch
    sk = V.range_key()
    as_vectors = lambda recs: [dict(c0=c0, c1=c1) for c0, c1, _ in recs]
    owners, flags = _open(ctx, sk, as_vectors(rb["injected"]), rb["pw_inj"])
    print("flags:", flags)
    assert [i for i, f in enumerate(flags) if f & BAD_CT] == rb["bad"]
    assert owners == [V.decode_owner(m) for _, _, m in rb["injected"]]
    assert not any(f & BAD_PROOF for f in flags)
    owners0, flags0 = _open(ctx, sk, as_vectors(rb["clean"]), rb["pw_clean"])
    assert not any(f & BAD_CT for f in flags0) and owners0 == [V.decode_owner(m) for _, _, m in rb["clean"]]
    assert [f for i, f in enumerate(flags) if i not in rb["bad"]] == [f for i, f in enumerate(flags0) if i not in rb["bad"]]
    # no random owner is a point whose hash is zero
    assert flags0 == [BAD_ID] * len(flags0) and [flags[i] for i in rb["bad"]] == [BAD_CT | BAD_ID] * len(rb["bad"])


def test_every_out_of_range_value_at_every_position(ctx):
    """q, q + 1, 2 q - 1 and 2^32 - 1 at each listed position, 48 records in one call: decrypted as the residues"""
    vs = V.out_of_range_vectors()
    owners, flags = _open(ctx, V.range_key(), vs)
    for v, who, f in zip(vs, owners, flags):
        assert who == V.decode_owner(v["msg"]) and f & BAD_CT and not f & BAD_PROOF, v["name"]


# ---------------------------------------------------------------------------------------------------------- k_shamir_combine
@pytest.mark.parametrize("t,n", V.shamir_shapes())
def test_shamir_reconstruct_secrets_and_centred_key(ctx, t, n):
    """both outputs in one call and each alone: secret_be is the secret, sk_mod_q its centred value mod q -- for secrets on
    both sides of (r - 1) / 2, around q and r - q, and with high limbs set, where the limb-wise reduction does the work"""
    c = V.shamir_case(t, n)
    xs = (ctypes.c_uint32 * t)(*c["xs"])
    ys = b"".join(y.to_bytes(32, "big") for row in c["ys"] for y in row)
    want_secret = b"".join(s.to_bytes(32, "big") for s in c["secrets"])
    for with_secret, with_sk in ((True, True), (True, False), (False, True)):
        secret = ctypes.create_string_buffer(32 * n) if with_secret else None
        sk = (ctypes.c_uint32 * n)(*([0xFFFFFFFF] * n)) if with_sk else None
        rc = ctx.L.spp_shamir_reconstruct(ctx.h, t, ctypes.cast(xs, ctypes.c_void_p), ys, n,
                                          ctypes.cast(secret, ctypes.c_void_p) if with_secret else None,
                                          ctypes.cast(sk, ctypes.c_void_p) if with_sk else None)
        assert rc == 0
        if with_secret:
            assert secret.raw == want_secret, (with_secret, with_sk)
        if with_sk:
            got = list(sk)
            print("values that differ:", [(i, hex(c["secrets"][i])) for i in range(n) if got[i] != c["sk_mod_q"][i]][:8])
            assert got == c["sk_mod_q"], (with_secret, with_sk)
