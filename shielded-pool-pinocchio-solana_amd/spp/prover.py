"""Thin object layer over the C ABI: Context (one GPU), CircuitHandle (R1CS + pk + tables in HBM)."""
import ctypes
import numpy as np
from . import lib
from .lib import load_library, check, SppError, PROOF_LEN, SPP_ERR_UNSAT, AUDIT_PW_LEN, SPP_AUDIT_RESIDENT, SPP_TREE_SIZE_NOW


def build_circuit(circuit_id, out_path, aux=None):
    """`sunspot compile` equivalent (host only): writes the SPPC container, returns nbConstraints."""
    L = load_library()
    n = ctypes.c_uint32(0)
    auxbuf = None
    if aux is not None:
        auxbuf = (ctypes.c_uint32 * len(aux))(*[int(v) for v in aux])
    check(L.spp_circuit_build(int(circuit_id), auxbuf, out_path.encode(), ctypes.byref(n)))
    return n.value


def verify(vk_bytes, proof_bytes, pw_bytes):
    """`sunspot verify vk proof pw`: True / False; raises SppError on malformed inputs. Host only (no GPU)."""
    L = load_library()
    ok = ctypes.c_int(0)
    check(L.spp_verify(vk_bytes, len(vk_bytes), proof_bytes, len(proof_bytes), pw_bytes, len(pw_bytes), ctypes.byref(ok)))
    return bool(ok.value)


def pairing_check_host(pairs):
    """prod e(P, Q) == 1 with the product's host pairing (no GPU). pairs: list of (g1 64 B, g2 128 B)."""
    L = load_library()
    ok = ctypes.c_int(0)
    check(L.spp_pairing_check_host(len(pairs), b"".join(p for p, _ in pairs), b"".join(q for _, q in pairs), ctypes.byref(ok)))
    return bool(ok.value)


class Context:
    def __init__(self, device=0):
        self.L = load_library()
        h = ctypes.c_void_p()
        check(self.L.spp_init(int(device), ctypes.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            self.L.spp_free_ctx(self.h)
            self.h = None

    def setup(self, circuit_path, seed32, pk_path, vk_path):
        assert len(seed32) == 32
        check(self.L.spp_setup(self.h, circuit_path.encode(), bytes(seed32), pk_path.encode(), vk_path.encode()))

    def setup_contribute(self, pk_in, vk_in, pk_out, vk_out, entropy=None):
        """One contribution to the delta of a proving key (spp_setup_contribute): writes pk_out / vk_out, returns the 160-byte
        receipt.  entropy: 32 bytes, or None for the operating system's randomness (what every real contribution uses)."""
        assert entropy is None or len(entropy) == 32
        receipt = ctypes.create_string_buffer(lib.SPP_CONTRIB_RECEIPT_LEN)
        check(self.L.spp_setup_contribute(self.h, pk_in.encode(), vk_in.encode(), None if entropy is None else bytes(entropy),
                                          pk_out.encode(), vk_out.encode(), ctypes.cast(receipt, ctypes.c_void_p)))
        return receipt.raw

    def setup_verify_contribution(self, pk_before, vk_before, pk_after, vk_after, receipt):
        """One link of a ceremony chain (spp_setup_verify_contribution): (accepted, reason) with reason one of lib.SPP_CONTRIB_*
        (0 when accepted; lib.CONTRIB_REASON_NAMES has the names).  A refusal is a result, not an SppError."""
        assert len(receipt) == lib.SPP_CONTRIB_RECEIPT_LEN
        ok, reason = ctypes.c_int(0), ctypes.c_uint32(0)
        check(self.L.spp_setup_verify_contribution(self.h, pk_before.encode(), vk_before.encode(), pk_after.encode(), vk_after.encode(),
                                                   bytes(receipt), ctypes.byref(ok), ctypes.byref(reason)))
        return bool(ok.value), reason.value

    def setup_contribute_sigma(self, pk_in, vk_in, pk_out, vk_out, entropy=None):
        """One contribution to the sigma of a key's commitment (spp_setup_contribute_sigma): writes pk_out / vk_out, returns the
        160-byte receipt.  entropy as in setup_contribute."""
        assert entropy is None or len(entropy) == 32
        receipt = ctypes.create_string_buffer(lib.SPP_CONTRIB_RECEIPT_LEN)
        check(self.L.spp_setup_contribute_sigma(self.h, pk_in.encode(), vk_in.encode(), None if entropy is None else bytes(entropy),
                                                pk_out.encode(), vk_out.encode(), ctypes.cast(receipt, ctypes.c_void_p)))
        return receipt.raw

    def setup_verify_sigma_contribution(self, pk_before, vk_before, pk_after, vk_after, receipt):
        """One sigma link (spp_setup_verify_sigma_contribution): (accepted, reason) with reason one of lib.SPP_SIGMA_*
        (lib.SIGMA_REASON_NAMES has the names).  A refusal is a result, not an SppError."""
        assert len(receipt) == lib.SPP_CONTRIB_RECEIPT_LEN
        ok, reason = ctypes.c_int(0), ctypes.c_uint32(0)
        check(self.L.spp_setup_verify_sigma_contribution(self.h, pk_before.encode(), vk_before.encode(), pk_after.encode(),
                                                         vk_after.encode(), bytes(receipt), ctypes.byref(ok), ctypes.byref(reason)))
        return bool(ok.value), reason.value

    def ptau_new(self, domain_log, path):
        """The transcript of tau = alpha = beta = 1 for domains up to 2^domain_log (spp_ptau_new; host only)."""
        check(self.L.spp_ptau_new(int(domain_log), path.encode()))

    def ptau_contribute(self, in_path, out_path, entropy=None):
        """One contribution to a powers-of-tau transcript (spp_ptau_contribute): writes out_path, returns the 480-byte receipt.
        entropy: 32 bytes, or None for the operating system's randomness (what every real contribution uses)."""
        assert entropy is None or len(entropy) == 32
        receipt = ctypes.create_string_buffer(lib.SPP_PTAU_RECEIPT_LEN)
        check(self.L.spp_ptau_contribute(self.h, in_path.encode(), None if entropy is None else bytes(entropy), out_path.encode(),
                                         ctypes.cast(receipt, ctypes.c_void_p)))
        return receipt.raw

    def ptau_verify_contribution(self, before_path, after_path, receipt):
        """One link of a transcript chain (spp_ptau_verify_contribution): (accepted, reason) with reason one of lib.SPP_PTAU_*
        (0 when accepted; lib.PTAU_REASON_NAMES has the names).  A refusal is a result, not an SppError."""
        assert len(receipt) == lib.SPP_PTAU_RECEIPT_LEN
        ok, reason = ctypes.c_int(0), ctypes.c_uint32(0)
        check(self.L.spp_ptau_verify_contribution(self.h, before_path.encode(), after_path.encode(), bytes(receipt), ctypes.byref(ok),
                                                  ctypes.byref(reason)))
        return bool(ok.value), reason.value

    def _mul_each(self, call, size, points_bytes, scalars):
        n = len(scalars)
        assert len(points_bytes) == size * n
        out = ctypes.create_string_buffer(max(size * n, 1))
        sc = b"".join(int(s).to_bytes(32, "big") for s in scalars)
        check(call(self.h, points_bytes, n, sc, ctypes.cast(out, ctypes.c_void_p)))
        return out.raw[:size * n]

    def g1_mul_each(self, points_bytes, scalars):
        """scalars[i] * P_i for every 64-byte point of points_bytes (spp_g1_mul_each): the transcript's kernel on its own."""
        return self._mul_each(self.L.spp_g1_mul_each, 64, points_bytes, scalars)

    def g2_mul_each(self, points_bytes, scalars):
        """The same over 128-byte G2 points (spp_g2_mul_each)."""
        return self._mul_each(self.L.spp_g2_mul_each, 128, points_bytes, scalars)

    def setup_from_ptau(self, circuit_path, ptau_path, pk_path, vk_path):
        """A circuit's proving and verifying key from a powers-of-tau transcript (spp_setup_from_ptau): no secret, gamma = delta =
        sigma = rho = 1; the delta contributions (setup_contribute) come after it."""
        check(self.L.spp_setup_from_ptau(self.h, circuit_path.encode(), ptau_path.encode(), pk_path.encode(), vk_path.encode()))

    def _ec_intt(self, call, size, points_bytes, logn):
        n = 1 << logn
        assert len(points_bytes) == size * n
        out = ctypes.create_string_buffer(size * n)
        check(call(self.h, points_bytes, int(logn), ctypes.cast(out, ctypes.c_void_p)))
        return out.raw

    def ec_intt_g1(self, points_bytes, logn):
        """out[k] = (1 / n) sum_i w^(-k i) P_i over 2^logn 64-byte points (spp_ec_intt_g1): monomial powers to Lagrange points."""
        return self._ec_intt(self.L.spp_ec_intt_g1, 64, points_bytes, logn)

    def ec_intt_g2(self, points_bytes, logn):
        """The same over 128-byte G2 points (spp_ec_intt_g2)."""
        return self._ec_intt(self.L.spp_ec_intt_g2, 128, points_bytes, logn)

    def ec_intt_timed(self, group, points_bytes, logn, host_butterflies=0):
        """(outputs, ms of the stages, ms of the scaling, ms of one host thread over host_butterflies butterflies); group 1 or 2"""
        size = 64 if group == 1 else 128
        assert len(points_bytes) == size << logn
        out = ctypes.create_string_buffer(size << logn)
        ms, host_ms = (ctypes.c_float * 2)(), ctypes.c_float(0)
        check(self.L.spp_ec_intt_timed(self.h, int(group), points_bytes, int(logn), ctypes.cast(out, ctypes.c_void_p), ms,
                                       int(host_butterflies), ctypes.byref(host_ms)))
        return out.raw, ms[0], ms[1], host_ms.value

    def g1_scale_points(self, points_bytes, scalar):
        """scalar * P for every 64-byte point of points_bytes (spp_g1_scale_points): the ceremony's kernel on its own."""
        n = len(points_bytes) // 64
        assert len(points_bytes) == 64 * n
        out = ctypes.create_string_buffer(max(64 * n, 1))
        check(self.L.spp_g1_scale_points(self.h, points_bytes, n, int(scalar).to_bytes(32, "big"), ctypes.cast(out, ctypes.c_void_p)))
        return out.raw[:64 * n]

    def g1_scale_points_timed(self, points_bytes, scalar, host_points=0):
        """(scaled points, ms of the kernel alone, ms of one host thread over the first host_points points)"""
        n = len(points_bytes) // 64
        out = ctypes.create_string_buffer(max(64 * n, 1))
        kernel_ms, host_ms = ctypes.c_float(0), ctypes.c_float(0)
        check(self.L.spp_g1_scale_points_timed(self.h, points_bytes, n, int(scalar).to_bytes(32, "big"), ctypes.cast(out, ctypes.c_void_p),
                                               ctypes.byref(kernel_ms), int(host_points), ctypes.byref(host_ms)))
        return out.raw[:64 * n], kernel_ms.value, host_ms.value

    def load_circuit(self, circuit_path, pk_path, window_bits=0, bits=None):
        """bits: 7 planned window sizes (plan_windows) instead of window_bits / a budget of this circuit's own."""
        return CircuitHandle(self, circuit_path, pk_path, window_bits, bits)

    def plan_windows(self, pk_paths, budget_bytes=240e9):
        """Window bits for circuits that are to be resident TOGETHER: one greedy split of the budget over the union of their MSM
        sets (spp_plan_windows).  Returns one list of 7 per proving key, in the order of CircuitHandle.msm_sizes()."""
        n = len(pk_paths)
        sizes = (ctypes.c_uint32 * (7 * n))()
        for k, path in enumerate(pk_paths):
            one = (ctypes.c_uint32 * 7)()
            check(self.L.spp_pk_msm_sizes(path.encode(), one))
            sizes[7 * k:7 * k + 7] = list(one)
        bits = (ctypes.c_uint32 * (7 * n))()
        check(self.L.spp_plan_windows(n, sizes, float(budget_bytes), bits))
        return [list(bits[7 * k:7 * k + 7]) for k in range(n)]

    def ntt(self, values, inverse=False):
        """values: list of ints (len 2^k) -> list of ints, natural order."""
        n = len(values)
        logn = n.bit_length() - 1
        assert 1 << logn == n
        buf = ctypes.create_string_buffer(b"".join(int(v).to_bytes(32, "big") for v in values), 32 * n)
        check(self.L.spp_ntt_fr(self.h, ctypes.cast(buf, ctypes.c_void_p), logn, 1 if inverse else 0))
        raw = buf.raw                                   # one copy: buf.raw per element is quadratic in n
        return [int.from_bytes(raw[32 * i:32 * i + 32], "big") for i in range(n)]

    def debug_arith(self, selector, rows, out_words, arg=0):
        """Test only (spp_debug_arith): one function of csrc/bn254.hpp / f29.hpp / gnark_hints.hpp on the device, on RAW uint32 limbs.  rows: n cases of
        operand words (n x in_words, anything numpy turns into uint32) -> n x out_words uint32 array; nothing is converted,
        reduced or checked on either side.  selector = SPP_ARITH_FR / SPP_ARITH_FQ | operation code of csrc/arith_probe.hpp."""
        a = np.ascontiguousarray(rows, dtype=np.uint32)
        assert a.ndim == 2
        out = np.empty((a.shape[0], int(out_words)), dtype=np.uint32)
        check(self.L.spp_debug_arith(self.h, int(selector), int(arg), a.shape[0], a.ctypes.data_as(ctypes.c_void_p), a.shape[1],
                                     out.ctypes.data_as(ctypes.c_void_p), out.shape[1]))
        return out

    def msm_g1(self, bases_bytes, scalars, window_bits=8):
        n = len(scalars)
        out = ctypes.create_string_buffer(64)
        sc = b"".join(int(s).to_bytes(32, "big") for s in scalars)
        check(self.L.spp_msm_g1(self.h, bases_bytes, sc, n, int(window_bits), ctypes.cast(out, ctypes.c_void_p)))
        return out.raw

    def msm_g2(self, bases_bytes, scalars, window_bits=8):
        out = ctypes.create_string_buffer(128)
        sc = b"".join(int(s).to_bytes(32, "big") for s in scalars)
        check(self.L.spp_msm_g2(self.h, bases_bytes, sc, len(scalars), int(window_bits), ctypes.cast(out, ctypes.c_void_p)))
        return out.raw

    def msm_flat(self, group, bases_bytes, scalar_rows, window_bits=8):
        """The flat table walk of the proving sets over caller-supplied bases (spp_msm_flat_unit): group 1 = G1, 2 = G2;
        scalar_rows = P lists of n ints.  Returns (list of P points as raw bytes, lanes summed again by the redo kernel)."""
        size = 64 if group == 1 else 128
        n = len(scalar_rows[0])
        assert all(len(r) == n for r in scalar_rows) and len(bases_bytes) == size * n
        out = ctypes.create_string_buffer(size * len(scalar_rows))
        sc = b"".join(int(s).to_bytes(32, "big") for r in scalar_rows for s in r)
        redo = ctypes.c_uint32(0)
        check(self.L.spp_msm_flat_unit(self.h, int(group), bases_bytes, n, sc, len(scalar_rows), int(window_bits),
                                       ctypes.cast(out, ctypes.c_void_p), ctypes.byref(redo)))
        return [out.raw[size * p:size * (p + 1)] for p in range(len(scalar_rows))], redo.value

    def debug_msm_digits(self, scalar_rows, rows, window_bits):
        """Test only (spp_debug_msm_digits): the signed-digit planes of the table walks, nothing summed.  scalar_rows = M lists of P
        ints (scalar row m, proof p); rows = N indices < M.  Returns (int16 array W x N x Pp, Pp): digit j of (base i, proof p) at
        [j][i][p]; entries with p >= P are unspecified."""
        M, P, N = len(scalar_rows), len(scalar_rows[0]), len(rows)
        assert all(len(r) == P for r in scalar_rows)
        W = (254 + int(window_bits) - 1) // int(window_bits)
        sc = b"".join(int(s).to_bytes(32, "big") for r in scalar_rows for s in r)
        idx = np.ascontiguousarray(rows, dtype=np.uint32)
        buf = np.zeros(W * N * ((P + 63) // 64 * 64), dtype=np.int16)
        pp = ctypes.c_uint32(0)
        check(self.L.spp_debug_msm_digits(self.h, sc, M, P, idx.ctypes.data_as(ctypes.c_void_p), N, int(window_bits),
                                          buf.ctypes.data_as(ctypes.c_void_p), buf.size, ctypes.byref(pp)))
        return buf[:W * N * pp.value].reshape(W, N, pp.value), pp.value

    def msm_g1_pippenger(self, bases_bytes, scalars):
        out = ctypes.create_string_buffer(64)
        sc = b"".join(int(s).to_bytes(32, "big") for s in scalars)
        check(self.L.spp_msm_g1_pippenger(self.h, bases_bytes, sc, len(scalars), ctypes.cast(out, ctypes.c_void_p)))
        return out.raw

    def msm_g2_pippenger(self, bases_bytes, scalars):
        out = ctypes.create_string_buffer(128)
        sc = b"".join(int(s).to_bytes(32, "big") for s in scalars)
        check(self.L.spp_msm_g2_pippenger(self.h, bases_bytes, sc, len(scalars), ctypes.cast(out, ctypes.c_void_p)))
        return out.raw

    def pairing_check(self, pairs):
        """prod e(P, Q) == 1 on the GPU with the batched verifier's device pairing code (spp_pairing_check)."""
        ok = ctypes.c_int(0)
        check(self.L.spp_pairing_check(self.h, len(pairs), b"".join(p for p, _ in pairs), b"".join(q for _, q in pairs), ctypes.byref(ok)))
        return bool(ok.value)

    def verify_batch(self, vk, proofs, pws, want_ms=False):
        """`sunspot verify` for many proofs against one key, on the GPU (spp_verify_batch). proofs / pws: lists of bytes.
        Returns a list of booleans (and the kernel time in ms when want_ms)."""
        count = len(proofs)
        assert count == len(pws)
        pw_len = len(pws[0]) if count else 12
        ok = (ctypes.c_int32 * max(count, 1))()
        ms = ctypes.c_float(0)
        check(self.L.spp_verify_batch(self.h, vk, len(vk), count, b"".join(proofs), b"".join(pws), pw_len,
                                      ctypes.cast(ok, ctypes.c_void_p), ctypes.byref(ms)))
        res = [bool(ok[i]) for i in range(count)]
        return (res, ms.value) if want_ms else res

    def verify_batch_rlc(self, vk, proofs, pws, seed=None, group=0, flags=0, want_stats=False, want_ms=False):
        """verify_batch by random linear combination (spp_verify_batch_rlc): the key-side pairings and the final exponentiation
        once per group of `group` proofs (0: the default), a refused group settled proof by proof.  Same verdicts as verify_batch
        except with probability ~2^-127 per call, PROVIDED the prover cannot know or influence `seed`: leave it None (32 bytes
        from the OS per call) or draw it after the batch is fixed.  flags: lib.SPP_RLC_*.  Returns a list of booleans, then
        (groups, groups refused, proofs re-verified, proofs dropped) when want_stats, then the kernel time in ms when want_ms."""
        count = len(proofs)
        assert count == len(pws)
        if seed is not None and len(seed) != 32:
            raise ValueError("seed must be 32 bytes")
        pw_len = len(pws[0]) if count else 12
        ok = (ctypes.c_int32 * max(count, 1))()
        stats = (ctypes.c_uint32 * 4)()
        ms = ctypes.c_float(0)
        check(self.L.spp_verify_batch_rlc(self.h, vk, len(vk), count, b"".join(proofs), b"".join(pws), pw_len,
                                          None if seed is None else bytes(seed), group, flags, ctypes.cast(ok, ctypes.c_void_p), stats,
                                          ctypes.byref(ms)))
        res = [bool(ok[i]) for i in range(count)]
        if not (want_stats or want_ms):
            return res
        return (res,) + ((tuple(stats),) if want_stats else ()) + ((ms.value,) if want_ms else ())

    def audit_open(self, vk, sk_mod_q, proofs, pws, c0, c1, rlc=False, group=0, want_stats=False, partials=None):
        """Opens audit records in one pass on the GPU (spp_audit_open_batch): verification, ciphertext binding, decryption,
        identity binding.  rlc: verify by random linear combination (spp_audit_open_batch_rlc; groups of `group`, 0 = 256, a fresh
        seed from the OS) -- the same flags except with probability ~2^-127 per call; want_stats (with rlc): a third result,
        (groups, groups refused, proofs re-verified, proofs dropped).  vk: bytes, or None for records already verified elsewhere (proofs may then be None); sk_mod_q: 1024
        ints (witness.reconstruct_sk); proofs / pws: lists of bytes (or one bytes object each); c0 [count, 64], c1 [count, 1024].
        partials: the threshold form (spp_audit_open_batch_partials) -- sk_mod_q is then None and partials holds the results of
        witness.rlwe_partial_decrypt of the t auditors of one set on these ciphertexts, [t, count, 64, 32]; nobody holds the key,
        and SPP_AUDIT_BAD_PARTIALS (8) joins the flags.  Not with rlc.
        Returns (owners, flags): owners[i] = (owner_x, owner_y) as decrypted, flags[i] = SPP_AUDIT_* bits, 0 = all three hold."""
        c0 = np.ascontiguousarray(c0, dtype=np.uint32).reshape(-1, 64)
        count = c0.shape[0]
        c1 = np.ascontiguousarray(c1, dtype=np.uint32).reshape(count, 1024)
        if (partials is None) == (sk_mod_q is None):
            raise ValueError("audit_open: exactly one of sk_mod_q and partials")
        if partials is not None:
            if rlc:
                raise ValueError("audit_open: partials do not go with rlc=True")
            from .witness import _partials_array
            parts = _partials_array(partials, count) if count else np.zeros((max(len(partials), 1), 0, 64, 32), dtype=np.uint8)
        else:
            sk = np.ascontiguousarray(sk_mod_q, dtype=np.uint32)
            if sk.shape != (1024,):
                raise ValueError("sk_mod_q must hold 1024 coefficients")
        join = lambda v: None if v is None else (bytes(v) if isinstance(v, (bytes, bytearray)) else b"".join(v))
        pb, wb = join(proofs), join(pws)
        if wb is None or len(wb) != AUDIT_PW_LEN * count or (pb is not None and len(pb) != PROOF_LEN * count):
            raise ValueError("audit_open: %d ciphertexts need %d public witnesses of %d bytes (and as many proofs of %d)"
                             % (count, count, AUDIT_PW_LEN, PROOF_LEN))
        owners = np.zeros((max(count, 1), 64), dtype=np.uint8)
        flags = np.zeros(max(count, 1), dtype=np.uint32)
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        stats = (ctypes.c_uint32 * 4)()
        if rlc:
            check(self.L.spp_audit_open_batch_rlc(self.h, vk, len(vk) if vk is not None else 0, p(sk), count, pb, wb, p(c0), p(c1), int(group),
                                                  p(owners), p(flags), stats))
        else:
            if group or want_stats:
                raise ValueError("audit_open: group and want_stats go with rlc=True")
            if partials is not None:
                check(self.L.spp_audit_open_batch_partials(self.h, vk, len(vk) if vk is not None else 0, parts.shape[0], parts.tobytes(), count,
                                                           pb, wb, p(c0), p(c1), p(owners), p(flags)))
            else:
                check(self.L.spp_audit_open_batch(self.h, vk, len(vk) if vk is not None else 0, p(sk), count, pb, wb, p(c0), p(c1), p(owners), p(flags)))
        res = ([(int.from_bytes(owners[i, :32].tobytes(), "big"), int.from_bytes(owners[i, 32:].tobytes(), "big")) for i in range(count)],
               [int(f) for f in flags[:count]])
        return res + (tuple(int(v) for v in stats),) if want_stats else res

    def withdrawal_audit_plan(self, keys, pool=None):
        """Which notes of a batch still need an audit record (spp_withdrawal_audit_plan).  keys: one wa_commitment per note, ints
        or 32-byte strings compared bytewise (word 2 of ShieldedPoolMerkleTree.sync's records); pool: a Pool of this Context whose
        audit-record set is consulted and not changed.  Returns (audit_of, audit_note): audit_note the ascending list of the notes
        that are the first of an identity the pool does not hold, audit_of[i] the position of note i's identity in it, or
        SPP_AUDIT_RESIDENT."""
        buf = b"".join(int(k).to_bytes(32, "big") if isinstance(k, int) else bytes(k) for k in keys)
        if len(buf) % 32:
            raise ValueError("a key is 32 bytes")
        count = len(buf) // 32
        audit_of = (ctypes.c_uint32 * max(count, 1))()
        audit_note = (ctypes.c_uint32 * max(count, 1))()
        n = ctypes.c_uint32(0)
        check(self.L.spp_withdrawal_audit_plan(self.h, None if pool is None else pool.h, count, buf, ctypes.cast(audit_of, ctypes.c_void_p),
                                               ctypes.cast(audit_note, ctypes.c_void_p), ctypes.byref(n)))
        return list(audit_of)[:count], list(audit_note)[:n.value]

    def msm_g1_pippenger_bench(self, n, seed=5, scale=None, iters=1, small_permille=0):
        """Returns (result bytes, ms per MSM, ms of the bucket kernel). small_permille: share of byte-sized scalars."""
        out = ctypes.create_string_buffer(64)
        t, k = ctypes.c_float(0), ctypes.c_float(0)
        sb = None if scale is None else int(scale).to_bytes(32, "big")
        check(self.L.spp_msm_g1_pippenger_bench_dist(self.h, n, seed, int(small_permille), sb, iters, ctypes.cast(out, ctypes.c_void_p),
                                                     ctypes.byref(t), ctypes.byref(k)))
        return out.raw, t.value, k.value


    def msm_g1_pippenger_bench_shard(self, n_total, first, count, seed=5, scale=None, iters=1, small_permille=0):
        """The partial sum of points [first, first + count) of the n_total-point synthetic MSM (one rank's share): (bytes, ms, bucket ms)."""
        out = ctypes.create_string_buffer(64)
        t, k = ctypes.c_float(0), ctypes.c_float(0)
        sb = None if scale is None else int(scale).to_bytes(32, "big")
        check(self.L.spp_msm_g1_pippenger_bench_shard(self.h, n_total, first, count, seed, int(small_permille), sb, iters,
                                                      ctypes.cast(out, ctypes.c_void_p), ctypes.byref(t), ctypes.byref(k)))
        return out.raw, t.value, k.value


class CircuitHandle:
    def __init__(self, ctx, circuit_path, pk_path, window_bits=0, bits=None):
        self.ctx = ctx
        self.L = ctx.L
        h = ctypes.c_void_p()
        if bits is not None:
            arr = (ctypes.c_uint32 * 7)(*[int(b) for b in bits])
            check(self.L.spp_load_circuit_with_windows(ctx.h, circuit_path.encode(), pk_path.encode(), arr, ctypes.byref(h)))
        else:
            check(self.L.spp_load_circuit(ctx.h, circuit_path.encode(), pk_path.encode(), int(window_bits), ctypes.byref(h)))
        self.h = h
        info = (ctypes.c_uint32 * 8)()
        check(self.L.spp_circuit_info(self.h, info))
        (self.circuit_id, self.n_public, self.n_secret, self.n_wires, self.n_constraints, self.domain_log,
         self.n_inputs, self.window_bits) = list(info)
        self.pw_len = 12 + 32 * self.n_public

    def close(self):
        if self.h:
            self.L.spp_free_circuit(self.h)
            self.h = None

    def msm_sizes(self):
        s = (ctypes.c_uint32 * 7)()
        check(self.L.spp_circuit_msm_sizes(self.h, s))
        return list(s)

    def msm_windows(self):
        s = (ctypes.c_uint32 * 7)()
        check(self.L.spp_circuit_msm_windows(self.h, s))
        return list(s)

    def small_rows(self):
        """(rows of the matrix evaluation summed as integers, byte-ranged wires they read) -- spp_circuit_small_rows"""
        s = (ctypes.c_uint32 * 2)()
        check(self.L.spp_circuit_small_rows(self.h, s))
        return list(s)

    def lookup_buckets(self):
        """(lookup-inverse wires summed by byte bucket, smallest batch that does so) -- spp_circuit_lookup_buckets"""
        s = (ctypes.c_uint32 * 2)()
        check(self.L.spp_circuit_lookup_buckets(self.h, s))
        return list(s)

    PLAN_STATS = ("n_runs", "max_row_terms", "sm_nrows", "sm_nslots", "lg_n", "items_seq", "items_par", "items_levels",
                  "items_level_stream", "stream_chunks", "tracks", "max_wide_div", "wide_steps", "wide_divs", "generic_rows", "generic_divs")

    def plan_stats(self):
        """what the load-time planners made of the circuit, by name (spp_circuit_plan_stats in include/spp.h)"""
        s = (ctypes.c_uint32 * 16)()
        check(self.L.spp_circuit_plan_stats(self.h, s))
        return dict(zip(self.PLAN_STATS, list(s)))

    def msm_table_rows(self):
        """table rows per base and set: 1 = single-row tables walked once per window (window_bits = 0)"""
        s = (ctypes.c_uint32 * 7)()
        check(self.L.spp_circuit_msm_table_rows(self.h, s))
        return list(s)

    @property
    def table_bytes(self):
        return int(self.L.spp_circuit_table_bytes(self.h))

    def prove_batch(self, inputs, rs=None):
        """inputs: list (per proof) of lists of ints; rs: list of (r, s) ints or None (OS randomness).
        Returns (proofs, pws, status) with status[i] == 0 or SPP_ERR_UNSAT."""
        count = len(inputs)
        buf = b"".join(int(v).to_bytes(32, "big") for row in inputs for v in row)
        assert len(buf) == count * self.n_inputs * 32
        rsb = None
        if rs is not None:
            rsb = b"".join(int(r).to_bytes(32, "big") + int(s).to_bytes(32, "big") for r, s in rs)
        proofs = ctypes.create_string_buffer(PROOF_LEN * count)
        pws = ctypes.create_string_buffer(self.pw_len * count)
        status = (ctypes.c_int32 * count)()
        rc = self.L.spp_prove_batch(self.h, count, buf, rsb, ctypes.cast(proofs, ctypes.c_void_p),
                                    ctypes.cast(pws, ctypes.c_void_p), ctypes.cast(status, ctypes.c_void_p))
        if rc != 0 and rc != SPP_ERR_UNSAT:
            check(rc)
        return ([proofs.raw[PROOF_LEN * i:PROOF_LEN * (i + 1)] for i in range(count)],
                [pws.raw[self.pw_len * i:self.pw_len * (i + 1)] for i in range(count)], list(status))

    def commitment_challenge(self, inputs):
        """The commitment challenge the prover derives for each (possibly partial) input row: spp_commitment_challenge."""
        if isinstance(inputs, (bytes, bytearray)):      # rows already serialised: n_inputs x 32 B big-endian each
            buf = bytes(inputs)
            count = len(buf) // (self.n_inputs * 32)
        else:
            count = len(inputs)
            buf = b"".join(int(v).to_bytes(32, "big") for row in inputs for v in row)
        assert len(buf) == count * self.n_inputs * 32
        out = ctypes.create_string_buffer(32 * count)
        check(self.L.spp_commitment_challenge(self.h, count, buf, ctypes.cast(out, ctypes.c_void_p)))
        return [int.from_bytes(out.raw[32 * i:32 * i + 32], "big") for i in range(count)]

    def prove_batch_device(self, count, d_inputs, d_rs, d_proofs, d_pws, d_status):
        """All arguments are raw device pointers (ints), e.g. torch tensors' data_ptr()."""
        check(self.L.spp_prove_batch_device(self.h, count, d_inputs, d_rs, d_proofs, d_pws, d_status))

    def prove_audit_from_secrets_device(self, count, d_pk_a, d_pk_b, d_sk, d_r, d_e1, d_e2, d_rs, d_proofs, d_pws, d_status):
        """Audit proofs from (secret_key, r, e1, e2) resident on the device (spp_prove_audit_from_secrets_device): the input pipeline of
        scripts/generate_audit.py:468-641 runs on the proving stream in front of the solver.  Raw device pointers (ints)."""
        check(self.L.spp_prove_audit_from_secrets_device(self.h, count, d_pk_a, d_pk_b, d_sk, d_r, d_e1, d_e2, d_rs, d_proofs, d_pws, d_status))

    def prove_audit_records_device(self, count, d_pk_a, d_pk_b, d_sk, d_r, d_e1, d_e2, d_rs, d_proofs, d_pws, d_status, d_c0, d_c1):
        """prove_audit_from_secrets_device plus the ciphertext each proof commits to (spp_prove_audit_records_device): d_c0
        count*64 u32, d_c1 count*1024 u32, written on the batch's proving stream.  Raw device pointers (ints)."""
        check(self.L.spp_prove_audit_records_device(self.h, count, d_pk_a, d_pk_b, d_sk, d_r, d_e1, d_e2, d_rs, d_proofs, d_pws, d_status,
                                                    d_c0, d_c1))

    def prove_audit_records(self, pk_a, pk_b, sks, r, e1, e2, rs=None):
        """Audit records from the provers' secrets, host buffers (spp_prove_audit_records): sks list of ints, r / e2 [count, 1024]
        and e1 [count, 64] int8, rs list of (r, s) ints or None (OS randomness).  Returns (proofs, pws, status, c0, c1): lists of
        bytes, status[i] == 0 or SPP_ERR_UNSAT, c0 [count, 64] / c1 [count, 1024] uint32 -- the ciphertext.json of each proof
        (spp.witness.ciphertext_json)."""
        count = len(sks)
        r = np.ascontiguousarray(r, dtype=np.int8).reshape(count, 1024)
        e1 = np.ascontiguousarray(e1, dtype=np.int8).reshape(count, 64)
        e2 = np.ascontiguousarray(e2, dtype=np.int8).reshape(count, 1024)
        a = np.ascontiguousarray(pk_a, dtype=np.uint32)
        b = np.ascontiguousarray(pk_b, dtype=np.uint32)
        if a.shape != (1024,) or b.shape != (1024,):
            raise ValueError("the public key is two polynomials of 1024 coefficients")
        skb = b"".join(int(v).to_bytes(32, "big") for v in sks)
        rsb = None
        if rs is not None:
            rsb = b"".join(int(x).to_bytes(32, "big") + int(y).to_bytes(32, "big") for x, y in rs)
        proofs = ctypes.create_string_buffer(PROOF_LEN * max(count, 1))
        pws = ctypes.create_string_buffer(self.pw_len * max(count, 1))
        status = (ctypes.c_int32 * max(count, 1))()
        c0 = np.zeros((count, 64), dtype=np.uint32)
        c1 = np.zeros((count, 1024), dtype=np.uint32)
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        rc = self.L.spp_prove_audit_records(self.h, p(a), p(b), count, skb, p(r), p(e1), p(e2), rsb, ctypes.cast(proofs, ctypes.c_void_p),
                                            ctypes.cast(pws, ctypes.c_void_p), ctypes.cast(status, ctypes.c_void_p), p(c0), p(c1))
        if rc != 0 and rc != SPP_ERR_UNSAT:
            check(rc)
        return ([proofs.raw[PROOF_LEN * i:PROOF_LEN * (i + 1)] for i in range(count)],
                [pws.raw[self.pw_len * i:self.pw_len * (i + 1)] for i in range(count)], list(status)[:count], c0, c1)

    def prove_withdraw_notes(self, tree, notes, rs=None, size=None):
        """Withdraw proofs from notes (spp.witness.pack_withdraw_notes tuples) against the resident tree `tree`
        (ShieldedPoolMerkleTree of this handle's Context): spp_prove_withdraw_notes.  Same return shape as prove_batch.
        size: against the tree of the first `size` leaves (spp_prove_withdraw_notes_at) -- Pool.root_sizes(tree) tells which size
        a pool accepts."""
        from .witness import pack_withdraw_notes
        count = len(notes)
        buf = pack_withdraw_notes(notes)
        rsb = None
        if rs is not None:
            rsb = b"".join(int(r).to_bytes(32, "big") + int(s).to_bytes(32, "big") for r, s in rs)
        proofs = ctypes.create_string_buffer(PROOF_LEN * max(count, 1))
        pws = ctypes.create_string_buffer(self.pw_len * max(count, 1))
        status = (ctypes.c_int32 * max(count, 1))()
        outs = (ctypes.cast(proofs, ctypes.c_void_p), ctypes.cast(pws, ctypes.c_void_p), ctypes.cast(status, ctypes.c_void_p))
        if size is None:
            rc = self.L.spp_prove_withdraw_notes(self.h, tree.h, count, buf, rsb, *outs)
        else:
            rc = self.L.spp_prove_withdraw_notes_at(self.h, tree.h, int(size), count, buf, rsb, *outs)
        if rc != 0 and rc != SPP_ERR_UNSAT:
            check(rc)
        return ([proofs.raw[PROOF_LEN * i:PROOF_LEN * (i + 1)] for i in range(count)],
                [pws.raw[self.pw_len * i:self.pw_len * (i + 1)] for i in range(count)], list(status)[:count])

    def prove_withdraw_notes_device(self, tree, count, d_notes, d_rs, d_proofs, d_pws, d_status, size=None):
        """Withdraw proofs from notes resident on the device against the resident tree (spp_prove_withdraw_notes_device):
        asynchronous until sync(), every proof against the root at call time.  Raw device pointers (ints).
        size: against the tree of the first `size` leaves (spp_prove_withdraw_notes_at_device)."""
        if size is None:
            check(self.L.spp_prove_withdraw_notes_device(self.h, tree.h, count, d_notes, d_rs, d_proofs, d_pws, d_status))
        else:
            check(self.L.spp_prove_withdraw_notes_at_device(self.h, tree.h, int(size), count, d_notes, d_rs, d_proofs, d_pws, d_status))

    def prove_deposits(self, tree, first_index, deposits, rs=None):
        """Deposit proofs (spp_prove_deposits) for leaves first_index .. first_index + len(deposits) - 1 of `tree`, which must already
        hold them (tree.deposit first; ShieldedPoolMerkleTree.deposit_proved does both).  deposits: (secret_key, amount, randomness)
        tuples.  Same return shape as prove_batch; the public witness is old_root | new_root | commitment | amount | index."""
        from .witness import pack_deposits
        count = len(deposits)
        buf = pack_deposits(deposits)
        rsb = None
        if rs is not None:
            rsb = b"".join(int(r).to_bytes(32, "big") + int(s).to_bytes(32, "big") for r, s in rs)
        proofs = ctypes.create_string_buffer(PROOF_LEN * max(count, 1))
        pws = ctypes.create_string_buffer(self.pw_len * max(count, 1))
        status = (ctypes.c_int32 * max(count, 1))()
        rc = self.L.spp_prove_deposits(self.h, tree.h, int(first_index), count, buf, rsb, ctypes.cast(proofs, ctypes.c_void_p),
                                       ctypes.cast(pws, ctypes.c_void_p), ctypes.cast(status, ctypes.c_void_p))
        if rc != 0 and rc != SPP_ERR_UNSAT:
            check(rc)
        return ([proofs.raw[PROOF_LEN * i:PROOF_LEN * (i + 1)] for i in range(count)],
                [pws.raw[self.pw_len * i:self.pw_len * (i + 1)] for i in range(count)], list(status)[:count])

    def prove_deposits_device(self, tree, first_index, count, d_deposits, d_rs, d_proofs, d_pws, d_status):
        """Deposit proofs from records resident on the device (spp_prove_deposits_device): asynchronous until sync().  Raw device
        pointers (ints)."""
        check(self.L.spp_prove_deposits_device(self.h, tree.h, int(first_index), count, d_deposits, d_rs, d_proofs, d_pws, d_status))

    def sync(self):
        check(self.L.spp_sync(self.h))

    def last_timings(self, which=0):
        """which=0: last enqueued batch; 1: the batch before it (see spp_timings in include/spp.h)."""
        ms = (ctypes.c_float * 9)()
        check(self.L.spp_timings(self.h, int(which), ms))
        return list(ms)

    def msm_kernel_ms(self, which=0):
        """durations of the MSM kernel launches of a batch: [commitment, A, B1, K, Z, PoK, G2] (spp_msm_kernel_ms)."""
        ms = (ctypes.c_float * 7)()
        check(self.L.spp_msm_kernel_ms(self.h, int(which), ms))
        return list(ms)

    def set_serial(self, on):
        check(self.L.spp_set_serial(self.h, 1 if on else 0))

    def debug_witness(self):
        buf = ctypes.create_string_buffer(32 * self.n_wires)
        check(self.L.spp_debug_witness(self.h, ctypes.cast(buf, ctypes.c_void_p), self.n_wires))
        return [int.from_bytes(buf.raw[32 * i:32 * i + 32], "big") for i in range(self.n_wires)]


class WithdrawalBundle:
    """What prove_withdrawals returns: everything the relayer has to post for a batch of notes.
    proofs, pws, status           the withdraw side, per note (as CircuitHandle.prove_withdraw_notes)
    audit_of, audit_note          the plan: audit_note[s] is the note whose secrets made record s, audit_of[i] the record of note
                                  i's identity or SPP_AUDIT_RESIDENT when the pool already holds it
    audit_proofs, audit_pws, audit_status, c0, c1
                                  the audit records, per entry of audit_note (as CircuitHandle.prove_audit_records)"""

    def __init__(self, proofs, pws, status, audit_of, audit_note, audit_proofs, audit_pws, audit_status, c0, c1):
        self.proofs, self.pws, self.status = proofs, pws, status
        self.audit_of, self.audit_note = audit_of, audit_note
        self.audit_proofs, self.audit_pws, self.audit_status, self.c0, self.c1 = audit_proofs, audit_pws, audit_status, c0, c1

    @property
    def n_audits(self):
        return len(self.audit_note)

    def log(self, addresses):
        """The instruction list Pool.settle_log takes, in the relayer's order (demo-frontend/app/api/relay/withdraw/route.ts:238-287):
        for note i its submit_audit first, if note i is the one whose record was proved, then its withdraw to addresses[i]."""
        if len(addresses) != len(self.proofs):
            raise ValueError("log: one 32-byte account address per note")
        out = []
        for i, address in enumerate(addresses):
            s = self.audit_of[i]
            if s != SPP_AUDIT_RESIDENT and self.audit_note[s] == i:
                out.append(("submit_audit", self.audit_proofs[s], self.audit_pws[s]))
            out.append(("withdraw", self.proofs[i], self.pws[i], bytes(address)))
        return out


def prove_withdrawals(withdraw_handle, audit_handle, tree, notes, pk_a, pk_b, r=None, e1=None, e2=None, pool=None, size=None,
                      rs_withdraw=None, rs_audit=None, audit_cap=None):
    """Both proofs of a batch of withdrawals, one audit record per identity the pool does not hold yet (spp_prove_withdrawals).
    withdraw_handle / audit_handle: the two CircuitHandles, tree (ShieldedPoolMerkleTree) and pool (Pool, optional) of one Context;
    notes: (recipient, amount, secret_key, randomness, index) tuples, e.g. from ShieldedPoolMerkleTree.sync; pk_a, pk_b: the RLWE
    public key; r / e2 [count, 1024] and e1 [count, 64] int8 per NOTE, or all None for noise from the operating system; size: prove
    against the tree of the first `size` leaves (Pool.root_sizes); rs_withdraw / rs_audit: lists of (r, s) ints per NOTE or None;
    audit_cap: room for audit records (default: one per note).  Returns a WithdrawalBundle; a refused row has a non-zero status on
    its side and zero proof bytes.  Raises SppError when the batch needs more than audit_cap records."""
    from .witness import pack_withdraw_notes
    L = withdraw_handle.L
    count = len(notes)
    buf = pack_withdraw_notes(notes)
    cap = count if audit_cap is None else int(audit_cap)
    if (r is None) != (e1 is None) or (r is None) != (e2 is None):
        raise ValueError("r, e1 and e2: all three or none")
    p = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)
    if r is not None:
        r = np.ascontiguousarray(r, dtype=np.int8).reshape(count, 1024)
        e1 = np.ascontiguousarray(e1, dtype=np.int8).reshape(count, 64)
        e2 = np.ascontiguousarray(e2, dtype=np.int8).reshape(count, 1024)
    a = np.ascontiguousarray(pk_a, dtype=np.uint32)
    b = np.ascontiguousarray(pk_b, dtype=np.uint32)
    if a.shape != (1024,) or b.shape != (1024,):
        raise ValueError("the public key is two polynomials of 1024 coefficients")
    rsb = lambda rs: None if rs is None else b"".join(int(x).to_bytes(32, "big") + int(y).to_bytes(32, "big") for x, y in rs)
    if any(rs is not None and len(rs) != count for rs in (rs_withdraw, rs_audit)):
        raise ValueError("rs_withdraw / rs_audit: one (r, s) pair per note")
    wpl, apl = withdraw_handle.pw_len, audit_handle.pw_len
    proofs = ctypes.create_string_buffer(PROOF_LEN * max(count, 1))
    pws = ctypes.create_string_buffer(wpl * max(count, 1))
    status = (ctypes.c_int32 * max(count, 1))()
    audit_of = (ctypes.c_uint32 * max(count, 1))()
    audit_note = (ctypes.c_uint32 * max(cap, 1))()
    n = ctypes.c_uint32(0)
    aproofs = ctypes.create_string_buffer(PROOF_LEN * max(cap, 1))
    apws = ctypes.create_string_buffer(apl * max(cap, 1))
    astatus = (ctypes.c_int32 * max(cap, 1))()
    c0 = np.zeros((max(cap, 1), 64), dtype=np.uint32)
    c1 = np.zeros((max(cap, 1), 1024), dtype=np.uint32)
    vp = lambda x: ctypes.cast(x, ctypes.c_void_p)
    rc = L.spp_prove_withdrawals(withdraw_handle.h, audit_handle.h, tree.h, None if pool is None else pool.h,
                                 SPP_TREE_SIZE_NOW if size is None else int(size), p(a), p(b), count, buf, p(r), p(e1), p(e2),
                                 rsb(rs_withdraw), rsb(rs_audit), vp(proofs), vp(pws), vp(status), vp(audit_of), vp(audit_note),
                                 ctypes.byref(n), cap, vp(aproofs), vp(apws), vp(astatus), p(c0), p(c1))
    if rc != 0 and rc != SPP_ERR_UNSAT:
        check(rc)
    na = n.value
    return WithdrawalBundle([proofs.raw[PROOF_LEN * i:PROOF_LEN * (i + 1)] for i in range(count)],
                            [pws.raw[wpl * i:wpl * (i + 1)] for i in range(count)], list(status)[:count], list(audit_of)[:count],
                            list(audit_note)[:na], [aproofs.raw[PROOF_LEN * s:PROOF_LEN * (s + 1)] for s in range(na)],
                            [apws.raw[apl * s:apl * (s + 1)] for s in range(na)], list(astatus)[:na], c0[:na], c1[:na])
