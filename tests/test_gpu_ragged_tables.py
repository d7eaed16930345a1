"""Ragged MSM tables on the device (csrc/msm_ragged.hpp, k_msm_flat / k_build_table in csrc/msm_table.hpp): the rows of bases
whose wire is a bit or a byte are 1 / 128 / 256 entries long instead of 2^(c-1), which leaves the 240 GB budget room for 16-bit
windows on all five flat sets of the audit circuit.  SPP_RAGGED=0 loads the tables with full rows for every base, for comparison.
Reference behaviour: the proof bytes of `sunspot prove` (scripts/generate_audit.py:680) through the C oracle."""
import ctypes
import random

import pytest
import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime, torch's is the one that has to be loaded first)

pytestmark = pytest.mark.gpu
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
N_IN = 3360
R0 = 2 + 157 + 1     # input index of r[0] in an audit row (tests/test_host_cpu.py::test_audit_circuit_semantics)


@pytest.fixture(scope="module")
def ctx():
    import spp
    c = spp.Context(0)
    yield c
    c.close()


def _prove_raw(h, count, rows, rs_vals):
    rsb = b"".join(r.to_bytes(32, "big") + s.to_bytes(32, "big") for r, s in rs_vals)
    proofs = ctypes.create_string_buffer(388 * count)
    pws = ctypes.create_string_buffer(h.pw_len * count)
    status = (ctypes.c_int32 * count)()
    rc = h.L.spp_prove_batch(h.h, count, bytes(rows), rsb, ctypes.cast(proofs, ctypes.c_void_p), ctypes.cast(pws, ctypes.c_void_p),
                             ctypes.cast(status, ctypes.c_void_p))
    return rc, [proofs.raw[388 * i:388 * (i + 1)] for i in range(count)], [pws.raw[h.pw_len * i:h.pw_len * (i + 1)] for i in range(count)], list(status)


def test_ragged_audit_tables_windows_guard_and_comparison_switch(ctx, audit_artifacts, rlwe_pk, monkeypatch):
    """Default load of the audit circuit: the five flat sets at 16 bits inside the 240 GB budget.
    A batch of 128 rows in which row 5 has r[0] = 200 (outside [-128, 127]: a digit above the 128 entries of its base's rows in
    window 0) and row 70 has r[3] = 2^40 (non-zero digits above window 0, which every pass must skip): the call returns, exactly
    those two rows are refused, every other row's proof and public witness are the oracle's bytes.  One call, not repeated.
    Then 256 rows under the default load and under SPP_RAGGED=0 (the parent's tables and windows): the same bytes."""
    from spp import workload
    from oracle import native
    monkeypatch.delenv("SPP_TABLE_BUDGET_GB", raising=False)
    monkeypatch.delenv("SPP_RAGGED", raising=False)
    rng = random.Random(41)
    B, Bg = 256, 128
    rows = workload.audit_rows(ctx, rlwe_pk["a"], rlwe_pk["b"], B, first=3000)
    rs_vals = [(rng.randrange(1, R), rng.randrange(1, R)) for _ in range(B)]
    guard_rows = bytearray(workload.audit_rows(ctx, rlwe_pk["a"], rlwe_pk["b"], Bg, first=5000))
    for i, idx, v in ((5, R0 + 0, 200), (70, R0 + 3, 1 << 40)):
        off = 32 * (N_IN * i + idx)
        guard_rows[off:off + 32] = v.to_bytes(32, "big")
    bad = {5, 70}

    # The loader caps the table budget at 85 % of the FREE memory, and 16 bits for all five sets take 227 GB of the 309 GB: give
    # back what this process still holds from earlier tests -- the circuits the drop-in helper keeps resident for the life of the
    # process (spp/proof_helper.py: the audit circuit at 8-bit windows alone is ~40 GB; it reloads them on demand) and what the
    # torch allocator caches.
    import gc
    from spp import proof_helper
    for key in list(proof_helper._HANDLES):
        proof_helper._HANDLES.pop(key).close()
    gc.collect()
    reserved = torch.cuda.memory_reserved()
    torch.cuda.empty_cache()
    free_b, total_b = torch.cuda.mem_get_info()
    print("before the load: %.4g of %.4g bytes free (torch had %.4g reserved)" % (free_b, total_b, reserved))
    h = ctx.load_circuit(audit_artifacts["sppc"], audit_artifacts["pk"], 0)
    try:
        bits, trows, tb = h.msm_windows(), h.msm_table_rows(), h.table_bytes
        print("ragged: windows", bits, "table bytes %.4g" % tb)
        assert bits[:4] + [bits[6]] == [16] * 5 and trows[:4] + [trows[6]] == [1] * 5 and tb <= 240e9, (bits, trows, tb)
        rc_g, pl_g, wl_g, st_g = _prove_raw(h, Bg, guard_rows, rs_vals[:Bg])
        rc, pl, wl, st = _prove_raw(h, B, rows, rs_vals)
        assert h.n_inputs == N_IN
    finally:
        h.close()
    assert rc_g == -4 and [i for i in range(Bg) if st_g[i] != 0] == sorted(bad), (rc_g, st_g)
    assert rc == 0 and st == [0] * B and len(set(pl)) == B

    monkeypatch.setenv("SPP_RAGGED", "0")
    h = ctx.load_circuit(audit_artifacts["sppc"], audit_artifacts["pk"], 0)
    try:
        bits0, tb0 = h.msm_windows(), h.table_bytes
        print("SPP_RAGGED=0: windows", bits0, "table bytes %.4g" % tb0)
        assert bits0 == [16, 16, 15, 15, 9, 9, 16] and tb0 <= 240e9, (bits0, tb0)
        rc0, pl0, wl0, st0 = _prove_raw(h, B, rows, rs_vals)
    finally:
        h.close()
    monkeypatch.delenv("SPP_RAGGED")
    assert rc0 == 0 and st0 == [0] * B
    assert pl0 == pl and wl0 == wl
    assert tb < tb0 + 5e9      # all five sets at 16 bits in about the bytes the parent's 15-bit K and Z took

    orc = native.Prover(audit_artifacts["sppc"], audit_artifacts["pk"])
    for i in range(Bg):
        rc_o, proof, pw = orc.prove(workload.row_ints(bytes(guard_rows), N_IN, i), *rs_vals[i])
        if i in bad:
            assert rc_o != 0, i
        else:
            assert rc_o == 0 and pl_g[i] == proof and wl_g[i] == pw, i
    for i in (0, 63, 64, B - 1):
        rc_o, proof, pw = orc.prove(workload.row_ints(rows, N_IN, i), *rs_vals[i])
        assert rc_o == 0 and pl[i] == proof and wl[i] == pw, i


def test_row_per_window_tables_keep_the_uniform_layout(ctx, withdraw_artifacts, withdraw_kat):
    """The withdraw circuit at explicit window_bits = 8 (a table row per window, k_msm_rows): equal to the oracle."""
    from oracle import native, circuit as C
    h = ctx.load_circuit(withdraw_artifacts["sppc"], withdraw_artifacts["pk"], 8)
    try:
        assert h.msm_windows() == [8] * 7 and h.msm_table_rows() == [32] * 7
        good = C.withdraw_inputs(withdraw_kat)
        batch = [good] * 70
        rs = [(i + 1, 5 * i + 3) for i in range(len(batch))]
        proofs, pws, status = h.prove_batch(batch, rs)
    finally:
        h.close()
    assert status == [0] * len(batch)
    orc = native.Prover(withdraw_artifacts["sppc"], withdraw_artifacts["pk"])
    for i in (0, 1, 63, 64, 69):
        rc, proof, pw = orc.prove(batch[i], *rs[i])
        assert rc == 0 and proofs[i] == proof and pws[i] == pw, i
