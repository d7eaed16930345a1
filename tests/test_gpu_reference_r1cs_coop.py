"""The reference's own R1CS with its solver (spp/ccs.py to_sppc_solved) on the cooperative solver: one handle as loaded by default
(k_solve_coop at these batch sizes), one loaded under SPP_NO_COOP=1 (k_solve), both with 8-bit windows, next to the oracle's prover
of the all-inputs container of the same system under the same seed.  Wires are compared with gnark's solver loop as restated in
spp/ccs.py solve_partial, proofs with the oracle's bytes."""
import os
import types
import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None
from test_acir_ccs import program, _reference_system, _fresh_note_inputs, EDGE_KEYS  # noqa: F401  (program: a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lab(program, tmp_path_factory):
    import spp
    from spp import ccs
    from oracle import native
    tmp = tmp_path_factory.mktemp("solved_coop")
    c, s, pure = _reference_system(tmp)
    solved = str(tmp / "solved.sppc")
    n, ss = ccs.to_sppc_solved(s, c, program, solved)
    assert n == 12452
    pk, vk, opk, ovk = (str(tmp / x) for x in ("s.pk", "s.vk", "o.pk", "o.vk"))
    seed = b"\x0b" * 32
    saved = {k: os.environ.pop(k, None) for k in ("SPP_NO_COOP", "SPP_COOP_MAX", "SPP_NO_LEVEL_STREAM", "SPP_COOP_ONE_TRACK")}
    ctx = spp.Context(0)
    try:
        ctx.setup(solved, seed, pk, vk)
        native.setup(pure, seed, opk, ovk)
        assert open(vk, "rb").read() == open(ovk, "rb").read()
        h = ctx.load_circuit(solved, pk, 8)
        os.environ["SPP_NO_COOP"] = "1"
        try:
            h_lane = ctx.load_circuit(solved, pk, 8)
        finally:
            del os.environ["SPP_NO_COOP"]
        try:
            yield types.SimpleNamespace(c=c, s=s, ss=ss, ctx=ctx, h=h, h_lane=h_lane, vkb=open(vk, "rb").read(), orc=native.Prover(pure, opk))
        finally:
            h.close()
            h_lane.close()
    finally:
        ctx.close()
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v


def _nine_rows(withdraw_kat):
    """the KAT row, a note for every key of EDGE_KEYS and one for lambda mod 2^128"""
    from spp import ccs
    from oracle import circuit as C
    keys = EDGE_KEYS + (ccs.GLV_LAMBDA % (1 << 128),)
    rows = [C.withdraw_inputs(withdraw_kat)] + [_fresh_note_inputs(300 + i, sk=k) for i, k in enumerate(keys)]
    assert len(rows) == 9 and [r[5] for r in rows[1:]] == list(keys)
    return rows


def _reference_wires(L, program, row, rs, challenge, challenge_fn=None):
    from spp import ccs, acir
    from oracle import circuit as C
    wa = acir.execute(program, row)
    ref, st = ccs.solve_partial(L.s, L.c, row[:5], {"__witness_%d" % k: v for k, v in wa.items()}, challenge=challenge,
                                challenge_fn=challenge_fn, randomizer=C.mask_value(*rs))
    assert not st["rows_skipped"] and not st["hints_skipped"]
    return ref, not st["rows_unsatisfied"]


def test_plan_names_the_generic_rows(lab):
    st = lab.h.plan_stats()
    assert st["generic_rows"] == 12131 and st["generic_divs"] == 752 and st["tracks"] >= 1, st
    assert st["items_levels"] + st["items_level_stream"] > 0, st
    off = lab.h_lane.plan_stats()
    assert off["generic_rows"] == 0 and off["generic_divs"] == 0, off


def test_lone_proofs_on_the_cooperative_solver(lab, program, withdraw_kat):
    """the KAT row and the eight edge-key rows, each alone: every wire equals solve_partial, the proof the oracle's bytes; a key that
    solve_partial refuses is refused in place.  The same nine rows then go first in a batch of 65 on the SPP_NO_COOP=1 handle: the
    bytes are those of the lone proofs, which keeps the hints covered in k_solve."""
    rows = _nine_rows(withdraw_kat)
    rs = [(7919 * i + 3, (1 << 190) + 31 * i) for i in range(65)]
    alone, accepted = [], []
    for i, row in enumerate(rows):
        r = rs[i]
        proofs, pws, status = lab.h.prove_batch([row], [r])
        dev = lab.h.debug_witness()
        ref, ok = _reference_wires(lab, program, row, r, dev[lab.ss.challenge_wire])
        alone.append(proofs[0])
        accepted.append(ok)
        if not ok:
            assert status[0] != 0 and proofs[0] == bytes(388), i
            continue
        assert status == [0], i
        assert [dev[lab.ss.perm[g]] for g in range(lab.s.n_wires)] == ref, i           # every wire
        rc, proof, pw = lab.orc.prove(ref[1:], r[0], r[1])
        assert rc == 0 and proofs[0] == proof and pws[0] == pw, i
    assert accepted[0] and accepted[-1]
    batch = rows + [_fresh_note_inputs(400 + k) for k in range(56)]
    proofs, pws, status = lab.h_lane.prove_batch(batch, rs)
    assert [st == 0 for st in status] == accepted + [True] * 56
    assert proofs[:9] == alone
    live = [k for k in range(65) if status[k] == 0]
    assert all(lab.ctx.verify_batch(lab.vkb, [proofs[k] for k in live], [pws[k] for k in live]))


def test_batch_of_17_with_one_spoiled_row(lab, program):
    """17 fresh notes, one with a wrong amount: refused alone; every accepted proof is the oracle's bytes and verifies"""
    from spp import ccs
    from oracle import native
    batch = [_fresh_note_inputs(500 + k) for k in range(17)]
    bad = list(batch[7]); bad[3] += 1
    batch[7] = bad
    rs = [(3 * k + 1, 5 * k + 2) for k in range(17)]
    proofs, pws, status = lab.h.prove_batch(batch, rs)
    assert [k for k in range(17) if status[k] != 0] == [7] and proofs[7] == bytes(388)
    good = [k for k in range(17) if k != 7]
    cw, full = ccs.challenge_wire(lab.s), []
    for k in good:
        # the oracle's solver runs the commitment step on the wires of the first phase and shows the challenge
        ref, ok = _reference_wires(lab, program, batch[k], rs[k], None, challenge_fn=lambda ws: lab.orc.prove(
            [0 if v is None else v for v in ws[1:]], rs[k][0], rs[k][1], want_wires=True)[3][cw])
        assert ok, k
        full.append(ref[1:])
    rc, want_proofs, want_pws = native.prove_many(lab.orc, full, [rs[k] for k in good])
    assert rc == 0
    assert [proofs[k] for k in good] == want_proofs and [pws[k] for k in good] == want_pws
    assert all(lab.ctx.verify_batch(lab.vkb, want_proofs, want_pws))
