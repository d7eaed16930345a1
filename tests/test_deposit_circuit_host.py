"""The deposit circuit and the chain rule without a GPU: the container spp_circuit_build(SPP_CIRCUIT_DEPOSIT) writes, interpreted by
the oracle (oracle/circuit.py, oracle/native.py) over rows of the Python model (tests/deposit_model.py); which gadget refuses which
wrong row; every wire constrained; a proof by the oracle's CPU prover under the Python pairing verifier; the chain model on a crafted
log; the declarations, the NULL refusals and the command-line parsers.

Constraint layout, restated from the statement (not read from csrc/): byte recomposition of amount [0]; the t=5 hash, 8 x 5 + 60
S-boxes of four rows [1, 401); commitment == hash [401]; 16 boolean rows and the recomposition of index [402, 419); per level and
chain one selection row and a t=3 hash of 8 x 3 + 57 S-boxes [419, 10819); old_root [10819]; new_root [10820]; then the lookup
argument and the public-input rows."""
import ctypes
import json
import os
import random
import re

import pytest

from conftest import ROOT
import deposit_model as M

R = M.R
AMOUNT_LIMBS, COMMITMENT_EQ, INDEX_BITS, OLD_ROOT_EQ, NEW_ROOT_EQ = 0, 401, range(402, 419), 10819, 10820
ROOT_EQS = (OLD_ROOT_EQ, NEW_ROOT_EQ)


@pytest.fixture(scope="module")
def deposit_artifacts(workdir):
    """SPPC built by the product's builder (host), pk/vk by the ORACLE's CPU setup (seed 6)."""
    import spp
    from oracle import native
    sppc, pk, vk = (os.path.join(workdir, "deposit." + e) for e in ("sppc", "pk", "vk"))
    n = spp.build_circuit(6, sppc)
    native.setup(sppc, b"\x06" * 32, pk, vk)
    return dict(sppc=sppc, pk=pk, vk=vk, n_constraints=n)


@pytest.fixture(scope="module")
def good_rows():
    """rows at indices 0..3 of a real tree, then 2^15 and 2^16 - 1 over random siblings (the circuit does not care what they are)"""
    rng = random.Random(0xDE905)
    records = [(rng.randrange(1, R), rng.randrange(1 << 64), rng.randrange(R)) for _ in range(4)]
    _, rows = M.rows_for_deposits(records)
    for index in (1 << 15, (1 << 16) - 1):
        owner, c = M.commitment_of((rng.randrange(1, R), rng.randrange(1 << 64), rng.randrange(R)))
        rows.append(M.row_from_parts(owner, 123456789, 987654321, index, [rng.randrange(R) for _ in range(M.DEPTH)]))
    return records, rows


def test_container_shape(deposit_artifacts):
    from oracle import circuit as C
    circ = C.Circuit(deposit_artifacts["sppc"])
    assert circ.id == 6 and circ.n_public - 1 == 5 and circ.n_secret == 19 and circ.n_inputs() == M.ROW_FIELDS
    assert circ.n_constraints == deposit_artifacts["n_constraints"] == 11093 and circ.domain_log == 14
    assert len(circ.aux) == 0                                                # no Grumpkin ladder: no window tables
    masks = __import__("test_circuit_soundness")._mask_wires(circ)
    assert len(masks) == 1 and circ.challenge_wire > masks[0]


def test_model_rows_satisfy_the_circuit_public_wires_in_order(deposit_artifacts, good_rows):
    from oracle import circuit as C, native
    circ = C.Circuit(deposit_artifacts["sppc"])
    _, rows = good_rows
    assert [r[4] for r in rows] == [0, 1, 2, 3, 1 << 15, (1 << 16) - 1]
    for row in rows[:2] + rows[-1:]:
        w = C.solve(circ, row, lambda w_: 0x5eed)
        assert C.first_unsatisfied(circ, w) == -1
        assert w[1:6] == row[:5]                                             # old_root | new_root | commitment | amount | index
    p = native.Prover(deposit_artifacts["sppc"], deposit_artifacts["pk"])
    assert native.check_many(p, rows) == [-1] * len(rows)
    # the chain of old and new roots of a real tree
    assert rows[0][0] == M.Tree().root() and all(rows[k + 1][0] == rows[k][1] for k in range(3))


def test_wrong_rows_are_refused_by_the_gadget_one_expects(deposit_artifacts, good_rows):
    from oracle import native
    p = native.Prover(deposit_artifacts["sppc"], deposit_artifacts["pk"])
    records, rows = good_rows
    good = rows[3]                                                           # index 3: both left siblings are real nodes
    cases = []
    for i in range(M.ROW_FIELDS):
        for d in (1, -1):
            x = list(good)
            x[i] = (x[i] + d) % R
            want = ((OLD_ROOT_EQ,), (NEW_ROOT_EQ,), (COMMITMENT_EQ,), (COMMITMENT_EQ,), ROOT_EQS)[i] if i < 5 else \
                (COMMITMENT_EQ,) if i < 8 else ROOT_EQS
            cases.append(("input %d %+d" % (i, d), x, want))
    x = list(good); x[3] = 1 << 64
    cases.append(("amount 2^64", x, (AMOUNT_LIMBS,)))
    x = list(good); x[4] = 1 << 16
    cases.append(("index 2^16", x, (INDEX_BITS[-1],)))
    x = list(good); x[0] = good[1]                                           # the root of a tree where slot 3 is occupied
    cases.append(("occupied slot", x, (OLD_ROOT_EQ,)))
    x = list(good); x[0], x[1] = good[1], good[0]
    cases.append(("swapped roots", x, (OLD_ROOT_EQ,)))
    x = list(rows[0]); x[1] = x[0]                                           # "nothing was appended"
    cases.append(("new_root = old_root", x, (NEW_ROOT_EQ,)))
    res = native.check_many(p, [c[1] for c in cases])
    for (name, _, want), got in zip(cases, res):
        assert got in want, (name, got, want)


def test_every_wire_is_constrained(deposit_artifacts, good_rows):
    from oracle import circuit as C
    from test_circuit_soundness import _free_wires, _mask_wires
    circ = C.Circuit(deposit_artifacts["sppc"])
    rng = random.Random(13)
    w = C.solve(circ, good_rows[1][3], lambda w_: 0xabcdef0123)
    free = _free_wires(circ, w, [1, rng.randrange(2, R)])
    assert free == _mask_wires(circ), "under-constrained deposit wires: %r" % free[:20]


def test_oracle_proof_verifies_and_a_flipped_public_word_does_not(deposit_artifacts, good_rows):
    from oracle import native, groth16
    p = native.Prover(deposit_artifacts["sppc"], deposit_artifacts["pk"])
    row = good_rows[1][2]
    rc, proof, pw = p.prove(row, 3, 4)
    assert rc == 0 and len(pw) == 172 and pw == groth16.public_witness_bytes(row[:5])
    vk = open(deposit_artifacts["vk"], "rb").read()
    assert len(vk) == 1296
    assert groth16.verify(vk, proof, pw)
    bad = bytearray(pw); bad[12 + 32 + 31] ^= 1                              # new_root
    assert not groth16.verify(vk, proof, bytes(bad))


def _pw(words):
    return (5).to_bytes(4, "big") + bytes(4) + (5).to_bytes(4, "big") + b"".join(M.word(v) for v in words)


def test_chain_model_on_a_crafted_log():
    rng = random.Random(77)
    roots = [rng.randrange(R) for _ in range(12)]
    link = lambda a, b, idx, amount=5: _pw([roots[a], roots[b], 9, amount, idx])
    #           0 ok        1 amount        2 ok(on 0)   3 stale         4 index       5 proof       6 ok          7 built on 5: stale
    pws = [link(0, 1, 10), link(1, 2, 11, 6), link(1, 2, 11), link(1, 3, 12), link(2, 3, 13), link(2, 4, 12), link(2, 5, 12), link(4, 6, 13),
           link(5, 7, 13)]                                                   # 8 ok
    ok = [True, True, True, True, True, False, True, True, True]
    codes, end_root, end_index = M.check_chain(pws, ok, M.word(roots[0]), 10, lamports=[5] * 9)
    assert [M.NAMES[c] for c in codes] == ["OK", "BAD_AMOUNT", "OK", "STALE_ROOT", "BAD_INDEX", "BAD_PROOF", "OK", "STALE_ROOT", "OK"]
    assert end_root == M.word(roots[7]) and end_index == 14
    # order of the checks: amount before root before index before proof
    both = _pw([roots[9], roots[1], 9, 6, 99])
    assert M.check_chain([both], [False], M.word(roots[0]), 10, [5])[0] == [M.BAD_AMOUNT]
    assert M.check_chain([both], [False], M.word(roots[0]), 10, None)[0] == [M.STALE_ROOT]
    assert M.check_chain([_pw([roots[0], roots[1], 9, 6, 99])], [False], M.word(roots[0]), 10, None)[0] == [M.BAD_INDEX]
    # nothing accepted: the end state is the start state
    assert M.check_chain([both], [True], M.word(roots[0]), 10, None)[1:] == (M.word(roots[0]), 10)
    assert M.check_chain([], [], M.word(roots[3]), 4) == ([], M.word(roots[3]), 4)


def test_header_declares_the_calls_and_python_mirrors_them():
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "spp.h")).read())
    for decl in ("#define SPP_CIRCUIT_DEPOSIT 6", "#define SPP_DEPOSIT_PW_LEN 172", "#define SPP_DEPOSIT_INPUTS 24",
                 "#define SPP_DEPOSIT_OK 0", "#define SPP_DEPOSIT_BAD_AMOUNT 1", "#define SPP_DEPOSIT_STALE_ROOT 2",
                 "#define SPP_DEPOSIT_BAD_INDEX 3", "#define SPP_DEPOSIT_BAD_PROOF 4",
                 "int spp_deposit_rows_from_tree(spp_merkle_tree* t, uint64_t first_index, size_t count, const uint8_t* deposits, uint8_t* rows);",
                 "int spp_prove_deposits_device(spp_circuit* c, spp_merkle_tree* t, uint64_t first_index, size_t count, const void* d_deposits, "
                 "const void* d_rs, void* d_proofs, void* d_pws, void* d_status);",
                 "int spp_prove_deposits(spp_circuit* c, spp_merkle_tree* t, uint64_t first_index, size_t count, const uint8_t* deposits, "
                 "const uint8_t* rs, uint8_t* proofs, uint8_t* pws, int32_t* status);",
                 "int spp_verify_deposit_chain(spp_ctx* ctx, const uint8_t* vk, size_t vk_len, size_t count, const uint8_t* proofs, "
                 "const uint8_t* pws, const uint64_t* lamports /* optional */, const uint8_t start_root[32], uint64_t start_index, "
                 "uint32_t* codes, uint8_t end_root[32], uint64_t* end_index);"):
        assert decl in hdr, decl
    assert "deposit.rs:31-36,73" in hdr and "does NOT verify" in hdr
    import spp
    from spp import lib, prover, witness
    L = spp.load_library()
    for name in ("spp_deposit_rows_from_tree", "spp_prove_deposits_device", "spp_prove_deposits", "spp_verify_deposit_chain"):
        assert hasattr(L, name), name
    assert lib.SPP_CIRCUIT_DEPOSIT == 6 and lib.DEPOSIT_PW_LEN == 172 and lib.DEPOSIT_INPUTS == 24
    assert lib.DEPOSIT_RESULT_NAMES == tuple(M.NAMES)
    assert callable(witness.ShieldedPoolMerkleTree.deposit_rows) and callable(witness.ShieldedPoolMerkleTree.deposit_proved)
    assert callable(witness.verify_deposit_chain) and callable(prover.CircuitHandle.prove_deposits)


def test_the_calls_refuse_null_without_a_device():
    import spp
    L = spp.load_library()
    buf = ctypes.create_string_buffer(4096)
    vp = ctypes.cast(buf, ctypes.c_void_p)
    calls = (lambda: L.spp_deposit_rows_from_tree(None, 0, 1, bytes(96), vp),
             lambda: L.spp_deposit_rows_from_tree(None, 0, 0, None, None),
             lambda: L.spp_prove_deposits_device(None, None, 0, 1, vp, vp, vp, vp, vp),
             lambda: L.spp_prove_deposits(None, None, 0, 1, bytes(96), None, vp, vp, vp),
             lambda: L.spp_verify_deposit_chain(None, bytes(1296), 1296, 0, None, None, None, bytes(32), 0, vp, vp, None),
             lambda: L.spp_verify_deposit_chain(vp, None, 0, 0, None, None, None, bytes(32), 0, vp, vp, None),
             lambda: L.spp_verify_deposit_chain(vp, bytes(1296), 1296, 1, None, None, None, bytes(32), 0, vp, vp, None))
    for k, call in enumerate(calls):
        L.spp_verify(None, 0, None, 0, None, 0, None)     # leaves another message behind
        assert call() == -1 and "NULL" in spp.last_error(), k


def test_cli_parsers_and_pool_replay_ignores_the_extra_keys(tmp_path, capsys):
    from spp import cli
    recs = cli.parse_deposit_records(['{"secretKey": "0x10", "amount": 5, "randomness": "7"}', "", '{"secretKey": 3, "amount": "9", "randomness": 1}'])
    assert recs == [(16, 5, 7), (3, 9, 1)]
    for bad in ('{"secretKey": 0, "amount": 5, "randomness": 7}', '{"secretKey": 1, "amount": %d, "randomness": 7}' % (1 << 64),
                '{"secretKey": 1, "amount": 5}', "[]"):
        with pytest.raises(ValueError, match="line 1"):
            cli.parse_deposit_records([bad])
    line = json.dumps({"deposit": {"root": "11" * 32, "commitment": "%064x" % 5, "amount": 7, "proof": "00" * 388, "pw": "22" * 172}})
    other = json.dumps({"withdraw": {"proof": "00" * 388, "pw": "00" * 172, "recipient": "11" * 32}})
    assert cli.parse_deposit_log([line, other, ""]) == [(1, bytes(388), b"\x22" * 172, 7)]
    with pytest.raises(ValueError, match="line 2"):
        cli.parse_deposit_log([line, json.dumps({"deposit": {"root": "11" * 32}})])
    with pytest.raises(ValueError, match="line 1"):
        cli.parse_deposit_log([json.dumps({"deposit": {"root": "11" * 32, "amount": 7, "proof": "00" * 387, "pw": "22" * 172}})])
    # pool-replay reads such a line as the deposit it always read: the root, and the commitment it already knew about
    assert cli.parse_pool_log([line, other]) == [("deposit", (b"\x11" * 32,)), ("withdraw", (bytes(388), bytes(172), b"\x11" * 32))]
    assert cli.parse_pool_commitments([line, other]) == [5]
    # argument errors touch no device
    log = str(tmp_path / "log.jsonl"); vk = str(tmp_path / "d.vk")
    open(vk, "wb").write(b"x"); open(log, "w").write(json.dumps({"deposit": {"root": "11" * 32}}) + "\n")
    assert cli.main(["deposit-verify", vk, log]) == 2 and "line 1" in capsys.readouterr().err
    assert cli.main(["deposit-prove", str(tmp_path / "none.jsonl"), vk, vk, log, "--out", str(tmp_path / "o")]) == 2
    assert "spp deposit-prove:" in capsys.readouterr().err
