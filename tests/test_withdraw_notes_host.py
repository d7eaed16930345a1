"""Withdraw proofs from notes, host side (no GPU): the note layout spp.witness.pack_withdraw_notes hands to
spp_withdraw_rows_from_tree / spp_prove_withdraw_notes(_device), and the C declarations of those entry points."""
import ctypes
import os
import re
import pytest
from conftest import ROOT

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def test_pack_withdraw_notes_layout_and_field_order():
    from spp import witness as W
    notes = [(0xA1, 5 * 10 ** 9, 0x1234567890ABCDEF, R - 1, 7), (1, 0, 2, 3, (1 << 16) + 5)]
    buf = W.pack_withdraw_notes(notes)
    assert len(buf) == 2 * 160
    # recipient | amount | secret_key | randomness | index, 32-byte big-endian each (noir_circuit/src/main.nr:38-51)
    expect = b"".join(int(v).to_bytes(32, "big") for note in notes for v in note)
    assert buf == expect
    assert buf[31] == 0xA1 and buf[:31] == bytes(31)
    assert int.from_bytes(buf[32:64], "big") == 5 * 10 ** 9
    assert int.from_bytes(buf[64:96], "big") == 0x1234567890ABCDEF
    assert int.from_bytes(buf[96:128], "big") == R - 1
    assert int.from_bytes(buf[128:160], "big") == 7
    assert int.from_bytes(buf[160 + 128:320], "big") == (1 << 16) + 5
    assert W.pack_withdraw_notes([]) == b""


@pytest.mark.parametrize("field", range(5))
def test_pack_withdraw_notes_rejects_non_canonical_values(field):
    from spp import witness as W
    for bad in (R, R + 1, 1 << 256, -1):
        note = [1, 2, 3, 4, 5]
        note[field] = bad
        with pytest.raises(ValueError) as e:
            W.pack_withdraw_notes([(1, 1, 1, 1, 0), tuple(note)])
        assert "note 1" in str(e.value) and W.NOTE_FIELDS[field] in str(e.value)


def test_pack_withdraw_notes_rejects_wrong_tuple_length():
    from spp import witness as W
    for note in ((1, 2, 3, 4), (1, 2, 3, 4, 5, 6), ()):
        with pytest.raises(ValueError):
            W.pack_withdraw_notes([note])


def test_header_declares_the_notes_entry_points():
    hdr = open(os.path.join(ROOT, "include", "spp.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert "int spp_withdraw_rows_from_tree(spp_merkle_tree* t, size_t count, const uint8_t* notes, uint8_t* rows);" in flat
    assert ("int spp_prove_withdraw_notes_device(spp_circuit* c, spp_merkle_tree* t, size_t count, const void* d_notes, const void* d_rs, "
            "void* d_proofs, void* d_pws, void* d_status);") in flat
    assert ("int spp_prove_withdraw_notes(spp_circuit* c, spp_merkle_tree* t, size_t count, const uint8_t* notes, const uint8_t* rs, "
            "uint8_t* proofs, uint8_t* pws, int32_t* status);") in flat
    assert re.search(r"#define SPP_NOTE_LEN 160\b", hdr)


def test_notes_entry_points_refuse_null_arguments_without_a_device():
    import spp
    from spp.lib import NOTE_LEN
    L = spp.load_library()
    assert NOTE_LEN == 160
    note = bytes(160)
    out = ctypes.create_string_buffer(26 * 32)
    assert L.spp_withdraw_rows_from_tree(None, 1, note, ctypes.cast(out, ctypes.c_void_p)) == -1
    assert L.spp_prove_withdraw_notes(None, None, 1, note, None, None, None, None) == -1
    assert L.spp_prove_withdraw_notes_device(None, None, 1, None, None, None, None, None) == -1
    assert "NULL" in spp.last_error()
