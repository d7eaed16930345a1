"""The scalar families of tests/msm_digit_vectors.py hold what they are for -- conditions on the inputs of the GPU tests, checked by
the reference recoding alone, for every window width 4..16.  No device, no library."""
import pytest

import msm_digit_vectors as D


@pytest.mark.parametrize("c", D.WIDTHS)
def test_families_reconstruct_and_stay_in_range(c):
    """Every member of every family: W digits in [-2^(c-1), 2^(c-1) - 1] -- none equals +2^(c-1) -- whose weighted sum is the
    signed representative."""
    half, fam = 1 << (c - 1), D.families(c)
    assert tuple(fam) == D.FAMILIES
    for name, members in fam.items():
        assert members, name
        for s in members + D.random_scalars(50, c):
            assert 0 <= s < D.R, (name, s)
            d = D.digits(s, c)
            assert len(d) == D.windows(c)
            assert all(-half <= x <= half - 1 for x in d), (name, s, d)
            assert half not in d
            assert sum(x << (c * j) for j, x in enumerate(d)) == D.signed(s), (name, s)


@pytest.mark.parametrize("c", D.WIDTHS)
def test_edges_are_the_listed_values(c):
    half = 1 << (c - 1)
    assert D.families(c)["edges"] == [0, 1, D.R - 1, (D.R - 1) // 2, (D.R + 1) // 2, 255, half - 1, half, half + 1, 2 * half - 1, 2 * half]
    assert D.signed((D.R - 1) // 2) == (D.R - 1) // 2 and D.signed((D.R + 1) // 2) == -((D.R - 1) // 2) and D.signed(D.R - 1) == -1


@pytest.mark.parametrize("c", D.WIDTHS)
def test_chain_carries_through_every_window(c):
    """chain is 2^(c-1) in every window it has: window 0 recodes to -2^(c-1) with a carry, and the carry keeps every window above it
    off that value (exactly one such digit).  Its twin r - chain is -2^(c-1) in every one of those windows: W - 1 of them."""
    half, W = 1 << (c - 1), D.windows(c)
    chain, twin = D.families(c)["chain"]
    assert chain <= D.HALF_R < twin and twin == D.R - chain
    d, t = D.digits(chain, c), D.digits(twin, c)
    assert d[0] == -half and d.count(-half) == 1
    assert t.count(-half) == W - 1 and t[:W - 1] == [-half] * (W - 1) and t[W - 1] == 0


@pytest.mark.parametrize("c", D.WIDTHS)
def test_allmax_has_the_largest_positive_digit_everywhere(c):
    """2^(c-1) - 1 in every window: no carry at all, and the twin is the largest negative magnitude without one."""
    half = 1 << (c - 1)
    allmax, twin = D.families(c)["allmax"]
    d, t = D.digits(allmax, c), D.digits(twin, c)
    n = sum(1 for x in d if x)
    assert n >= D.windows(c) - 1 and d[:n] == [half - 1] * n
    assert t[:n] == [1 - half] * n and not any(t[n:])


@pytest.mark.parametrize("c", D.WIDTHS)
def test_toponly_and_carrytop(c):
    """toponly: one digit, in window jt.  carrytop = 2^(c jt) - 1: every lower window is full, so window 0 recodes to -1, the carry
    runs through zeros and the top digit +1 exists by carry alone; the twin mirrors it."""
    jt = D.top_window(c)
    assert jt in (D.windows(c) - 1, D.windows(c) - 2)
    top, ntop, high = D.families(c)["toponly"]
    assert D.digits(top, c) == [0] * jt + [1] + [0] * (D.windows(c) - jt - 1)
    assert D.digits(ntop, c) == [0] * jt + [-1] + [0] * (D.windows(c) - jt - 1)
    dh = D.digits(high, c)
    assert high <= D.HALF_R and not any(dh[:jt]) and dh[jt] != 0
    ct, nct = D.families(c)["carrytop"]
    d, t = D.digits(ct, c), D.digits(nct, c)
    assert d[0] == -1 and d[jt] == 1 and not any(d[1:jt]) and not any(d[jt + 1:])
    assert t[0] == 1 and t[jt] == -1 and not any(t[1:jt]) and not any(t[jt + 1:])


@pytest.mark.parametrize("c", D.WIDTHS)
def test_sparse_has_two_digits(c):
    jt = D.top_window(c)
    for s in D.families(c)["sparse"]:
        d = D.digits(s, c)
        assert [j for j, x in enumerate(d) if x] == [0, jt], (s, d)


@pytest.mark.parametrize("c", D.WIDTHS)
def test_flat_walk_rows_are_what_they_are_for(c):
    """Row 7 has no digit above window 0 (every pass above 0 sums to infinity: Horner starts from infinity and stays there until the
    last pass); row 8 has digits in windows 0 and jt only, of both signs (the passes between, and the top pass where jt is not the
    top window, are at infinity); row 0 holds every edge."""
    rows = D.flat_walk_rows(c, 130)
    assert len(rows) == 9 and all(len(r) == 130 for r in rows)
    assert all(0 <= s < D.R for r in rows for s in r)
    assert any(rows[7]) and all(not any(D.digits(s, c)[1:]) for s in rows[7])
    signs = set()
    for s in rows[8]:
        d = D.digits(s, c)
        assert [j for j, x in enumerate(d) if x] == [0, D.top_window(c)]
        signs.add(d[0] > 0)
    assert signs == {True, False}
    assert set(D.families(c)["edges"]) <= set(rows[0])
    for k, name in enumerate(D.FAMILIES):
        assert set(rows[1 + k]) == set(D.families(c)[name])


def test_the_whole_int16_range_is_reached_at_16_bits():
    """At c = 16 a digit fills int16: some family member has -32768 in its top non-zero window, and 32767 occurs as well."""
    tops, seen = [], set()
    for members in D.families(16).values():
        for s in members:
            d = D.digits(s, 16)
            seen.update(d)
            nz = [x for x in d if x]
            if nz:
                tops.append(nz[-1])
    assert -32768 in tops
    assert 32767 in seen and 32768 not in seen


def test_reference_against_a_plain_restatement():
    """The five-line reference against the schoolbook form of the same contract: unsigned c-bit windows of |v| with a carry whenever
    a window exceeds the range, the sign applied at the end -- for a negative v the excluded value flips side."""
    for c in D.WIDTHS:
        half = 1 << (c - 1)
        for s in [x for m in D.families(c).values() for x in m] + D.random_scalars(200, 1000 + c):
            v = D.signed(s)
            mag, neg, carry, out = abs(v), v < 0, 0, []
            for _ in range(D.windows(c)):
                d = (mag & ((1 << c) - 1)) + carry
                mag >>= c
                over = d > half if neg else d >= half
                carry = 1 if over else 0
                d = d - (1 << c) if over else d
                out.append(-d if neg else d)
            assert mag == 0 and carry == 0
            assert out == D.digits(s, c), (c, s)


def test_padded_batch():
    assert [D.padded_batch(P) for P in (1, 8, 9, 63, 64, 65, 128, 129)] == [1, 8, 9, 63, 64, 128, 128, 192]
