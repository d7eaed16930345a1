"""GPU: both table walks on their own at every window width that ships, bit for bit against the CPU oracle's MSM.

The planner gives a flat set any width from 6 to 16, the commitment sets walk row-per-window tables at 9 bits and a circuit loads
at any width in 4..16; apart from this file those widths are reached through whole-proof comparisons only.  Here:

* the row-per-window walk (spp_msm_g1 / spp_msm_g2: k_msm_rows, one proof) at every width for G1 and at 5, 7, 9, 10, 11, 13, 15, 16
  for G2 -- the widths at which the last chunk of the rows of a base holds 1, 2, 4 rows or a full chunk, and 10, where the eighth
  chunk is empty (26 rows, 8 lanes per base, 4 rows each: it would start at row 28);
* the flat walk (spp_msm_flat_unit: k_msm_flat, its redo kernel, the radix-8 folds, k_msm_horner) at every width for G1 and at 6, 9,
  12, 13, 14, 15, 16 for G2, nine scalar rows per call (the per-lane fold, rows of 9 lanes: a wave straddles slices);
* the folds and the padding rule at the batch sizes where they switch (8 | 9: shuffle fold | per-lane fold; 63 | 64 | 65: Pp),
  over 300 bases: 75 slices, three fold levels (75 -> 10 -> 2 -> 1);
* a fold and Horner meeting their own point: a doubling and a cancellation in the additions behind the walk.

Scalars come from tests/msm_digit_vectors.py: per width the families that reach the recoder's edges (at 16 bits a digit fills
int16), and random rows that do not depend on the width, so the oracle sums them once."""
import random

import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None

import msm_digit_vectors as D
from msm_group import Group

pytestmark = pytest.mark.gpu

GROUPS = (1, 2)
N_FLAT = 130        # the flat walk: more than one 64-row block, 33 slices, two fold levels
N_FOLDS = 300       # 75 slices: three fold levels
ROWS_WIDTHS = {1: D.WIDTHS, 2: (5, 7, 9, 10, 11, 13, 15, 16)}
FLAT_WIDTHS = {1: D.WIDTHS, 2: (6, 9, 12, 13, 14, 15, 16)}
BOUNDARY_BATCHES = (8, 9, 63, 64, 65)


@pytest.fixture(scope="module")
def ctx():
    import spp
    c = spp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def groups():
    return {g: Group(g, N_FOLDS) for g in GROUPS}


def _pairs(table):
    return [(g, c) for g in GROUPS for c in table[g]]


def _members(c):
    return [s for m in D.families(c).values() for s in m]


# ---- the row-per-window walk --------------------------------------------------------------------------------------------

def rows_walk_bases(c):
    """2^(c-1) serial additions build a table row: 24 bases from 13 bits on (24 x 16 rows x 2^15 points at 16 bits), 150 below"""
    return 24 if c >= 13 else 150


@pytest.mark.parametrize("group,c", _pairs(ROWS_WIDTHS))
def test_row_per_window_walk(ctx, groups, group, c):
    """Every family member of the width and random scalars over distinct bases.  With 150 bases one call holds both (the 24
    family members at every 7th base); with 24 bases the families fill one call and the random scalars a second."""
    G = groups[group]
    n, members = rows_walk_bases(c), _members(c)
    bases = G.raw(G.random_pts[:n])
    rnd = D.random_scalars(n, 77)
    if n >= 150:
        row = list(rnd)
        for k, s in enumerate(members):
            row[7 * k % n] = s
        assert sorted(s for s in row if s in set(members)) == sorted(members)
        G.check_rows_walk(ctx, bases, row, "families among random", c)
    else:
        assert len(members) == n
        G.check_rows_walk(ctx, bases, members, "families", c)
        G.check_rows_walk(ctx, bases, rnd, "random", c)


# ---- the flat walk ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("group,c", _pairs(FLAT_WIDTHS))
def test_flat_walk(ctx, groups, group, c):
    """Nine rows, one call: every row is the oracle's sum, and no lane was walked again (the bases are distinct)."""
    G = groups[group]
    assert G.check(ctx, G.raw(G.random_pts[:N_FLAT]), D.flat_walk_rows(c, N_FLAT), "families", window=c) == 0


# ---- folds and batch boundaries -----------------------------------------------------------------------------------------

def boundary_rows(n, P):
    """the first P of 65 rows that do not depend on the batch size: random scalars, the 8-bit edges at other bases in every row"""
    return [D.with_edges(D.random_scalars(n, 9000 + p), 8, p) for p in range(P)]


@pytest.mark.parametrize("P", BOUNDARY_BATCHES)
@pytest.mark.parametrize("group", GROUPS)
def test_batch_boundaries_three_fold_levels(ctx, groups, group, P):
    """300 bases: 75 slices of four, folded 75 -> 10 -> 2 -> 1.  8 rows take the shuffle fold, 9 the per-lane fold; 63 and 64 rows
    keep their count as the plane and lane stride, 65 are padded to 128.  (msm_plan on the host: 75 slices for every case here but
    G2 at 65 rows, where two waves per slice at two waves per SIMD make 64 slices fill the last round best: 64 -> 8 -> 1.)"""
    G = groups[group]
    assert G.check(ctx, G.raw(G.random_pts[:N_FOLDS]), boundary_rows(N_FOLDS, P), "boundaries", window=8) == 0


@pytest.mark.parametrize("group", GROUPS)
def test_both_fold_paths_give_the_same_bytes(ctx, groups, group):
    """Row k of the 8-row call (shuffle fold) and row k of the 9-row call (per-lane fold) over the same scalars."""
    G = groups[group]
    bases = G.raw(G.random_pts[:N_FOLDS])
    rows = boundary_rows(N_FOLDS, 9)
    got8, _ = ctx.msm_flat(group, bases, rows[:8], 8)
    got9, _ = ctx.msm_flat(group, bases, rows, 8)
    assert got9[:8] == got8


@pytest.mark.parametrize("group", GROUPS)
def test_padded_batch_at_16_bits(ctx, groups, group):
    """65 rows (two waves per slice, the second with one live lane) where a digit fills int16"""
    G = groups[group]
    rows = [D.with_edges(D.random_scalars(N_FLAT, 9000 + p), 16, p) for p in range(65)]
    assert G.check(ctx, G.raw(G.random_pts[:N_FLAT]), rows, "65 rows", window=16) == 0


@pytest.mark.parametrize("P", (1, 9))
@pytest.mark.parametrize("c", (8, 16))
@pytest.mark.parametrize("group", GROUPS)
def test_fold_meets_its_own_point(ctx, groups, group, c, P):
    """Bases 0 and 1 are the same point g with the same full-size scalar, every other base is random with scalar 0.  Bases are
    dealt to slices in turn, so the two copies are summed by different lanes and meet in a fold (or, their pass sums being equal
    multiples, in Horner) -- redo_lanes == 0 proves that no walk saw the doubling.  Then base 1 = -g: every pass sum cancels and
    the result is the point at infinity, in the oracle's bytes."""
    G = groups[group]
    rng = random.Random(600 + 10 * c + P)
    rows = [[s, s] + [0] * (N_FLAT - 2) for s in (rng.randrange(G.B.R // 4, G.B.R) for _ in range(P))]
    rest = G.random_pts[:N_FLAT - 2]
    assert G.check(ctx, G.raw([G.g, G.g] + rest), rows, "fold doubles", window=c) == 0
    cancel = G.raw([G.g, G.neg(G.g)] + rest)
    assert G.check(ctx, cancel, rows, "fold cancels", window=c) == 0
    assert G.oracle(cancel, rows[0]) == G.to_bytes(None)


@pytest.mark.parametrize("c", (8, 13, 16))
@pytest.mark.parametrize("group", GROUPS)
def test_horner_meets_its_own_point(ctx, groups, group, c):
    """Base 0 = g, base 1 = 2^c g (computed here; to the device an ordinary distinct base), 64 more bases with scalar 0.  Scalars
    (2^c, 1): pass 1 holds g, pass 0 holds 2^c g, and after c doublings Horner's last addition is a doubling.  Scalars
    (2^c, r - 1): pass 0 holds -2^c g and the last addition cancels.  No walk adds more than one point: redo_lanes == 0."""
    G = groups[group]
    bases = G.raw([G.g, G.mul(G.g, 1 << c)] + G.random_pts[:64])
    rows = [[1 << c, 1] + [0] * 64, [1 << c, G.B.R - 1] + [0] * 64]
    assert G.check(ctx, bases, rows, "horner doubles, cancels", window=c) == 0
    assert G.oracle(bases, rows[0]) == G.to_bytes(G.mul(G.g, 1 << (c + 1)))
    assert G.oracle(bases, rows[1]) == G.to_bytes(None)
