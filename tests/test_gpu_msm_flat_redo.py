"""The flat table walk with the same-x case out of its loop (k_msm_flat with madd_distinct, k_msm_flat_redo behind it) through the
unit entry spp_msm_flat_unit: one table row per base, 8-bit windows (32 passes, 128 entries per row), 130 bases (more than one
64-row block, more than one group of four prefetched digits per slice) and 1, 3 or 70 scalar rows (70 is padded to 128 lanes per
slice: two waves, the second partly filled).  Every row is compared with the CPU oracle's MSM over the same bases and scalars,
bit for bit; redo_lanes tells which kernel produced the sums."""
import random

import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None

from msm_group import Group

pytestmark = pytest.mark.gpu

N = 130
WINDOW = 8
GROUPS = (1, 2)
BATCHES = (1, 3, 70)


@pytest.fixture(scope="module")
def ctx():
    import spp
    c = spp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def groups():
    return {g: Group(g, N, WINDOW) for g in GROUPS}


def _edge_rows(B, rng, P):
    rows = []
    for p in range(P):
        row = [rng.randrange(B.R) for _ in range(N)]
        for k, v in enumerate((0, 1, B.R - 1, (B.R - 1) // 2, (B.R + 1) // 2, 255)):
            row[(7 * p + 11 * k) % N] = v       # the edge scalars meet other bases in every row
        rows.append(row)
    return rows


@pytest.mark.parametrize("P", BATCHES)
@pytest.mark.parametrize("group", GROUPS)
def test_distinct_bases_take_the_fast_walk(ctx, groups, group, P):
    """Random distinct bases, scalars with 0, 1, r-1, (r-1)/2, (r+1)/2 and 255 among them: the oracle's sums, and no lane walked
    again -- the fast walk produced them."""
    G = groups[group]
    rows = _edge_rows(G.B, random.Random(7 * group + P), P)
    assert G.check(ctx, G.raw(G.random_pts), rows, "distinct") == 0


@pytest.mark.parametrize("P", BATCHES)
@pytest.mark.parametrize("group", GROUPS)
def test_one_base_repeated_is_summed_by_the_redo_kernel(ctx, groups, group, P):
    """All bases equal g: every addition after a lane's first is a doubling.  Once with every scalar 5 (one pass has work), once
    with one full-size scalar shared by all bases (every pass has)."""
    G = groups[group]
    bases = G.raw([G.g] * N)
    full = random.Random(31 + group).randrange(G.B.R // 2, G.B.R)
    for what, s in (("same, scalar 5", 5), ("same, full-size scalar", full)):
        assert G.check(ctx, bases, [[s] * N for _ in range(P)], what) > 0


@pytest.mark.parametrize("P", BATCHES)
@pytest.mark.parametrize("group", GROUPS)
def test_cancelling_bases(ctx, groups, group, P):
    """g and -g alternate with scalar 77 (a lane's sum returns to infinity over and over), a last base `other` with scalar 3."""
    G = groups[group]
    pts = [G.g if i % 2 == 0 else G.neg(G.g) for i in range(N)]
    pts[-1] = G.other
    row = [77] * (N - 1) + [3]
    G.check(ctx, G.raw(pts), [list(row) for _ in range(P)], "cancel")


@pytest.mark.parametrize("group", GROUPS)
def test_marked_and_unmarked_lanes_share_a_wave(ctx, groups, group):
    """65 random bases, then 65 copies of g; 70 rows.  Even rows put 5 on every copy, odd rows 0.  Only (pass 0, even row) lanes can
    meet a doubling: at most 35 rows x 33 slices (a slice has at least 4 of the 130 bases), far below the 32 x slices x 70 lanes of
    the call; the odd rows alone need no redo.
    With full-size scalars on the random bases a lane reaches the copies with the sum of its random bases in the accumulator, so
    the second copy is no doubling and nothing is marked (measured: 0 lanes).  The second half therefore gives the random bases of
    the even rows scalars that are multiples of 2^8 below r/2 (digit 0 in pass 0): there the even lanes of a pass-0 wave add 5g to
    5g and leave the fast walk, while the odd lanes beside them walk their random digits to the end."""
    G = groups[group]
    P = 70
    bases = G.raw(G.random_pts[:65] + [G.g] * 65)
    rng = random.Random(57 + group)
    rows = [[rng.randrange(G.B.R) for _ in range(65)] + [5 if p % 2 == 0 else 0] * 65 for p in range(P)]
    assert G.check(ctx, bases, rows, "mixed") <= 35 * 33
    assert G.check(ctx, bases, rows[1::2], "mixed, odd rows alone") == 0
    for p in range(0, P, 2):
        rows[p][:65] = [rng.randrange(1 << 240) << 8 for _ in range(65)]
    assert 0 < G.check(ctx, bases, rows, "mixed, even rows idle in pass 0 before the copies") <= 35 * 33
    assert G.check(ctx, bases, rows[1::2], "mixed, odd rows alone") == 0


@pytest.mark.parametrize("P", BATCHES)
@pytest.mark.parametrize("group", GROUPS)
def test_bases_at_infinity_add_nothing(ctx, groups, group, P):
    """Zero bytes in place of every 7th base: the oracle's sum over the bases that are kept, whatever the scalars of the holes."""
    G = groups[group]
    raw = bytearray(G.raw(G.random_pts))
    holes = set(range(0, N, 7))
    for i in holes:
        raw[G.size * i:G.size * (i + 1)] = bytes(G.size)
    keep = [i for i in range(N) if i not in holes]
    kept_bases = b"".join(bytes(raw[G.size * i:G.size * (i + 1)]) for i in keep)
    rows = _edge_rows(G.B, random.Random(77 * group + P), P)
    assert G.check(ctx, bytes(raw), rows, "infinity bases", oracle_bases=kept_bases, keep=keep) == 0
