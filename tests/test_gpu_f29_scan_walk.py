"""The flat table walks with product-scanning Montgomery products (csrc/f29.hpp, MsmWalk<F>::product_form) at the window size of
the proving tables: spp_msm_flat_unit, G1 and G2, 16-bit windows (16 passes over one row of 2^15 entries per base), 70 bases (the
table crosses a 64-row block) and 65 scalar rows (padded to 128 lanes per slice: two waves, the second with one live lane).  These
are the smallest shapes at which a wrong carry between columns, a plan that does not fit the occupancy the kernel is built for, or a
broken redo marker can show.  Every row is compared with the CPU oracle's MSM over the same bases and scalars, bit for bit."""
import ctypes
import random

import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None

pytestmark = pytest.mark.gpu

N = 70
P = 65
WINDOW = 16
GROUPS = (1, 2)


@pytest.fixture(scope="module")
def ctx():
    import spp
    c = spp.Context(0)
    yield c
    c.close()


class Group:
    def __init__(self, group):
        from oracle import bn254 as B, native
        self.B, self.group, self.size = B, group, 64 if group == 1 else 128
        rng = random.Random(500 + group)
        if group == 1:
            gen, add, mul, self.to_bytes = B.G1_GEN, B.g1_add, B.g1_mul, B.g1_to_bytes
            self.orc = native.lib().orc_msm_g1
        else:
            gen, add, mul, self.to_bytes = B.G2_GEN, B.g2_add, B.g2_mul, B.g2_to_bytes
            self.orc = native.lib().orc_msm_g2
        pts, p = [], gen
        for _ in range(N):
            p = add(p, mul(gen, rng.randrange(1, 1 << 64)))
            pts.append(p)
        self.pts = pts
        self.g = mul(gen, 0x7654321)

    def raw(self, pts):
        return b"".join(self.to_bytes(q) for q in pts)

    def oracle(self, bases, row):
        out = ctypes.create_string_buffer(self.size)
        self.orc(bases, b"".join(int(s).to_bytes(32, "big") for s in row), len(row), ctypes.cast(out, ctypes.c_void_p))
        return out.raw

    def check(self, ctx, bases, rows, what):
        got, redo = ctx.msm_flat(self.group, bases, rows, WINDOW)
        print("%s G%d: redo_lanes %d" % (what, self.group, redo))
        for p, row in enumerate(rows):
            assert got[p] == self.oracle(bases, row), (what, self.group, p)
        return redo


@pytest.fixture(scope="module")
def groups():
    return {g: Group(g) for g in GROUPS}


@pytest.mark.parametrize("group", GROUPS)
def test_distinct_bases_at_16_bit_windows(ctx, groups, group):
    """Full-size random scalars with 0, 1, r-1, (r-1)/2 and (r+1)/2 among them in every row (each row puts them on other bases):
    the oracle's sums, and the fast walk alone produced them."""
    G = groups[group]
    rng = random.Random(11 * group)
    R = G.B.R
    rows = []
    for p in range(P):
        row = [rng.randrange(R) for _ in range(N)]
        for k, v in enumerate((0, 1, R - 1, (R - 1) // 2, (R + 1) // 2)):
            row[(7 * p + 13 * k) % N] = v
        rows.append(row)
    assert G.check(ctx, G.raw(G.pts), rows, "distinct, 16-bit") == 0


@pytest.mark.parametrize("group", GROUPS)
def test_one_base_repeated_at_16_bit_windows(ctx, groups, group):
    """Every base is g and every scalar of a row the same full-size value: each addition after a lane's first meets the accumulated
    point again, the lanes are marked, and the redo kernel's sums are the oracle's."""
    G = groups[group]
    rng = random.Random(23 * group)
    rows = [[rng.randrange(G.B.R // 2, G.B.R)] * N for _ in range(P)]
    assert G.check(ctx, G.raw([G.g] * N), rows, "one base repeated, 16-bit") > 0
