"""Points, bytes and the oracle of one group, shared by the unit tests of the table walks (test_gpu_msm_flat_redo.py,
test_gpu_msm_windows.py): distinct random bases, two fixed points, and the CPU oracle's MSM with its sums cached per
(bases, scalar row) -- a row that several window widths or batch sizes share is summed by the oracle once."""
import ctypes
import random


class Group:
    """Points, bytes and the oracle of one group; the oracle's sum of a (bases, scalar row) pair is computed once."""

    def __init__(self, group, n=130, window=8):
        from oracle import bn254 as B, native
        self.B, self.group, self.size, self.window = B, group, 64 if group == 1 else 128, window
        rng = random.Random(100 + group)
        if group == 1:
            self.gen, self.add, self.mul, self.to_bytes = B.G1_GEN, B.g1_add, B.g1_mul, B.g1_to_bytes
            self.neg = lambda q: (q[0], (B.P - q[1]) % B.P)
            self.orc = native.lib().orc_msm_g1
        else:
            self.gen, self.add, self.mul, self.to_bytes = B.G2_GEN, B.g2_add, B.g2_mul, B.g2_to_bytes
            self.neg = B.g2_neg
            self.orc = native.lib().orc_msm_g2
        pts, p = [], self.gen
        for _ in range(n):
            p = self.add(p, self.mul(self.gen, rng.randrange(1, 1 << 64)))
            pts.append(p)
        self.random_pts = pts
        self.g = self.mul(self.gen, 0x1234567)
        self.other = self.mul(self.gen, 99)
        self.cache = {}

    def raw(self, pts):
        return b"".join(self.to_bytes(q) for q in pts)

    def oracle(self, bases, row):
        key = (bases, tuple(row))
        if key not in self.cache:
            out = ctypes.create_string_buffer(self.size)
            self.orc(bases, b"".join(int(s).to_bytes(32, "big") for s in row), len(row), ctypes.cast(out, ctypes.c_void_p))
            self.cache[key] = out.raw
        return self.cache[key]

    def check(self, ctx, bases, rows, what, oracle_bases=None, keep=None, window=None):
        """The flat walk (spp_msm_flat_unit) of every row against the oracle; returns the lanes the redo kernel walked again."""
        window = self.window if window is None else window
        got, redo = ctx.msm_flat(self.group, bases, rows, window)
        print("%s G%d c=%d P=%d: redo_lanes %d" % (what, self.group, window, len(rows), redo))
        for p, row in enumerate(rows):
            exp = self.oracle(bases, row) if keep is None else self.oracle(oracle_bases, [row[i] for i in keep])
            assert got[p] == exp, (what, self.group, window, len(rows), p)
        return redo

    def check_rows_walk(self, ctx, bases, row, what, window):
        """The row-per-window walk (spp_msm_g1 / spp_msm_g2, one proof) against the oracle."""
        got = (ctx.msm_g1 if self.group == 1 else ctx.msm_g2)(bases, row, window)
        assert got == self.oracle(bases, row), (what, self.group, window, len(row))
