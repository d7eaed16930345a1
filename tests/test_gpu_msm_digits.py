"""GPU: the signed-digit planes of the table walks on their own (k_msm_digits through spp_debug_msm_digits), entry by entry against
the reference recoding of tests/msm_digit_vectors.py, at every window width 4..16.

Through a group sum a wrong plane can cancel, and the walks only ever pass rows[i] = i.  Here the planes are read back as they
are: every scalar family of msm_digit_vectors plus 200 random scalars in every proof column, batches of 1, 63, 64 and 65 proofs
(the padding rule of the plane rows switches between 63, 64 and 65), a row indirection that is a non-identity permutation with
repeats, and more scalar rows than bases.  Entries of the padding (p >= P) are unspecified and not looked at."""
import ctypes
import random

import numpy as np
import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None

import msm_digit_vectors as D

pytestmark = pytest.mark.gpu

M = 280              # scalar rows
DISTINCT = 250       # of which the bases point at this many ...
REPEATS = 14         # ... and at some of them twice: N = 264 bases < M
BATCHES = (1, 63, 64, 65)


@pytest.fixture(scope="module")
def ctx():
    import spp
    c = spp.Context(0)
    yield c
    c.close()


def _rows(seed):
    """N row indices < M: DISTINCT distinct scalar rows in shuffled order, REPEATS of them a second time, shuffled again."""
    rng = random.Random(seed)
    used = rng.sample(range(M), DISTINCT)
    rows = used + rng.sample(used, REPEATS)
    rng.shuffle(rows)
    assert rows != sorted(rows) and len(set(rows)) == DISTINCT < len(rows) < M
    return used, rows


@pytest.mark.parametrize("c", D.WIDTHS)
def test_planes_match_the_reference(ctx, c):
    pool = [s for members in D.families(c).values() for s in members] + D.random_scalars(200, 4242)
    assert len(pool) <= DISTINCT
    table = np.array([D.digits(s, c) for s in pool], dtype=np.int64)          # [pool index][window]
    assert table.min() >= -(1 << (c - 1)) and table.max() <= (1 << (c - 1)) - 1
    W = D.windows(c)
    used, rows = _rows(1000 + c)
    slot = {m: k for k, m in enumerate(used)}                                  # scalar row -> position among the used rows
    for P in BATCHES:
        # pool index of (scalar row m, proof p): a used row walks through the pool with the proof index, so that every proof column
        # holds the whole pool; rows no base points at hold other values, which must not show anywhere
        which = np.empty((M, P), dtype=np.int64)
        for m in range(M):
            for p in range(P):
                which[m, p] = (slot[m] + 37 * p) % len(pool) if m in slot else (m + p) % len(pool)
        for p in range(P):
            assert len(set(which[used, p].tolist())) == len(pool)
        planes, Pp = ctx.debug_msm_digits([[pool[k] for k in which[m]] for m in range(M)], rows, c)
        assert Pp == D.padded_batch(P), (c, P, Pp)
        assert planes.shape == (W, len(rows), Pp) and planes.dtype == np.int16
        exp = table[which[rows, :]].transpose(2, 0, 1)                         # [window][base][proof]
        got = planes[:, :, :P].astype(np.int64)
        bad = np.argwhere(got != exp)
        assert bad.size == 0, "c=%d P=%d: %d entries differ; first (window, base, proof) = %s: device %d, reference %d, scalar %#x" % (
            c, P, len(bad), tuple(bad[0]), got[tuple(bad[0])], exp[tuple(bad[0])], pool[which[rows[bad[0][1]], bad[0][2]]])


def test_entry_refuses_bad_arguments(ctx):
    import spp
    from spp.lib import SPP_ERR_BAD_INPUT
    L = ctx.L
    sc = b"".join(int(s).to_bytes(32, "big") for s in (1, 2, 3, 4, 5, 6))     # M = 3, P = 2
    rows = np.array([2, 0], dtype=np.uint32)
    bad_rows = np.array([2, 3], dtype=np.uint32)
    W = D.windows(8)
    buf = np.zeros(W * 2 * 2, dtype=np.int16)
    pr, pbad, pb = (a.ctypes.data_as(ctypes.c_void_p) for a in (rows, bad_rows, buf))
    pp = ctypes.c_uint32(0)
    assert L.spp_debug_msm_digits(ctx.h, sc, 3, 2, pr, 2, 8, pb, buf.size, ctypes.byref(pp)) == 0
    assert pp.value == 2 and buf.reshape(W, 2, 2)[0].tolist() == [[5, 6], [1, 2]] and not buf.reshape(W, 2, 2)[1:].any()
    for args in ((None, sc, 3, 2, pr, 2, 8, pb, buf.size, ctypes.byref(pp)), (ctx.h, None, 3, 2, pr, 2, 8, pb, buf.size, ctypes.byref(pp)),
                 (ctx.h, sc, 3, 2, None, 2, 8, pb, buf.size, ctypes.byref(pp)), (ctx.h, sc, 3, 2, pr, 2, 8, None, buf.size, ctypes.byref(pp)),
                 (ctx.h, sc, 3, 2, pr, 2, 8, pb, buf.size, None),
                 (ctx.h, sc, 3, 2, pr, 2, 3, pb, buf.size, ctypes.byref(pp)), (ctx.h, sc, 3, 2, pr, 2, 17, pb, buf.size, ctypes.byref(pp)),
                 (ctx.h, sc, 3, 2, pr, 2, 0, pb, buf.size, ctypes.byref(pp)),           # no default width here
                 (ctx.h, sc, 0, 2, pr, 2, 8, pb, buf.size, ctypes.byref(pp)), (ctx.h, sc, 3, 0, pr, 2, 8, pb, buf.size, ctypes.byref(pp)),
                 (ctx.h, sc, 3, 2, pr, 0, 8, pb, buf.size, ctypes.byref(pp)),
                 (ctx.h, sc, 3, 2, pbad, 2, 8, pb, buf.size, ctypes.byref(pp)),         # a row index that is no scalar row
                 (ctx.h, sc, 3, 2, pr, 2, 8, pb, buf.size - 1, ctypes.byref(pp)),       # a buffer one digit short
                 (ctx.h, sc, 3, 2, pr, 2, 4, pb, buf.size, ctypes.byref(pp))):          # 64 windows do not fit it either
        assert L.spp_debug_msm_digits(*args) == SPP_ERR_BAD_INPUT, args[2:9]
        assert spp.last_error()
