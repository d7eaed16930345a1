"""GPU: the general-base Pippenger MSM (csrc/kernels_pippenger.hip, spp_msm_g1_pippenger / spp_msm_g2_pippenger and the synthetic
spp_msm_g1_pippenger_bench calls) on crafted digits, buckets, segment shapes and sizes, against the closed-form oracle of
tests/pippenger_model.py: every base is k_j G with k_j known, so the expected sum is ONE scalar multiplication by
sum_i k_idx(i) s_i mod r, at any n.  Byte equality throughout.  tests/test_pippenger_model_host.py holds every case built here to
the shape it claims (the bucket spans exactly 13 segments, this digit is -2^15 in window 9, ...) and the closed form to the oracle."""
import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None

import pippenger_model as M

pytestmark = pytest.mark.gpu

W = M.W


@pytest.fixture(scope="module")
def ctx():
    import spp
    c = spp.Context(0)
    yield c
    c.close()


def _run(ctx, group, case):
    pl = M.pool(group)
    msm = ctx.msm_g1_pippenger if group == "g1" else ctx.msm_g2_pippenger
    got = msm(pl.bases(case.idx), case.scalars)
    want = pl.expected(case.idx, case.scalars)
    assert got == want, case.name
    return got


# ------------------------------------------------------------------------------------------------------------------------ G1
def test_g1_digit_edges(ctx):
    """every edge value in every window under both fold signs, 0xffff runs, 0x8000 everywhere, carry chains into the top window"""
    _run(ctx, "g1", M.case_digit_edges(M.pool("g1")))


@pytest.mark.parametrize("window", [0, 7, 15])
def test_g1_bucket_weights(ctx, window):
    """one point per bucket at every single-bit chunk number, chunk 2047 and the places around a chunk's edge"""
    _run(ctx, "g1", M.case_bucket_weights(M.pool("g1"), window))


@pytest.mark.parametrize("opposite", [False, True], ids=["equal", "opposite"])
def test_g1_equal_and_opposite_chunk_sums(ctx, opposite):
    """the same base in buckets b and b + 16 2^k, k = 0..10: equal (or opposite) partial sums in the trees of k_pip_bits"""
    pl = M.pool("g1")
    for k in range(11):
        got = _run(ctx, "g1", M.case_chunk_pair(pl, 7, k, opposite))
        assert got != b"\x00" * 64, k                                # (b + 1) P -+ (b2 + 1) P is never infinity: b2 != b
    _run(ctx, "g1", M.case_bucket_cancels(pl))


def test_g1_host_horner(ctx):
    """the accumulator equal to the next window sum; cancelling to infinity with lower windows to come; all scalars zero; only the
    top window occupied"""
    pl = M.pool("g1")
    _run(ctx, "g1", M.case_horner_equal(pl))
    _run(ctx, "g1", M.case_horner_cancel(pl))
    assert _run(ctx, "g1", M.case_all_zero(pl)) == b"\x00" * 64
    _run(ctx, "g1", M.case_top_window_only(pl))


@pytest.mark.parametrize("window", [0, 15])
@pytest.mark.parametrize("c", M.SEGMENT_COUNTS)
def test_g1_segment_shapes(ctx, c, window):
    """a bucket of c entries from offset 0 of the window's list and one of 300 behind it: one segment, the last sequential fix-up
    (12 segments past the first), the first heavy one (13), 64 and 65 head partials; random bases, one base throughout (equal
    partials), one base with half the signs turned (infinity)"""
    pl = M.pool("g1")
    for filling in M.SEGMENT_FILLINGS:
        _run(ctx, "g1", M.case_segments(pl, c, window, filling))


def test_g1_infinity_bases(ctx):
    pl = M.pool("g1")
    _run(ctx, "g1", M.case_infinity_bases(pl))
    assert _run(ctx, "g1", M.case_all_infinity(pl)) == b"\x00" * 64


@pytest.mark.parametrize("n", M.SORT_SIZES)
def test_g1_sort_piece_edges(ctx, monkeypatch, n):
    """n at, one below and one above the sizes of a level-2 piece, a level-1 piece and two level-1 pieces, in both sort forms"""
    case = M.case_sort_pieces(M.pool("g1"), n)
    packed = _run(ctx, "g1", case)
    monkeypatch.setenv("SPP_PIP_UNPACKED", "1")
    assert _run(ctx, "g1", case) == packed


_BENCH_LOGS = {}


def _bench_expected(n, seed, permille, first=0):
    key = (n, seed, permille, first)
    if key not in _BENCH_LOGS:
        _BENCH_LOGS[key] = M.log_to_g1_bytes(M.bench_log(n, seed, permille, first))
    return _BENCH_LOGS[key]


@pytest.mark.parametrize("permille", [0, 700])
def test_bench_generator_2p18_matches_closed_form(ctx, permille):
    n = 1 << 18
    assert ctx.msm_g1_pippenger_bench(n, seed=5, small_permille=permille)[0] == _bench_expected(n, 5, permille)


def test_bench_generator_two_counting_tiles(ctx):
    """2^20 + 3 points: a second counting tile, nearly empty"""
    n = (1 << 20) + 3
    assert ctx.msm_g1_pippenger_bench(n, seed=5, small_permille=700)[0] == _bench_expected(n, 5, 700)


def test_bench_generator_shard_across_the_tile_edge(ctx):
    n, first, count = (1 << 20) + 3, (1 << 20) - 5, 8
    assert ctx.msm_g1_pippenger_bench_shard(n, first, count, seed=5, small_permille=700)[0] == _bench_expected(count, 5, 700, first)


# ------------------------------------------------------------------------------------------------------------------------ G2
def test_g2_digit_edges(ctx):
    _run(ctx, "g2", M.case_digit_edges(M.pool("g2")))


def test_g2_host_horner(ctx):
    pl = M.pool("g2")
    _run(ctx, "g2", M.case_horner_equal(pl))
    _run(ctx, "g2", M.case_horner_cancel(pl))


@pytest.mark.parametrize("window", [0, 15])
@pytest.mark.parametrize("c", [257, 3073, 3329])
def test_g2_segment_shapes(ctx, c, window):
    pl = M.pool("g2")
    for filling in ("same", "half"):
        _run(ctx, "g2", M.case_segments(pl, c, window, filling))


def test_g2_infinity_bases(ctx):
    pl = M.pool("g2")
    _run(ctx, "g2", M.case_infinity_bases(pl))
    assert _run(ctx, "g2", M.case_all_infinity(pl)) == b"\x00" * 128
