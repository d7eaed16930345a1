"""CPU: tests/pippenger_model.py held to what it says -- the recoding identity on the special, crafted and random scalars, the
closed-form oracle against orc_msm_g1 / orc_msm_g2 and a plain sum of scalar multiplications, every crafted case of
tests/test_gpu_pippenger_edges.py against the shape it claims under layout(), and bench_points against the generator written out
in 32-bit words, the way tests/test_gpu_parity.py carried it inline before it imported bench_points."""
import ctypes
import random

import pytest

import pippenger_model as M
from oracle import bn254 as O

R, HALF, W, C, B = M.R, M.HALF, M.W, M.C, M.B

CASES = {"g1": M.all_cases("g1"), "g2": M.all_cases("g2")}


def _ids(group):
    return ["%s-%s" % (f.__name__[5:], "-".join(str(a) for a in args[1:])) for f, args in CASES[group]]


def _check_recoding(s):
    dg, carry = M.digits_and_carry(s)
    assert len(dg) == W and carry == 0, hex(s)                        # the top window takes no carry
    assert all(-B <= d <= B - 1 for d in dg), (hex(s), dg)            # every digit is an int16
    total = sum(d << (C * j) for j, d in enumerate(dg))
    assert total == (s if s <= HALF else s - R), hex(s)               # ... and they say s, or s - r for a folded scalar
    assert abs(dg[W - 1]) <= M.TOP_MAX + 1


def test_recoding_identity_special_and_random_scalars():
    rng = random.Random(1)
    special = [0, 1, R - 1, (R - 1) // 2, (R + 1) // 2, 0x8000, 0x8001, 0xffff, R - 0x8000, R - 0x8001, R - 0xffff, 1 << 252]
    for s in special + [rng.randrange(R) for _ in range(1000)]:
        _check_recoding(s)
    # the rule for a window value of exactly 2^15: carries under a + fold, stays under a - fold; the stored digit is -2^15 in both
    for j in range(W - 1):
        assert M.digits(M.scalar_with({j: B}))[j:j + 2] == [-B, 1]
        assert M.digits(M.scalar_with({j: B}, True))[j:j + 2] == [-B, 0]
    assert M.TOP_MAX == 0x1832
    with pytest.raises(AssertionError):
        M.scalar_with({W - 1: M.TOP_MAX + 1})


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_recoding_identity_on_every_crafted_scalar(group):
    seen = set()
    for f, args in CASES[group]:
        seen.update(f(*args).scalars)
    assert len(seen) > 300
    for s in seen:
        _check_recoding(s)


def test_layout_counts_offsets_and_paths():
    """layout() on a list small enough to read: buckets of 1, 3073, 3329 and 2 entries in window 0 and one entry in window 2"""
    sc = [1] + [2] * 3073 + [R - 3] * 3329 + [7, R - 7] + [5 << 32]
    lay = M.layout(sc)
    w0 = lay[0]
    assert w0["total"] == 1 + 3073 + 3329 + 2 and w0["counts"] == {0: 1, 1: 3073, 2: 3329, 6: 2} and w0["offsets"] == {0: 0, 1: 1, 2: 3074, 6: 6403}
    b = w0["buckets"]
    assert (b[0]["s0"], b[0]["s1"], b[0]["path"]) == (0, 0, "direct")
    assert (b[1]["s0"], b[1]["s1"], b[1]["path"]) == (0, 12, "sequential")                # 12 segments past the first: the last sequential
    assert (b[2]["s0"], b[2]["s1"], b[2]["path"]) == (12, 25, "heavy")                    # 13: the first heavy
    assert b[6]["members"] == [(6403, False), (6404, True)] and b[6]["path"] == "direct" and b[6]["s0"] == b[6]["s1"] == 25
    assert b[2]["ends_on_boundary"] is False and M.layout([4] * 512)[0]["buckets"][3]["ends_on_boundary"] is True
    assert lay[2]["counts"] == {4: 1} and [lay[j]["total"] for j in range(W)] == [6405, 0, 1] + [0] * 13


def _small_instance(pl, rng, n):
    idx = [rng.randrange(len(pl)) for _ in range(n)]
    idx[:4] = [pl.INF_IDX, pl.P_IDX, pl.NEG_IDX, pl.WIDE_IDX]                             # infinity, P and -P, a 254-bit logarithm
    sc = [rng.randrange(R) for _ in range(n)]
    sc[1] = sc[2]                                                                         # s P + s (-P)
    sc[4:9] = [0, 1, R - 1, HALF, HALF + 1]
    return idx, sc


def test_closed_form_matches_the_g1_oracle_and_a_plain_sum():
    from oracle import native
    pl = M.pool("g1")
    assert len(pl) == 251 and pl.point_bytes(pl.INF_IDX) == b"\x00" * 64 and pl.logs[pl.INF_IDX] == 0
    assert O.g1_from_bytes(pl.point_bytes(pl.Q_IDX)) == O.g1_mul(O.g1_from_bytes(pl.point_bytes(pl.P_IDX)), 1 << 16)
    assert O.g1_from_bytes(pl.point_bytes(pl.NEG_IDX)) == O.g1_neg(O.g1_from_bytes(pl.point_bytes(pl.P_IDX)))
    assert O.g1_from_bytes(pl.point_bytes(pl.TWO_IDX)) == O.g1_mul(O.g1_from_bytes(pl.point_bytes(pl.P_IDX)), 2)
    rng = random.Random(2)
    for n in (0, 1, 9, 64):
        idx, sc = _small_instance(pl, rng, 64)
        idx, sc = idx[:n], sc[:n]
        bases = pl.bases(idx)
        out = ctypes.create_string_buffer(64)
        native.lib().orc_msm_g1(bases, b"".join(s.to_bytes(32, "big") for s in sc), n, ctypes.cast(out, ctypes.c_void_p))
        assert pl.expected(idx, sc) == out.raw, n
        acc = None
        for i, s in enumerate(sc):
            acc = O.g1_add(acc, O.g1_mul(O.g1_from_bytes(bases[64 * i:64 * i + 64]), s))
        assert pl.expected(idx, sc) == O.g1_to_bytes(acc), n
    assert pl.expected([pl.P_IDX, pl.NEG_IDX], [5, 5]) == b"\x00" * 64


def test_closed_form_matches_the_g2_oracle_and_a_plain_sum():
    from oracle import native
    pl = M.pool("g2")
    assert len(pl) == 16 and pl.point_bytes(pl.INF_IDX) == b"\x00" * 128
    assert O.g2_from_bytes(pl.point_bytes(pl.Q_IDX)) == O.g2_mul(O.g2_from_bytes(pl.point_bytes(pl.P_IDX)), 1 << 16)
    rng = random.Random(3)
    for n in (0, 1, 9, 64):
        idx, sc = _small_instance(pl, rng, 64)
        idx, sc = idx[:n], sc[:n]
        bases = pl.bases(idx)
        out = ctypes.create_string_buffer(128)
        native.lib().orc_msm_g2(bases, b"".join(s.to_bytes(32, "big") for s in sc), n, ctypes.cast(out, ctypes.c_void_p))
        assert pl.expected(idx, sc) == out.raw, n
        if n <= 9:
            acc = None
            for i, s in enumerate(sc):
                acc = O.g2_add(acc, O.g2_mul(O.g2_from_bytes(bases[128 * i:128 * i + 128]), s))
            assert pl.expected(idx, sc) == O.g2_to_bytes(acc), n


@pytest.mark.parametrize("k", range(len(CASES["g1"])), ids=_ids("g1"))
def test_g1_case_has_the_shape_it_claims(k, record_property):
    f, args = CASES["g1"][k]
    case = f(*args)
    assert case.claim, case.name                          # a case whose shape cannot be asserted does not go in
    record_property("shape", M.check_claim(args[0], case))


@pytest.mark.parametrize("k", range(len(CASES["g2"])), ids=_ids("g2"))
def test_g2_case_has_the_shape_it_claims(k, record_property):
    f, args = CASES["g2"][k]
    case = f(*args)
    assert case.claim, case.name
    record_property("shape", M.check_claim(args[0], case))


def test_crafted_cases_reach_the_edges_the_kernels_switch_at():
    """the shapes the segment cases are there for, said once more in the kernels' own numbers"""
    pl = M.pool("g1")
    want = {255: (0, "direct"), 256: (0, "direct"), 257: (1, "sequential"), 512: (1, "sequential"), 3073: (12, "sequential"),
            3329: (13, "heavy"), 16385: (64, "heavy"), 16641: (65, "heavy")}
    assert sorted(want) == sorted(M.SEGMENT_COUNTS)
    for c, (s1, path) in want.items():
        for w in (0, W - 1):
            got = M.case_segments(pl, c, w, "same").claim["buckets"][(w, 0)]
            assert (got["s0"], got["s1"], got["path"]) == (0, s1, path), (c, w)      # s1 - s0 head partials: 64, then 65
    for w in (0, 7):
        chunks = {b // M.CHUNK for b in M.weight_buckets(w)}
        assert {1 << k for k in range(11)} <= chunks and 2047 in chunks and 0 in chunks
    assert max(M.weight_buckets(W - 1)) + 1 <= M.TOP_MAX and {1 << k for k in range(9)} <= {b // M.CHUNK for b in M.weight_buckets(W - 1)}
    # the digit-edge launch holds every edge value in every window under both fold signs
    case = M.case_digit_edges(pl)
    assert len(case.scalars) == 300
    for j in range(W - 1):
        for v in M.EDGE_VALUES:
            assert M.scalar_with({j: v}) in case.scalars and M.scalar_with({j: v}, True) in case.scalars
    assert any(d[W - 1] == M.TOP_MAX and d[0] == -1 for d in case.claim["digits"].values())      # a carry chain into the top window
    assert any(d[:W - 1] == [-B] * (W - 1) for d in case.claim["digits"].values())                # 0x8000 everywhere, - fold
    assert any(d[9] == -B for d in case.claim["digits"].values())


def test_bench_points_reproduces_the_inline_generator():
    """the generator in 32-bit words as spp_msm_g1_pippenger_bench_shard fills them, which is how tests/test_gpu_parity.py wrote it
    out twice before it imported bench_points (seed 9; small_permille 0 and 700), first 64 points"""
    rinv = pow(1 << 256, -1, R)
    for permille in (0, 700):
        x = (9 * 6364136223846793005 + 1442695040888963407) % (1 << 64)

        def nxt():
            nonlocal x
            x = (x * 6364136223846793005 + 1442695040888963407) % (1 << 64)
            return x
        want = []
        for _ in range(64):
            k = nxt() | 1
            w = []
            for _ in range(4):
                v = nxt()
                w += [v & 0xffffffff, v >> 32]
            w[7] &= 0x1fffffff
            if permille and (nxt() >> 20) % 1000 < permille:
                want.append((k, w[0] & 0xff))
            else:
                want.append((k, sum(l << (32 * i) for i, l in enumerate(w)) * rinv % R))
        assert M.bench_points(64, 9, permille) == want
        assert M.bench_points(8, 9, permille, first=56) == want[56:]                  # the jump over the points before `first`
        assert M.bench_log(64, 9, permille) == sum(k * s for k, s in want) % R
        assert M.bench_log(8, 9, permille, first=56) == sum(k * s for k, s in want[56:]) % R
    assert sum(1 for _, s in M.bench_points(64, 9, 700) if s < 256) > 30
    assert M.lcg_jump(5, 0) == 5 and M.lcg_jump(5, 1) == (5 * M.LCG_A + M.LCG_C) & M.M64
