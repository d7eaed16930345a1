"""The crafted circuits of tests/derive_circuits.py without a GPU: every generator has the properties it claims, recomputed here from
desc.A / B / C with the gather's constants restated; the two Python restatements of the derivation agree on them (the oracle's seeded
setup brought to gamma = delta = 1 against ptau_format.derived_key); and csrc/ptau.hpp's column gather on the host, over Fq (mode
gather) and over Fq2 (mode gather2, the instance the G2 kernel compiles), through tests/host/ec_ntt_check.cpp on every kind of
coefficient and on a column whose two chunks cancel, against oracle/bn254.py big integers."""
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shielded-pool-pinocchio-solana_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tests"))

PT_GATHER_CHUNK = 16
WAVE = 64


def _read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def crafted():
    import derive_circuits as D
    return {name: gen() for name, gen in D.GENERATORS.items()}


# --------------------------------------------------------------------------------------------------------------------------
# the generators sit on their edges
# --------------------------------------------------------------------------------------------------------------------------
def _column(desc, matrix, wire):
    """the (row, coefficient) terms of a wire's column in the order the library lists them"""
    return [(k, v) for k, terms in enumerate(getattr(desc, matrix)) for w, v in terms if w == wire]


def _k_column(desc, wire):
    return [t for m in "ABC" for t in _column(desc, m, wire)]


def _chunks(terms):
    return (len(terms) + PT_GATHER_CHUNK - 1) // PT_GATHER_CHUNK


def _bit_length(c):
    from oracle.bn254 import R
    return min(c % R, R - c % R).bit_length()


def _sum_by_row(terms):
    from oracle.bn254 import R
    out = {}
    for k, v in terms:
        out[k] = (out.get(k, 0) + v) % R
    return out


@pytest.mark.parametrize("name", ["coeff_kinds", "column_shapes", "meetings", "smallest"])
def test_expect_is_what_the_matrices_hold(crafted, name):
    g = crafted[name]
    d, e = g.desc, g.expect
    W = d.n_wires
    assert len(d.A) == len(d.B) == len(d.C) == d.n_constraints <= 1 << d.domain_log and d.n_constraints > (1 << d.domain_log) // 2
    assert all(0 <= w < W for m in (d.A, d.B, d.C) for terms in m for w, _ in terms)
    assert d.domain_log <= 7 and W <= 160 and e["domain_log"] == d.domain_log and e["n_wires"] == W
    # the vk's K, the private K, CB and CS all carry wires of the circuit
    assert d.n_public >= 2 and d.n_public <= d.challenge_wire < W and d.committed and all(d.n_public <= w < W for w in d.committed)
    assert d.challenge_wire not in d.committed and len(d.committed) + d.n_public + 1 < W
    for w in list(range(d.n_public)) + [d.challenge_wire] + d.committed:
        assert _k_column(d, w), w
    for m in "ABC":
        assert e["col_len"][m] == [len(_column(d, m, w)) for w in range(W)]
    assert e["k_len"] == [len(_k_column(d, w)) for w in range(W)]
    assert e["chunks_g1"] == sum(_chunks(_column(d, "A", w)) + _chunks(_column(d, "B", w)) + _chunks(_k_column(d, w)) for w in range(W))
    assert e["chunks_g2"] == sum(_chunks(_column(d, "B", w)) for w in range(W))
    assert e["max_col"] == max(e["k_len"]) and e["max_col_chunks"] == max(_chunks(_k_column(d, w)) for w in range(W))
    assert e["bit_lengths"] == {_bit_length(v) for m in (d.A, d.B, d.C) for terms in m for _, v in terms}
    assert d.program[-1] == 0 and len(d.program) == 1


def test_coeff_kinds_has_every_kind_in_every_matrix(crafted):
    import derive_circuits as D
    from oracle.bn254 import R
    g = crafted["coeff_kinds"]
    ks = D.coefficient_kinds()
    want = [0, 1, R - 1, 2, R - 2, 3, (1 << 28) - 1, (R - 1) // 2, (R + 1) // 2, R - (1 << 32), R - ((1 << 32) - 1)]
    for k in range(1, 8):
        want += [1 << (32 * k - 1), (1 << (32 * k)) - 1, 1 << (32 * k)]
    assert set(want) <= set(ks) and len(ks) == len(set(ks)) == len(want) + 2 == g.desc.n_wires
    assert all(_bit_length(c) > 250 for c in ks[-2:])                       # the two random ones are full-size
    assert {32 * k for k in range(1, 8)} | {32 * k + 1 for k in range(1, 8)} | {0, 1, 2, 28, 253} <= g.expect["bit_lengths"]
    assert _bit_length((R + 1) // 2) == _bit_length((R - 1) // 2) == 253 and _bit_length(R - (1 << 32)) == 33 and _bit_length(R - ((1 << 32) - 1)) == 32
    rows = set()
    for i, c in enumerate(ks):
        cols = [_column(g.desc, m, i) for m in "ABC"]
        assert all(len(col) == 1 and col[0][1] == c for col in cols), i
        assert len({col[0][0] for col in cols}) == 3                        # on three different rows
        rows |= {col[0][0] for col in cols}
    assert rows == set(range(g.desc.n_constraints))                         # spread over the whole domain
    assert g.expect["vanish"] == {"A": [0], "B": [0], "K": [0], "K_equal": [], "K_opposite": []}     # the stored zero alone


def test_column_shapes_lengths_and_chunk_counts(crafted):
    import derive_circuits as D
    g = crafted["column_shapes"]
    d, e = g.desc, g.expect
    assert d.domain_log == 7 and d.n_constraints > 64
    assert D.SHAPE_LENGTHS == (0, 1, 15, 16, 17, 32, 33)
    for t in D.SHAPE_LENGTHS:
        w = g.wire["len_%d" % t]
        for m in "ABC":
            col = _column(d, m, w)
            assert len(col) == t and len({k for k, _ in col}) == t, (t, m)
    assert not any(w == g.wire["len_0"] for m in (d.A, d.B, d.C) for terms in m for w, _ in terms)
    for t in (15, 16, 17):
        assert len(_k_column(d, g.wire["k_len_%d" % t])) == t
    long = g.wire["long"]
    for m in "AB":
        col = _column(d, m, long)
        assert len(col) >= PT_GATHER_CHUNK * WAVE + 1 and _chunks(col) > WAVE               # more than a wave of partials for one column
        sizes = sorted(_bit_length(v) for _, v in col)
        assert sizes[len(sizes) // 2] <= 32 and 3 <= sum(1 for s in sizes if s > 150) <= 32   # mostly short loops, a few full-size
        assert len(col) > len(set(col))                                                     # (wire, c) repeats inside rows
    for count in (e["chunks_g1"], e["chunks_g2"]):
        assert count > WAVE and count % WAVE
    assert (3 * d.n_wires) % WAVE and d.n_wires % WAVE and d.n_wires > WAVE          # the G2 combine step runs two workgroups too ...
    assert all(g.wire[name] >= WAVE for name in g.wire if name.startswith(("len_", "k_len_")))   # ... and meets these in the second
    assert e["max_col"] == 2 * (PT_GATHER_CHUNK * WAVE + 1) and e["max_col_chunks"] == 2 * WAVE + 1


def test_meetings_columns_meet_as_named(crafted):
    from oracle.bn254 import R
    g = crafted["meetings"]
    d, w = g.desc, g.wire
    for name in ("twice_1", "twice_minus_1", "twice_5", "twice_big"):
        for m in "AB":
            col = _column(d, m, w[name])
            assert len(col) == 2 and col[0] == col[1], name
    assert _column(d, "A", w["twice_1"])[0][1] == 1 and _column(d, "A", w["twice_minus_1"])[0][1] == R - 1
    assert _bit_length(_column(d, "A", w["twice_5"])[0][1]) > 1 and _bit_length(_column(d, "A", w["twice_big"])[0][1]) > 250
    for name in ("ab_1", "ab_6", "ab_big", "ab_1_committed", "ab_1_then", "ab_big_then"):
        col = _k_column(d, w[name])
        assert col[0] == col[1] == _column(d, "A", w[name])[0] == _column(d, "B", w[name])[0], name
        assert len(col) == (3 if name.endswith("_then") else 2)
        assert not name.endswith("_then") or col[2][1] != 0
    a, b = _column(d, "A", w["ab_opposite_6"]), _column(d, "B", w["ab_opposite_6"])
    assert len(a) == len(b) == 1 and a[0][0] == b[0][0] and (a[0][1] + b[0][1]) % R == 0 and not _column(d, "C", w["ab_opposite_6"])
    for m in "AB":
        col = _column(d, m, w["chunks_cancel"])
        first, second = col[:PT_GATHER_CHUNK], col[PT_GATHER_CHUNK:]
        assert len(col) == 2 * PT_GATHER_CHUNK and second == [(k, (R - v) % R) for k, v in first]
        assert _sum_by_row(first) != {first[0][0]: 0} and {1, 32, 33} <= {_bit_length(v) for _, v in first} and max(_bit_length(v) for _, v in first) > 250
    col = _k_column(d, w["k_chunks"])
    assert len(col) == 2 * PT_GATHER_CHUNK and col[:PT_GATHER_CHUNK] == col[PT_GATHER_CHUNK:] == _column(d, "A", w["k_chunks"]) == _column(d, "B", w["k_chunks"])
    assert len({k for k, _ in col}) == PT_GATHER_CHUNK
    for name in ("cancel_1", "cancel_big", "cancel_1_then", "cancel_9_then"):
        for m in "AB":
            col = _column(d, m, w[name])
            assert col[0][0] == col[1][0] and (col[0][1] + col[1][1]) % R == 0 and len(col) == (3 if name.endswith("_then") else 2), name
    named = lambda names: sorted(w[x] for x in names)
    gone = named(["chunks_cancel", "cancel_1", "cancel_big"])
    assert g.expect["vanish"]["A"] == g.expect["vanish"]["B"] == g.expect["vanish"]["K"] == gone
    assert g.expect["vanish"]["K_equal"] == named(["ab_opposite_6"])
    assert g.expect["vanish"]["K_opposite"] == named(["twice_1", "twice_minus_1", "twice_5", "twice_big", "ab_1", "ab_6", "ab_big", "ab_1_committed", "k_chunks"])
    assert w["ab_1_committed"] in d.committed and w["twice_5"] == d.challenge_wire     # these keep a place, with the point at infinity


def test_smallest_is_the_smallest_domain(crafted):
    d = crafted["smallest"].desc
    assert d.n_constraints == 2 and d.domain_log == 1


@pytest.mark.parametrize("secrets", ["generic", "equal", "opposite", "opposite_swapped"])
def test_wires_vanish_from_the_expected_key_as_the_model_says(crafted, secrets):
    import derive_circuits as D
    import ptau_format as F
    import sppk_format as S
    from oracle.bn254 import R
    g = crafted["meetings"]
    d, v = g.desc, g.expect["vanish"]
    alpha, beta = {"generic": (D.ALPHA, D.BETA), "equal": (D.ALPHA, D.ALPHA), "opposite": (1, R - 1), "opposite_swapped": (R - 1, 1)}[secrets]
    key = S.Sppk(F.derived_key(d, D.TAU, alpha, beta)[0])
    every = set(range(d.n_wires))
    present = lambda m: {w for w in every if _column(d, m, w)}
    assert set(key.wires["A"]) == present("A") - set(v["A"]) and set(key.wires["B1"]) == set(key.wires["B2"]) == present("B") - set(v["B"])
    gone = set(v["K"]) | set({"equal": v["K_equal"], "opposite": v["K_opposite"], "opposite_swapped": v["K_opposite"]}.get(secrets, []))
    private = every - set(range(d.n_public)) - {d.challenge_wire} - set(d.committed)
    assert set(key.wires["K"]) == private - gone
    assert gone & private and (secrets == "generic" or len(gone & private) > len(set(v["K"]) & private))
    for w, p in zip(key.wires["CB"], key.points["CB"]):                       # a committed wire keeps its place, with infinity
        assert (p == bytes(64)) == (w in gone), w


# --------------------------------------------------------------------------------------------------------------------------
# the two restatements of the derivation agree on the crafted circuits
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["coeff_kinds", "meetings"])
def test_seeded_setup_of_the_oracle_gives_the_derived_key(crafted, tmp_path, name):
    import ptau_format as F
    import synth_circuits as S
    import verify_vectors as V
    from oracle import native
    seed = b"\x07" * 32
    sppc, ref_pk, ref_vk = (str(tmp_path / n) for n in ("c.sppc", "ref.pk", "ref.vk"))
    S.write_sppc(crafted[name].desc, sppc)
    tau, alpha, beta, gamma, delta, _, _ = V.trapdoor(seed)
    native.setup(sppc, seed, ref_pk, ref_vk)
    assert F.derived_from_reference(_read(ref_pk), _read(ref_vk), gamma, delta) == F.derived_key(crafted[name].desc, tau, alpha, beta)


# --------------------------------------------------------------------------------------------------------------------------
# csrc/ptau.hpp's gather on the host, in G1 and in G2
# --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("derive") / "ec_ntt_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "ec_ntt_check.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("mode", ["gather", "gather2"])
def test_gather_on_every_coefficient_kind_and_cancelling_chunks(check_exe, tmp_path, mode):
    """column 0: every kind once, three chunks; columns 1 .. K: one kind each, so that a wrong kind is named; then a column of two
    full chunks on distinct rows, the second the first negated (the combine step adds P and -P), the same with the second chunk
    equal (it doubles), and one whose second chunk is followed by a third"""
    import derive_circuits as D
    from oracle import bn254 as O
    g1 = mode == "gather"
    gen, add, mul, enc = (O.G1_GEN, O.g1_add, O.g1_mul, O.g1_to_bytes) if g1 else (O.G2_GEN, O.g2_add, O.g2_mul, O.g2_to_bytes)
    rng = random.Random(46)
    R, chunk = O.R, PT_GATHER_CHUNK
    ks = D.coefficient_kinds()
    bases = [mul(gen, rng.randrange(1, R)) for _ in range(4)] + [None]
    coeffs = ks + [(R - c) % R for c in ks]                                    # index len(ks) + i: the negative of kind i
    entries = [(0, i % 4, i) for i in range(len(ks))] + [(1 + i, (i + 1) % 4, i) for i in range(len(ks))]
    pair = [(rng.randrange(5), rng.choice([1, 2, 5, 8, 9, 12, 13, 28, 30, 31, 32])) for _ in range(chunk)]   # (row, kind): 1, -1, 2^32, full-size ...
    c0 = 1 + len(ks)
    entries += [(c0, r, i) for r, i in pair] + [(c0, r, len(ks) + i) for r, i in pair]
    entries += [(c0 + 1, r, i) for r, i in pair] + [(c0 + 1, r, i) for r, i in pair]
    entries += [(c0 + 2, r, i) for r, i in pair] + [(c0 + 2, r, len(ks) + i) for r, i in pair] + [(c0 + 2, 2, 3)]
    ncols = c0 + 3
    lines = ["%d %d %d %d" % (len(bases), len(coeffs), ncols, len(entries))] + [enc(b).hex() for b in bases]
    lines += ["%064x" % c for c in coeffs] + ["%d %d %d" % e for e in entries]
    path = tmp_path / "gather.txt"
    path.write_text("\n".join(lines) + "\n")
    proc = subprocess.run([check_exe, mode, str(path)], capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    got = proc.stdout.strip().splitlines()
    head = got[0].split(" | ")
    assert head[0] == "PLAN 1"
    col_ptr = [int(v) for v in head[3].split()]
    assert [col_ptr[j + 1] - col_ptr[j] for j in range(ncols)] == [3] + [1] * len(ks) + [2, 2, 3]
    product = {}
    wrong = []
    for j in range(ncols):
        want = None
        for col, r, i in entries:
            if col == j:
                if (r, i) not in product:
                    product[(r, i)] = mul(bases[r], coeffs[i]) if bases[r] is not None and coeffs[i] else None
                want = add(want, product[(r, i)])
        if got[1 + j] != "COL " + enc(want).hex():
            wrong.append(j)
    assert not wrong, "columns %s (column 1 + i holds kind i alone: %s)" % (wrong, ["%x" % ks[j - 1] for j in wrong if 1 <= j <= len(ks)])
    assert got[1 + c0] == "COL " + "00" * (64 if g1 else 128)
