"""GPU: what hipcc makes of csrc/bn254.hpp, csrc/f29.hpp and csrc/gnark_hints.hpp for gfx950, function by function, on raw words
chosen to break it.

spp_debug_arith runs one header function per lane on the operand words as they are (no conversion, reduction or domain change on
either side); tests/arith_vectors.py supplies the words -- a fixed edge list per operation (limbs all ones, top limb 0 / 1 /
maximal, 2^k, p +- 2^k, operands at exactly the limb bounds the lazy forms state, k*p +- a bit for the zero tests, accumulator
scripts through the doubling and cancellation paths) plus 2000 seeded random cases -- and the predicate on every result, in Python
integers.  tests/test_arith_raw_host.py puts the same batches through the g++ build of the same dispatch, so a failure here
that does not show there is the device compile (as the 24-bit multiply behind Fp::hide24 was).

The groups of gnark_hints.hpp (the solver's wide integers and its three hints) also count the cases per branch class -- search
radius and ring position of the scalar decomposition, sign of its quotients and of the carries, the ladder's equal-point steps --
and every class must hold a case: the solver's own inputs (tests/test_acir_ccs.py) reach two of the sixteen decomposition classes."""
import ctypes

import pytest
try:
    import torch  # noqa: F401  (before libspp: both must share ONE HIP runtime; torch's has to be loaded first)
except Exception:  # pragma: no cover
    torch = None

import arith_vectors as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import spp
    c = spp.Context(0)
    yield c
    c.close()


def run_group(ctx, group):
    bs = V.batches(group)
    assert all(len(b.rows) % 64 for b in bs)                # a ragged last block in every launch
    outs = [ctx.debug_arith(b.selector, b.rows, b.out_words, b.arg).tolist() for b in bs]
    counts = V.verify_group(group, bs, outs)
    print(group, counts)
    return counts


def test_fp_raw_words(ctx):
    counts = run_group(ctx, "fp")
    assert len(counts) == 2 * 16 and min(counts.values()) > 300


def test_fp_inv_raw_words(ctx):
    assert len(run_group(ctx, "inv")) == 4


def test_fq2_raw_words(ctx):
    assert len(run_group(ctx, "fq2")) == 3


def test_f29_field_ops_raw_limbs(ctx):
    assert len(run_group(ctx, "f29")) == 2 * 17


def test_f29_is_zero_mod_p(ctx):
    assert len(run_group(ctx, "is_zero_mod_p")) == 4


def test_f29x2_raw_limbs(ctx):
    assert len(run_group(ctx, "f29x2")) == 8


def test_g1_accumulator_scripts(ctx):
    assert len(run_group(ctx, "scripts_g1")) == 3


def test_g2_accumulator_scripts(ctx):
    assert len(run_group(ctx, "scripts_g2")) == 3


def run_hint_group(ctx, group):
    counts = run_group(ctx, group)
    assert sorted(counts) == sorted(V.HINT_CLASSES[group]) and min(counts.values()) > 0, counts
    return counts


def test_bigs_raw_words(ctx, tmp_path):
    """BigS<12> and big_mul_acc.  BigS::lt outside its stated domain (the difference overflows 384 bits) has no right answer: there
    the device build and the g++ build of the same header must agree, case by case."""
    import test_arith_raw_host as host
    assert len(run_hint_group(ctx, "bigs")) == 30
    lt = [b for b in V.batches("bigs") if b.op == "BIGS_LT"]
    dev = V.lt_overflow_record(lt, [ctx.debug_arith(lt[0].selector, lt[0].rows, 1).tolist()])
    twin, _ = host.run_twin(host.build_twin(str(tmp_path / "arith_raw_check")), tmp_path, lt)
    assert len(dev) >= 200 and dev == V.lt_overflow_record(lt, twin)


def test_glv_split_every_search_class(ctx):
    """dev_glv_split on the container's lattice constants, on other bases of the same lattice, on index-2 sublattices and on skewed
    bases built to need rings 2 .. 5 or to have no pair: bit-equal to the restatement of ccs.glv_split; every class is reached with
    all components below 2^128 and the quotients inside the step cap."""
    assert len(run_hint_group(ctx, "hint_glv")) == 16


def test_emulated_reduce_edges(ctx):
    assert len(run_hint_group(ctx, "hint_emul")) == 12


def test_grumpkin_mul_edges(ctx):
    """the ladder's equal-point branch (H = 0, Rr = 0) IS reached: by k = order + 2 (and 2 order + 4, 2 order + 5), not by any of
    0 .. 3, 2^127 .. 2^256 - 1, order - 1 .. order + 1, 2 order, 2 order + 1"""
    assert len(run_hint_group(ctx, "hint_gk")) == 5


def test_probe_refuses_bad_arguments(ctx):
    import numpy as np
    import spp
    from spp.lib import SPP_ERR_BAD_INPUT
    L = ctx.L
    one = np.zeros((1, 16), dtype=np.uint32)
    out = np.zeros((1, 8), dtype=np.uint32)
    pi, po = one.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
    mul = V.OPS["FP_MUL"][0]
    assert L.spp_debug_arith(ctx.h, mul, 0, 1, pi, 16, po, 8) == 0
    wide, wideo = np.zeros((1, 64), dtype=np.uint32), np.zeros((1, 136), dtype=np.uint32)
    big, bigo = wide.ctypes.data_as(ctypes.c_void_p), wideo.ctypes.data_as(ctypes.c_void_p)
    assert L.spp_debug_arith(ctx.h, V.OPS["BIGS_ADD_SMALL_MUL"][0], -64 & 0xffff, 1, big, 24, bigo, 12) == 0
    for args in ((None, mul, 0, 1, pi, 16, po, 8), (ctx.h, mul, 0, 1, None, 16, po, 8), (ctx.h, mul, 0, 1, pi, 16, None, 8),
                 (ctx.h, mul, 0, 0, pi, 16, po, 8),                                    # no cases
                 (ctx.h, 0, 0, 1, pi, 16, po, 8), (ctx.h, 0xff, 0, 1, pi, 16, po, 8),  # unknown operations
                 (ctx.h, 0x200 | mul, 0, 1, pi, 16, po, 8),                            # unknown field
                 (ctx.h, V.OPS["FQ2_SQR"][0], 0, 1, pi, 16, po, 16),                   # an Fq-only operation over Fr
                 (ctx.h, mul, 0, 1, pi, 8, po, 8), (ctx.h, mul, 0, 1, pi, 16, po, 9),  # not the operation's word counts
                 (ctx.h, V.OPS["FP_MUL_SMALL"][0], 1 << 16, 1, pi, 8, po, 8),          # mul_small takes k < 2^16
                 (ctx.h, 0x100 | V.OPS["F29X2_SQR"][0], 3, 1, pi, 18, po, 18),         # no SUBC_3P_1
                 (ctx.h, 0x100 | V.OPS["HINT_GLV_SPLIT"][0], 0, 1, big, 32, bigo, 9),  # the hints are Fr only
                 (ctx.h, 0x100 | V.OPS["HINT_EMUL_REDUCE"][0], 0, 1, big, 64, bigo, 136), (ctx.h, 0x100 | V.OPS["BIGS_LT"][0], 0, 1, big, 24, bigo, 1),
                 (ctx.h, V.OPS["HINT_GLV_SPLIT"][0], 0, 1, big, 28, bigo, 9), (ctx.h, V.OPS["HINT_EMUL_REDUCE"][0], 0, 1, big, 64, bigo, 88),
                 (ctx.h, V.OPS["HINT_GRUMPKIN_MUL"][0], 0, 1, big, 8, bigo, 17), (ctx.h, V.OPS["BIG_MUL_ACC_8X8_8"][0], 0, 1, big, 24, bigo, 12),
                 (ctx.h, V.OPS["BIGS_ADD_SMALL_MUL"][0], 65, 1, big, 24, bigo, 12),    # |m| <= 64
                 (ctx.h, V.OPS["BIGS_ADD_SMALL_MUL"][0], -65 & 0xffff, 1, big, 24, bigo, 12),
                 (ctx.h, V.OPS["BIGS_ADD_SMALL_MUL"][0], 0x10001, 1, big, 24, bigo, 12)):
        assert L.spp_debug_arith(*args) == SPP_ERR_BAD_INPUT, args[1:4]
        assert spp.last_error()
