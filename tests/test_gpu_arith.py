"""GPU: what hipcc makes of csrc/bn254.hpp and csrc/f29.hpp for gfx950, function by function, on raw words chosen to break it.

spp_debug_arith runs one header function per lane on the operand words as they are (no conversion, reduction or domain change on
either side); tests/arith_vectors.py supplies the words -- a fixed edge list per operation (limbs all ones, top limb 0 / 1 /
maximal, 2^k, p +- 2^k, operands at exactly the limb bounds the lazy forms state, k*p +- a bit for the zero tests, accumulator
scripts through the doubling and cancellation paths) plus 2000 seeded random cases -- and the predicate on every result, in Python
integers.  tests/test_arith_raw_host.py puts the same batches through the g++ build of the same dispatch, so a failure here
that does not show there is the device compile (as the 24-bit multiply behind Fp::hide24 was)."""
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
    for args in ((None, mul, 0, 1, pi, 16, po, 8), (ctx.h, mul, 0, 1, None, 16, po, 8), (ctx.h, mul, 0, 1, pi, 16, None, 8),
                 (ctx.h, mul, 0, 0, pi, 16, po, 8),                                    # no cases
                 (ctx.h, 0, 0, 1, pi, 16, po, 8), (ctx.h, 0xff, 0, 1, pi, 16, po, 8),  # unknown operations
                 (ctx.h, 0x200 | mul, 0, 1, pi, 16, po, 8),                            # unknown field
                 (ctx.h, V.OPS["FQ2_SQR"][0], 0, 1, pi, 16, po, 16),                   # an Fq-only operation over Fr
                 (ctx.h, mul, 0, 1, pi, 8, po, 8), (ctx.h, mul, 0, 1, pi, 16, po, 9),  # not the operation's word counts
                 (ctx.h, V.OPS["FP_MUL_SMALL"][0], 1 << 16, 1, pi, 8, po, 8),          # mul_small takes k < 2^16
                 (ctx.h, 0x100 | V.OPS["F29X2_SQR"][0], 3, 1, pi, 18, po, 18)):        # no SUBC_3P_1
        assert L.spp_debug_arith(*args) == SPP_ERR_BAD_INPUT, args[1:4]
        assert spp.last_error()
