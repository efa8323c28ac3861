"""Every regime of the LUT forward (csrc/lut_linear.hip, lut_gemm.hip, gemm_h16.hip) at edge shapes, in guarded buffers.

The forward is a family of kernels chosen by a plan; tests/lut_arena.py lists, per regime, the developer options that force it and
a covering set of (bits, dtype, M, m, n, variant).  Per case:
  1. `debug_lut_plan` (the plan functions the forward itself calls) reports exactly the regime, split factor and
     fused-or-addend handling the case names -- a forced option the shape cannot follow is a failure, not a silent fallback;
  2. Gaussian inputs through `lut_arena.forward` (the C ABI entry on an arena with NaN / pattern guard bands, a workspace of exactly
     the sizer's bytes, y pre-filled): inside the project's fp64 bound (check() of tests/test_hip_lut_gemm.py; reference() /
     flip_slack() of tests/test_hip_lora.py with an adapter), and the public wrapper on the same tensors returns the same bits;
  3. integer inputs (every reference value exactly representable, every fp32 partial sum exact): torch.equal with the fp64 reference.
The four-wave developer kernel of GANQ_GEMM_H16_BM=512 is not a regime of the enum and is left out."""
import pytest
import torch

import lut_arena as la
from test_lut_regime_cases import BOUNDARIES, GEMM_FAMILY, assert_side, dense_boundaries, expected_modes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from ganq_amd import _lib

    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.selftest()
    return _lib


@pytest.mark.parametrize("case", la.CASES, ids=la.case_id)
def test_regime_case(hip, lib_options, case):
    c = case
    lib_options(reset=la.PLAN_OPTIONS, **c.opts)
    p = hip.debug_lut_plan(c.M, c.m, c.n, c.bits, r=la.rank_of(c.variant), outliers=la.has_outliers(c.variant))
    assert (p["regime"], p["KS"], p["outliers"], p["adapter"]) == (c.regime, c.KS) + expected_modes(c), p
    la.run_case(hip, c.bits, c.dtype, c.M, c.m, c.n, c.variant, la.case_seed(c))


def test_shape_driven_boundaries(hip, lib_options):
    """no option set: the plan changes regime exactly where the comments of lut_plan() / lut_dense_path() say (CU count from the
    device), and both sides of every boundary compute the right thing"""
    lib_options(reset=la.PLAN_OPTIONS)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    seen = set()
    for k, (below, want_b, at, want_a) in enumerate(BOUNDARIES + dense_boundaries(ncu)):
        for shape, want in ((below, want_b), (at, want_a)):
            bits, dtype = la.PAIRS[k % len(la.PAIRS)]
            p = hip.debug_lut_plan(*shape, bits)
            assert p["ncu"] == ncu
            assert_side(p, want, shape)
            seen.add(p["regime"])
            la.run_case(hip, bits, dtype, *shape, la.VARIANTS[k % 4], 1000 + k)
    assert {"decode16", "decode32", "mfma_small"} <= seen and seen & set(GEMM_FAMILY) and seen & {"dense128", "dense256"}


def test_union_of_regimes_is_the_whole_enum(hip, lib_options):
    """what the cases of this file are planned as ON THIS DEVICE (their options set one case at a time) is every regime of the enum"""
    seen = set()
    for c in la.CASES:
        lib_options(reset=la.PLAN_OPTIONS, **c.opts)
        seen.add(hip.debug_lut_plan(c.M, c.m, c.n, c.bits, r=la.rank_of(c.variant), outliers=la.has_outliers(c.variant))["regime"])
    assert seen == set(hip.LUT_REGIMES)
