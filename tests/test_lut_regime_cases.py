"""The case list of the LUT-forward regime tests (tests/lut_arena.py), checked without a GPU: it covers what it claims to cover, stays
within its size budget, and its integer inputs keep the fp64 reference inside the exactly representable range.  Plus the plan
query of the library (ganq_debug_lut_plan) at 256 compute units: the regime changes exactly where the comments of lut_plan() /
lut_dense_path() say, and every case of the list is planned as the regime it names."""
import numpy as np
import pytest

import lut_arena as la


def by_regime():
    out = {r: [] for r in la.REGIMES}
    for c in la.CASES:
        out[c.regime].append(c)
    return out


def test_case_list_is_deterministic_and_within_budget():
    assert [la.case_id(c) for c in la.build_cases()] == [la.case_id(c) for c in la.CASES]
    assert len({la.case_id(c) for c in la.CASES}) == len(la.CASES) <= 600
    for c in la.CASES:
        assert c.M <= la.MAX_SHAPE[0] and c.m <= la.MAX_SHAPE[1] and c.n <= la.MAX_SHAPE[2], c
        assert c.n % 32 == 0 and c.variant in la.VARIANTS and c.dtype in ("fp16", "bf16")
    assert sum(c.M * c.m * c.n > la.LARGE_PRODUCT for c in la.CASES) <= 4


def test_axes_name_every_edge_value():
    """regime_axes() may only leave out what the library cannot serve in that regime (its docstring names the checks): together the
    regimes meet every edge value the issue lists"""
    for values, axis in ((la.M_EDGES, 0), (la.OUT_EDGES, 1), (la.IN_EDGES, 2), (la.VARIANTS, 3)):
        assert set(values) == set().union(*(la.regime_axes(r)[axis] for r in la.REGIMES))


@pytest.mark.parametrize("regime", la.REGIMES)
def test_every_regime_meets_every_edge(regime):
    cases = by_regime()[regime]
    Ms, ms, ns, variants = la.regime_axes(regime)
    assert {c.M for c in cases} == set(Ms)
    assert {c.m for c in cases} == set(ms)
    assert {c.n for c in cases} == set(ns)
    assert {(c.bits, c.dtype) for c in cases} == set(la.PAIRS)
    assert {c.variant for c in cases} == set(variants)
    assert sum(c.m == 8200 for c in cases) >= 1 and sum(c.n == 8192 for c in cases) >= 1
    if not regime.startswith("dense"):  # (the dense GEMM needs n = 0 mod 64)
        assert any(c.M % 16 and c.m % 16 and c.n % 64 == 32 for c in cases)
    # forced split factors, one of them not dividing the number of 32-column groups
    if regime in ("decode16", "decode32", "mfma_small"):
        for ks in (3, 5):
            assert any(c.KS == ks and c.opts["GANQ_LUT_KS"] == ks and (c.n // 32) % ks for c in cases), ks
    if regime == "gemm_splitk":
        assert any(c.KS == 3 and c.opts["GANQ_LUT_GEMM_RM"] == 3 and (c.n // 32) % 3 for c in cases)
        assert all(c.KS > 1 for c in cases)
    if regime in ("gemm", "gemm_pipe", "dense128", "dense256"):
        assert all(c.KS == 1 for c in cases)


@pytest.mark.parametrize("regime", la.REGIMES)
def test_integer_inputs_keep_the_reference_exactly_representable(regime):
    """on the reference alone: every output and every element of t = x lora_A^T an integer of magnitude <= 2048 (fp16) / 256 (bf16)"""
    for c in by_regime()[regime]:
        inp = la.integers(c.bits, c.M, c.m, c.n, c.variant, la.case_seed(c), c.dtype)
        ref, t = la.integer_reference_cpu(inp)
        lim = la.INT_LIMIT[c.dtype]
        for name, a in (("ref", ref), ("t", t)):
            if a is not None:
                assert np.array_equal(a, np.rint(a)) and float(np.abs(a).max()) <= lim, (la.case_id(c), name, float(np.abs(a).max()))
        assert float(np.abs(inp["x"]).max()) <= 1 and float(np.abs(inp["lut"]).max()) <= 2
        if c.M * c.m >= 256:  # a test that can see something: the outputs are not all zero
            assert float(np.abs(ref).max()) >= 1, la.case_id(c)


def test_gaussian_inputs_follow_the_adapter_tests_distributions():
    inp = la.gaussian(4, 64, 256, 1024, "adapter48_outliers", 7)
    assert inp["x"].shape == (64, 1024) and inp["A"].shape == (48, 1024) and inp["B"].shape == (256, 48)
    Wq = np.take_along_axis(inp["lut"], inp["Q"].astype(np.int64), axis=1).astype(np.float64)
    base = inp["x"].astype(np.float64) @ Wq.T
    ad = (inp["x"].astype(np.float64) @ inp["A"].T.astype(np.float64)) @ inp["B"].T.astype(np.float64)
    ratio = float(np.sqrt((ad ** 2).mean() / (base ** 2).mean()))
    assert 0.1 <= ratio <= 1.0, ratio
    rowptr, cols, vals = inp["outliers"]
    assert rowptr[-1] == cols.size == vals.size > 0
    for o in range(256):
        seg = cols[rowptr[o]:rowptr[o + 1]]
        assert np.all(np.diff(seg) > 0) and (seg.size == 0 or seg.max() < 1024)


# ---- the plan query, host only (ncu given: no GPU is touched)
NCU = 256
GEMM_FAMILY = ("gemm", "gemm_splitk", "gemm_pipe")
# (M, m, n) below / at each boundary the comments of lut_plan() and lut_dense_path() name, and the regimes on either side
BOUNDARIES = [
    ((16, 512, 512), ("decode16", 1), (17, 512, 512), ("decode16", 2)),         # one / two 16-row tiles
    ((32, 512, 512), ("decode16", 2), (33, 512, 512), ("mfma_small", 4)),       # the in-workgroup kernel serves M <= 32
    ((64, 512, 512), ("mfma_small", 4), (65, 512, 512), (GEMM_FAMILY, 1)),      # LUT_MAX_M
    ((8, 127, 512), ("mfma_small", 1), (8, 128, 512), ("decode16", 1)),         # "from 128 output features"
    ((1, 8160, 512), ("decode16", 1), (1, 8162, 512), ("decode32", 1)),         # (m + 31) / 32 reaches 256
    ((16, 8160, 512), ("decode16", 1), (16, 8162, 512), ("decode32", 1)),
    ((17, 8162, 512), ("decode16", 2), (16, 8161, 512), ("decode16", 1)),       # ... and only for M <= 16 and even m
]


def dense_boundaries(ncu):
    """M = 1023 / 1024 with a chip's worth of 128 x 256 tiles, and 1024 rows with one column of tiles fewer"""
    cols = -(-ncu // 8)  # 8 row tiles of 128 at M = 1024
    return [((1023, 256 * cols, 512), (GEMM_FAMILY, None), (1024, 256 * cols, 512), (("dense128", "dense256"), None)),
            ((1024, 256 * (cols - 1), 512), (GEMM_FAMILY, None), (1024, 256 * (cols - 1) + 4, 512), (("dense128", "dense256"), None))]


def assert_side(plan, want, what):
    regimes, rt = want
    assert plan["regime"] in ((regimes,) if isinstance(regimes, str) else regimes), (what, plan)
    if rt is not None:
        assert plan["row_tiles"] == rt, (what, plan)


def test_plan_changes_regime_at_the_documented_boundaries(lib_options):
    from ganq_amd import _lib

    lib_options(reset=la.PLAN_OPTIONS)
    for below, want_b, at, want_a in BOUNDARIES + dense_boundaries(NCU):
        for bits in (2, 3, 4):
            assert_side(_lib.debug_lut_plan(*below, bits, ncu=NCU), want_b, below)
            assert_side(_lib.debug_lut_plan(*at, bits, ncu=NCU), want_a, at)
    # the shapes the older tests reach the dense path with, and the one that only looks like it (128 tiles of 128 x 256 < 256 CUs)
    for M in (2048, 4096):
        for m in (4096, 14336):
            assert _lib.debug_lut_plan(M, m, 4096, 4, ncu=NCU)["regime"] in ("dense128", "dense256")
    assert _lib.debug_lut_plan(2048, 2048, 2048, 4, ncu=NCU)["regime"] in GEMM_FAMILY
    # outliers and the adapter: fused into the decode launch, an fp32 addend where the issue says so
    p = _lib.debug_lut_plan(16, 4096, 4096, 4, r=32, outliers=True, ncu=NCU)
    assert (p["outliers"], p["adapter"]) == ("fused", "fused") and p["t_KS"] >= 1
    p = _lib.debug_lut_plan(40, 64, 4096, 4, r=32, outliers=True, ncu=NCU)
    assert (p["regime"], p["outliers"], p["adapter"]) == ("mfma_small", "addend", "fused")
    p = _lib.debug_lut_plan(2048, 4096, 8192, 4, r=32, outliers=True, ncu=NCU)
    assert (p["regime"], p["outliers"], p["adapter"]) == ("dense128", "addend", "addend")
    p = _lib.debug_lut_plan(2048, 4096, 4096, 4, r=32, ncu=NCU)
    assert p["regime"] in GEMM_FAMILY and p["adapter"] == "fused" and p["outliers"] is None
    assert _lib.debug_lut_plan(2048, 4096, 4096, 4, ncu=NCU)["adapter"] is None
    with pytest.raises(_lib.GanqHipError):
        _lib.debug_lut_plan(16, 64, 48, 4, ncu=NCU)  # in_features not a multiple of 32
    with pytest.raises(_lib.GanqHipError):
        _lib.debug_lut_plan(16, 64, 64, 4, r=8, ncu=NCU)


def expected_modes(c):
    outl = None if not la.has_outliers(c.variant) else ("fused" if c.regime in ("decode16", "decode32") else "addend")
    adapter = None if not la.rank_of(c.variant) else ("addend" if c.regime.startswith("dense") else "fused")
    return outl, adapter


def test_every_case_is_planned_as_the_regime_it_names(lib_options):
    from ganq_amd import _lib

    seen = set()
    for ncu in (64, NCU, 304):  # forced regimes do not depend on the chip
        for c in la.CASES:
            lib_options(reset=la.PLAN_OPTIONS, **c.opts)
            p = _lib.debug_lut_plan(c.M, c.m, c.n, c.bits, r=la.rank_of(c.variant), outliers=la.has_outliers(c.variant), ncu=ncu)
            assert (p["regime"], p["KS"], p["outliers"], p["adapter"]) == (c.regime, c.KS) + expected_modes(c), (la.case_id(c), p)
            seen.add(p["regime"])
    assert seen == set(_lib.LUT_REGIMES) == set(la.REGIMES)
    # a forced option the shape cannot follow is reported, not hidden: 32 features per workgroup on an odd m, the dense path on
    # in_features = 32 mod 64, the pipelined kernel under a split
    lib_options(reset=la.PLAN_OPTIONS, GANQ_LUT_INWG=1, GANQ_LUT_NT=2)
    assert _lib.debug_lut_plan(8, 129, 512, 4, ncu=NCU)["regime"] == "decode16"
    lib_options(reset=la.PLAN_OPTIONS, GANQ_LUT_DENSE_M=1)
    assert _lib.debug_lut_plan(300, 512, 544, 4, ncu=NCU)["regime"] in GEMM_FAMILY
    lib_options(reset=la.PLAN_OPTIONS, GANQ_LUT_DENSE_M=0, GANQ_LUT_GEMM_RM=2, GANQ_LUT_GEMM_PIPE=1)
    assert _lib.debug_lut_plan(300, 512, 1024, 4, ncu=NCU)["regime"] == "gemm_splitk"
