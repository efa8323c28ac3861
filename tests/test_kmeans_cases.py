"""CPU: the oracle's codebook initialisation against an exact optimum that shares nothing with it (tests/kmeans_cases.py:
dense DP over all cluster starts on a West cost matrix), at the inputs the product produces; the sharpness of the cost
criterion the GPU tests use; and the launch plan of the kernel as the host-only query reports it.

c_cpu = kmeans_cases.C_CPU = 22.1: twice the largest (nearest_cost(T_oracle) - exhaustive_cost) / (2^-52 sum w x^2) this grid
gives, 11.05 (zeros40, n = 17, V = 2); test_oracle_is_optimal prints the figure of every family."""
import numpy as np
import pytest

import kmeans_cases as kc
from oracle import c_oracle

NS = (1, 2, 15, 16, 17, 33, 150, 200)
VS = (1, 2, 4, 5, 8, 16)
EPS = 2.0 ** -52


@pytest.mark.parametrize("family", kc.FAMILIES)
def test_oracle_is_optimal(family):
    worst = (0.0, (0, 0))
    for n in NS:
        for V in VS:  # V > n included
            x, w = kc.make_row(family, n, V, 7)
            T = c_oracle.kmeans_init(x[None], w, V)[0]
            assert np.all(np.diff(T) >= 0), (n, V, T)
            best, got, E = kc.exhaustive_cost(x, w, V), kc.nearest_cost(x, w, T), kc.total_energy(x, w)
            ratio = (got - best) / (EPS * E) if E > 0 else 0.0
            worst = max(worst, (ratio, (n, V)))
            assert got - best <= kc.C_CPU * EPS * E, (n, V, got, best, ratio)
            assert kc.lloyd_residual(x, w, T) <= 1e-6 * float(np.abs(x).max()), (n, V, T)
            if kc.distinct_count(x) <= V:  # the optimum is 0
                kc.assert_zero_optimum(x, w, T, (family, n, V))
    print(f"{family}: largest (nearest_cost(T_oracle) - exhaustive_cost) / (2^-52 sum w x^2) = {worst[0]:.3f} at (n, V) = {worst[1]}")
    assert 2.0 * worst[0] <= kc.C_CPU


@pytest.mark.parametrize("weights", kc.WEIGHT_FAMILIES)
def test_oracle_few_values_under_every_weighting(weights):
    """the rows of the GPU tests' matrices (every value family under every weighting) with at most V distinct values: exact.
    Two unlike values whose weights differ by 2^53 cost 0 together in prefix sums (offset row, n = 2, weights 1e8 : 1e-8:
    the merged pair cost 2.2e-12 before such rows were taken out of the dynamic programme)"""
    V = 16
    for n in (1, 2, 15, 16, 17, 33):
        W, w, fams = kc.make_matrix(n, V, 11, weights=weights)
        T = c_oracle.kmeans_init(W, w, V)
        for r, fam in enumerate(fams):
            if kc.distinct_count(W[r]) <= V:
                kc.assert_zero_optimum(W[r], w, T[r], (fam, weights, n))
            assert kc.lloyd_residual(W[r], w, T[r]) <= 1e-6 * float(np.abs(W[r]).max()), (fam, weights, n)


def test_references_on_a_known_row():
    # hand-checked: two clusters {0, 0, 1} | {10, 11}; weights 1 -> means 1/3 and 10.5, cost 2/3 + 1/2
    x = np.array([10, 0, 1, 11, 0], dtype=np.float32)
    assert kc.exhaustive_cost(x, None, 2) == pytest.approx(2.0 / 3.0 + 0.5, rel=1e-15)
    assert kc.exhaustive_cost(x, None, 1) == pytest.approx(125.2, rel=1e-14)  # 222 - 22^2 / 5
    assert kc.exhaustive_cost(x, None, 4) == 0.0 and kc.exhaustive_cost(x, None, 9) == 0.0  # four distinct values
    w = np.array([1, 0, 2, 1, 0], dtype=np.float64)  # the zeros carry no weight: {1} | {10, 11}
    assert kc.exhaustive_cost(x, w, 2) == pytest.approx(0.5, rel=1e-15)
    T = np.array([1.0 / 3.0, 10.5], dtype=np.float32)
    assert kc.nearest_cost(x, None, T) == pytest.approx(2.0 / 3.0 + 0.5, rel=1e-6)
    assert kc.lloyd_residual(x, None, T) < 1e-7
    assert kc.lloyd_residual(x, None, np.array([0.5, 10.5], dtype=np.float32)) == pytest.approx(0.5 - 1.0 / 3.0, rel=1e-6)
    assert kc.lloyd_residual(x, None, np.array([1.0 / 3.0, 10.5, 10.5], dtype=np.float32)) < 1e-7   # a repeated entry owns nothing
    assert kc.lloyd_residual(x, None, np.array([1.0 / 3.0, 5.0, 10.5], dtype=np.float32)) == pytest.approx(14.0 / 3.0, rel=1e-6)


@pytest.mark.parametrize("family", kc.TIE_FREE)
def test_cost_criterion_has_teeth(family):
    """the oracle's partition with ONE interior boundary moved by one distinct value must cost more than 100 x what the GPU
    tests allow above the oracle -- else that bound could not tell the optimum from its neighbour"""
    V = 16
    for n in (200, 1030, 4400):
        x, w = kc.make_row(family, n, V, 7)
        T = c_oracle.kmeans_init(x[None], w, V)[0]
        rise = kc.perturbed_cost(x, w, T) - kc.nearest_cost(x, w, T)
        bound = kc.GPU_COST_FACTOR * kc.C_CPU * EPS * kc.total_energy(x, w)
        print(f"{family} n={n}: rise / GPU bound = {rise / bound:.3g}")
        if family in kc.COST_PINNED:
            assert rise > 100.0 * bound, (n, rise, bound)
    assert set(kc.COST_PINNED) >= {"gauss", "zeros40", "heavy_tail"}


def test_plan_query_regimes(lib_options):
    """ganq_debug_kmeans_plan, host only: where kmeans_plan() changes kernel, workgroups per CU, queue and window"""
    from ganq_amd import _lib

    plan = _lib.debug_kmeans_plan
    for n in (1, 2, 15, 16, 17, 33, 257, 1024, 1025, 1030, 2048):
        p = plan(5, n, 16)
        assert p["resident"] and p["per_cu"] == 2 and p["grid"] == 5 and p["Wcap"] == 0 and p["span"] == 0, (n, p)
        assert p["P"] >= n and p["P"] < 2 * max(n, 1) and p["P"] & (p["P"] - 1) == 0
    assert plan(5, 1024, 16)["P"] == 1024 and plan(5, 1025, 16)["P"] == 2048
    p = plan(5, 2500, 16)
    assert p["resident"] and p["per_cu"] == 1 and p["qcap"] == 640  # (2500 / 4 + 63) / 64 * 64: not shrunk
    nmax = kc.largest_resident_n(plan)
    p, q = plan(4, nmax, 16), plan(4, nmax + 1, 16)
    assert 4096 < nmax < 4700 and p["resident"] and p["per_cu"] == 1 and 128 <= p["qcap"] < 1024, (nmax, p)  # queue shrunk from 1024
    assert p["lds_bytes"] <= 160 * 1024 - 1024
    assert not q["resident"] and q["per_cu"] == 1 and q["P"] == 8192 and q["Wcap"] > 0 and q["span"] == 512, q
    p = plan(257, 8192, 16)
    assert not p["resident"] and p["per_cu"] == 2 and p["grid"] == 257 and p["P"] == 8192
    assert plan(256, 8192, 16)["per_cu"] == 1  # the second workgroup per CU only with more rows than CUs
    p = plan(3, 8200, 16)
    assert not p["resident"] and p["per_cu"] == 1 and p["P"] == 16384
    p = plan(2, 16384, 16)
    assert not p["resident"] and p["P"] == 16384 and p["grid"] == 2 and 4 * 8 * p["Wcap"] + 2 * 2 * 16384 <= p["lds_bytes"]
    assert plan(1000, 1030, 16)["grid"] == 512 and plan(1000, 2500, 16)["grid"] == 256
    with pytest.raises(_lib.GanqHipError, match="16384"):
        plan(2, 16385, 16)
    # the developer options, as the launch will see them
    base = plan(4, 1030, 16)
    lib_options(GANQ_KMEANS_QCAP=4)
    assert plan(4, 1030, 16) == dict(base, qcap=4) and plan(4, nmax, 16)["qcap"] == 4
    lib_options(GANQ_KMEANS_QCAP=4096)
    assert plan(4, 1030, 16) == base  # never above the plan's own capacity
    lib_options(reset=("GANQ_KMEANS_QCAP",), GANQ_KMEANS_WCAP=200, GANQ_KMEANS_SPAN=64)
    p = plan(4, 1030, 16)
    assert not p["resident"] and p["Wcap"] == 200 and p["span"] == 64 and p["qcap"] == 0
    lib_options(reset=("GANQ_KMEANS_SPAN",), GANQ_KMEANS_WCAP=1024)
    assert plan(4, nmax, 16)["Wcap"] == 1024 and plan(4, nmax, 16)["span"] == 512
