"""GPU: the codebook initialisation (csrc/kmeans.hip) at the inputs the product produces and at every size where the launch
plan changes what runs, judged row by row -- never by a norm over the matrix, which dilutes one wrong row by sqrt(m V).

Inputs and references: tests/kmeans_cases.py.  Every shape's regime is asserted through the plan query (the plan function the
launch itself uses).  Per row: ascending; cost within 4 c_cpu 2^-52 sum w x^2 of the oracle's (test_kmeans_cases shows that
bound is 100 x sharper than moving one boundary, for the families it is claimed for); the Lloyd fixed point; on tie-free rows
the oracle's codebook to 1e-6 max|row|; rows with at most V distinct values exactly.  One test needs no oracle at all: the
exact optimum by a dense DP on the device.  The kernel variants (resident / windowed at any window, span-wise or level-wise
lower levels, any queue capacity down to an overflowing one) must agree bit for bit where the optimum is unique, and a row's
result may not depend on the rows its workgroup solved before it."""
import numpy as np
import pytest
import torch

import kmeans_cases as kc

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
OPTIONS = ("GANQ_KMEANS_WCAP", "GANQ_KMEANS_SPAN", "GANQ_KMEANS_QCAP")
SEED = 11


@pytest.fixture(scope="module")
def hip():
    from ganq_amd import _lib

    assert torch.cuda.is_available()
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def oracle():
    from oracle import c_oracle

    return c_oracle


@pytest.fixture(scope="module")
def nmax(hip):
    return kc.largest_resident_n(hip.debug_kmeans_plan)


def gpu_T(hip, W, w, V):
    return hip.kmeans_init(torch.tensor(W).cuda(), None if w is None else torch.tensor(w), V).cpu().numpy()


_CASES = {}  # inputs and the oracle's codebook per (n, V, weights, m): computed once, shared, read-only


def case(oracle, n, V, weights="gauss", m=None, values=kc.VALUE_FAMILIES):
    key = (n, V, weights, m, values)
    if key not in _CASES:
        W, w, fams = kc.make_matrix(n, V, SEED, weights=weights, values=values, m=m)
        Tref = oracle.kmeans_init(W, w, V)
        for a in (W, w, Tref):
            if a is not None:
                a.setflags(write=False)
        _CASES[key] = (W, w, fams, Tref)
    return _CASES[key]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_rows(W, w, fams, weights, T, Tref, V, what, rows=None):
    differ = 0
    for r in (range(len(fams)) if rows is None else rows):
        x, t, fam = W[r], T[r], fams[r]
        tag = (what, "row", r, fam, "weights", weights)
        assert np.all(np.isfinite(t)) and np.all(np.diff(t) >= 0), (tag, t)
        E, amax = kc.total_energy(x, w), float(np.abs(x).max())
        got, ref = kc.nearest_cost(x, w, t), kc.nearest_cost(x, w, Tref[r])
        assert got <= ref + kc.GPU_COST_FACTOR * kc.C_CPU * EPS * E, (tag, got, ref, (got - ref) / (EPS * E) if E > 0 else 0.0)
        res = kc.lloyd_residual(x, w, t)
        assert res <= 1e-6 * amax, (tag, res, amax)
        if kc.tie_free(fam, weights):
            err = float(np.abs(t.astype(np.float64) - Tref[r]).max())
            assert err <= 1e-6 * amax, (tag, err, amax)
        if kc.distinct_count(x) <= V:
            kc.assert_zero_optimum(x, w, t, tag)
        differ += not np.array_equal(bits(t), bits(Tref[r]))
    print(f"{what} weights={weights}: {differ} of {len(fams) if rows is None else len(rows)} rows not bit-identical to the oracle")


def assert_regime(hip, m, n, V, kind):
    p = hip.debug_kmeans_plan(m, n, V)
    nodes1 = n // 2  # nodes of the last level (spacing 1): positions 0, 2, .. < n - 1
    if kind == "small":       # no radix-16 level (P < 1024), no balanced level (< 512 nodes)
        assert p["resident"] and p["per_cu"] == 2 and p["P"] < 1024 and nodes1 < 512, p
    elif kind == "two_per_cu":  # radix-16 top, balanced bottom, two workgroups per CU
        assert p["resident"] and p["per_cu"] == 2 and p["P"] >= 1024 and nodes1 >= 512, p
    elif kind == "one_per_cu":
        assert p["resident"] and p["per_cu"] == 1 and nodes1 >= 512, p
    elif kind == "windowed1":
        assert not p["resident"] and p["per_cu"] == 1 and p["Wcap"] >= 512 and p["span"] == 512, p
    elif kind == "windowed2":
        assert not p["resident"] and p["per_cu"] == 2 and p["Wcap"] >= 512 and p["span"] == 512, p
    else:
        raise ValueError(kind)
    return p


SHAPES = [("small", n) for n in (1, 2, 15, 16, 17, 33, 257)] + [("two_per_cu", n) for n in (1024, 1025, 1030, 2048)] + \
         [("one_per_cu", 2500), ("one_per_cu", "nmax"), ("windowed1", "nmax+1"), ("windowed1", 8200)]


@pytest.mark.parametrize("kind,n", SHAPES, ids=[f"{k}-{n}" for k, n in SHAPES])
def test_every_regime_every_family(hip, oracle, nmax, kind, n):
    V = 16
    n = {"nmax": nmax, "nmax+1": nmax + 1}.get(n, n)
    for weights in kc.WEIGHT_FAMILIES:
        W, w, fams, Tref = case(oracle, n, V, weights)
        p = assert_regime(hip, len(fams), n, V, kind)
        if n == 1024:
            assert p["P"] == n and n // 2 == 512  # exactly the 512 nodes from which a level takes the balanced path
        if n == nmax:
            assert p["qcap"] < min(1024, (n // 4 + 63) // 64 * 64) and not hip.debug_kmeans_plan(len(fams), n + 1, V)["resident"]
        if n == 8200:
            assert p["P"] == 16384
        check_rows(W, w, fams, weights, gpu_T(hip, W, w, V), Tref, V, f"n={n} {kind}")


def test_windowed_two_per_cu_8192(hip, oracle):
    V, n, m = 16, 8192, 257
    for weights in ("gauss", "wide_w"):
        W, w, fams, Tref = case(oracle, n, V, weights, m=m)
        p = assert_regime(hip, m, n, V, "windowed2")
        assert p["grid"] == m and p["P"] == n
        check_rows(W, w, fams, weights, gpu_T(hip, W, w, V), Tref, V, "n=8192 m=257")


def test_windowed_at_the_limit_16384(hip, oracle):
    V, n = 16, 16384
    for weights in ("gauss", "zero_w"):
        W, w, fams, Tref = case(oracle, n, V, weights, values=("gauss", "stair"))
        p = assert_regime(hip, 2, n, V, "windowed1")
        assert p["P"] == n and p["grid"] == 2
        check_rows(W, w, fams, weights, gpu_T(hip, W, w, V), Tref, V, "n=16384")


def test_beyond_the_limit_is_an_error(hip):
    with pytest.raises(hip.GanqHipError, match="16384"):
        hip.debug_kmeans_plan(2, 16385, 16)
    W = torch.zeros(2, 16385, device="cuda")
    with pytest.raises(hip.GanqHipError, match="16384"):
        hip.kmeans_init(W, None, 16)
    torch.cuda.synchronize()  # nothing was launched, nothing is pending


def test_exact_optimum_without_the_oracle(hip):
    """n = 1030, V = 16, one row per family: the kernel's codebook against the dense DP over every cluster start, on the device"""
    V, n = 16, 1030
    rows = [(f, "gauss") for f in kc.VALUE_FAMILIES] + [("gauss", wf) for wf in ("wide_w", "zero_w", "unweighted")]
    worst = 0.0
    for weights in kc.WEIGHT_FAMILIES:
        values = tuple(f for f, wf in rows if wf == weights)
        W, w, fams = kc.make_matrix(n, V, SEED + 1, weights=weights, values=values)
        assert hip.debug_kmeans_plan(len(fams), n, V)["resident"]
        T = gpu_T(hip, W, w, V)
        for r, fam in enumerate(fams):
            best = kc.exhaustive_cost(W[r], w, V, device="cuda")
            got, E = kc.nearest_cost(W[r], w, T[r]), kc.total_energy(W[r], w)
            ratio = (got - best) / (EPS * E)
            worst = max(worst, ratio)
            assert got - best <= kc.C_CPU * EPS * E, (fam, weights, got, best, ratio)
            if kc.distinct_count(W[r]) <= V:
                assert best == 0.0
    print(f"largest (nearest_cost(T_gpu) - exhaustive_cost) / (2^-52 sum w x^2) = {worst:.3f}")


def variant_settings(n, nmax):
    return [dict(GANQ_KMEANS_WCAP=64), dict(GANQ_KMEANS_WCAP=200), dict(GANQ_KMEANS_WCAP=1024),
            dict(GANQ_KMEANS_WCAP=1024, GANQ_KMEANS_SPAN=0), dict(GANQ_KMEANS_WCAP=1024, GANQ_KMEANS_SPAN=64),
            dict(GANQ_KMEANS_QCAP=4), dict(GANQ_KMEANS_QCAP=32)]


@pytest.mark.parametrize("n", [1030, "nmax", "nmax+1"])
def test_variants_agree_bitwise(hip, oracle, nmax, lib_options, n):
    """where the optimum is unique every variant returns the same bits; a shorter queue changes who evaluates a candidate and
    nothing else, so there every row -- the stair rows with their long tied ranges too -- keeps its bits; tie-heavy rows under
    another kernel or window meet the cost criteria"""
    V = 16
    n = {"nmax": nmax, "nmax+1": nmax + 1}.get(n, n)
    for weights in ("gauss", "wide_w"):
        W, w, fams, Tref = case(oracle, n, V, weights)
        m = len(fams)
        lib_options(reset=OPTIONS)
        base_plan = hip.debug_kmeans_plan(m, n, V)
        base = gpu_T(hip, W, w, V)
        free = [r for r, f in enumerate(fams) if kc.tie_free(f, weights)]
        heavy = [r for r in range(m) if r not in free]
        assert len(free) >= 4 and "stair" in [fams[r] for r in heavy]
        if base_plan["resident"]:
            settings = variant_settings(n, nmax)
        else:  # the windowed kernel by itself: its lower levels span by span from another spacing, or level by level
            settings = [dict(GANQ_KMEANS_SPAN=0), dict(GANQ_KMEANS_SPAN=64), dict(GANQ_KMEANS_WCAP=200)]
        for opts in settings:
            lib_options(reset=OPTIONS, **opts)
            p = hip.debug_kmeans_plan(m, n, V)
            if "GANQ_KMEANS_QCAP" in opts:
                assert p == dict(base_plan, qcap=opts["GANQ_KMEANS_QCAP"]), p
                same = range(m)
            else:
                assert not p["resident"] and p["span"] == opts.get("GANQ_KMEANS_SPAN", 512), p
                assert p["Wcap"] == opts.get("GANQ_KMEANS_WCAP", base_plan["Wcap"]), p
                same = free
            T = gpu_T(hip, W, w, V)
            bad = [(r, fams[r]) for r in same if not np.array_equal(bits(T[r]), bits(base[r]))]
            assert not bad, (n, weights, opts, bad, [float(np.abs(T[r] - base[r]).max() / np.abs(W[r]).max()) for r, _ in bad])
            check_rows(W, w, fams, weights, T, Tref, V, f"n={n} {opts}", rows=[r for r in heavy if r not in same])
    lib_options(reset=OPTIONS)


def test_forced_queue_capacity_overflows(hip, nmax, lib_options):
    """GANQ_KMEANS_QCAP = 4 / 32 is below what a Gaussian row queues on a balanced level, the plan's own capacity is not: the
    comparison of test_variants_agree_bitwise is one of the in-place branch against the queue.  The count comes from the exact
    argmin table: a level queues the nodes that hold more than 12 candidates."""
    V = 16
    for n, forced in ((1030, (4,)), (nmax, (4, 32))):
        x, w = kc.make_row("gauss", n, V, SEED)
        arg = kc.exhaustive_dp(x, w, V, device="cuda")[1]
        demand = 0
        for hs in (1, 2, 4, 8):
            if (n - 1 - (hs - 1) + 2 * hs - 1) // (2 * hs) >= 512:  # the levels that take the balanced path
                demand = max(demand, max(kc.balanced_queue_demand(arg, n, hs)))
        own = hip.debug_kmeans_plan(1, n, V)["qcap"]
        print(f"n={n}: at most {demand} queued ranges per level, plan capacity {own}")
        assert max(forced) < demand <= own, (n, demand, own)
        base = gpu_T(hip, x[None], w, V)
        for q in forced:
            lib_options(GANQ_KMEANS_QCAP=q)
            assert hip.debug_kmeans_plan(1, n, V)["qcap"] == q
            assert np.array_equal(bits(gpu_T(hip, x[None], w, V)), bits(base)), (n, q)
        lib_options(reset=OPTIONS)


@pytest.mark.parametrize("n,wcap", [(1030, 0), (777, 200)])
def test_rows_do_not_depend_on_their_neighbours(hip, lib_options, n, wcap):
    """every persistent workgroup walks several unlike rows (m = 2 grid + 3, the families interleaved): a row's codebook has
    the bits of the same row solved alone, and of the matrix solved in reverse order"""
    V = 16
    if wcap:
        lib_options(GANQ_KMEANS_WCAP=wcap)
    m = 2 * hip.debug_kmeans_plan(4096, n, V)["grid"] + 3
    p = hip.debug_kmeans_plan(m, n, V)
    assert m == 2 * p["grid"] + 3 and p["resident"] == (wcap == 0) and p["per_cu"] == 2, p
    W, w, fams = kc.make_matrix(n, V, SEED + 2, weights="gauss", m=m)
    assert fams[0] != fams[p["grid"]] != fams[2 * p["grid"]]  # what one workgroup solves in turn
    Wd, wd = torch.from_numpy(W).cuda(), torch.from_numpy(w)
    T = hip.kmeans_init(Wd, wd, V)
    assert torch.equal(hip.kmeans_init(Wd, wd, V), T)  # and twice the same
    Trev = hip.kmeans_init(Wd.flip(0).contiguous(), wd, V).flip(0)
    bad = torch.nonzero((T.view(torch.int32) != Trev.view(torch.int32)).any(dim=1)).flatten().tolist()
    assert not bad, ("reversed", [(r, fams[r]) for r in bad[:8]])
    alone = torch.cat([hip.kmeans_init(Wd[r:r + 1].contiguous(), wd, V) for r in range(m)])
    bad = torch.nonzero((T.view(torch.int32) != alone.view(torch.int32)).any(dim=1)).flatten().tolist()
    assert not bad, ("alone", [(r, fams[r]) for r in bad[:8]])


@pytest.mark.parametrize("n", [1030, "nmax+1", 8200])
def test_repeat_gives_the_same_bits(hip, nmax, n):
    V = 16
    n = {"nmax+1": nmax + 1}.get(n, n)
    for weights in ("gauss", "zero_w"):
        W, w, fams = kc.make_matrix(n, V, SEED + 3, weights=weights)
        assert np.array_equal(bits(gpu_T(hip, W, w, V)), bits(gpu_T(hip, W, w, V)))


@pytest.mark.parametrize("V", [1, 2, 4, 5, 8, 16])
@pytest.mark.parametrize("n", [17, 1030])
def test_codebook_sizes(hip, oracle, n, V):
    for weights in kc.WEIGHT_FAMILIES:
        W, w, fams, Tref = case(oracle, n, V, weights)
        assert hip.debug_kmeans_plan(len(fams), n, V)["resident"]
        check_rows(W, w, fams, weights, gpu_T(hip, W, w, V), Tref, V, f"n={n} V={V}")
