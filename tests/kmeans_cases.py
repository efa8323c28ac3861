"""Inputs and references for the tests of the codebook initialisation (optimal weighted 1-D k-means per row), CPU and GPU.

Input families: the rows the product feeds the kernel (exact zeros behind the outlier split, blocks of identical values, fewer
distinct values than V, diag(Hinv)^-4 weights over many decades or zero, a large common offset) beside the Gaussian rows the
older tests use.  Every input is finite.

References, all torch fp64 on whatever device the inputs live on, none of them sharing code or assumptions with oracle/ or the
kernel: `exhaustive_cost` solves the dynamic programme densely over ALL start positions (no monotone argmin, no divide and
conquer) on a cluster cost matrix built by West's weighted mean / M2 update (no prefix-sum differences); `nearest_cost` and
`lloyd_residual` judge a codebook by itself."""
import numpy as np
import torch

TIE_FREE = ("gauss", "zeros40", "heavy_tail", "wide_w", "offset")
TIE_HEAVY = ("zero_w", "distinct1", "distinct5", "distinctV", "distinctV1", "distinct20", "stair", "coarse", "unweighted")
FAMILIES = TIE_FREE + TIE_HEAVY
# Bound of a codebook's cost above the exact optimum, in units of 2^-52 sum w x^2.  Twice 11.05, the largest
# (nearest_cost(T_oracle) - exhaustive_cost) / (2^-52 sum w x^2) over the grid of test_kmeans_cases.test_oracle_is_optimal
# (zeros40, n = 17, V = 2; per family 3.8 .. 11.05).  Most of it is the fp32 rounding of the centroids: a relative 2^-24 on a
# mean costs up to 2^-48 sum w mu^2 = 16 units.
C_CPU = 22.1
# the families the cost criterion pins (test_kmeans_cases.test_cost_criterion_has_teeth): a neighbouring partition costs
# more than 100 x the GPU bound.  Measured rise / GPU bound at n = 200 / 1030 / 4400, V = 16: gauss 1.2e6 / 1.5e6 / 1.1e4,
# zeros40 8e7 / 2e5 / 6e3, heavy_tail 2.4e7 / 1.2e6 / 5.6e4; NOT pinned by it: offset 3.5e4 / 17 / 2.1 (sum w x^2 is 2e4 times the
# spread the clusters divide) and wide_w -0.01 / 8e4 / -0.04 (the value that changes side may weigh 1e-16 of the row) -- their
# rows are held by the comparison with the oracle's codebook and by the Lloyd fixed point
COST_PINNED = ("gauss", "zeros40", "heavy_tail")
GPU_COST_FACTOR = 4.0  # two fp64 cost evaluations, and prefix sums whose rounding grows beyond the CPU sizes
STAIR_REPEAT = 14  # more than the 12 candidates a node of a balanced level evaluates itself


def _fp16(a):
    return np.asarray(a).astype(np.float16).astype(np.float32)


def _distinct(rng, n, D):
    vals = np.unique(_fp16(0.02 * rng.standard_normal(4 * D + 8)))
    vals = rng.permutation(vals)[:D]
    assert len(vals) == D
    return vals


def make_row(family, n, V, seed):
    """(x float32 [n], w float64 [n] or None)"""
    rng = np.random.default_rng([seed, n, V, FAMILIES.index(family)])
    x = _fp16(0.02 * rng.standard_normal(n))  # the generator of test_kmeans_vs_oracle
    w = rng.uniform(0.2, 3.0, n) ** -4
    if family == "gauss":
        pass
    elif family == "wide_w":
        w = 10.0 ** rng.uniform(-8.0, 8.0, n)
    elif family == "zero_w":
        w[rng.random(n) < 0.3] = 0.0
    elif family == "zeros40":
        x[rng.random(n) < 0.4] = 0.0
    elif family.startswith("distinct"):
        D = {"distinct1": 1, "distinct5": 5, "distinctV": V, "distinctV1": V + 1, "distinct20": 20}[family]
        x = _distinct(rng, n, D)[rng.integers(0, D, n)]
    elif family == "stair":
        D = max(1, min(n // STAIR_REPEAT, 3 * V + 1))
        x = rng.permutation(np.resize(_distinct(rng, n, D), n))  # every value n // D or n // D + 1 times
    elif family == "coarse":
        x = (np.round(x.astype(np.float64) * 200.0) / 200.0).astype(np.float32)
    elif family == "offset":
        x = (3.0 + x.astype(np.float64)).astype(np.float32)
    elif family == "heavy_tail":
        k = max(1, n // 100)
        x[rng.choice(n, k, replace=False)] *= 50.0
    elif family == "unweighted":
        w = None
    else:
        raise ValueError(family)
    x = np.ascontiguousarray(x, dtype=np.float32)
    assert np.all(np.isfinite(x)) and (w is None or (np.all(np.isfinite(w)) and np.all(w >= 0)))
    return x, w


VALUE_FAMILIES = ("gauss", "zeros40", "heavy_tail", "offset", "distinct1", "distinct5", "distinctV", "distinctV1", "distinct20", "stair",
                  "coarse")
WEIGHT_FAMILIES = ("gauss", "wide_w", "zero_w", "unweighted")


def make_matrix(n, V, seed, weights="gauss", values=VALUE_FAMILIES, m=None):
    """(W float32 [m, n], w float64 [n] or None, family of every row).  The kernel takes ONE weight vector per matrix, so a
    matrix holds the rows of the value families (cycled up to m rows, every row its own seed) under the weights of one of
    WEIGHT_FAMILIES; a row counts as tie-free when both its values and its weights come from a tie-free family."""
    m = len(values) if m is None else m
    fams = [values[r % len(values)] for r in range(m)]
    W = np.stack([make_row(f, n, V, seed + 1000 * r)[0] for r, f in enumerate(fams)])
    w = make_row(weights, n, V, seed)[1]
    return W, w, fams


def tie_free(value_family, weights="gauss"):
    return value_family in TIE_FREE and weights in TIE_FREE


def _t(a):
    return torch.as_tensor(np.array(a) if isinstance(a, np.ndarray) else a)  # a copy: the shared inputs are read-only arrays


def _sorted64(x, w, device=None):
    x = _t(x)
    device = device if device is not None else x.device
    x = x.to(device=device, dtype=torch.float64).flatten()
    w = torch.ones_like(x) if w is None else _t(w).to(device=device, dtype=torch.float64).flatten()
    order = torch.sort(x, stable=True).indices
    return x[order], w[order]


def cluster_costs(xs, ws):
    """C [n,n] fp64: C[j,i] = weighted within-cluster cost of the sorted points j..i (inf below the diagonal), by West's update
    of (weight, mean, M2) swept over i for all starts j at once.  Identical values give exactly 0."""
    n = xs.numel()
    C = torch.full((n, n), float("inf"), dtype=torch.float64, device=xs.device)
    W = torch.zeros(n, dtype=torch.float64, device=xs.device)
    mean = torch.zeros_like(W)
    M2 = torch.zeros_like(W)
    for i in range(n):
        xi, wi = xs[i], ws[i]
        Wn = W[: i + 1] + wi
        r = torch.where(Wn > 0, wi / Wn, torch.zeros_like(Wn))  # 1 exactly for the start j = i: the mean becomes x_i
        delta = xi - mean[: i + 1]
        mnew = mean[: i + 1] + delta * r
        M2[: i + 1] += wi * delta * (xi - mnew)
        mean[: i + 1] = mnew
        W[: i + 1] = Wn
        C[: i + 1, i] = M2[: i + 1]
    return C


def exhaustive_dp(x, w, V, device=None):
    """(optimal cost of at most V contiguous clusters of the sorted values, argmin table [V,n] of leftmost cluster starts).
    V - 1 dense min-plus layers over every start j <= i."""
    xs, ws = _sorted64(x, w, device)
    C = cluster_costs(xs, ws)
    n = xs.numel()
    D = C[0].clone()
    arg = torch.zeros((V, n), dtype=torch.int64, device=xs.device)
    zero = torch.zeros(1, dtype=torch.float64, device=xs.device)
    for k in range(1, V):
        prev = torch.cat([zero, D[:-1]])  # D[k-1][j-1]; j = 0: the clusters before are empty
        S = prev[:, None] + C
        D = S.min(dim=0).values
        arg[k] = (S == D[None, :]).to(torch.uint8).argmax(dim=0)  # the first of equal minima
    return float(D[n - 1]), arg


def exhaustive_cost(x, w, V, device=None):
    return exhaustive_dp(x, w, V, device)[0]


def total_energy(x, w):
    """sum w x^2: the scale of every rounding error of a cost"""
    xs, ws = _sorted64(x, w)
    return float((ws * xs * xs).sum())


def nearest_cost(x, w, T):
    """sum_i w_i min_k (x_i - T_k)^2 in fp64"""
    xs, ws = _sorted64(x, w)
    T = _t(T).to(device=xs.device, dtype=torch.float64).flatten()
    d = (xs[:, None] - T[None, :]) ** 2
    return float((ws * d.min(dim=1).values).sum())


def lloyd_residual(x, w, T):
    """largest violation of the Lloyd fixed point under nearest assignment (ties to the lower entry): an entry that owns
    weight must sit on the weighted mean of its points; an entry that owns no weight must repeat a neighbouring entry or, where
    it owns weightless points only, be one of them (any of them is a mean of nothing).  fp64."""
    xs, ws = _sorted64(x, w)
    T = _t(T).to(device=xs.device, dtype=torch.float64).flatten()
    V = T.numel()
    lab = ((xs[:, None] - T[None, :]) ** 2).argmin(dim=1)
    worst = 0.0
    for k in range(V):
        own = lab == k
        sw = float(ws[own].sum())
        if sw > 0:
            mu = float((ws[own] * xs[own]).sum() / ws[own].sum())
            worst = max(worst, abs(float(T[k]) - mu))
            continue
        near = [abs(float(T[k] - T[q])) for q in (k - 1, k + 1) if 0 <= q < V]
        if bool(own.any()):
            near.append(float((xs[own] - T[k]).abs().min()))
        worst = max(worst, min(near) if near else 0.0)
    return worst


def distinct_count(x):
    return int(np.unique(np.asarray(x)).size)


def assert_zero_optimum(x, w, T, what=""):
    """a row with at most V distinct values: the codebook reproduces them exactly"""
    T = np.asarray(T, dtype=np.float32) + np.float32(0.0)  # bits, with the two zeros counted as one value: a sum that starts
    vals = np.unique(np.asarray(x, dtype=np.float32)) + np.float32(0.0)  # at +0 returns +0 for a cluster of -0
    assert np.all(np.diff(T) >= 0), (what, T)
    assert np.all(np.isin(T.view(np.uint32), vals.view(np.uint32))), (what, T)
    assert nearest_cost(x, w, T) == 0.0, (what, nearest_cost(x, w, T))


def perturbed_cost(x, w, T):
    """teeth of the cost criterion: take the partition of codebook T (nearest assignment of the sorted values), move its most
    central interior boundary right by one distinct value, recompute the centroids -> cost of that neighbouring partition"""
    xs, ws = _sorted64(x, w)
    Td = torch.as_tensor(np.asarray(T, dtype=np.float64))
    lab = ((xs[:, None] - Td[None, :]) ** 2).argmin(dim=1)
    cuts = (torch.nonzero(lab[1:] != lab[:-1]).flatten() + 1).tolist()  # first index of every cluster but the first
    assert cuts, "one cluster: no interior boundary"
    b = cuts[len(cuts) // 2]
    nb = b
    while nb < len(xs) and xs[nb] == xs[b]:  # the whole block of the boundary's value changes side
        nb += 1
    bounds = [0] + [c for c in cuts if c != b and not b < c <= nb] + [nb, len(xs)]
    bounds = sorted(set(bounds))
    cost = 0.0
    for a, e in zip(bounds[:-1], bounds[1:]):
        sw = ws[a:e].sum()
        if float(sw) > 0:
            mu = (ws[a:e] * xs[a:e]).sum() / sw
            cost += float((ws[a:e] * (xs[a:e] - mu) ** 2).sum())
    return cost


def balanced_queue_demand(arg, n, hs=1, own=12):
    """how many nodes of level `hs` (positions hs - 1 + 2 hs t) of every DP layer hold more candidates than the `own` a node
    of a balanced level evaluates itself, from the exact argmin table: [V] counts.  A level queues exactly these nodes, so a
    queue shorter than the largest count overflows."""
    V = arg.shape[0]
    out = [0] * V
    idx = torch.arange(hs - 1, n - 1, 2 * hs, device=arg.device)
    for k in range(1, V - 1):  # the last layer solves position n - 1 only
        a = arg[k]
        left = torch.where(idx - hs >= 0, a[(idx - hs).clamp(min=0)], torch.zeros_like(idx))
        lo = torch.maximum(left, arg[k - 1][idx])
        hi = torch.maximum(lo, torch.minimum(idx, a[(idx + hs).clamp(max=n - 1)]))
        out[k] = int((hi - lo + 1 > own).sum())
    return out


def largest_resident_n(plan, V=16, m=4):
    """the largest n the plan keeps in the LDS-resident kernel (`plan` = ganq_amd._lib.debug_kmeans_plan)"""
    lo, hi = 1024, 16384
    assert plan(m, lo, V)["resident"] and not plan(m, hi, V)["resident"]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if plan(m, mid, V)["resident"] else (lo, mid)
    return lo
