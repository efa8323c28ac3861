"""Shared helper workgroups of the S-solve (csrc/solve_s.hip, "shared"): launches with more tiles than half the CUs but idle CUs
left over give every k = 2 .. 4 tiles of a ticket class ONE helper workgroup, which computes a far part of each of their residual
chains in turn.  Same matrix instructions in the same order on the same accumulator values as the single-workgroup solve, so in
every test

  * the reference is the same call with GANQ_SOLVE_DUO=0 (no helpers of any kind),
  * indices AND errors are compared as bits,
  * a sample of rows (the first 24, 16 from the middle, the last 8) is compared with the oracle,
  * and the plan query (ganq_debug_solve_plan, the function the kernel evaluates) confirms the regime and k that the test means to
    run -- a test of shared helpers would pass silently if none were launched.

Shapes are the smallest at which the mechanism can go wrong: chains longer than GANQ_SOLVE_DUO_CMIN panels (n = 1536: 24 panels),
several tiles per helper, a last group that is not full, a ragged last tile, a ragged last panel (n = 4100), rows longer than the
part of Err a helper keeps in LDS.
"""
import time

import numpy as np
import pytest
import torch

from test_hip_stages import dev, synth

pytestmark = pytest.mark.gpu

SHARE_OPTS = ("GANQ_SOLVE_DUO", "GANQ_SOLVE_SHARE", "GANQ_SOLVE_SHARE_K", "GANQ_SOLVE_SHARE2_XA", "GANQ_SOLVE_SHARE2_XB",
              "GANQ_SOLVE_SHARE3_XA", "GANQ_SOLVE_SHARE3_XB", "GANQ_SOLVE_SHARE4_XA", "GANQ_SOLVE_SHARE4_XB", "GANQ_SOLVE_DUO_XMIN",
              "GANQ_SOLVE_DUO_CMIN")


@pytest.fixture(scope="module")
def hip():
    from ganq_amd import _lib

    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.lib()
    _lib.selftest()
    return _lib


@pytest.fixture(scope="module")
def oracle():
    from oracle import c_oracle

    return c_oracle


_HL = {}


def layer(m, n, V, seed):
    """(W, H, L, T0) as test_hip_stages.synth(corr=0.1) makes them; H and L depend on n only and are computed once per n"""
    if n not in _HL:
        _, H, L, _ = synth(16, n, 16, 1000 + n, corr=0.1)
        _HL[n] = (H, L)
    H, L = _HL[n]
    rng = np.random.default_rng(seed)
    W = (0.02 * rng.standard_normal((m, n))).astype(np.float32)
    T0 = np.quantile(W, (np.arange(V) + 0.5) / V, axis=1).T.astype(np.float32).copy()
    return W, H, L, T0


def sample_rows(m):
    return np.unique(np.r_[0:min(m, 24), m // 2 - 8:m // 2 + 8, m - 8:m])


def run_and_compare(hip, oracle, lib_options, W, L, T0, runs, want):
    """runs: option sets; want(plan) -> bool says whether the plan under those options is the one the test is about"""
    m = W.shape[0]
    tiles = (m + 15) // 16
    Wd, Ld, Td = dev(W), dev(L), dev(T0)
    lib_options(reset=SHARE_OPTS, GANQ_SOLVE_DUO=0)
    Q0, E0 = hip.solve_s(Wd, Ld, Td, want_err=True)
    for opts in runs:
        lib_options(reset=SHARE_OPTS, **opts)
        plan = hip.debug_solve_plan(tiles)
        assert want(plan), f"{opts}: {tiles} tiles are planned as {plan}, not the regime under test"
        for _ in range(2):  # twice: the flags of the first launch must not satisfy the second
            Q1, E1 = hip.solve_s(Wd, Ld, Td, want_err=True)
            assert torch.equal(Q0, Q1), f"{opts}: {(Q0 != Q1).sum().item()} indices differ from the single-workgroup solve"
            assert torch.equal(E0.view(torch.int32), E1.view(torch.int32)), f"{opts}: errors differ"
    rows = sample_rows(m)
    Qo, Eo = oracle.solve_s(W[rows], L, T0[rows], want_err=True)
    assert np.array_equal(Q0.cpu().numpy()[rows], Qo)
    assert np.array_equal(E0.cpu().numpy()[rows], Eo, equal_nan=True)  # (values: the bits of a NaN error are not the oracle's business)
    return Q0


# ------------------------------------------------------------------------------------------ the real chip
@pytest.mark.parametrize("m,n,V,k", [(2300, 1536, 16, 2),    # 144 tiles, ragged last tile
                                     (2912, 1536, 16, 3),    # 182 tiles
                                     (3190, 1536, 16, 4),    # 200 tiles, ragged
                                     (2300, 4100, 8, 2)])    # ragged last panel, rows longer than the LDS-resident part
def test_shared_helpers_bit_identical(hip, oracle, m, n, V, k, lib_options):
    plan = hip.debug_solve_plan((m + 15) // 16)
    if (plan["regime"], plan["k"]) != ("shared", k):
        pytest.skip(f"{(m + 15) // 16} tiles are planned as {plan} on this part's CU count (k = {k} is meant for 256 CUs)")
    W, H, L, T0 = layer(m, n, V, 100 + k)
    run_and_compare(hip, oracle, lib_options, W, L, T0, [dict(GANQ_SOLVE_DUO=1)], lambda p: (p["regime"], p["k"]) == ("shared", k))


# ------------------------------------------------------------------------------------------ a pretended small chip
def pretended_case(hip, lib_options, k, single=False):
    """(CU count, m) with 300 <= m <= 400 where possible: the smallest ragged m whose tiles the plan serves with k tiles per helper
    under GANQ_SOLVE_CUS; single: some helper's last group is a single tile.  On 32 CUs no tile count is planned with k = 4
    (A + ceil(A / 4) per class fits 32 only up to A = 24, which k = 3 serves already; A = 25 needs 33 workgroups), so k = 4 is
    looked for on 40 CUs as well, where 29 tiles (m = 458) are the first."""
    for ncu in (32, 40):
        lib_options(reset=SHARE_OPTS, GANQ_SOLVE_CUS=ncu)
        for tiles in range(19, 32):
            m = 16 * tiles - 6
            if ncu == 32 and not 300 <= m <= 400:
                continue
            plan = hip.debug_solve_plan(tiles)
            if (plan["regime"], plan["k"]) != ("shared", k):
                continue
            roles = [hip.debug_solve_role(tiles, cls, tk) for cls in range(8) for tk in range(8)]
            serves = [r["serves"] for r in roles if r["tile"] is not None and r["stage"] == 1]
            assert len(serves) == plan["helpers"] and max(serves) == k
            if single and 1 not in serves:
                continue
            return ncu, m
    raise AssertionError(f"no tile count is planned with k = {k}")


@pytest.mark.parametrize("k,single", [(2, True), (3, False), (4, False)])
def test_shared_helpers_on_a_pretended_small_chip(hip, oracle, k, single, lib_options):
    ncu, m = pretended_case(hip, lib_options, k, single)
    W, H, L, T0 = layer(m, 1536, 16, 200 + k)
    T0[5, 3] = np.nan        # rows with a NaN codebook entry next to ordinary rows of the same tile
    T0[m - 20, 0] = np.nan
    run_and_compare(hip, oracle, lib_options, W, L, T0, [dict(GANQ_SOLVE_DUO=1, GANQ_SOLVE_CUS=ncu)],
                    lambda p: (p["regime"], p["k"]) == ("shared", k))


@pytest.mark.parametrize("k", [2, 3])
def test_shared_helpers_policy_extremes(hip, oracle, k, lib_options):
    """the tile keeps nearly nothing of its chains / nearly all of them, as the duo's test does"""
    ncu, m = pretended_case(hip, lib_options, k)
    W, H, L, T0 = layer(m, 1536, 16, 300 + k)
    xa, xb = f"GANQ_SOLVE_SHARE{k}_XA", f"GANQ_SOLVE_SHARE{k}_XB"
    base = dict(GANQ_SOLVE_DUO=1, GANQ_SOLVE_CUS=ncu)
    runs = [dict(base, **{xa: 0, xb: 0}, GANQ_SOLVE_DUO_XMIN=1, GANQ_SOLVE_DUO_CMIN=1),    # all but one panel far
            dict(base, **{xa: 60, xb: 0}, GANQ_SOLVE_DUO_XMIN=1, GANQ_SOLVE_DUO_CMIN=3),   # nearly all near
            dict(base, **{xa: 20, xb: 5}, GANQ_SOLVE_DUO_XMIN=3, GANQ_SOLVE_DUO_CMIN=12)]
    run_and_compare(hip, oracle, lib_options, W, L, T0, runs, lambda p: (p["regime"], p["k"]) == ("shared", k))


def test_shared_helpers_muted(hip, oracle, lib_options):
    """GANQ_SOLVE_DUO=2 mutes shared helpers too: every chain wave of a tile times out once (DUO_TIMEOUT, 0.5 ms) and computes its
    chains alone from then on -- same bits, and about one time-out longer than the launch without helpers."""
    ncu, m = pretended_case(hip, lib_options, 2)
    W, H, L, T0 = layer(m, 1536, 16, 400)
    Q0 = run_and_compare(hip, oracle, lib_options, W, L, T0, [dict(GANQ_SOLVE_DUO=2, GANQ_SOLVE_CUS=ncu)],
                         lambda p: (p["regime"], p["k"]) == ("shared", 2))
    d = (dev(W), dev(L), dev(T0))
    times = {}
    for duo in (0, 2):
        lib_options(reset=SHARE_OPTS, GANQ_SOLVE_DUO=duo, GANQ_SOLVE_CUS=ncu)
        hip.solve_s(*d)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        Q = hip.solve_s(*d)
        torch.cuda.synchronize()
        times[duo] = time.perf_counter() - t0
        assert torch.equal(Q, Q0)
    print(f"solve_s {m} x 1536 on {ncu} pretended CUs: without helpers {times[0] * 1e3:.2f} ms, muted shared helpers {times[2] * 1e3:.2f} ms")
    assert times[2] < 2.0 * times[0] + 5e-3, "a tile whose shared helper never answers must lose about one DUO_TIMEOUT, not more"


def test_forced_k_that_does_not_fit_runs_without_helpers(hip, oracle, lib_options):
    ncu, m = pretended_case(hip, lib_options, 3)
    tiles = (m + 15) // 16
    lib_options(reset=SHARE_OPTS, GANQ_SOLVE_CUS=ncu, GANQ_SOLVE_SHARE_K=2)
    assert hip.debug_solve_plan(tiles)["regime"] == "none"
    W, H, L, T0 = layer(m, 1536, 16, 500)
    run_and_compare(hip, oracle, lib_options, W, L, T0, [dict(GANQ_SOLVE_DUO=1, GANQ_SOLVE_CUS=ncu, GANQ_SOLVE_SHARE_K=2)],
                    lambda p: p["regime"] == "none" and p["helpers"] == 0)


# ------------------------------------------------------------------------------------------ the loop, concurrent launches
def test_shared_helpers_through_the_loop(hip, lib_options):
    """run_layer with and without helpers on 144 tiles: the active tile count sits in the shared range from iteration 0 on, and
    from iteration 2 on the row list compacts the rows that have not converged"""
    m, n, V, K = 2300, 1024, 16, 4
    plan = hip.debug_solve_plan((m + 15) // 16)
    if plan["regime"] != "shared":
        pytest.skip(f"144 tiles are planned as {plan} on this part's CU count")
    W, H, L, T0 = layer(m, n, V, 600)
    args = (dev(W), dev(H), dev(L), dev(T0), K)
    outs = []
    for helpers in (False, True):
        T, Q, d, bk = hip.run_layer(*args, alias_q=False, helpers=helpers)
        outs.append((T.clone(), Q.clone(), d.clone(), int(bk)))
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)), "codebooks differ"
    assert torch.equal(outs[0][1], outs[1][1]), f"{(outs[0][1] != outs[1][1]).sum().item()} indices differ"
    assert torch.equal(outs[0][2].view(torch.int64), outs[1][2].view(torch.int64)), "dists differ"
    assert outs[0][3] == outs[1][3]


def test_shared_helpers_on_two_streams(hip, lib_options):
    """Two shared launches side by side, each of 144 tiles and 72 helpers: together more workgroups than the chip has CUs, so some
    tiles and helpers start late.  The indices must be those of the launches run one after the other, and the pair must not take
    much longer than that (no tile waits for more than a time-out)."""
    m, n = 2300, 1536
    plan = hip.debug_solve_plan((m + 15) // 16)
    if plan["regime"] != "shared":
        pytest.skip(f"144 tiles are planned as {plan} on this part's CU count")
    assert 2 * ((m + 15) // 16 + plan["helpers"]) > torch.cuda.get_device_properties(0).multi_processor_count
    data = []
    for seed in (701, 702):
        W, H, L, T0 = layer(m, n, 16, seed)
        data.append((dev(W), dev(L), dev(T0)))
    lib_options(reset=SHARE_OPTS, GANQ_SOLVE_DUO=0)
    ref = [hip.solve_s(*d) for d in data]
    lib_options(reset=SHARE_OPTS)
    streams = [torch.cuda.Stream() for _ in data]
    for st, d in zip(streams, data):  # (a stream's first launch allocates its workspace: not timed)
        with torch.cuda.stream(st):
            hip.solve_s(*d)
    for d in data:
        hip.solve_s(*d)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    seq = [hip.solve_s(*d) for d in data]
    torch.cuda.synchronize()
    t_seq = time.perf_counter() - t0
    t0 = time.perf_counter()
    outs = []
    for st, d in zip(streams, data):
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            outs.append(hip.solve_s(*d))
    for st in streams:
        torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    t_conc = time.perf_counter() - t0
    print(f"solve_s {m} x {n}, two shared launches: one after the other {t_seq * 1e3:.2f} ms, side by side {t_conc * 1e3:.2f} ms")
    for o, s, r in zip(outs, seq, ref):
        assert torch.equal(s, r) and torch.equal(o, r)
    assert t_conc < 2.0 * t_seq + 5e-3, "shared launches side by side wait for each other (time-outs?)"
