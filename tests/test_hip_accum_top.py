"""The four-wave full bucket sum with sparse top digit planes of H kept off the matrix cores (GANQ_T_TOP, onehot_accum_w4_kernel with
2 or 3 dense planes + top_fixup_kernel on the exception lists of hquant_kernel) EXACTLY: against the host model of
tests/t_update_model.py and against the four-plane sum (GANQ_T_TOP=0).  Integer sums have one right answer, so everything is compared
with array_equal / bytes.  GANQ_ACCUM_W4=1 is forced; the plan, the exception counts and the number of dense planes D of the query
(ganq_debug_top_planes) are asserted before every run, so that no case passes on a path it did not mean.

Shapes: n = 256 every slice crosses the diagonal, 512 the first plain slice, 1280 the ring of LDS stages wraps; m = 1 a workgroup
with one row, 9 a wave with one row, 33 two row groups."""
import numpy as np
import pytest
import torch

import t_update_model as M

pytestmark = pytest.mark.gpu

OPTIONS = ("GANQ_ACCUM_W4", "GANQ_H_EXT", "GANQ_T_FULL", "GANQ_T_INCR_THR", "GANQ_MUPDATE_LDS", "GANQ_SOLVE_ALL_ROWS", "GANQ_T_JACOBI",
           "GANQ_WH_F64", "GANQ_T_TOP", "GANQ_T_TOP_CAP")
TOP_N = (256, 512, 1280)
TOP_M = (1, 9, 33)


@pytest.fixture(scope="module")
def hip():
    from ganq_amd import _lib

    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.lib()
    _lib.selftest()
    return _lib


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def entry(hip, W, H, Qseq, V):
    res = hip.debug_t_sums(dev(W), dev(H), dev(Qseq), V)
    return {k: (None if v is None else v.cpu().numpy()) for k, v in res.items()}


def model_counts(q):
    """(c3, c2) of the bytes the full sum reads: the entries u > v of the 31-bit word with a non-zero digit 3 / digit 2 or 3"""
    ds, rest = M.digits(q["I"], 4)
    assert not rest.any()
    up = np.triu(np.ones(q["I"].shape, dtype=bool), 1)
    return int(((ds[3] != 0) & up).sum()), int((((ds[2] != 0) | (ds[3] != 0)) & up).sum())


def use_top(hip, lib_options, m, n, H, ext_mode, top, cap, want_D, counts, **opts):
    """four-wave kernel, GANQ_T_TOP = top, GANQ_T_TOP_CAP = cap: the plan, the device's counts and its D are what the case means"""
    lib_options(reset=OPTIONS, GANQ_ACCUM_W4=1, GANQ_H_EXT=ext_mode, GANQ_T_TOP=top, GANQ_T_TOP_CAP=cap, **opts)
    assert hip.accum_plan(m, n)["kernel"] == "onehot_accum_w4", (m, n)
    got = hip.debug_top_planes(dev(H), m)
    assert (got["c3"], got["c2"]) == counts, (got, counts)
    assert got["D"] == want_D, (got, want_D)
    return got


def check_sums(hip, lib_options, m, n, V, ext_mode, H, Q, settings):
    """settings: [(cap, D)].  F_hi / F_lo of the loop's T-update and the A of the stateless stage call equal the model under every
    setting, and equal, byte for byte, what GANQ_T_TOP=0 gives."""
    W = M.weights(m, n)
    q = M.quantize(H, ext_mode)
    counts = model_counts(q)
    sums = M.model_sums(q, Q)
    WH = (W.astype(np.float64) @ H.astype(np.float64)).astype(np.float32)
    A_ref = M.A_fp32(q["scale"], q["ext"], sums["F_hi"], sums["D_hi"], sums["F_lo"], sums["D_lo"], V)
    got = []
    for top, cap, D in [(0, -1, 4)] + [(-1, cap, D) for cap, D in settings]:
        use_top(hip, lib_options, m, n, H, ext_mode, top, cap, D, counts)
        res = entry(hip, W, H, Q[None], V)
        assert int(res["ext"]) == ext_mode
        assert int(res["full_ran"][0]) == 1, (cap, D)
        bad = np.argwhere(res["F_hi"][0] != sums["F_hi"])
        assert np.array_equal(res["F_hi"][0], sums["F_hi"]), (cap, D, len(bad), bad[:4].tolist())
        assert np.array_equal(res["F_lo"][0], sums["F_lo"]), (cap, D)
        _, A, _ = hip.update_t(dev(WH), dev(H), dev(Q), V, want_ab=True)  # the stateless stage call
        assert M.bits_equal(A.cpu().numpy(), A_ref), (cap, D)
        got.append((res["F_hi"][0], res["F_lo"][0], A.cpu().numpy()))
    for other in got[1:]:
        for a, b in zip(got[0], other):
            assert a.tobytes() == b.tobytes()
    return counts


def _dealt(count):
    """(m, n) pairs in turn, V, the extension and the pattern dealt with strides coprime to the axis lengths"""
    cases = []
    for j in range(count):
        cases.append({"n": TOP_N[j % 3], "m": TOP_M[(j + j // 3) % 3], "V": M.FULL_V[(2 * j + j // 3) % 3],
                      "ext_mode": (j + j // 3) % 2, "pattern": M.PATTERNS[(2 * j + j // 5) % 5]})
    return cases


def case_id(c):
    return f"m{c['m']}-n{c['n']}-V{c['V']}-ext{c['ext_mode']}-{c['pattern']}"


MASSIVE_CASES = _dealt(9) + [{"n": 512, "m": 9, "V": 16, "ext_mode": 1, "pattern": "one_code_per_row"},
                             {"n": 256, "m": 33, "V": 8, "ext_mode": 0, "pattern": "unused_codes"}]


@pytest.mark.parametrize("case", MASSIVE_CASES, ids=[case_id(c) for c in MASSIVE_CASES])
def test_massive_hessian_two_and_three_dense_planes(hip, lib_options, case):
    """two features x 1000: a handful of entries above the second digit.  cap = c2: D = 2; cap = c2 - 1: the longer list overflows
    by one, D = 3; cap = 0: only an empty list qualifies"""
    m, n, V = case["m"], case["n"], case["V"]
    H = M.hessian("massive", n)
    c3, c2 = model_counts(M.quantize(H, case["ext_mode"]))
    assert 0 < c2 < 4096 and c3 < c2, (c3, c2)
    settings = [(c2, 2), (c2 - 1, 3), (0, 3 if c3 == 0 else 4)]
    check_sums(hip, lib_options, m, n, V, case["ext_mode"], H, M.pattern(case["pattern"], m, n, V), settings)


@pytest.mark.parametrize("m,n,V,ext_mode,pk", [(33, 256, 16, 0, "uniform"), (9, 512, 8, 1, "edge_columns"), (1, 1280, 4, 0, "unused_codes")])
def test_ordinary_hessian_keeps_four_planes_under_the_default_cap(hip, lib_options, m, n, V, ext_mode, pk):
    """off-diagonals of the size of the diagonal: digit 3 is dense, the parent's path, and the fix-up leaves the sums alone"""
    check_sums(hip, lib_options, m, n, V, ext_mode, M.hessian("ordinary", n), M.pattern(pk, m, n, V), [(-1, 4)])


@pytest.mark.parametrize("m,n,V,ext_mode", [(9, 256, 4, 1), (33, 512, 16, 0)])
def test_zero_hessian(hip, lib_options, m, n, V, ext_mode):
    H = M.hessian("zero", n)
    counts = check_sums(hip, lib_options, m, n, V, ext_mode, H, M.pattern("uniform", m, n, V), [(-1, 2), (0, 2)])
    assert counts == (0, 0)
    lib_options(reset=OPTIONS, GANQ_ACCUM_W4=1, GANQ_H_EXT=ext_mode)
    assert not entry(hip, M.weights(m, n), H, M.pattern("uniform", m, n, V)[None], V)["F_hi"].any()


def test_overflowing_lists_fall_back_to_the_dense_planes(hip, lib_options):
    """more exceptions than a list holds, under a cap clamped to that capacity: the counts stay exact, nothing is read past the
    lists, all four planes are summed"""
    m, n, V = 9, 1280, 8
    H = M.hessian("ordinary", n)
    c3, c2 = model_counts(M.quantize(H, 0))
    lib_options(reset=OPTIONS, GANQ_ACCUM_W4=1, GANQ_H_EXT=0, GANQ_T_TOP_CAP=10 ** 9)
    got = hip.debug_top_planes(dev(H), m)
    assert got["cap"] == got["list_max"] < c3 < c2, (got, c3, c2)
    check_sums(hip, lib_options, m, n, V, 0, H, M.pattern("uniform", m, n, V), [(10 ** 9, 4)])


PLANT_AT = lambda n: ((1, 0), (n - 1, 0), (n - 1, n - 2), (32, 31), (128, 127), (129, 127))  # noqa: E731  chunk and slice borders


def planted_hessian(n, ext_mode):
    """an "ordinary" H whose off-diagonals are scaled down until no entry reaches digit 2, then six planted symmetric entries:
    +-max|H| (I = +-2^30, digit 3 = +-64), digit 3 zero and digit 2 = 127 / -128, and one just below each threshold.
    -> (H, the six words I as the model quantises them)"""
    H = M.hessian("ordinary", n).astype(np.float64)
    d = np.diag(H).copy()
    off = H - np.diag(d)
    mx = float(np.float32(d.max()))
    off *= (mx * 2.0 ** -16) / np.abs(off).max()  # |I| <= 2^14 off the diagonal
    H = off + np.diag(d)
    unit = mx / 2.0 ** 30
    words = (2 ** 30, -2 ** 30, 127 * 65536 + 5 * 256 + 7, -128 * 65536 + 5 * 256 + 7, 32500, 127 * 65536 + 32000)
    for (u, v), w in zip(PLANT_AT(n), words):
        H[u, v] = H[v, u] = w * unit
        H[u, u] = H[v, v] = mx  # (keeps |H_uv| <= sqrt(H_uu H_vv))
    H = np.ascontiguousarray(H.astype(np.float32))
    assert np.array_equal(H, H.T)
    q = M.quantize(H, ext_mode)
    return H, q


@pytest.mark.parametrize("n,m,V,ext_mode,pk", [(256, 33, 16, 0, "uniform"), (256, 9, 4, 1, "one_code_per_group64"),
                                               (512, 1, 8, 0, "edge_columns"), (512, 33, 16, 1, "uniform"),
                                               (1280, 9, 8, 0, "unused_codes"), (1280, 1, 16, 1, "one_code_per_row")])
def test_planted_entries_at_chunk_and_slice_borders(hip, lib_options, n, m, V, ext_mode, pk):
    H, q = planted_hessian(n, ext_mode)
    ds, _ = M.digits(q["I"], 4)
    at = PLANT_AT(n)
    d3 = [int(ds[3][v, u]) for u, v in at]
    d2 = [int(ds[2][v, u]) for u, v in at]
    # what the six entries were planted for: both signs of the top digit, both ends of digit 2, and the two that stay below
    assert d3 == [64, -64, 0, 0, 0, 0] and d2 == [0, 0, 127, -128, 0, 127], (d3, d2)
    assert int(q["I"][at[4][1], at[4][0]]) > 32000 and int(q["I"][at[5][1], at[5][0]]) > 127 * 65536 + 31000
    assert model_counts(q) == (2, 5)  # nothing but the planted entries reaches digit 2
    check_sums(hip, lib_options, m, n, V, ext_mode, H, M.pattern(pk, m, n, V), [(5, 2), (4, 3), (2, 3), (1, 4)])


def massive_settings(n, ext_mode):
    H = M.hessian("massive", n)
    c3, c2 = model_counts(M.quantize(H, ext_mode))
    assert c3 < c2
    return H, (c3, c2), ((c2, 2), (c2 - 1, 3))


@pytest.mark.parametrize("m,n,V,ext_mode", [(33, 512, 16, 1), (9, 1280, 8, 0)])
def test_reaccumulation_keeps_no_state(hip, lib_options, m, n, V, ext_mode):
    """GANQ_T_FULL=1: both iterations of a sequence are summed in full into the same partial sums, fix-up included"""
    H, counts, settings = massive_settings(n, ext_mode)
    W = M.weights(m, n)
    q = M.quantize(H, ext_mode)
    Qs = np.stack([M.pattern("uniform", m, n, V), M.pattern("unused_codes", m, n, V, seed=1)])
    want = [M.model_sums(q, Qs[k]) for k in range(2)]
    for cap, D in settings:
        use_top(hip, lib_options, m, n, H, ext_mode, -1, cap, D, counts, GANQ_T_FULL=1)
        res = entry(hip, W, H, Qs, V)
        assert (res["full_ran"] == 1).all() and res["Qprev"] is None
        for k in range(2):
            assert np.array_equal(res["F_hi"][k], want[k]["F_hi"]), (D, k)
            assert np.array_equal(res["F_lo"][k], want[k]["F_lo"]), (D, k)


@pytest.mark.parametrize("m,n,V,ext_mode", [(33, 768, 16, 1), (8, 256, 4, 0)])
def test_gated_device_side_fallback(hip, lib_options, m, n, V, ext_mode):
    """GANQ_T_INCR_THR=0: the second iteration opens the gate and everything is summed again, fix-up included; an unchanged third
    iteration finds the gate shut: the fix-up, too, must leave the sums alone"""
    H, counts, settings = massive_settings(n, ext_mode)
    W = M.weights(m, n)
    q = M.quantize(H, ext_mode)
    Q0 = M.pattern("uniform", m, n, V)
    Q1 = Q0.copy()
    Q1[m // 2, [0, 31, 32, n - 1]] = (Q1[m // 2, [0, 31, 32, n - 1]] + 1) % V
    Q1[0, 129] = (Q1[0, 129] + 1) % V
    want = [M.model_sums(q, Q) for Q in (Q0, Q1)]
    for cap, D in settings:
        use_top(hip, lib_options, m, n, H, ext_mode, -1, cap, D, counts, GANQ_T_INCR_THR=0)
        res = entry(hip, W, H, np.stack([Q0, Q1, Q1]), V)
        assert res["full_ran"].tolist() == [1, 1, 0]
        for k, Q in enumerate((Q0, Q1, Q1)):
            s = want[min(k, 1)]
            assert np.array_equal(res["F_hi"][k], s["F_hi"]), (D, k)
            assert np.array_equal(res["F_lo"][k], s["F_lo"]), (D, k)
            assert np.array_equal(res["Qprev"][k], Q), (D, k)


@pytest.mark.parametrize("m,n,V,seed", [(64, 512, 16, 31), (33, 768, 8, 32)])
def test_run_layer_same_bytes_with_and_without_the_lists(hip, lib_options, m, n, V, seed):
    from test_hip_stages import synth

    W, H, L, T0 = synth(m, n, V, seed, corr=0.2)
    lib_options(reset=OPTIONS, GANQ_ACCUM_W4=1)
    got = hip.debug_top_planes(dev(H), m)
    c3, c2, top = got["c3"], got["c2"], got["list_max"]
    assert c3 <= top and c3 < c2, got  # three dense planes are within reach of the lists at both shapes
    settings = [(0, -1, 4), (-1, min(c3, c2 - 1), 3)] + ([(-1, c2, 2)] if c2 <= top else [])
    assert n != 512 or len(settings) == 3  # (130816 pairs fit a list: D = 2 as well)
    args = (dev(W), dev(H), dev(L), dev(T0), 3)
    outs = []
    for t, cap, D in settings:
        lib_options(reset=OPTIONS, GANQ_ACCUM_W4=1, GANQ_T_TOP=t, GANQ_T_TOP_CAP=cap)
        assert hip.accum_plan(m, n)["kernel"] == "onehot_accum_w4" and hip.debug_top_planes(dev(H), m)["D"] == D
        T, Q, d, bk = hip.run_layer(*args, alias_q=False)
        outs.append((T.cpu().numpy(), Q.cpu().numpy(), d.cpu().numpy(), int(bk)))
    for other in outs[1:]:
        for a, b in zip(outs[0][:3], other[:3]):
            assert a.tobytes() == b.tobytes()
        assert outs[0][3] == other[3]
