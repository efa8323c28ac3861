"""The four-wave full bucket sum (onehot_accum_w4_kernel, GANQ_ACCUM_W4=1) EXACTLY: against the host model of
tests/t_update_model.py and against the first kernel (GANQ_ACCUM_W4=0).  Integer sums have one right answer, so everything is
compared with array_equal / bitwise; the plan query is asserted before every run, so that no case passes on the fallback.

Shapes, the smallest at which the kernel can go wrong (slices of 128 columns, a ring of four LDS stages, chunks of 32 columns dealt
to eight parts): n = 256 every slice crosses the diagonal, one chunk per part; 512 the first plain slice, two chunks per part,
the request for the next chunk; 768; 1280 more slices than stages, the ring wraps; 2304 it wraps twice, many chunks per part.
m: half-filled row pairs, a wave with one row, a workgroup with one row, three row groups."""
import numpy as np
import pytest
import torch

import t_update_model as M

pytestmark = pytest.mark.gpu

OPTIONS = ("GANQ_ACCUM_W4", "GANQ_H_EXT", "GANQ_T_FULL", "GANQ_T_INCR_THR", "GANQ_MUPDATE_LDS", "GANQ_SOLVE_ALL_ROWS", "GANQ_T_JACOBI",
           "GANQ_WH_F64")
W4_N = (256, 512, 768, 1280, 2304)
W4_M = (1, 7, 8, 9, 31, 32, 33, 65)
W4_M_WIDE = (1, 7, 8, 9, 31, 32, 33)  # from n = 1280 on (host model time)
W4_HESSIANS = ("ordinary", "massive", "negative_offdiag", "clamp", "zero")


def _cases():
    """every n four times; m, V, the extension, the Hessian and the pattern dealt round-robin with strides coprime to the axis
    lengths; then the nasty pairs by hand"""
    cases = []
    for j in range(20):
        n = W4_N[j % 5]
        ms = W4_M if n < 1280 else W4_M_WIDE
        cases.append({"m": ms[j % len(ms)], "n": n, "V": M.FULL_V[(j + j // 5) % 3], "ext_mode": (j + j // 5) % 2,
                      "hessian": W4_HESSIANS[(2 * j + j // 5) % 5], "pattern": M.PATTERNS[(j + j // 10) % 5]})
    for m, n, V, ext_mode, hk, pk in [(65, 256, 16, 1, "clamp", "one_code_per_group64"),   # the diagonal block with digits at the ends of int8
                                      (1, 256, 4, 0, "clamp", "edge_columns"),             # a workgroup with one row
                                      (9, 512, 16, 1, "massive", "one_code_per_row"),      # a wave with one row, one bucket per row
                                      (33, 2304, 8, 1, "negative_offdiag", "edge_columns"),
                                      (65, 768, 16, 0, "zero", "uniform")]:
        cases.append({"m": m, "n": n, "V": V, "ext_mode": ext_mode, "hessian": hk, "pattern": pk})
    return cases


CASES = _cases()


def case_id(c):
    return f"m{c['m']}-n{c['n']}-V{c['V']}-ext{c['ext_mode']}-{c['hessian']}-{c['pattern']}"


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


def use_kernel(hip, lib_options, w4, m, n, **opts):
    lib_options(reset=OPTIONS, GANQ_ACCUM_W4=w4, **opts)
    want = "onehot_accum_w4" if w4 else "onehot_accum"
    assert hip.accum_plan(m, n)["kernel"] == want, (m, n, hip.accum_plan(m, n))


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_full_accumulation_w4(hip, lib_options, case):
    m, n, V = case["m"], case["n"], case["V"]
    H, W = M.hessian(case["hessian"], n), M.weights(m, n)
    Q = M.pattern(case["pattern"], m, n, V)
    q = M.quantize(H, case["ext_mode"])
    sums = M.model_sums(q, Q)
    WH = (W.astype(np.float64) @ H.astype(np.float64)).astype(np.float32)
    A_ref = M.A_fp32(q["scale"], q["ext"], sums["F_hi"], sums["D_hi"], sums["F_lo"], sums["D_lo"], V)
    got = {}
    for w4 in (1, 0):
        use_kernel(hip, lib_options, w4, m, n, GANQ_H_EXT=case["ext_mode"])
        res = entry(hip, W, H, Q[None], V)
        assert int(res["ext"]) == case["ext_mode"]
        assert int(res["full_ran"][0]) == 1, w4
        bad = np.argwhere(res["F_hi"][0] != sums["F_hi"])
        assert np.array_equal(res["F_hi"][0], sums["F_hi"]), (w4, len(bad), bad[:4].tolist())
        assert np.array_equal(res["F_lo"][0], sums["F_lo"]), w4
        assert np.array_equal(res["Qprev"][0], Q), w4
        _, A, _ = hip.update_t(dev(WH), dev(H), dev(Q), V, want_ab=True)  # the stateless stage call
        assert M.bits_equal(A.cpu().numpy(), A_ref), w4
        got[w4] = (res["F_hi"][0], res["F_lo"][0], A.cpu().numpy())
    # the two kernels agree with each other, not only with the model
    for a, b in zip(got[1], got[0]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("m,n,V,ext_mode,hk", [(33, 512, 16, 1, "massive"), (9, 1280, 8, 0, "ordinary")])
def test_reaccumulation_keeps_no_state(hip, lib_options, m, n, V, ext_mode, hk):
    """GANQ_T_FULL=1: both iterations of a sequence are summed in full into the same partial sums"""
    H, W = M.hessian(hk, n), M.weights(m, n)
    q = M.quantize(H, ext_mode)
    Qs = np.stack([M.pattern("uniform", m, n, V), M.pattern("unused_codes", m, n, V, seed=1)])
    use_kernel(hip, lib_options, 1, m, n, GANQ_H_EXT=ext_mode, GANQ_T_FULL=1)
    res = entry(hip, W, H, Qs, V)
    assert (res["full_ran"] == 1).all() and res["Qprev"] is None
    for k in range(2):
        s = M.model_sums(q, Qs[k])
        assert np.array_equal(res["F_hi"][k], s["F_hi"]), k
        assert np.array_equal(res["F_lo"][k], s["F_lo"]), k


@pytest.mark.parametrize("m,n,V,ext_mode,hk", [(33, 768, 16, 1, "massive"), (8, 256, 4, 0, "ordinary")])
def test_gated_device_side_fallback(hip, lib_options, m, n, V, ext_mode, hk):
    """GANQ_T_INCR_THR=0: the second iteration changes a few indices, which is more than the threshold, so the device opens the gate
    and the four-wave kernel sums everything again -- behind the incremental kernels that left at once; an unchanged third iteration
    finds the gate shut and must leave the sums alone"""
    H, W = M.hessian(hk, n), M.weights(m, n)
    q = M.quantize(H, ext_mode)
    Q0 = M.pattern("uniform", m, n, V)
    Q1 = Q0.copy()
    Q1[m // 2, [0, 31, 32, n - 1]] = (Q1[m // 2, [0, 31, 32, n - 1]] + 1) % V
    Q1[0, 129] = (Q1[0, 129] + 1) % V
    use_kernel(hip, lib_options, 1, m, n, GANQ_H_EXT=ext_mode, GANQ_T_INCR_THR=0)
    res = entry(hip, W, H, np.stack([Q0, Q1, Q1]), V)
    assert res["full_ran"].tolist() == [1, 1, 0]
    for k, Q in enumerate((Q0, Q1, Q1)):
        s = M.model_sums(q, Q)
        assert np.array_equal(res["F_hi"][k], s["F_hi"]), k
        assert np.array_equal(res["F_lo"][k], s["F_lo"]), k
        assert np.array_equal(res["Qprev"][k], Q), k


@pytest.mark.parametrize("m,n,V,seed", [(64, 512, 16, 31), (33, 768, 8, 32)])
def test_run_layer_same_bytes_under_both_kernels(hip, lib_options, m, n, V, seed):
    from test_hip_stages import synth

    W, H, L, T0 = synth(m, n, V, seed, corr=0.2)
    args = (dev(W), dev(H), dev(L), dev(T0), 3)
    outs = {}
    for w4 in (0, 1):
        use_kernel(hip, lib_options, w4, m, n)
        T, Q, d, bk = hip.run_layer(*args, alias_q=False)
        outs[w4] = (T.clone(), Q.clone(), d.clone(), int(bk))
    for a, b in zip(outs[0][:3], outs[1][:3]):
        assert torch.equal(a, b) and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert outs[0][3] == outs[1][3]
