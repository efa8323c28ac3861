"""The incremental bucket sums on the matrix cores reading only the dense digit planes of H (GANQ_MU_TOP, m_update_mfma_kernel with
D < 4 planes + the per-column index of the exception list, top_index_kernel) EXACTLY: after every iteration both words' sums, Qprev
and the path probe are compared with the host model of tests/t_update_model.py and, byte for byte, with GANQ_MU_TOP=0.  The cases
live in tests/mupdate_top_cases.py (tests/test_mupdate_top_model.py checks without a GPU that they are what they claim).
Every case runs under GANQ_MU_TOP = -1 (the full sum's planes), 3 (those, but at least three) and 0 (all four).
GANQ_ACCUM_W4=1 is forced so that lists exist at these sizes; every case asserts the device's exception counts, the D of the full sum
(ganq_debug_top_planes) and of the incremental kernel (ganq_debug_mu_planes), and that the incremental path ran."""
import numpy as np
import pytest
import torch

import mupdate_top_cases as C
import t_update_model as M

pytestmark = pytest.mark.gpu

OPTIONS = ("GANQ_ACCUM_W4", "GANQ_H_EXT", "GANQ_T_FULL", "GANQ_T_INCR_THR", "GANQ_MUPDATE_LDS", "GANQ_SOLVE_ALL_ROWS", "GANQ_T_JACOBI",
           "GANQ_WH_F64", "GANQ_T_TOP", "GANQ_T_TOP_CAP", "GANQ_MU_TOP")


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


def mu_planes(D_full, mu_top):
    """mu_dense_planes: the D of the incremental kernel where the full sum takes D_full"""
    return 4 if mu_top == 0 else (3 if D_full == 2 and mu_top == 3 else D_full)


def in_force(hip, lib_options, case, H, counts, cap, mu_top):
    """the options of the case with GANQ_MU_TOP = mu_top; the plan, the device's counts and both D are what the case means"""
    m, n = case["m"], case["n"]
    lib_options(reset=OPTIONS, GANQ_ACCUM_W4=1, GANQ_H_EXT=case["ext_mode"], GANQ_T_TOP_CAP=cap, GANQ_MU_TOP=mu_top, **case["options"])
    assert hip.accum_plan(m, n)["kernel"] == "onehot_accum_w4"
    got = hip.debug_top_planes(dev(H), m)
    assert (got["c3"], got["c2"]) == counts, (got, counts)
    assert got["D"] == case["D"], got
    assert hip.debug_mu_planes(m, n, got["c3"], got["c2"]) == {"D": mu_planes(case["D"], mu_top), "D_full": case["D"]}


@pytest.mark.parametrize("case", C.CASES, ids=[c["name"] for c in C.CASES])
def test_incremental_sums_with_dense_planes_only(hip, lib_options, case):
    m, n, V = case["m"], case["n"], case["V"]
    H, q, counts, cap, Qseq, changes, _, _ = C.build(case)
    W = M.weights(m, n)
    want = {}
    for Q in Qseq:
        if Q.tobytes() not in want:
            want[Q.tobytes()] = M.model_sums(q, Q)
    got = []
    for mu_top in (-1, 3, 0):
        in_force(hip, lib_options, case, H, counts, cap, mu_top)
        res = entry(hip, W, H, Qseq, V)
        assert int(res["ext"]) == case["ext_mode"]
        path = "".join("F" if f else "I" for f in res["full_ran"])
        assert path == case["expect"], (mu_top, path)
        for k, Q in enumerate(Qseq):
            s = want[Q.tobytes()]
            bad = np.argwhere(res["F_hi"][k] != s["F_hi"])
            assert np.array_equal(res["F_hi"][k], s["F_hi"]), (mu_top, k, len(bad), bad[:4].tolist())
            assert np.array_equal(res["F_lo"][k], s["F_lo"]), (mu_top, k)
            assert np.array_equal(res["Qprev"][k], Q), (mu_top, k)
            assert np.array_equal(res["chgcnt"][k], changes[k]), (mu_top, k)
        got.append((res["F_hi"], res["F_lo"], res["Qprev"], res["full_ran"]))
    for other in got[:2]:
        for a, b in zip(other, got[2]):
            assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("m,n,V,seed", [(64, 512, 16, 41), (33, 768, 8, 42)])
def test_run_layer_same_bytes_with_all_and_with_dense_planes(hip, lib_options, m, n, V, seed):
    W, H, L, T0 = C.massive_layer(m, n, V, seed)
    lib_options(reset=OPTIONS, GANQ_ACCUM_W4=1)
    got = hip.debug_top_planes(dev(H), m)
    c3, c2 = got["c3"], got["c2"]
    assert 0 < c2 <= got["list_max"] and c3 < c2, got
    args = (dev(W), dev(H), dev(L), dev(T0), 4)
    outs = []
    for mu_top in (-1, 3, 0):
        lib_options(reset=OPTIONS, GANQ_ACCUM_W4=1, GANQ_T_TOP_CAP=c2, GANQ_MU_TOP=mu_top)
        assert hip.debug_top_planes(dev(H), m)["D"] == 2
        assert hip.debug_mu_planes(m, n, c3, c2) == {"D": mu_planes(2, mu_top), "D_full": 2}
        T, Q, d, bk = hip.run_layer(*args, alias_q=False)
        # the incremental path did real work: iteration 1 moves its changes when the default gate (m n / 16) is shut, iterations 2
        # and 3 carry no gate at all
        Qa = hip.run_layer_rows(*args, want_q_all=True)["Q_all"].cpu().numpy()
        changed = [int((Qa[k] != Qa[k - 1]).sum()) for k in range(1, 4)]
        assert sum(c for k, c in enumerate(changed, 1) if k >= 2 or c <= (m * n) >> 4) > 0, changed
        outs.append((T.cpu().numpy(), Q.cpu().numpy(), d.cpu().numpy(), int(bk)))
    for other in outs[:2]:
        for a, b in zip(other[:3], outs[2][:3]):
            assert a.tobytes() == b.tobytes()
        assert other[3] == outs[2][3]
