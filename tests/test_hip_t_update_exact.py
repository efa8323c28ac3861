"""The T-update's fixed point and bucket sums, EXACTLY (csrc/update_t.hip against tests/t_update_model.py).

update_t.hip promises that A_i = S_i H S_i^T is formed exactly: H becomes scale * (I + J / 65536) once, the bucket sums of I and J
are int64 integers from a full pass on the int8 matrix cores or moved incrementally between iterations.  The closed-form loss, the
incremental path and the sharded best-of-K decision lean on that.  A tolerance cannot pin it (tests/test_t_update_model.py shows
a dropped digit plane and an ignored extension word staying under the 1e-6 the other A assertions use), but integer sums have one
right answer: everything integer here, and the fp32 A made from it, is compared with array_equal / bitwise.

  a. test_fixed_point_conversion      scale, I, J, the diagonals           (ganq_debug_t_sums)
  b. test_full_accumulation           F of the full pass, stateful and under GANQ_T_FULL=1; A_out of ganq_update_t bitwise;
  d.                                  b_out of ganq_update_t within one fp32 rounding of the fp64 sum
  c. test_incremental_sequence        prescribed per-row change counts, all three move kernels, the gate read off the device

Measured wall time on an MI355X host: see README.md (test overview).
"""
import numpy as np
import pytest
import torch

import t_update_model as M
from conftest import rel_fro

pytestmark = pytest.mark.gpu

TOL_T = 1e-5           # the project's codebook bar (test_hip_stages.py)
TOL_LOSS = 1e-6        # loss on ordinary Hessians (test_hip_stages.py: relative, on the sum over the rows)
TOL_LOSS_ROW = 1e-4    # per-row loss on massive-feature Hessians (test_hip_massive.py: max over rows, relative to the largest row)
OPTIONS = ("GANQ_H_EXT", "GANQ_T_FULL", "GANQ_T_INCR_THR", "GANQ_MUPDATE_LDS", "GANQ_SOLVE_ALL_ROWS", "GANQ_T_JACOBI", "GANQ_WH_F64")


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


bits_equal = M.bits_equal


def assert_conversion(res, q):
    assert float(res["scale"]) == q["scale"]
    assert np.array_equal(res["Hint"], q["I"])
    assert np.array_equal(res["J"], q["J"])
    assert np.array_equal(res["hdiag_int"], np.diag(q["I"]))
    assert np.array_equal(res["hdiag_j"], np.diag(q["J"]))


# ------------------------------------------------------------------------------------------------ a. fixed-point conversion
@pytest.mark.parametrize("kind,n,ext_mode", M.CONVERSION_CASES, ids=[f"{k}-n{n}-ext{e}" for k, n, e in M.CONVERSION_CASES])
def test_fixed_point_conversion(hip, lib_options, kind, n, ext_mode):
    if ext_mode < 0:
        lib_options(reset=OPTIONS)
    else:
        lib_options(reset=OPTIONS, GANQ_H_EXT=ext_mode)
    H = M.hessian(kind, n)
    res = entry(hip, M.weights(1, n), H, np.zeros((1, 1, n), dtype=np.uint8), 4)
    ext = int(res["ext"])
    if ext_mode >= 0:
        assert ext == ext_mode
    else:
        margin = M.ext_margin(H)
        if margin > 2.0 or margin < 0.5:  # far from the boundary: the summation order of the diagonal cannot decide
            assert ext == M.quantize(H, -1)["ext"], margin
    q = M.quantize(H, ext)
    assert_conversion(res, q)
    # the planes the matrix cores read are these words' digits: their sums over the one bucket of this all-zero index row
    sums = M.model_sums(q, np.zeros((1, n), dtype=np.uint8))
    assert np.array_equal(res["F_hi"][0], sums["F_hi"]) and np.array_equal(res["F_lo"][0], sums["F_lo"])


# ------------------------------------------------------------------------------------------------ b. + d. full accumulation
def case_id(c):
    return f"m{c['m']}-n{c['n']}-V{c['V']}-ext{c['ext_mode']}-{c['hessian']}-{c['pattern']}"


@pytest.mark.parametrize("case", M.FULL_CASES, ids=[case_id(c) for c in M.FULL_CASES])
def test_full_accumulation(hip, lib_options, case):
    m, n, V = case["m"], case["n"], case["V"]
    lib_options(reset=OPTIONS, GANQ_H_EXT=case["ext_mode"])
    H, W = M.hessian(case["hessian"], n), M.weights(m, n)
    Q = M.pattern(case["pattern"], m, n, V)
    q = M.quantize(H, case["ext_mode"])
    sums = M.model_sums(q, Q)

    # the loop's first iteration (sums kept for the incremental moves)
    res = entry(hip, W, H, Q[None], V)
    assert int(res["ext"]) == case["ext_mode"]
    assert_conversion(res, q)
    assert np.array_equal(res["F_hi"][0], sums["F_hi"])
    assert np.array_equal(res["F_lo"][0], sums["F_lo"])
    assert np.array_equal(res["Qprev"][0], Q) and int(res["full_ran"][0]) == 1
    assert not res["chgcnt"].any() and (res["active_count"] == -1).all()

    # the public stage call: A_out bitwise, b_out within one fp32 rounding of an fp64 sum of at most n terms
    WH = (W.astype(np.float64) @ H.astype(np.float64)).astype(np.float32)
    _, A, b = hip.update_t(dev(WH), dev(H), dev(Q), V, want_ab=True)
    A_ref = M.A_fp32(q["scale"], q["ext"], sums["F_hi"], sums["D_hi"], sums["F_lo"], sums["D_lo"], V)
    assert bits_equal(A.cpu().numpy(), A_ref)
    b_ref = M.bucket_vector(WH, Q)[:, :V]
    b_abs = M.bucket_vector(WH, Q, absolute=True)[:, :V]
    err = np.abs(b.cpu().numpy().astype(np.float64) - b_ref)
    bound = 2.0 ** -24 * np.abs(b_ref) + n * 2.0 ** -52 * b_abs
    assert (err <= bound).all(), float((err - bound).max())

    # every iteration re-accumulated (GANQ_T_FULL=1): the NP partial sums, summed and symmetrised
    if n <= 1000 or m <= 3:
        lib_options(GANQ_T_FULL=1)
        Q1 = M.pattern("uniform", m, n, V, seed=1)
        res = entry(hip, W, H, np.stack([Q, Q1]), V)
        sums1 = M.model_sums(q, Q1)
        assert (res["full_ran"] == 1).all() and res["Qprev"] is None
        for k, s in enumerate((sums, sums1)):
            assert np.array_equal(res["F_hi"][k], s["F_hi"]), k
            assert np.array_equal(res["F_lo"][k], s["F_lo"]), k


# ------------------------------------------------------------------------------------------------ c. incremental moves
@pytest.mark.parametrize("seq", M.SEQUENCES, ids=[s["name"] for s in M.SEQUENCES])
def test_incremental_sequence(hip, lib_options, seq):
    """After EVERY iteration: both words' sums equal the model's sums of Q_k from scratch, Qprev == Q_k, the change counts are the
    prescribed ones, the active-row list is the changed rows in ascending order, unchanged rows keep codebook and loss bitwise, the
    path (full / incremental) is the expected one, and codebooks and losses meet the project's bars against fp64."""
    m, n, V = seq["m"], seq["n"], seq["V"]
    lib_options(reset=OPTIONS, **seq["options"])  # the extension is decided by the device rule: the cases are far from its boundary
    H, W = M.hessian(seq["hessian"], n), M.weights(m, n)
    Qseq, counts = M.build_sequence(seq)
    K = len(Qseq)
    res = entry(hip, W, H, Qseq, V)
    assert int(res["ext"]) == seq["ext_mode"]
    q = M.quantize(H, seq["ext_mode"])
    assert_conversion(res, q)
    WH = hip.debug_wh_product(dev(W), dev(H))[0].cpu().numpy()  # the entry's own W @ H_fixed, fp64
    wHw = (W.astype(np.float64) * WH).sum(axis=1)
    massive = seq["hessian"] == "massive"
    path = "".join("F" if f else "I" for f in res["full_ran"])
    print(f"[{seq['name']}] path {path}, changed per iteration {counts.sum(axis=1).tolist()}")
    cache = {}
    for k in range(K):
        Q = Qseq[k]
        key = Q.tobytes()
        if key not in cache:
            cache[key] = M.model_sums(q, Q)
        s = cache[key]
        assert np.array_equal(res["F_hi"][k], s["F_hi"]), (k, np.argwhere(res["F_hi"][k] != s["F_hi"])[:4].tolist())
        assert np.array_equal(res["F_lo"][k], s["F_lo"]), (k, np.argwhere(res["F_lo"][k] != s["F_lo"])[:4].tolist())
        assert np.array_equal(res["Qprev"][k], Q), k
        assert np.array_equal(res["chgcnt"][k], counts[k]), k
        assert path[k] == seq["expect"][k], (k, path, seq["expect"])
        if k >= 1:
            changed = np.flatnonzero(counts[k] > 0)
            assert int(res["active_count"][k]) == len(changed), k
            assert np.array_equal(res["active_rows"][k][:len(changed)], changed), k
            same = np.flatnonzero(counts[k] == 0)
            assert bits_equal(res["T_all"][k][same], res["T_all"][k - 1][same]), k
            assert np.array_equal(res["loss_rows_all"][k][same].view(np.uint64), res["loss_rows_all"][k - 1][same].view(np.uint64)), k
        else:
            assert int(res["active_count"][0]) == -1
        # codebooks: fp64 minimum-norm solve of the model's fp32 A with b the fp64 bucket sum of the entry's own W @ H_fixed
        A32 = M.A_fp32(q["scale"], q["ext"], s["F_hi"], s["D_hi"], s["F_lo"], s["D_lo"], V)
        b64 = M.bucket_vector(WH, Q)[:, :V]
        T_ref = M.solve_fp64(A32, b64.astype(np.float32), V)
        e_t = rel_fro(res["T_all"][k], T_ref)
        # losses: w^T H w - 2 t^T b + t^T A t in fp64 with the unrounded A, at the device's own codebook
        t = res["T_all"][k].astype(np.float64)
        A64 = M.A_fp64(q["scale"], q["ext"], s["F_hi"], s["D_hi"], s["F_lo"], s["D_lo"], V)
        loss_ref = wHw - 2.0 * (t * b64).sum(axis=1) + np.einsum("ia,iab,ib->i", t, A64, t)
        got = res["loss_rows_all"][k]
        e_sum = abs(got.sum() - loss_ref.sum()) / abs(loss_ref.sum())
        e_row = np.abs(got - loss_ref).max() / np.abs(loss_ref).max()
        print(f"[{seq['name']}] iteration {k}: codebook rel. Frobenius {e_t:.3e}, loss sum {e_sum:.3e}, loss rows {e_row:.3e}")
        assert e_t < TOL_T, (k, e_t)
        if massive:
            assert e_row < TOL_LOSS_ROW, (k, e_row)
        else:
            assert e_sum <= TOL_LOSS, (k, e_sum)
