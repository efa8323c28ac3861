"""GPU parity tests: every stage of the HIP path, called through the C-ABI (ganq_amd._lib), against
the CPU oracle on the same inputs and against the committed golden vectors.

Bars (BASELINE.json north_star): assignment indices bit-exact; codebooks / reconstructed weights within
1e-5 relative Frobenius; the loss is checked to 1e-6 relative.
"""
import numpy as np
import pytest
import torch

import t_update_model
from conftest import golden_names, load_golden, rel_fro

pytestmark = pytest.mark.gpu

TOL_T = 1e-5
TOL_LOSS = 1e-6


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


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def synth(m, n, V, seed, corr=0.0):
    """seeded synthetic (W, H, L, T0) with a well-conditioned Hessian"""
    rng = np.random.default_rng(seed)
    W = (0.02 * rng.standard_normal((m, n))).astype(np.float32)
    p = max(2 * n, 256)
    X = rng.standard_normal((p, n)).astype(np.float32) * (0.1 + rng.random(n)).astype(np.float32)
    if corr:
        X = (1 - corr) * X + corr * (X @ (rng.standard_normal((n, n)) / np.sqrt(n)).astype(np.float32))
    H = (2.0 / p) * (X.T.astype(np.float64) @ X.astype(np.float64))
    H += 0.01 * np.mean(np.diag(H)) * np.eye(n)
    H = H.astype(np.float32)
    Hd = H.astype(np.float64)
    off = np.clip(np.abs(Hd).sum(1) - 2 * np.diag(Hd), 1e-8, None)
    L = np.linalg.cholesky(Hd + np.diag(off)).astype(np.float32)
    qs = (np.arange(V) + 0.5) / V
    T0 = np.quantile(W, qs, axis=1).T.astype(np.float32).copy()
    return W, H, L, T0


# ------------------------------------------------------------------------------------------ S-solve
@pytest.mark.parametrize("name", golden_names())
def test_solve_s_golden_bit_exact(hip, name):
    g = load_golden(name)
    for k in range(int(g["K"])):
        Q = hip.solve_s(dev(g["W_perm"]), dev(g["L"]), dev(g["T"][k])).cpu().numpy()
        assert np.array_equal(Q, g["Q"][k]), f"{name} it {k}: {(Q != g['Q'][k]).sum()} mismatches vs the reference"


@pytest.mark.parametrize("m,n,V,seed", [(16, 64, 16, 1), (40, 200, 16, 2), (64, 320, 8, 3), (17, 100, 4, 4),
                                        (256, 1024, 16, 5), (100, 1536, 8, 6),
                                        # wider than the 1792 Err columns kept in LDS, ragged panel / k-group counts
                                        (20, 1850, 16, 7), (33, 2001, 8, 8), (16, 1793, 16, 9), (18, 3000, 16, 10)])
def test_solve_s_vs_oracle_bit_exact(hip, oracle, m, n, V, seed):
    W, H, L, T0 = synth(m, n, V, seed, corr=0.2 if seed % 2 else 0.0)
    Q, Err = hip.solve_s(dev(W), dev(L), dev(T0), want_err=True)
    Qo, Erro = oracle.solve_s(W, L, T0, want_err=True)
    Q = Q.cpu().numpy()
    assert np.array_equal(Q, Qo), f"{(Q != Qo).sum()} of {Q.size} indices differ"
    assert np.array_equal(Err.cpu().numpy(), Erro)


def test_solve_s_reference_test_recipe(hip, oracle):
    # the reference's own kernel test recipe (tests/test_ganq_solve_s_kernel.py:7-13): m,v,n = 768,16,2304,
    # W ~ N(0,1), L = tril(N(0,1)), codebook ~ N(0,1); it asserts exact index equality kernel vs loop
    g = torch.Generator().manual_seed(42)
    m, v, n = 768, 16, 2304
    W = torch.randn(m, n, generator=g)
    L = torch.tril(torch.randn(n, n, generator=g))
    C = torch.randn(m, v, generator=g)
    Q = hip.solve_s(W.cuda(), L.cuda(), C.cuda()).cpu().numpy()
    Qo = oracle.solve_s(W.numpy(), L.numpy(), C.numpy())
    assert np.array_equal(Q, Qo), f"{(Q != Qo).sum()} of {Q.size} indices differ"


def test_solve_s_ties_and_duplicates(hip, oracle):
    # duplicate codebook entries and exact ties: first minimum must win (ganq.py:115, :547)
    W, H, L, T0 = synth(32, 128, 16, 9)
    T0[:, 5] = T0[:, 4]
    T0[:, 9] = 0.0
    T0[:, 10] = 0.0
    W[:, ::7] = 0.0
    Q = hip.solve_s(dev(W), dev(L), dev(T0)).cpu().numpy()
    assert np.array_equal(Q, oracle.solve_s(W, L, T0))
    assert not (Q == 5).any() and not (Q == 10).any()


@pytest.mark.parametrize("case", ["unsorted", "reversed_midpoints", "signed_zeros", "near_duplicates", "huge_residuals",
                                  "nan_codebook", "one_value", "descending"])
def test_solve_s_threshold_path_adversarial_codebooks(hip, oracle, case, lib_options):
    """the S-solve decides the argmin by per-lane thresholds on the SORTED codebook and falls back to the first-minimum
    reductions where that is not exact; both must give the oracle's indices on codebooks built to break the shortcut, and
    the same bits as the reductions alone (GANQ_SOLVE_VARIANT=1)"""
    m, n, V = 48, 256, 16
    W, H, L, T0 = synth(m, n, V, 21, corr=0.1)
    rng = np.random.default_rng(4)
    if case == "unsorted":
        T0 = rng.permuted(T0, axis=1)
    elif case == "reversed_midpoints":
        # pairs of entries whose mid-point is hit EXACTLY by weights, with the larger value at the smaller index: a tie must
        # go to the smaller ORIGINAL index, i.e. to the larger value
        T0 = np.tile(np.array([0.5, 0.25, 0.125, 0.0625, -0.5, -0.25, -0.125, -0.0625, 1.0, 2.0, 3.0, 4.0, -1.0, -2.0, -3.0, -4.0],
                              dtype=np.float32), (m, 1))
        W[:, ::3] = 0.375   # mid-point of 0.5 and 0.25
        W[:, 1::5] = -0.1875
        L = np.eye(n, dtype=np.float32)  # no residual: eff == w exactly
    elif case == "signed_zeros":
        T0[:, 3] = 0.0
        T0[:, 7] = -0.0
        T0[:, 11] = 0.0
        W[:, ::4] = 0.0
    elif case == "near_duplicates":
        T0[:, 5] = np.nextafter(T0[:, 4], np.float32(1.0))  # one float apart: no collision-free range -> reductions
        T0[:, 9] = np.nextafter(np.nextafter(T0[:, 8], np.float32(1.0)), np.float32(1.0))
    elif case == "huge_residuals":
        W[::2, -1] = 3.0e6   # the first solved column leaves residuals far outside the codebook's range
        W[1::4, -2] = -1.0e30
    elif case == "nan_codebook":
        T0[3, 6] = np.nan
        T0[10, 0] = np.nan
    elif case == "one_value":
        T0[:] = 0.01
    elif case == "descending":
        T0 = np.ascontiguousarray(T0[:, ::-1])
    outs = []
    for variant in (0, 1):
        lib_options(GANQ_SOLVE_VARIANT=variant)
        outs.append(hip.solve_s(dev(W), dev(L), dev(T0)).cpu().numpy())
    assert np.array_equal(outs[0], outs[1]), f"{case}: threshold path differs from the reductions in {(outs[0] != outs[1]).sum()} indices"
    if True:  # (NaN entries included: the oracle scans like torch.argmin -- first NaN wins -- pinned by tests/test_golden_large.py)
        assert np.array_equal(outs[0], oracle.solve_s(W, L, T0)), case
    if case == "reversed_midpoints":  # the ties went to the smaller original index (= the value of larger magnitude here)
        assert (outs[0][:, 3] == 0).all() and (outs[0][:, 1] == 5).all()


@pytest.mark.parametrize("m,n,V,seed", [(300, 1536, 16, 31), (2048, 2048, 16, 32), (37, 4100, 8, 33), (130, 700, 16, 34)])
def test_solve_s_helper_workgroups_bit_identical(hip, oracle, m, n, V, seed, lib_options):
    """Launches with at most half as many tiles as CUs give every tile a helper workgroup that computes the far part of each
    residual chain on another CU and hands the accumulators over through memory (solve_s.hip, "duo").  Same MFMAs in the same
    order: the indices AND the errors must be the bits of the single-workgroup solve, whatever the split policy -- and also
    when the helpers never answer (GANQ_SOLVE_DUO=2: the tile's chain waves time out once and compute everything themselves)."""
    W, H, L, T0 = synth(m, n, V, seed, corr=0.1)
    if seed == 31:  # rows with a NaN codebook entry next to ordinary rows of the same tile (MFMA rows are independent)
        T0[5, 3] = np.nan
        T0[170, 0] = np.nan
    Wd, Ld, Td = dev(W), dev(L), dev(T0)
    lib_options(GANQ_SOLVE_DUO=0)
    Q0, E0 = hip.solve_s(Wd, Ld, Td, want_err=True)
    runs = [dict(GANQ_SOLVE_DUO=1), dict(GANQ_SOLVE_DUO=2), dict(GANQ_SOLVE_DUO=1, GANQ_SOLVE_TRIO=0),
            # two helpers per tile (launches with at most a third as many tiles as CUs): the tile keeps nearly nothing / nearly all
            dict(GANQ_SOLVE_DUO=1, GANQ_SOLVE_TRIO=1, GANQ_SOLVE_TRIO_XA=0, GANQ_SOLVE_TRIO_XB=0),
            dict(GANQ_SOLVE_DUO=1, GANQ_SOLVE_TRIO=1, GANQ_SOLVE_TRIO_XA=56, GANQ_SOLVE_TRIO_XB=2),
            dict(GANQ_SOLVE_DUO=2, GANQ_SOLVE_TRIO=1, GANQ_SOLVE_TRIO_XA=26, GANQ_SOLVE_TRIO_XB=8),
            dict(GANQ_SOLVE_DUO=1, GANQ_SOLVE_DUO_XA=0, GANQ_SOLVE_DUO_XB=0, GANQ_SOLVE_DUO_XMIN=1, GANQ_SOLVE_DUO_CMIN=1),   # all but one panel far
            dict(GANQ_SOLVE_DUO=1, GANQ_SOLVE_DUO_XA=60, GANQ_SOLVE_DUO_XB=0, GANQ_SOLVE_DUO_XMIN=1, GANQ_SOLVE_DUO_CMIN=3),  # nearly all near
            dict(GANQ_SOLVE_DUO=1, GANQ_SOLVE_DUO_XA=20, GANQ_SOLVE_DUO_XB=5, GANQ_SOLVE_DUO_XMIN=3, GANQ_SOLVE_DUO_CMIN=12)]
    for opts in runs:
        lib_options(reset=("GANQ_SOLVE_TRIO", "GANQ_SOLVE_TRIO_XA", "GANQ_SOLVE_TRIO_XB"), **opts)
        for _ in range(2):  # twice: the flags of the first launch must not satisfy the second
            Q1, E1 = hip.solve_s(Wd, Ld, Td, want_err=True)
            assert torch.equal(Q0, Q1), f"{opts}: {(Q0 != Q1).sum().item()} indices differ from the single-workgroup solve"
            assert torch.equal(E0.view(torch.int32), E1.view(torch.int32)), f"{opts}: errors differ"
    rows = np.unique(np.r_[0:min(m, 24), 160:min(m, 176), m - 8:m])
    assert np.array_equal(Q0.cpu().numpy()[rows], oracle.solve_s(W[rows], L, T0[rows]))


def test_solve_s_helper_workgroups_on_concurrent_streams(hip, lib_options):
    """Three helped launches at once (round 3's looper quantized the followers of a group on side streams with helpers; a
    second process on the GPU does the same to any launch): each asks for 128 tiles + 128 helpers, together three times the
    chip.  Whatever subset of the workgroups is resident, a tile either has its helper or finishes without it -- the indices
    must be those of the launches run one after the other -- and a helper that is not resident may cost a tile ONE wait of
    DUO_TIMEOUT (0.5 ms since round 4; 0.2 s before), so the three launches side by side must not take much longer than one
    after the other; the same bound holds for helpers that never answer (GANQ_SOLVE_DUO=2)."""
    import time

    outs, data = [], []
    for seed in (41, 42, 43):
        W, H, L, T0 = synth(2048, 1024, 16, seed, corr=0.1)
        data.append((dev(W), dev(L), dev(T0)))
    ref = [hip.solve_s(*d) for d in data]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        for d in data:
            hip.solve_s(*d)
    torch.cuda.synchronize()
    t_seq = (time.perf_counter() - t0) / 3
    streams = [torch.cuda.Stream() for _ in data]
    t_conc = []
    for rnd in range(4):  # (round 0 is not timed: a stream's first launch allocates its workspace -- 18 ms on a cold allocator)
        outs = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for st, d in zip(streams, data):
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                outs.append(hip.solve_s(*d))
        for st in streams:
            torch.cuda.current_stream().wait_stream(st)
        torch.cuda.synchronize()
        if rnd:
            t_conc.append(time.perf_counter() - t0)
        for o, r in zip(outs, ref):
            assert torch.equal(o, r)
    lib_options(GANQ_SOLVE_DUO=2)  # helpers that never answer: every chain wave times out once, then works alone
    hip.solve_s(*data[0])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    Qm = hip.solve_s(*data[0])
    torch.cuda.synchronize()
    t_muted = time.perf_counter() - t0
    assert torch.equal(Qm, ref[0])
    print(f"solve_s 2048 x 1024, three launches: one after the other {t_seq * 1e3:.2f} ms, side by side {min(t_conc) * 1e3:.2f} .. "
          f"{max(t_conc) * 1e3:.2f} ms; one launch with muted helpers {t_muted * 1e3:.2f} ms")
    assert max(t_conc) < 2.0 * t_seq + 5e-3, "helped launches side by side wait for each other (time-outs?)"
    assert t_muted < t_seq / 3 * 2.0 + 5e-3, "a tile whose helper never answers must lose about one DUO_TIMEOUT, not more"


def test_solve_s_helper_workgroups_beside_another_process(hip):
    """A second PROCESS keeps every CU busy with large matrix products while helped S-solve launches run: the helper of a tile may
    then not be resident for a long time.  The indices must be those of the quiet run, and no launch may take anywhere near the
    old 9 ms (20 M shader cycles) per abandoned helper wait, let alone hang: the tile-side wait is 0.5 ms since round 4."""
    import subprocess
    import sys
    import time

    W, H, L, T0 = synth(1024, 2048, 16, 51, corr=0.1)   # 64 tiles: two helpers per tile when the chip is free
    d = (dev(W), dev(L), dev(T0))
    ref = hip.solve_s(*d)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        hip.solve_s(*d)
    torch.cuda.synchronize()
    quiet = (time.perf_counter() - t0) / 5
    busy = ("import torch, time, sys\n"
            "a = torch.randn(8192, 8192, device='cuda', dtype=torch.float16)\n"
            "torch.cuda.synchronize(); print('busy', flush=True)\n"
            "t0 = time.time()\n"
            "while time.time() - t0 < 8.0:\n"
            "    for _ in range(20): b = a @ a\n"
            "    torch.cuda.synchronize()\n")
    proc = subprocess.Popen([sys.executable, "-c", busy], stdout=subprocess.PIPE, text=True)
    try:
        assert proc.stdout.readline().strip() == "busy"
        time.sleep(0.2)
        worst = 0.0
        for _ in range(10):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            Q = hip.solve_s(*d)
            torch.cuda.synchronize()
            worst = max(worst, time.perf_counter() - t0)
            assert torch.equal(Q, ref)
    finally:
        proc.kill()
        proc.wait()
    print(f"solve_s 1024 x 2048 with helpers: {quiet * 1e3:.2f} ms alone, worst of 10 beside a process saturating the GPU {worst * 1e3:.2f} ms")
    assert worst < 0.25, "a helped launch beside another process took longer than 0.25 s"


def test_solve_s_strided_L_and_empty(hip, oracle):
    W, H, L, T0 = synth(16, 96, 16, 10)
    Lbig = torch.zeros(96, 160, device="cuda")
    Lbig[:, :96] = dev(L)
    Q = hip.solve_s(dev(W), Lbig[:, :96], dev(T0)).cpu().numpy()
    assert np.array_equal(Q, oracle.solve_s(W, L, T0))
    Qe = hip.solve_s(torch.empty(0, 96, device="cuda"), dev(L), torch.empty(0, 16, device="cuda"))
    assert Qe.shape == (0, 96)


def test_solve_s_rejects_unsupported(hip):
    W, H, L, T0 = synth(16, 64, 16, 11)
    with pytest.raises(hip.GanqHipError):
        hip.solve_s(dev(W), dev(L), torch.zeros(16, 256, device="cuda"))  # bits=8 not implemented
    with pytest.raises(hip.GanqHipError):
        hip.solve_s(torch.from_numpy(W), dev(L), dev(T0))  # CPU tensor: no fallback


# ------------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("m,k,n", [(64, 64, 64), (100, 77, 130), (256, 512, 384), (31, 1000, 17)])
def test_matmul_f32(hip, m, k, n):
    g = torch.Generator().manual_seed(m + k + n)
    A = torch.randn(m, k, generator=g)
    B = torch.randn(k, n, generator=g)
    C = hip.matmul_f32(A.cuda(), B.cuda()).cpu()
    ref = (A.double() @ B.double())
    assert rel_fro(C.numpy(), ref.numpy()) < 2e-7 * np.sqrt(k)


# ------------------------------------------------------------------------------------------ T-update
@pytest.mark.parametrize("name", golden_names())
def test_update_t_golden(hip, name):
    g = load_golden(name)
    V = 2 ** int(g["bits"])
    W, H = dev(g["W_perm"]), dev(g["Xxt_damped"])
    WH = hip.matmul_f32(W, H)
    for k in range(int(g["K"])):
        T, A, b = hip.update_t(WH, H, dev(g["Q"][k]), V, want_ab=True)
        assert rel_fro(A.cpu().numpy(), g["A"][k]) < 1e-6
        assert t_update_model.bits_equal(A.cpu().numpy(), t_update_model.stage_A(g["Xxt_damped"], g["Q"][k], V))  # exact integer sums
        assert rel_fro(b.cpu().numpy(), g["B"][k]) < 1e-6
        assert rel_fro(T.cpu().numpy(), g["T"][k + 1]) < TOL_T


@pytest.mark.parametrize("m,n,V,seed", [(48, 300, 16, 21), (64, 640, 8, 22), (33, 130, 4, 23), (96, 1024, 16, 24)])
def test_update_t_vs_oracle(hip, oracle, m, n, V, seed):
    W, H, L, T0 = synth(m, n, V, seed, corr=0.3)
    Q = oracle.solve_s(W, L, T0)
    WH = oracle.matmul(W, H)
    To, Ao, bo = oracle.update_t(WH, H, Q, V, want_ab=True)
    T, A, b = hip.update_t(dev(WH), dev(H), dev(Q), V, want_ab=True)
    assert rel_fro(A.cpu().numpy(), Ao) < 1e-6
    assert t_update_model.bits_equal(A.cpu().numpy(), t_update_model.stage_A(H, Q, V))  # exact integer sums (t_update_model.py)
    assert rel_fro(b.cpu().numpy(), bo) < 1e-6
    assert rel_fro(T.cpu().numpy(), To) < TOL_T


def test_update_t_unused_code_is_zero(hip, oracle):
    # SURVEY 7 hard part 1: an unused codebook entry must come out as exactly the min-norm 0
    W, H, L, T0 = synth(32, 256, 16, 25)
    Q = oracle.solve_s(W, L, T0)
    Q[Q == 7] = 8
    Q[5, Q[5] == 3] = 2
    WH = oracle.matmul(W, H)
    T = hip.update_t(dev(WH), dev(H), dev(Q), 16).cpu().numpy()
    assert np.all(np.abs(T[:, 7]) < 1e-7) and abs(T[5, 3]) < 1e-7
    assert rel_fro(T, oracle.update_t(WH, H, Q, 16)) < TOL_T


# ------------------------------------------------------------------------------------------ loss / outputs
@pytest.mark.parametrize("name", golden_names())
def test_quad_loss_and_outputs_golden(hip, name):
    g = load_golden(name)
    W, H = dev(g["W_perm"]), dev(g["Xxt_damped"])
    K = int(g["K"])
    for k in range(K):
        d = float(hip.quad_loss(W, H, dev(g["T"][k + 1]), dev(g["Q"][k])).cpu())
        assert abs(d - g["dists"][k]) <= TOL_LOSS * abs(g["dists"][k])
    best_k = int(np.argmin(g["dists"]))
    Wq, Lo = hip.dequant_losses(W, dev(g["T"][best_k + 1]), dev(g["Q"][K - 1]), dev(g["Hinv_diag"]))
    assert np.array_equal(Wq.cpu().numpy(), g["Wq_loop"])
    assert rel_fro(Lo.cpu().numpy(), g["Losses"]) < 1e-6


# ------------------------------------------------------------------------------------------ whole loop
@pytest.mark.parametrize("name", golden_names())
def test_run_layer_golden(hip, name):
    g = load_golden(name)
    K = int(g["K"])
    T, Q, dists, best_k = hip.run_layer(dev(g["W_perm"]), dev(g["Xxt_damped"]), dev(g["L"]), dev(g["T"][0]), K,
                                        alias_q=True)
    torch.cuda.synchronize()
    assert int(best_k) == int(np.argmin(g["dists"]))
    assert np.allclose(dists.cpu().numpy(), g["dists"], rtol=1e-5)
    Qn = Q.cpu().numpy()
    mism = int((Qn != g["Q"][K - 1]).sum())
    # indices depend on the codebooks of earlier iterations, which agree to ~1e-6 only: report, and require
    # exactness on these small cases where no near-tie occurs
    assert mism == 0, f"{mism} of {Qn.size} indices differ from the reference after {K} iterations"
    Wq = np.take_along_axis(T.cpu().numpy(), Qn.astype(np.int64), axis=1)
    assert rel_fro(Wq, g["Wq_loop"]) < TOL_T


def test_run_layer_alias_vs_fixed(hip, oracle):
    g = load_golden("b32x64_b3")  # distances are not monotone here: best_k = 1 of 3
    K = int(g["K"])
    args = (dev(g["W_perm"]), dev(g["Xxt_damped"]), dev(g["L"]), dev(g["T"][0]), K)
    Ta, Qa, _, bka = hip.run_layer(*args, alias_q=True)
    Tf, Qf, _, bkf = hip.run_layer(*args, alias_q=False)
    assert int(bka) == int(bkf) == 1
    assert np.array_equal(Qa.cpu().numpy(), g["Q"][K - 1])
    assert np.array_equal(Qf.cpu().numpy(), g["Q"][1])
    assert torch.equal(Ta, Tf)


@pytest.mark.parametrize("m,n,V,K,seed", [(64, 512, 16, 3, 31), (128, 768, 8, 2, 32)])
def test_run_layer_vs_oracle(hip, oracle, m, n, V, K, seed):
    W, H, L, T0 = synth(m, n, V, seed, corr=0.2)
    To, Qo, do, bko = oracle.run_layer(W, H, L, T0, K, alias_q=True)
    T, Q, d, bk = hip.run_layer(dev(W), dev(H), dev(L), dev(T0), K, alias_q=True)
    assert int(bk) == bko
    assert np.allclose(d.cpu().numpy(), do, rtol=1e-5)
    frac = float((Q.cpu().numpy() != Qo).mean())
    assert frac < 1e-3, f"index mismatch fraction {frac}"
    assert rel_fro(T.cpu().numpy(), To) < 1e-3 if frac > 0 else rel_fro(T.cpu().numpy(), To) < TOL_T


@pytest.mark.parametrize("half_w", [True, False])
def test_run_layer_ten_iterations_vs_oracle(hip, oracle, half_w):
    # K = 10 as in the benchmark: rows converge and are skipped by the later S-solves, the codebooks come from the
    # Cholesky fast path, W @ H from the split-fp16 product (fp16-valued weights skip its third term) -- the indices of
    # the last iteration, the best codebook and every distance must still be the oracle's
    m, n, V, K = 80, 2048, 16, 10
    W, H, L, T0 = synth(m, n, V, 91, corr=0.15)
    if half_w:
        W = W.astype(np.float16).astype(np.float32)
    To, Qo, do, bko = oracle.run_layer(W, H, L, T0, K, alias_q=True)
    T, Q, d, bk = hip.run_layer(dev(W), dev(H), dev(L), dev(T0), K, alias_q=True)
    assert int(bk) == bko
    assert np.allclose(d.cpu().numpy(), do, rtol=1e-6)
    assert np.array_equal(Q.cpu().numpy(), Qo)
    assert rel_fro(T.cpu().numpy(), To) < TOL_T


@pytest.mark.parametrize("m,n,V,K,seed", [(96, 1024, 16, 6, 41), (40, 777, 8, 5, 42), (33, 250, 4, 4, 43), (64, 4112, 16, 3, 44)])
def test_run_layer_incremental_equals_full(hip, m, n, V, K, seed, lib_options):
    # the loop keeps the integer bucket sums between iterations and only moves the entries of changed indices;
    # that must be bit-identical to re-accumulating everything, also through the device-side fallback
    W, H, L, T0 = synth(m, n, V, seed, corr=0.2)
    args = (dev(W), dev(H), dev(L), dev(T0), K)
    ref = None
    for env in ({"GANQ_T_FULL": 1}, {}, {"GANQ_T_INCR_THR": 0}, {"GANQ_T_INCR_THR": m * n // 400}):
        lib_options(reset=("GANQ_T_FULL", "GANQ_T_INCR_THR"), **env)
        T, Q, d, bk = hip.run_layer(*args, alias_q=False)
        out = (T.clone(), Q.clone(), d.clone(), int(bk))
        if ref is None:
            ref = out
        else:
            assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1]) and torch.equal(out[2], ref[2]), env
            assert out[3] == ref[3]


def test_run_layer_incremental_many_changes(hip, lib_options):
    # a poor initial codebook makes a large share of the indices change in the first update: more than 32 per pass and
    # more than the 512 per row the matrix-core kernel caches in LDS; never falling back must equal always re-accumulating
    m, n, V, K = 24, 2048, 16, 3
    W, H, L, T0 = synth(m, n, V, 77, corr=0.1)
    rng = np.random.default_rng(5)
    T0 = np.sort(rng.uniform(-0.1, 0.1, size=T0.shape).astype(np.float32), axis=1)  # unrelated to the weights
    args = (dev(W), dev(H), dev(L), dev(T0), K)
    q_first = hip.run_layer(*args[:4], 1, alias_q=True)[1]   # with the aliasing: the indices of the last iteration
    q_second = hip.run_layer(*args[:4], 2, alias_q=True)[1]
    per_row = (q_first != q_second).sum(dim=1)
    assert int(per_row.max()) > 512 and int(per_row.min()) > 32, per_row
    outs = []
    for env in ({"GANQ_T_FULL": 1}, {"GANQ_T_INCR_THR": m * n}, {"GANQ_T_INCR_THR": m * n, "GANQ_MUPDATE_LDS": 1}):
        lib_options(reset=("GANQ_T_FULL", "GANQ_T_INCR_THR", "GANQ_MUPDATE_LDS"), **env)
        T, Q, d, bk = hip.run_layer(*args, alias_q=False)
        outs.append((T.clone(), Q.clone(), d.clone(), int(bk)))
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1]) and torch.equal(o[2], outs[0][2])


@pytest.mark.parametrize("m,n,V", [(256, 1024, 16), (64, 512, 8), (37, 300, 4)])
def test_update_t_cholesky_path_equals_jacobi_path(hip, oracle, m, n, V, lib_options):
    # rows whose A is provably above the gelsd cut-off are solved by Cholesky; forcing the eigen-solve for every row
    # must give the same codebook (both solve the same fp32-rounded system in fp64)
    W, H, L, T0 = synth(m, n, V, seed=m + V, corr=0.3)
    Q = oracle.solve_s(W, L, T0)
    Q[3, :] = Q[3, :] % (V - 1)  # one row with an unused code: singular A, takes the eigen-solve in both runs
    WH = oracle.matmul(W, H)
    outs = []
    for jac in (0, 1):
        lib_options(GANQ_T_JACOBI=jac)
        outs.append(hip.update_t(dev(WH), dev(H), dev(Q.astype(np.uint8)), V).cpu().numpy())
    lib_options(reset=("GANQ_T_JACOBI",))
    assert rel_fro(outs[0], outs[1]) < 1e-9
    assert (outs[0] == outs[1]).mean() > 0.98  # identical floats but for a rare last-bit rounding of the fp64 result
    To = oracle.update_t(WH, H, Q, V)
    assert rel_fro(outs[0], To) < TOL_T


def test_reciprocal_quotient_equals_ieee_division(hip):
    # the S-solve replaces r / L[j][j] by a reciprocal-based sequence that must round like the division
    bad, first = hip.debug_div_check(1 << 30, seed=7)
    assert bad == 0, f"{bad} of 2^30 quotients differ from IEEE division, e.g. a,b = {first}"


@pytest.mark.parametrize("m,n,half_w", [(128, 128, True), (96, 200, False), (300, 1000, True), (257, 2050, False),
                                        (64, 4096, True)])
def test_wh_product_split_fp16(hip, m, n, half_w):
    """W @ H_fixed of the fused driver (fp16 matrix cores, operands split into two fp16 pieces, wh_gemm.hip) against the
    same product in fp64: the error must stay in the class of the reference's fp32 `W @ H` (ganq.py:590)"""
    g = torch.Generator().manual_seed(m * 7 + n)
    W = 0.02 * torch.randn(m, n, generator=g)
    if half_w:
        W = W.half().float()  # fp16 module: the low pieces of W vanish and the third product is skipped
    W[m // 2] *= 1e-3  # rows of very different magnitude get their own power-of-two scale
    W[0, : n // 2] = 0.0
    X = torch.randn(4 * n, n, generator=g) * (0.05 + 3.0 * torch.rand(n, generator=g))
    H = (X.T @ X / X.shape[0]).float()
    WH, Hf = hip.debug_wh_product(W.cuda(), H.cuda())
    Hf, WH = Hf.cpu(), WH.cpu()
    assert (Hf - H.double()).abs().max() <= H.abs().max().double() * 2.0 ** -30  # 31-bit fixed point
    ref = W.double() @ Hf
    err = (WH - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-300)
    ref32 = (W @ Hf.float()).double()
    err32 = (ref32 - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-300)
    assert err.max() < 2e-6, (float(err.max()), float(err32.max()))
    assert err.median() < 1e-6
