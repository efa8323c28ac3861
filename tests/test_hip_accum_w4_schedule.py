"""The schedule of the four-wave full bucket sum (onehot_accum_w4_kernel): accumulator tiles born in a chunk's first slice, the
bucketing pass on the transposed tile (lane = (row, code), registers = columns), a bucket nobody reads for codes outside 0 .. 15, and
digit sums recombined in 32-bit halves.  The sums are integers, so every case compares the A of the four-wave kernel bit for bit with the A of the first kernel
(GANQ_ACCUM_W4=0) on the same inputs, and the fixed-point sums of ganq_debug_t_sums with the host model of tests/t_update_model.py.
The plan and the number of dense planes D (ganq_debug_top_planes) are asserted before every run.

Shapes: n = 256 two slices and one chunk per part, the chunk of parts 4-7 has a single slice (prologue, diagonal slice and bucketing
meet); n = 512 / 768 two and three chunks per part, the last chunk of parts 4-7 single-slice behind a multi-slice one; n = 1280 a slice
count that is no power of two.  m = 1 a row group with one live row, 9 a wave with one row, 33 one row beyond a full group, 64 two
full groups."""
import numpy as np
import pytest
import torch

import t_update_model as M
from test_hip_accum_top import OPTIONS, dev, entry, model_counts, use_top

pytestmark = pytest.mark.gpu

SCHED_N = (256, 512, 768, 1280)
SCHED_M = (1, 9, 33, 64)
LIST_MAX = 131072  # entries of an exception list (asserted against the library in every case)


@pytest.fixture(scope="module")
def hip():
    from ganq_amd import _lib

    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.lib()
    _lib.selftest()
    return _lib


def words_hessian(n, words):
    """H = I 2^-30 with a unit diagonal (I = 2^30) and I[u][v] = words[u][v] (|word| < 2^24: an fp32 value) off it, made symmetric
    from the entries u > v"""
    I = np.tril(np.asarray(words, dtype=np.int64), -1)
    assert np.abs(I).max() < 2 ** 24
    I = I + I.T
    H = I.astype(np.float64) * 2.0 ** -30
    np.fill_diagonal(H, 1.0)
    H32 = np.ascontiguousarray(H.astype(np.float32))
    assert np.array_equal(H32.astype(np.float64), H)
    return H32


def dense2_hessian(n, seed=0):
    """digits 0 .. 2 dense (|I| <= 8 000 000 off the diagonal: below the carry into digit 3), digit 3 only in two planted entries of
    +-(2^30 - 2^22)"""
    rng = np.random.default_rng(900 + 7 * seed + n)
    H = words_hessian(n, rng.integers(-8000000, 8000001, size=(n, n)))
    for (u, v), s in (((n - 1, 0), 1.0), ((n // 2 + 1, n // 2), -1.0)):
        H[u, v] = H[v, u] = np.float32(s * (1.0 - 2.0 ** -8))
    return H


def hessian_of(kind, n):
    return dense2_hessian(n) if kind == "dense2" else M.hessian(kind, n)


def first_kernel_A(hip, lib_options, m, n, V, ext_mode, WH, H, Q):
    lib_options(reset=OPTIONS, GANQ_ACCUM_W4=0, GANQ_H_EXT=ext_mode)
    assert hip.accum_plan(m, n)["kernel"] == "onehot_accum", (m, n)
    _, A, _ = hip.update_t(dev(WH), dev(H), dev(Q), V, want_ab=True)
    return A.cpu().numpy()


def plane_settings(hip, lib_options, m, n, H, ext_mode):
    """-> (counts, [(GANQ_T_TOP, GANQ_T_TOP_CAP, D)]): four planes always, three and two where the lists can hold the exceptions"""
    c3, c2 = counts = model_counts(M.quantize(H, ext_mode))
    lib_options(reset=OPTIONS, GANQ_ACCUM_W4=1)
    assert hip.debug_top_rule(m, n, 0, 0)["list_max"] == LIST_MAX
    settings = [(0, -1, 4)]
    if c3 < c2 and c3 <= LIST_MAX:
        settings.append((-1, min(c2 - 1, LIST_MAX), 3))
    if c2 <= LIST_MAX:
        settings.append((-1, c2, 2))
    return counts, settings


def check_schedule(hip, lib_options, m, n, V, ext_mode, H, Q, want_D, model=True):
    """every D of want_D: the four-wave kernel's A equals the first kernel's byte for byte; with `model`, the fixed-point sums and A
    equal the host model as well"""
    W = M.weights(m, n)
    WH = (W.astype(np.float64) @ H.astype(np.float64)).astype(np.float32)
    counts, settings = plane_settings(hip, lib_options, m, n, H, ext_mode)
    assert sorted(D for _, _, D in settings) == sorted(want_D), (counts, settings, want_D)
    A_first = first_kernel_A(hip, lib_options, m, n, V, ext_mode, WH, H, Q)
    if model:
        q = M.quantize(H, ext_mode)
        sums = M.model_sums(q, Q)
        A_ref = M.A_fp32(q["scale"], q["ext"], sums["F_hi"], sums["D_hi"], sums["F_lo"], sums["D_lo"], V)
        assert M.bits_equal(A_first, A_ref)
    for top, cap, D in settings:
        use_top(hip, lib_options, m, n, H, ext_mode, top, cap, D, counts)
        _, A, _ = hip.update_t(dev(WH), dev(H), dev(Q), V, want_ab=True)
        A = A.cpu().numpy()
        bad = np.argwhere(A.view(np.int32) != A_first.view(np.int32))
        assert np.array_equal(A.view(np.int32), A_first.view(np.int32)), (D, len(bad), bad[:4].tolist())
        if model:
            res = entry(hip, W, H, Q[None], V)
            assert int(res["ext"]) == ext_mode and int(res["full_ran"][0]) == 1, D
            assert np.array_equal(res["F_hi"][0], sums["F_hi"]), D
            assert np.array_equal(res["F_lo"][0], sums["F_lo"]), D


def _grid():
    """every (n, m): V, the extension, the Hessian kind and the index pattern dealt so that each n sees both extension settings, both
    kinds and all three V"""
    cases = []
    for i, n in enumerate(SCHED_N):
        for j, m in enumerate(SCHED_M):
            kind = ("dense2", "massive")[(i + j) % 2]
            cases.append({"n": n, "m": m, "V": M.FULL_V[(i + 2 * j) % 3], "ext_mode": (i + j // 2) % 2, "kind": kind,
                          "pattern": M.PATTERNS[(3 * i + j) % 5],
                          "D": (2, 3, 4) if kind == "massive" or n <= 512 else (3, 4)})
    return cases


GRID = _grid()


def grid_id(c):
    return f"n{c['n']}-m{c['m']}-V{c['V']}-ext{c['ext_mode']}-{c['kind']}-{c['pattern']}"


@pytest.mark.parametrize("case", GRID, ids=[grid_id(c) for c in GRID])
def test_schedule_against_first_kernel_and_model(hip, lib_options, case):
    m, n, V = case["m"], case["n"], case["V"]
    H = hessian_of(case["kind"], n)
    check_schedule(hip, lib_options, m, n, V, case["ext_mode"], H, M.pattern(case["pattern"], m, n, V), case["D"])


def test_grid_covers_every_instantiation_at_256_and_768():
    for n in (256, 768):
        mine = [c for c in GRID if c["n"] == n]
        assert {D for c in mine for D in c["D"]} == {2, 3, 4} and {c["ext_mode"] for c in mine} == {0, 1}
        assert {c["V"] for c in mine} == {4, 8, 16} and {c["m"] for c in mine} == set(SCHED_M)


@pytest.mark.parametrize("n,m,kind,want_D", [(512, 33, "massive", (2, 3, 4)), (256, 9, "dense2", (2, 3, 4)), (768, 64, "dense2", (3, 4))])
def test_codes_outside_the_buckets_add_nothing(hip, lib_options, n, m, kind, want_D):
    """a few columns hold a code >= 16: the first kernel adds zero for such a column, the four-wave kernel sends it to the bucket nobody
    reads.  (The host model clamps codes, so only the two kernels are compared.)"""
    V = 16
    Q = M.pattern("uniform", m, n, V)
    Q[:, [0, 31, 32, 129, n - 1]] = 16
    Q[m // 2, 200] = 255
    Q[0, 5:9] = (17, 31, 128, 240)
    check_schedule(hip, lib_options, m, n, V, 0, hessian_of(kind, n), Q, want_D, model=False)


@pytest.mark.parametrize("digits,want_D", [(2, (2, 4)), (3, (3, 4))])
def test_extreme_digit_sums(hip, lib_options, digits, want_D):
    """every digit of a column at -128 (even columns) or +127 (odd columns), every index the same code: each accumulator element of a
    chunk's column v is (n - 1 - v) times the digit, the largest magnitude a plane's sum can have at this n, in all planes at once"""
    m, n, V = 9, 1280, 16
    unit = sum(256 ** d for d in range(digits))
    col = np.where(np.arange(n) % 2 == 0, -128, 127).astype(np.int64) * unit
    H = words_hessian(n, np.broadcast_to(col[None, :], (n, n)))
    ds, rest = M.digits(M.quantize(H, 0)["I"][1:, 0], 4)
    assert all((ds[d] == -128).all() for d in range(digits)) and not any(ds[d].any() for d in range(digits, 4)) and not rest.any()
    Q = np.full((m, n), 3, dtype=np.uint8)
    Q[1] = (np.arange(n) % 2) * 15  # (one row with two codes: each bucket pair holds one sign)
    check_schedule(hip, lib_options, m, n, V, 0, H, Q, want_D)


@pytest.mark.parametrize("m,n,V,ext_mode,kind", [(64, 768, 16, 1, "massive"), (9, 256, 8, 0, "dense2")])
def test_reaccumulation_keeps_no_state(hip, lib_options, m, n, V, ext_mode, kind):
    """GANQ_T_FULL=1: two iterations with different indices are summed in full on the same workspace"""
    H = hessian_of(kind, n)
    W = M.weights(m, n)
    q = M.quantize(H, ext_mode)
    Qs = np.stack([M.pattern("uniform", m, n, V), M.pattern("unused_codes", m, n, V, seed=1)])
    want = [M.model_sums(q, Qs[k]) for k in range(2)]
    counts, settings = plane_settings(hip, lib_options, m, n, H, ext_mode)
    assert sorted(D for _, _, D in settings) == [2, 3, 4]
    for top, cap, D in settings:
        use_top(hip, lib_options, m, n, H, ext_mode, top, cap, D, counts, GANQ_T_FULL=1)
        res = entry(hip, W, H, Qs, V)
        assert (res["full_ran"] == 1).all() and res["Qprev"] is None
        for k in range(2):
            assert np.array_equal(res["F_hi"][k], want[k]["F_hi"]), (D, k)
            assert np.array_equal(res["F_lo"][k], want[k]["F_lo"]), (D, k)


@pytest.mark.parametrize("m,n,V,seed", [(64, 512, 16, 41), (33, 768, 8, 42)])
def test_run_layer_same_bytes_as_first_kernel(hip, lib_options, m, n, V, seed):
    from test_hip_stages import synth

    W, H, L, T0 = synth(m, n, V, seed, corr=0.2)
    args = (dev(W), dev(H), dev(L), dev(T0), 3)
    outs = []
    for w4 in (0, 1):
        lib_options(reset=OPTIONS, GANQ_ACCUM_W4=w4)
        assert hip.accum_plan(m, n)["kernel"] == ("onehot_accum_w4" if w4 else "onehot_accum")
        T, Q, d, bk = hip.run_layer(*args, alias_q=False)
        outs.append((T.cpu().numpy(), Q.cpu().numpy(), d.cpu().numpy(), int(bk)))
    for a, b in zip(outs[0][:3], outs[1][:3]):
        assert a.tobytes() == b.tobytes()
    assert outs[0][3] == outs[1][3]
