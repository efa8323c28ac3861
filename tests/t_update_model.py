"""Host model of the T-update's integer arithmetic (ganq_amd/csrc/update_t.hip), numpy only.

The library converts H once to fixed point, H ~= scale * (I + J / 65536), and forms the bucket sums of I and J as exact int64
integers.  Integer sums have one right answer, so this model reproduces the conversion operation by operation in fp64 (the
library is built with -ffp-contract=off) and the sums exactly, and the tests compare with array_equal -- no tolerance.

  quantize(H, ext_mode)            absmax_kernel + prep_scale_kernel + hquant_kernel
  digits(x, count)                 the balanced base-256 digit planes of hquant_kernel
  bucket_sums(I, Q)                F[i][a][b] = sum_{u != v} [Q_iu = a][Q_iv = b] I[u][v] and D[i][a] = sum_{u in a} I[u][u], exact
  bucket_sums_int64(I, Q, rows)    the same by int64 arithmetic only (the cross-check)
  A_fp32(...)                      t_solve_kernel's A = float32(scale * (x + xl / 65536)), x = F + diag(D)
  stage_A(H, Q, V)                 all of the above: the A_out of ganq_update_t, bit for bit
  bucket_vector(X, Q)              b[i][a] = sum_{u in a} X[i][u] in fp64
  solve_fp64(A, b, V, rcond)       minimum-norm least squares per row, fp64

The case lists of tests/test_hip_t_update_exact.py live here as well (hessian(), pattern(), CONVERSION_CASES, FULL_CASES,
SEQUENCES, build_sequence()), so that tests/test_t_update_model.py can check without a GPU that they cover what they claim.
"""
import numpy as np

JMAX = 32639            # two balanced base-256 digits hold [-32896, 32639]
LIM = 1073741824.0      # 2^30
EXT_UNIT = 1.0 / 65536.0


# ------------------------------------------------------------------------------------------------ fixed-point conversion
def quantize(H, ext_mode=-1):
    """-> dict(scale, ext, I, J): I, J int64 [n,n].  ext_mode: -1 the device rule, 0 never, 1 always (GANQ_H_EXT)."""
    H = np.ascontiguousarray(H, dtype=np.float32)
    n = H.shape[0]
    mx = np.float32(np.abs(H).max())
    ok = bool(mx > 0) and bool(np.isfinite(mx))
    scale = float(mx) / LIM if ok else 0.0
    mean_diag = float(np.sum(np.diag(H).astype(np.float64))) / n  # the device sums in another order: see ext_margin()
    wide = ok and not (float(mx) <= 16.0 * mean_diag)
    ext = bool(wide) if ext_mode < 0 else bool(ext_mode)
    inv = 1.0 / scale if scale > 0.0 else 0.0
    x = np.minimum(np.maximum(H.astype(np.float64) * inv, -LIM), LIM)
    xi = np.rint(x)  # ties to even, like __builtin_rint
    xj = np.zeros_like(x)
    if ext:
        xj = np.rint((x - xi) * 65536.0)
        carry = xj > JMAX
        xi = xi + carry
        xj = xj - 65536.0 * carry
    return {"scale": scale, "ext": int(ext), "I": xi.astype(np.int64), "J": xj.astype(np.int64)}


def ext_margin(H):
    """max|H| / (16 mean(diag H)): the device switches the extension on above 1.  Far from 1 the summation order of the diagonal
    cannot matter and a test may assert the decision; near 1 it takes it from the device."""
    H = np.asarray(H, dtype=np.float32)
    mean_diag = float(np.sum(np.diag(H).astype(np.float64))) / H.shape[0]
    mx = float(np.abs(H).max())
    if mx == 0.0:
        return 0.0
    return np.inf if mean_diag <= 0 else mx / (16.0 * mean_diag)


def digits(x, count):
    """balanced base-256 digits of hquant_kernel: x = sum_p d_p 256^p + r 256^count, d_p in [-128, 127]; -> (list of d_p, r)"""
    r = np.asarray(x, dtype=np.int64).copy()
    out = []
    for _ in range(count):
        d = ((r + 128) & 255) - 128
        r = (r - d) >> 8
        out.append(d)
    return out, r


def recombine(ds):
    return sum(d.astype(np.int64) << (8 * p) for p, d in enumerate(ds))


# ------------------------------------------------------------------------------------------------ exact bucket sums
def _onehot(Q):
    m, n = Q.shape
    S = np.zeros((m, 16, n), dtype=np.float64)
    S[np.arange(m)[:, None], np.minimum(Q, 15), np.arange(n)[None, :]] = 1.0  # the kernels clamp codes to 15
    return S


def bucket_sums(I, Q):
    """-> (F [m,16,16] int64 without the diagonal terms, D [m,16] int64 diagonal buckets), exact.
    I is split into 16-bit halves, I = hi * 65536 + lo with lo in [0, 65535]: every partial sum of a half is an integer below
    n * n * 65535 < 2^53, so fp64 BLAS adds them without rounding, in any order."""
    I = np.asarray(I, dtype=np.int64)
    Q = np.asarray(Q)
    m, n = Q.shape
    assert I.shape == (n, n)
    assert n * n * 65535 < 2 ** 53
    assert np.abs(I).max(initial=0) <= 2 ** 31
    lo = I & 0xFFFF
    hi = I >> 16  # floor: hi * 65536 + lo == I, |hi| <= 2^15
    S = _onehot(Q)
    S2 = S.reshape(m * 16, n)
    full = np.zeros((m, 16, 16), dtype=np.int64)
    for part, shift in ((lo, 0), (hi, 16)):
        Y = (S2 @ part.astype(np.float64)).reshape(m, 16, n)   # Y[i][a][v] = sum_{u in a} part[u][v]
        P = np.matmul(Y, S.transpose(0, 2, 1))                 # P[i][a][b] = sum_{v in b} Y[i][a][v]
        assert np.array_equal(P, np.rint(P))
        full += P.astype(np.int64) << shift
    D = np.rint(S @ np.diag(I).astype(np.float64)).astype(np.int64)  # |I_uu| <= 2^31, n terms: exact
    F = full.copy()
    F[:, np.arange(16), np.arange(16)] -= D
    return F, D


def bucket_sums_int64(I, Q, rows):
    """the rows `rows` of bucket_sums by int64 arithmetic only -> (F [len(rows),16,16], D [len(rows),16])"""
    I = np.asarray(I, dtype=np.int64)
    n = I.shape[0]
    off = I.copy()
    off[np.arange(n), np.arange(n)] = 0
    dg = np.diag(I)
    F = np.zeros((len(rows), 16, 16), dtype=np.int64)
    D = np.zeros((len(rows), 16), dtype=np.int64)
    for k, i in enumerate(rows):
        q = np.minimum(np.asarray(Q[i], dtype=np.int64), 15)
        Y = np.zeros((16, n), dtype=np.int64)
        np.add.at(Y, q, off)            # Y[a][v] = sum_{u in a} off[u][v]
        np.add.at(F[k].T, q, Y.T)       # F[a][b] = sum_{v in b} Y[a][v]
        np.add.at(D[k], q, dg)
    return F, D


def A_fp32(scale, ext, F_hi, D_hi, F_lo=None, D_lo=None, V=16):
    """t_solve_kernel: x = F (+ D on the diagonal), xd = double(x) (+ double(xl) * 2^-16), A = float32(scale * xd) -> [m,V,V]"""
    idx = np.arange(16)
    x = np.array(F_hi, dtype=np.int64)
    x[:, idx, idx] += D_hi
    xd = x.astype(np.float64)
    if ext:
        xl = np.array(F_lo, dtype=np.int64)
        xl[:, idx, idx] += D_lo
        xd = xd + xl.astype(np.float64) * EXT_UNIT
    return (np.float64(scale) * xd).astype(np.float32)[:, :V, :V]


def A_fp64(scale, ext, F_hi, D_hi, F_lo=None, D_lo=None, V=16):
    """the same without the final rounding (what the loss is formed with)"""
    idx = np.arange(16)
    x = np.array(F_hi, dtype=np.int64)
    x[:, idx, idx] += D_hi
    xd = x.astype(np.float64)
    if ext:
        xl = np.array(F_lo, dtype=np.int64)
        xl[:, idx, idx] += D_lo
        xd = xd + xl.astype(np.float64) * EXT_UNIT
    return (np.float64(scale) * xd)[:, :V, :V]


def model_sums(q, Q):
    """bucket sums of both words of quantize()'s result for the indices Q -> dict(F_hi, D_hi, F_lo, D_lo)"""
    F_hi, D_hi = bucket_sums(q["I"], Q)
    if q["ext"]:
        F_lo, D_lo = bucket_sums(q["J"], Q)
    else:
        F_lo, D_lo = np.zeros_like(F_hi), np.zeros_like(D_hi)
    return {"F_hi": F_hi, "D_hi": D_hi, "F_lo": F_lo, "D_lo": D_lo}


def stage_A(H, Q, V, ext_mode=-1):
    """the fp32 A [m,V,V] that ganq_update_t hands out for (H, Q), bit for bit"""
    if ext_mode < 0:  # the device sums the diagonal in another order: its decision is only known off the boundary
        assert abs(ext_margin(H) - 1.0) > 1e-6
    q = quantize(H, ext_mode)
    s = model_sums(q, Q)
    return A_fp32(q["scale"], q["ext"], s["F_hi"], s["D_hi"], s["F_lo"], s["D_lo"], V)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def bucket_vector(X, Q, absolute=False):
    """b[i][a] = sum_{u in a} X[i][u] in fp64 (absolute: of |X|) -> [m,16]"""
    X = np.asarray(X, dtype=np.float64)
    if absolute:
        X = np.abs(X)
    return np.einsum("iau,iu->ia", _onehot(np.asarray(Q)), X)


def solve_fp64(A, b, V, rcond=None):
    """minimum-norm least squares per row in fp64 (the gelsd branch of the reference, cut-off rcond * sigma_max)"""
    rcond = 1.1920928955078125e-07 * V if rcond is None or rcond < 0 else rcond
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.stack([np.linalg.lstsq(A[i, :V, :V], b[i, :V], rcond=rcond)[0] for i in range(A.shape[0])])


# ------------------------------------------------------------------------------------------------ inputs of the GPU cases
HESSIANS = ("ordinary", "massive", "negative_offdiag", "clamp", "carry", "zero")


def hessian(kind, n, seed=0):
    """symmetric fp32 [n,n] (the kernels visit only u > v)"""
    rng = np.random.default_rng(1000 * seed + n)
    p = max(2 * n, 64) if n <= 1024 else n + 64
    scales = 0.1 + rng.random(n)
    if kind == "massive" and n >= 2:
        scales[rng.choice(n, size=2, replace=False)] *= 1000.0  # two massive features (H_ii 10^6 x)
    X = rng.standard_normal((p, n)) * scales
    H = (2.0 / p) * (X.T @ X)
    H += 0.01 * np.mean(np.diag(H)) * np.eye(n)
    H = H.astype(np.float32)
    if kind in ("ordinary", "massive"):
        pass
    elif kind == "negative_offdiag":
        s = np.where(rng.random(n) < 0.5, -1.0, 1.0).astype(np.float32)
        H = H * np.outer(s, s)
    elif kind == "clamp":  # entries equal to +max|H| and -max|H|: x = +-2^30 exactly, the ends of the clamp
        mx = np.float32(np.abs(H).max())
        H[0, 0] = mx
        if n >= 2:
            H[1, 1] = mx
            H[0, 1] = H[1, 0] = -mx
    elif kind == "carry":
        # max|H| = 1 makes scale 2^-30 and x = H * 2^30 exact: entries (k + f) 2^-30 with remainders f around the carry limit
        # 32640 / 65536 (the first that carries), 32639 / 65536 (the last that does not) and the ties k + 1/2 for even and odd k
        fr = np.array([32640, 32639, 32768, 32641, 32767, 0, 1, 65535 - 32896], dtype=np.float64) / 65536.0
        k = rng.integers(-100, 100, size=(n, n)).astype(np.float64)  # 7 + 16 bits: an fp32 value
        f = fr[rng.integers(0, len(fr), size=(n, n))]
        Hc = np.triu((k + f) * 2.0 ** -30)
        Hc = Hc + np.triu(Hc, 1).T
        Hc[0, 0] = 1.0
        H = Hc.astype(np.float32)
        assert np.array_equal(H.astype(np.float64), Hc)  # every entry is an fp32 value
    elif kind == "zero":
        H = np.zeros((n, n), dtype=np.float32)
    else:
        raise ValueError(kind)
    assert np.array_equal(H, H.T)
    return np.ascontiguousarray(H)


PATTERNS = ("uniform", "one_code_per_row", "one_code_per_group64", "unused_codes", "edge_columns")


def pattern(kind, m, n, V, seed=0):
    """index matrix uint8 [m,n] with codes < V"""
    rng = np.random.default_rng(7000 + 13 * seed + n + 131 * m)
    if kind == "uniform":
        Q = rng.integers(0, V, size=(m, n))
    elif kind == "one_code_per_row":
        Q = np.repeat((np.arange(m) % V)[:, None], n, axis=1)
    elif kind == "one_code_per_group64":
        Q = (np.arange(n)[None, :] // 64 + np.arange(m)[:, None]) % V
    elif kind == "unused_codes":  # odd codes never appear: zero rows and columns of A
        Q = 2 * rng.integers(0, V // 2, size=(m, n))
    elif kind == "edge_columns":  # code V-1 only in column 0, code V-2 only in column n-1
        Q = rng.integers(0, V - 2, size=(m, n))
        Q[:, n - 1] = V - 2
        Q[:, 0] = V - 1
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(Q.astype(np.uint8))


def weights(m, n, seed=0):
    rng = np.random.default_rng(500 + seed + 3 * n + m)
    return (0.02 * rng.standard_normal((m, n))).astype(np.float32)


# a. fixed-point conversion: every Hessian kind at every n, extension forced off and on, plus the device rule on the two kinds it is
# meant for
CONVERSION_N = (1, 3, 17, 255, 256, 257, 1000)
CONVERSION_CASES = [(kind, n, ext_mode) for n in CONVERSION_N for kind in HESSIANS for ext_mode in (0, 1)] + \
                   [(kind, n, -1) for n in CONVERSION_N for kind in ("ordinary", "massive")]

# b. full accumulation.  Every n twice, the partners dealt round-robin with strides that are coprime to the axis lengths, so
# that every value of every axis meets many of the others; then the nastier pairs by hand.
FULL_M = (1, 3, 31, 32, 33, 65)
FULL_N = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 513, 1000, 2080, 4100)
FULL_V = (4, 8, 16)


def _full_cases():
    cases = []
    for rnd in range(2):
        for i, n in enumerate(FULL_N):
            j = i + 26 * rnd
            m = FULL_M[j % 6]
            if n == 4100:
                m = (33, 3)[rnd]      # the big one: few rows (host model time)
            if n == 2080:
                m = (65, 31)[rnd]
            cases.append({"m": m, "n": n, "V": FULL_V[(j // 2) % 3], "ext_mode": (i // 3 + rnd) % 2,  # each n with the extension off and on
                          "hessian": ("ordinary", "massive", "negative_offdiag")[(j // 5) % 3] if n > 2 else "ordinary",
                          "pattern": PATTERNS[j % 5]})
    # by hand: padded row pairs at tile edges, the diagonal-crossing first tile with every pattern, more chunks than parts
    for m, n, V, ext_mode, hk, pk in [(33, 257, 16, 1, "massive", "edge_columns"), (65, 256, 16, 1, "massive", "one_code_per_group64"),
                                      (31, 255, 4, 0, "ordinary", "edge_columns"), (1, 513, 16, 1, "negative_offdiag", "uniform"),
                                      (3, 64, 8, 1, "carry", "one_code_per_row"), (32, 65, 16, 0, "clamp", "unused_codes"),
                                      (65, 1000, 8, 1, "carry", "unused_codes"), (33, 511, 4, 1, "clamp", "uniform"),
                                      (1, 1, 4, 1, "ordinary", "uniform"), (3, 2, 16, 1, "ordinary", "edge_columns"),
                                      (32, 17, 16, 0, "zero", "uniform")]:
        cases.append({"m": m, "n": n, "V": V, "ext_mode": ext_mode, "hessian": hk, "pattern": pk})
    return cases


FULL_CASES = _full_cases()

# c. incremental moves.  A step is ("counts", [c0, c1, ..]) -- row i changes counts[i % len] columns chosen at random ("n" = every
# column) --, ("columns", [u0, u1, ..]) -- every row changes exactly these columns (negative: from the end) --, ("rows_columns",
# rows, count) -- only the rows listed change `count` columns --, or ("back", k) -- return to the index matrix of iteration k.
# Every changed index gets a DIFFERENT code.  "expect" names the path of every iteration, read off the device: F full, I incremental.
CHANGE_COUNTS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 511, 512, 513, "n")
_MIXED_A = list(CHANGE_COUNTS)
_MIXED_B = list(CHANGE_COUNTS[7:] + CHANGE_COUNTS[:7])


def _kernel_sequences():
    seqs = []
    # the three kernel choices, each with the extension off and on; m = 35 is not a multiple of 16 (q_diff_kernel's padding waves)
    # and gives every count to at least two rows.  The forced threshold m * n keeps every step on the incremental path.
    for name, n, opts in (("mfma", 1024, {}), ("scalar_n%4=1", 1001, {}), ("scalar_vec_n%16=12", 1004, {}),
                          ("lds_switch", 1024, {"GANQ_MUPDATE_LDS": 1})):
        for ext_mode in (0, 1):
            seqs.append({"name": f"{name}_ext{ext_mode}", "m": 35, "n": n, "V": 16, "ext_mode": ext_mode,
                         "hessian": "massive" if ext_mode else "ordinary", "options": dict(opts, GANQ_T_INCR_THR=35 * n),
                         "steps": [("counts", _MIXED_A), ("counts", _MIXED_B), ("back", 0), ("columns", [0]), ("columns", [-1]),
                                   ("columns", list(range(-(n % 64 or 64), 0))), ("back", 2)],
                         "expect": "FIIIIIII"})
    # every column of a 4096-class row: cnt^2 pair corrections, a handful of rows
    seqs.append({"name": "all_columns_4096_mfma", "m": 3, "n": 4096, "V": 16, "ext_mode": 1, "hessian": "massive",
                 "options": {"GANQ_T_INCR_THR": 3 * 4096}, "steps": [("counts", ["n", 513, 0]), ("counts", [65, "n", 1])],
                 "expect": "FII"})
    seqs.append({"name": "all_columns_4100_scalar", "m": 2, "n": 4100, "V": 8, "ext_mode": 0, "hessian": "ordinary",
                 "options": {"GANQ_T_INCR_THR": 2 * 4100}, "steps": [("counts", ["n", 512])], "expect": "FI"})
    return seqs


def _gate_sequences():
    seqs = []
    m, n, t = 8, 256, 40
    for ext_mode in (0, 1):
        hk = "massive" if ext_mode else "ordinary"
        # forced threshold t: exactly t changed indices move incrementally, t + 1 re-accumulate -- at iteration 1 and, the forced
        # threshold keeping the gate, at iteration 2
        seqs.append({"name": f"thr_exact_ext{ext_mode}", "m": m, "n": n, "V": 16, "ext_mode": ext_mode, "hessian": hk,
                     "options": {"GANQ_T_INCR_THR": t}, "steps": [("counts", [5]), ("counts", [6, 5, 5, 5, 5, 5, 5, 5]), ("counts", [5]),
                                                                  ("counts", [5, 5, 5, 5, 5, 5, 5, 6])],
                     "expect": "FIFIF"})
        # the default gate m * n / 16 = 128 at iteration 1: 128 changes move, 129 re-accumulate
        seqs.append({"name": f"default_gate_at_ext{ext_mode}", "m": m, "n": n, "V": 16, "ext_mode": ext_mode, "hessian": hk,
                     "options": {}, "steps": [("counts", [16])], "expect": "FI"})
        # ... and from iteration 2 on the incremental path is taken however many indices change
        seqs.append({"name": f"default_gate_above_ext{ext_mode}", "m": m, "n": n, "V": 16, "ext_mode": ext_mode, "hessian": hk,
                     "options": {}, "steps": [("counts", [17, 16, 16, 16, 16, 16, 16, 16]), ("counts", ["n"]), ("counts", [0, "n", 64])],
                     "expect": "FFII"})
    # the scalar kernel behind the default gate, too
    seqs.append({"name": "default_gate_scalar", "m": 5, "n": 250, "V": 4, "ext_mode": 1, "hessian": "massive", "options": {},
                 "steps": [("counts", [15, 15, 15, 15, 18]), ("counts", ["n", 0, 1, 0, 250]), ("rows_columns", [3], 7)],
                 "expect": "FIII"})   # 78 = 5 * 250 >> 4 changes: at the threshold
    seqs.append({"name": "default_gate_scalar_above", "m": 5, "n": 250, "V": 4, "ext_mode": 0, "hessian": "ordinary", "options": {},
                 "steps": [("counts", [15, 15, 15, 15, 19])], "expect": "FF"})
    return seqs


SEQUENCES = _kernel_sequences() + _gate_sequences()


def build_sequence(seq):
    """-> (Qseq uint8 [K,m,n], counts int [K,m]): Q_0 uniform random, then the steps"""
    m, n, V = seq["m"], seq["n"], seq["V"]
    rng = np.random.default_rng(sum(map(ord, seq["name"])) + 31 * n + m)
    Qs = [rng.integers(0, V, size=(m, n)).astype(np.uint8)]
    counts = [np.zeros(m, dtype=np.int64)]
    for step in seq["steps"]:
        Q = Qs[-1].copy()
        if step[0] == "back":
            Q = Qs[step[1]].copy()
        else:
            for i in range(m):
                if step[0] == "counts":
                    c = step[1][i % len(step[1])]
                    cols = rng.choice(n, size=n if c == "n" else c, replace=False)
                elif step[0] == "columns":
                    cols = np.array(step[1]) % n
                elif step[0] == "rows_columns":
                    cols = rng.choice(n, size=step[2], replace=False) if i in step[1] else np.array([], dtype=np.int64)
                else:
                    raise ValueError(step[0])
                cols = np.asarray(cols, dtype=np.int64)
                Q[i, cols] = (Q[i, cols].astype(np.int64) + 1 + rng.integers(0, V - 1, size=len(cols))) % V  # never the old code
        counts.append((Q != Qs[-1]).sum(axis=1))
        Qs.append(Q)
    return np.ascontiguousarray(np.stack(Qs)), np.stack(counts)
