"""Cases of tests/test_hip_mupdate_top.py (the incremental bucket sums reading only the dense digit planes of H), numpy only, so that
tests/test_mupdate_top_model.py can check without a GPU that every case is what it claims: which D it means, which columns have
listed partners, which change counts it reaches.

A case: m, n, V, ext_mode, hessian kind, cap (GANQ_T_TOP_CAP; "c2", "c2-1", "c3-1" are resolved against the model's counts), the D it
means, extra options, and steps.  A step is ("counts", [c0, c1, ..]) -- row i changes counts[i % len] random columns ("n": all) --,
("columns", [names]) -- every row changes the named columns (column_sets) --, or ("back", k)."""
import numpy as np

import t_update_model as M

MU_N = (256, 512, 768)
MU_M = (3, 9, 33)
BORDER_COUNTS = (0, 1, 15, 16, 17, 31, 32, 33)  # tiles of 16 changes, passes of 32
PLANT_AT = lambda n: ((1, 0), (n - 1, 0), (n - 1, n - 2), (32, 31), (128, 127), (129, 127))  # noqa: E731


def planted_hessian(n):
    """an "ordinary" H with off-diagonals below digit 2 and six planted symmetric entries (tests/test_hip_accum_top.py): digit 3 = +64
    and -64, digit 2 = 127 / -128 with digit 3 zero, and two that stay below the thresholds: c3 = 2, c2 = 5"""
    H = M.hessian("ordinary", n).astype(np.float64)
    d = np.diag(H).copy()
    off = H - np.diag(d)
    mx = float(np.float32(d.max()))
    off *= (mx * 2.0 ** -16) / np.abs(off).max()
    H = off + np.diag(d)
    unit = mx / 2.0 ** 30
    words = (2 ** 30, -2 ** 30, 127 * 65536 + 5 * 256 + 7, -128 * 65536 + 5 * 256 + 7, 32500, 127 * 65536 + 32000)
    for (u, v), w in zip(PLANT_AT(n), words):
        H[u, v] = H[v, u] = w * unit
        H[u, u] = H[v, v] = mx
    H = np.ascontiguousarray(H.astype(np.float32))
    assert np.array_equal(H, H.T)
    return H


def hessian(kind, n):
    return planted_hessian(n) if kind == "planted" else M.hessian(kind, n)


def model_counts(q):
    """(c3, c2): the entries u > v of the 31-bit word with a non-zero digit 3 / digit 2 or 3"""
    ds, rest = M.digits(q["I"], 4)
    assert not rest.any()
    up = np.triu(np.ones(q["I"].shape, dtype=bool), 1)
    return int(((ds[3] != 0) & up).sum()), int((((ds[2] != 0) | (ds[3] != 0)) & up).sum())


def resolve_cap(cap, counts):
    c3, c2 = counts
    return {"c2": c2, "c2-1": c2 - 1, "c3-1": c3 - 1}.get(cap, cap)


def rule(c3, c2, cap):
    """top_dense_planes"""
    if cap < 0:
        return 4
    return 2 if c2 <= cap else (3 if c3 <= cap else 4)


def default_cap(n):
    return min(n * n // 1024, 131072)


def partner_counts(q, D):
    """per column: off-diagonal entries of its row whose digits above the D dense ones are not all zero (its listed partners)"""
    ds, _ = M.digits(q["I"], 4)
    top = np.zeros(q["I"].shape, dtype=bool)
    for p in range(D, 4):
        top |= ds[p] != 0
    np.fill_diagonal(top, False)
    return top.sum(axis=1), top


def column_sets(q, D):
    """named columns of a case: "massive" the column with the most listed partners, "partner" a partner of it with the fewest of its
    own, "pair" both of them, "lonely" a column without a listed partner (none: a column with the fewest), "edges" 0 and n - 1"""
    n = q["I"].shape[0]
    cnt, top = partner_counts(q, min(D, 3))  # (a D = 4 case: the columns the three-plane split would list)
    big = int(np.argmax(cnt))
    sets = {"edges": [0, n - 1]}
    if cnt[big] > 0:
        ps = np.flatnonzero(top[big])
        small = int(ps[np.argmin(cnt[ps])])
        sets.update(massive=[big], partner=[small], pair=[big, small])
    else:
        sets.update(massive=[n // 2], partner=[n // 2 + 1], pair=[n // 2, n // 2 + 1])
    lonely = np.flatnonzero(cnt == cnt.min())
    sets["lonely"] = [int(lonely[len(lonely) // 2])]
    return sets, cnt


KINDS = (("massive", "c2", 2), ("massive", "c2-1", 3), ("planted", 5, 2), ("planted", 4, 3), ("ordinary", -1, 4), ("zero", -1, 2))


def _cases():
    cases = []
    # a. change counts at the tile and pass borders, every kind at every n; m, V and the extension dealt
    for i, (kind, cap, D) in enumerate(KINDS):
        for j, n in enumerate(MU_N):
            m = MU_M[(i + j) % 3]
            steps = [("counts", list(BORDER_COUNTS[s:] + BORDER_COUNTS[:s])) for s in ((0, 3, 6) if m == 3 else (0, 5))]
            cases.append({"name": f"borders-{kind}-D{D}-n{n}", "m": m, "n": n, "V": M.FULL_V[(i + 2 * j) % 3], "ext_mode": (i + j) % 2,
                          "hessian": kind, "cap": cap, "D": D, "options": {}, "steps": steps})
    # b. the columns that matter
    for i, (kind, cap, D) in enumerate(KINDS[:4]):
        for j in range(2):
            n, m = MU_N[(i + 2 * j) % 3], MU_M[(i + j + 1) % 3]
            if (kind, D, n) == ("massive", 3, 256):  # (no entry of that matrix reaches digit 3: the list would be empty)
                n = 768
            cases.append({"name": f"columns-{kind}-D{D}-n{n}", "m": m, "n": n, "V": M.FULL_V[(i + j) % 3], "ext_mode": (i + j + 1) % 2,
                          "hessian": kind, "cap": cap, "D": D, "options": {},
                          "steps": [("columns", ["massive"]), ("columns", ["partner"]), ("columns", ["pair"]), ("columns", ["lonely"]),
                                    ("columns", ["edges"]), ("back", 0), ("columns", ["massive", "partner", "lonely", "edges"])]})
    # c. more changes in a row than the kernel's LDS copy of the list holds (512), every column among them; and a long list: the
    # "ordinary" H at n = 768 has 69753 entries with a digit 3, which a cap at the lists' capacity accepts
    for kind, cap, D, ext_mode, V in (("massive", "c2", 2, 1, 16), ("planted", 4, 3, 0, 8), ("ordinary", 10 ** 9, 3, 0, 4)):
        cases.append({"name": f"long-{kind}-D{D}", "m": 3, "n": 768, "V": V, "ext_mode": ext_mode, "hessian": kind, "cap": cap, "D": D,
                      "options": {}, "steps": [("counts", [513, "n", 0]), ("counts", [65, 511, "n"])]})
    # d. lists that overflow the cap: four planes
    cases.append({"name": "overflow-ordinary", "m": 9, "n": 512, "V": 16, "ext_mode": 0, "hessian": "ordinary", "cap": 1000, "D": 4,
                  "options": {}, "steps": [("counts", list(BORDER_COUNTS)), ("columns", ["massive", "edges"])]})
    cases.append({"name": "overflow-massive", "m": 33, "n": 768, "V": 8, "ext_mode": 1, "hessian": "massive", "cap": "c3-1", "D": 4,
                  "options": {}, "steps": [("counts", list(BORDER_COUNTS)), ("columns", ["pair"])]})
    for c in cases:
        c["options"] = dict(c["options"], GANQ_T_INCR_THR=c["m"] * c["n"])  # every step stays on the incremental path
        c["expect"] = "F" + "I" * len(c["steps"])
    # e. a forced threshold t = 40: 36 and exactly 40 changed indices move, 45 are summed again in full -- and the sums moved after
    # that start from the restored state
    for kind, cap, D, ext_mode in (("massive", "c2", 2, 1), ("planted", 4, 3, 0)):
        cases.append({"name": f"gate-{kind}-D{D}", "m": 9, "n": 256, "V": 16, "ext_mode": ext_mode, "hessian": kind, "cap": cap, "D": D,
                      "options": {"GANQ_T_INCR_THR": 40},
                      "steps": [("counts", [4]), ("counts", [5]), ("counts", [4]), ("counts", [5, 4, 4, 4, 4, 4, 4, 4, 7]), ("columns", ["pair"])],
                      "expect": "FIFIII"})
    return cases


CASES = _cases()


def build(case):
    """-> (H, q, counts (c3, c2), cap, Qseq uint8 [K,m,n], changes int [K,m], column sets, partner counts)"""
    m, n, V = case["m"], case["n"], case["V"]
    H = hessian(case["hessian"], n)
    q = M.quantize(H, case["ext_mode"])
    counts = model_counts(q)
    cap = resolve_cap(case["cap"], counts)
    sets, pc = column_sets(q, case["D"])
    rng = np.random.default_rng(sum(map(ord, case["name"])) + 31 * n + m)
    Qs = [rng.integers(0, V, size=(m, n)).astype(np.uint8)]
    for step in case["steps"]:
        Q = Qs[-1].copy()
        if step[0] == "back":
            Q = Qs[step[1]].copy()
        else:
            for i in range(m):
                if step[0] == "counts":
                    c = step[1][i % len(step[1])]
                    cols = rng.choice(n, size=n if c == "n" else c, replace=False)
                else:
                    cols = np.unique(np.concatenate([sets[name] for name in step[1]]))
                cols = np.asarray(cols, dtype=np.int64)
                Q[i, cols] = (Q[i, cols].astype(np.int64) + 1 + rng.integers(0, V - 1, size=len(cols))) % V  # never the old code
        Qs.append(Q)
    Qseq = np.ascontiguousarray(np.stack(Qs))
    changes = np.stack([np.zeros(m, dtype=np.int64)] + [(Qseq[k] != Qseq[k - 1]).sum(axis=1) for k in range(1, len(Qseq))])
    return H, q, counts, cap, Qseq, changes, sets, pc


def massive_layer(m, n, V, seed):
    """(W, H, L, T0) of a run_layer case with two massive features (tests/test_hip_stages.py:synth with M.hessian("massive"))"""
    rng = np.random.default_rng(seed)
    W = (0.02 * rng.standard_normal((m, n))).astype(np.float32)
    H = M.hessian("massive", n, seed=seed)
    Hd = H.astype(np.float64)
    off = np.clip(np.abs(Hd).sum(1) - 2 * np.diag(Hd), 1e-8, None)
    L = np.linalg.cholesky(Hd + np.diag(off)).astype(np.float32)
    T0 = np.quantile(W, (np.arange(V) + 0.5) / V, axis=1).T.astype(np.float32).copy()
    return W, H, L, T0
