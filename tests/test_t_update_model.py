"""The host model behind tests/test_hip_t_update_exact.py, checked on its own (no GPU), and the case lists of that file checked
for what they claim to cover.  The whole file takes about 5 s.

It also documents WHY the GPU file compares exactly: two plausible defects of the integer path -- the lowest digit plane of I
dropped, the extension word ignored -- move the fp32 A in most of its entries and still stay under the 1e-6 relative Frobenius
every other A assertion of the suite uses.
"""
import numpy as np

import t_update_model as M
from conftest import rel_fro


def fp64_bucket_A(H, Q, V):
    """A = S H S^T by fp64 sums of the fp32 entries (what the reference's fp32 einsum approximates)"""
    S = M._onehot(Q)
    return np.matmul(np.matmul(S, H.astype(np.float64)), S.transpose(0, 2, 1))[:, :V, :V]


def model_A(H, Q, V, ext_mode=-1):
    q = M.quantize(H, ext_mode)
    s = M.model_sums(q, Q)
    return q, s, M.A_fp32(q["scale"], q["ext"], s["F_hi"], s["D_hi"], s["F_lo"], s["D_lo"], V)


CASES = [("ordinary", 48, 1024, 16), ("ordinary", 33, 300, 16), ("massive", 24, 768, 8), ("negative_offdiag", 5, 130, 4)]


def test_blas_halves_equal_int64_sums():
    for kind, m, n, V in CASES:
        H, Q = M.hessian(kind, n), M.pattern("uniform", m, n, V)
        q = M.quantize(H, 1)
        rows = [0, m // 2, m - 1]
        for word in ("I", "J"):
            F, D = M.bucket_sums(q[word], Q)
            F2, D2 = M.bucket_sums_int64(q[word], Q, rows)
            assert np.array_equal(F[rows], F2) and np.array_equal(D[rows], D2), (kind, word)
            assert np.array_equal(F, F.transpose(0, 2, 1))  # H symmetric
            # all of the word is in the buckets
            assert np.array_equal(F.sum(axis=(1, 2)) + D.sum(axis=1), np.full(m, q[word].sum()))


def test_model_A_agrees_with_fp64_bucket_sums():
    for kind, m, n, V in CASES:
        H, Q = M.hessian(kind, n), M.pattern("uniform", m, n, V)
        q, s, A = model_A(H, Q, V)
        assert q["ext"] == (kind == "massive")
        ref = fp64_bucket_A(H, Q, V)
        # the fixed point itself: the model's A before its rounding to fp32 (that rounding alone is ~2.5e-8)
        e = rel_fro(M.A_fp64(q["scale"], q["ext"], s["F_hi"], s["D_hi"], s["F_lo"], s["D_lo"], V), ref)
        e32 = rel_fro(A, ref.astype(np.float32))
        print(f"{kind} {m}x{n}: ext {q['ext']}, model A vs fp64 bucket sums {e:.2e}; both rounded to fp32 {e32:.2e}")
        assert e < 5e-8 and e32 < 5e-8, (kind, e, e32)


def test_tolerance_cannot_replace_the_exact_test():
    # the lowest digit plane of I dropped entirely
    for kind, m, n, V in CASES[:2]:
        H, Q = M.hessian(kind, n), M.pattern("uniform", m, n, V)
        q, s, A = model_A(H, Q, V)
        d0 = M.digits(q["I"], 1)[0][0]
        F, D = M.bucket_sums(q["I"] - d0, Q)
        A_mut = M.A_fp32(q["scale"], 0, F, D, V=V)
        changed, e = float((A_mut != A).mean()), rel_fro(A_mut, A)
        print(f"plane 0 dropped, {m}x{n}: {100 * changed:.0f} % of the entries of A change, rel. Frobenius {e:.2e}")
        assert changed > 0.9 and e < 1e-6
    # the extension word ignored on a Hessian with two 1000x massive features (the device rule switches it on there)
    kind, m, n, V = CASES[2]
    H, Q = M.hessian(kind, n), M.pattern("uniform", m, n, V)
    q, s, A = model_A(H, Q, V)
    assert q["ext"] == 1
    A_mut = M.A_fp32(q["scale"], 0, s["F_hi"], s["D_hi"], V=V)
    changed, e = float((A_mut != A).mean()), rel_fro(A_mut, A)
    print(f"extension ignored, {m}x{n}: {100 * changed:.0f} % of the entries of A change, rel. Frobenius {e:.2e}")
    assert changed > 0.5 and e < 1e-6


def test_quantize_edge_cases():
    # max|H| = 1: scale = 2^-30 and x = H * 2^30 exactly
    def h(x00, x01, x11):
        return (np.array([[1.0, 0.0, 0.0], [0.0, x00, x01], [0.0, x01, x11]]) * 2.0 ** -30 + np.diag([1.0 - 2.0 ** -30, 0, 0])).astype(np.float32)

    f = lambda j: j / 65536.0  # noqa: E731
    q = M.quantize(h(5 + f(32639), 5 + f(32640), -5 + f(32640)), 1)
    assert q["scale"] == 2.0 ** -30 and q["I"][0, 0] == 2 ** 30 and q["J"][0, 0] == 0
    assert (q["I"][1, 1], q["J"][1, 1]) == (5, 32639)           # the last remainder without a carry
    assert (q["I"][1, 2], q["J"][1, 2]) == (6, 32640 - 65536)    # the first with one
    assert (q["I"][2, 2], q["J"][2, 2]) == (-4, 32640 - 65536)   # negative entry: rint(-4.502) = -5, remainder +0.498 carries
    q = M.quantize(h(4.5, 5.5, -4.5), 1)                         # ties go to the even integer, the half carries or is negative
    assert (q["I"][1, 1], q["J"][1, 1]) == (5, -32768) and (q["I"][1, 2], q["J"][1, 2]) == (6, -32768)
    assert (q["I"][2, 2], q["J"][2, 2]) == (-4, -32768)
    q0 = M.quantize(h(4.5, 5.5, -4.5), 0)                        # without the extension: plain rint
    assert (q0["I"][1, 1], q0["I"][1, 2], q0["I"][2, 2]) == (4, 6, -4) and not q0["J"].any()
    # entries equal to +-max|H| sit on the ends of the clamp
    H = M.hessian("clamp", 17)
    q = M.quantize(H, 1)
    assert q["I"][0, 0] == 2 ** 30 and q["I"][0, 1] == -2 ** 30 and q["J"][0, 0] == 0 and q["J"][0, 1] == 0
    # all-zero H
    q = M.quantize(np.zeros((5, 5), dtype=np.float32), -1)
    assert q["scale"] == 0.0 and q["ext"] == 0 and not q["I"].any() and not q["J"].any()
    assert M.quantize(np.zeros((5, 5), dtype=np.float32), 1)["ext"] == 1
    # every kind: the words reproduce H to half a unit of the last word, the balanced digits recombine to the words, J fits two digits
    for kind in M.HESSIANS:
        for n in (1, 3, 17, 257):
            H = M.hessian(kind, n)
            for ext_mode in (0, 1):
                q = M.quantize(H, ext_mode)
                d_i, r_i = M.digits(q["I"], 4)
                d_j, r_j = M.digits(q["J"], 2)
                assert not r_i.any() and not r_j.any(), (kind, n)
                assert all(d.min() >= -128 and d.max() <= 127 for d in d_i + d_j)
                assert np.array_equal(M.recombine(d_i), q["I"]) and np.array_equal(M.recombine(d_j), q["J"])
                assert q["J"].min() >= -32896 and q["J"].max() <= 32639 and np.abs(q["I"]).max() <= 2 ** 30
                back = q["scale"] * (q["I"] + q["J"] / 65536.0)
                unit = q["scale"] * (2.0 ** -16 if ext_mode else 1.0)
                # (half a unit, plus the fp64 rounding of H / scale: 2^-53 * 2^30 units of I)
                assert np.abs(back - H.astype(np.float64)).max() <= 0.51 * unit + 1e-15 * np.abs(H).max(), (kind, n, ext_mode)
    # the crafted carry Hessian really holds the remainders around the limit, on and off the diagonal
    q = M.quantize(M.hessian("carry", 64), 1)
    assert {-32896, -32768, 32639}.issubset(set(np.unique(q["J"]).tolist()))


def test_gpu_case_lists_cover_what_they_claim():
    # a. conversion
    assert {n for _, n, _ in M.CONVERSION_CASES} == {1, 3, 17, 255, 256, 257, 1000}
    for n in M.CONVERSION_N:
        for kind in M.HESSIANS:
            assert (kind, n, 0) in M.CONVERSION_CASES and (kind, n, 1) in M.CONVERSION_CASES
        assert ("massive", n, -1) in M.CONVERSION_CASES and ("ordinary", n, -1) in M.CONVERSION_CASES
    assert M.quantize(M.hessian("massive", 1000), -1)["ext"] == 1 and M.ext_margin(M.hessian("massive", 1000)) > 4
    assert M.quantize(M.hessian("ordinary", 1000), -1)["ext"] == 0 and M.ext_margin(M.hessian("ordinary", 1000)) < 0.25
    # b. full accumulation: every value of every axis, each with several partners
    C = M.FULL_CASES
    assert {c["m"] for c in C} == {1, 3, 31, 32, 33, 65}
    assert {c["n"] for c in C} == {1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 513, 1000, 2080, 4100}
    assert {c["V"] for c in C} == {4, 8, 16} and {c["ext_mode"] for c in C} == {0, 1}
    assert {c["pattern"] for c in C} == set(M.PATTERNS) and {c["hessian"] for c in C} == set(M.HESSIANS)
    for n in M.FULL_N:
        mine = [c for c in C if c["n"] == n]
        assert len({c["m"] for c in mine}) >= 2 and len({c["pattern"] for c in mine}) >= 2, n
        if n > 2:
            assert {c["ext_mode"] for c in mine} == {0, 1}, n
    for key, values in (("m", M.FULL_M), ("V", M.FULL_V), ("pattern", M.PATTERNS)):
        for v in values:
            mine = [c for c in C if c[key] == v]
            assert {c["ext_mode"] for c in mine} == {0, 1} and len({c["n"] for c in mine}) >= 4, (key, v)
    for c in C:
        assert c["n"] <= 4100 and c["m"] <= 65
        Q = M.pattern(c["pattern"], c["m"], c["n"], c["V"])
        assert Q.shape == (c["m"], c["n"]) and Q.max() < c["V"]
        if c["pattern"] == "edge_columns" and c["n"] >= 2:
            assert ((Q == c["V"] - 1).sum(axis=1) == 1).all() and (Q[:, 0] == c["V"] - 1).all()
            assert ((Q == c["V"] - 2).sum(axis=1) == 1).all() and (Q[:, -1] == c["V"] - 2).all()
        if c["pattern"] == "unused_codes":
            assert not (Q & 1).any()
    # nastier partners: a row count off the 32-row workgroup with a width off the 256-column tile, with the extension
    assert any(c["m"] % 32 and c["n"] % 256 and c["n"] > 256 and c["ext_mode"] for c in C)
    assert any(c["n"] > 32 * 8 * 2 and c["m"] > 32 for c in C)  # more chunks than parts, more than one row group
    # c. incremental sequences
    S = M.SEQUENCES
    assert len({s["name"] for s in S}) == len(S)
    built = {s["name"]: M.build_sequence(s) for s in S}
    for s in S:
        Qseq, counts = built[s["name"]]
        assert len(s["expect"]) == len(Qseq) == len(counts) and s["expect"][0] == "F" and Qseq.max() < s["V"]
        # the device rule decides the extension: the case must be far from its boundary
        margin = M.ext_margin(M.hessian(s["hessian"], s["n"]))
        assert (margin > 4) if s["ext_mode"] else (margin < 0.25), (s["name"], margin)
        # the expected path follows from the gate as update_t.hip states it
        thr = s["options"].get("GANQ_T_INCR_THR", (s["m"] * s["n"]) >> 4)
        for k in range(1, len(Qseq)):
            gated = "GANQ_T_INCR_THR" in s["options"] or k < 2
            assert s["expect"][k] == ("F" if gated and counts[k].sum() > thr else "I"), (s["name"], k)

    def kernel_of(s):
        if s["n"] % 16 == 0 and not s["options"].get("GANQ_MUPDATE_LDS"):
            return "mfma"
        return "lds_switch" if s["n"] % 16 == 0 else ("scalar_vec" if s["n"] % 4 == 0 else "scalar")

    want = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 511, 512, 513]
    for kern in ("mfma", "lds_switch", "scalar_vec", "scalar"):
        for ext in (0, 1):
            mine = [s for s in S if kernel_of(s) == kern and s["ext_mode"] == ext and s["m"] % 16]
            for it, label in ((1, "iteration 1"), (2, "iteration >= 2")):
                seen = set()
                for s in mine:
                    _, counts = built[s["name"]]
                    if s["expect"][it:it + 1] == "I" and len(counts) > it:
                        seen |= set(counts[it].tolist()) | ({"n"} if (counts[it] == s["n"]).any() else set())
                        assert len(set(counts[it].tolist())) > 4 or s["m"] < 10  # mixed over the rows of one matrix
                assert set(want) | {"n"} <= seen, (kern, ext, label, sorted(map(str, seen)))
            # a step that returns to an earlier index matrix, and the confined changes
            for s in mine:
                if len(s["steps"]) < 7:
                    continue
                Qseq, counts = built[s["name"]]
                assert np.array_equal(Qseq[3], Qseq[0]) and np.array_equal(Qseq[7], Qseq[2]) and counts[3].sum() > 0
                assert ((Qseq[4] != Qseq[3]).nonzero()[1] == 0).all() and ((Qseq[5] != Qseq[4]).nonzero()[1] == s["n"] - 1).all()
                last = (Qseq[6] != Qseq[5]).nonzero()[1]
                assert last.min() == (s["n"] - 1) // 64 * 64 and len(last) == s["m"] * (s["n"] - (s["n"] - 1) // 64 * 64)
    # all columns of a 4096-class row: a handful of rows
    big = [s for s in S if s["n"] >= 4096]
    assert {kernel_of(s) for s in big} == {"mfma", "scalar_vec"} and all(s["m"] <= 4 for s in big)
    assert all((built[s["name"]][1] == s["n"]).any() for s in big)
    # the gate: exactly t moves, t + 1 re-accumulates (forced threshold and default), iteration >= 2 stays incremental
    for ext in (0, 1):
        forced = [s for s in S if s["options"].get("GANQ_T_INCR_THR") == 40 and s["ext_mode"] == ext]
        assert forced and all(built[s["name"]][1].sum(axis=1).tolist() == [0, 40, 41, 40, 41] and s["expect"] == "FIFIF" for s in forced)
        default = [s for s in S if "GANQ_T_INCR_THR" not in s["options"] and s["ext_mode"] == ext]
        at = [(s["m"] * s["n"]) >> 4 for s in default if built[s["name"]][1][1].sum() == (s["m"] * s["n"]) >> 4 and s["expect"][1] == "I"]
        above = [s for s in default if built[s["name"]][1][1].sum() == ((s["m"] * s["n"]) >> 4) + 1 and s["expect"][1] == "F"]
        assert at and above
        assert any(len(s["expect"]) > 2 and s["expect"][2] == "I" and built[s["name"]][1][2].sum() > ((s["m"] * s["n"]) >> 4) for s in default)
