"""developer: where the exception lists of the T-update's full bucket sum stop paying (GANQ_T_TOP, GANQ_T_TOP_CAP; the default cap in
csrc/update_t.hip comes from this sweep).  Per in_features n (square layers): a Hessian with a unit diagonal and small off-diagonals,
plus k planted entries, k swept over powers of two up to the capacity of a list, alternating in one process
    D = 3 + fix-up of k entries  against  D = 4 (GANQ_T_TOP=0)     off-diagonals that fill digit 2, planted entries +-max|H|
    D = 2 + fix-up of k entries  against  D = 3 (cap 0)            off-diagonals below digit 2, planted entries in digit 2
The time is the full accumulation's own (HIP events around the launches of the bucket sum and the fix-up, ganq_profile_*), per call,
median of the repeats; the A of the two settings is asserted equal bit for bit.
usage: python tools/dev/accum_top_sweep.py [n ...] [--V 16] [--repeats 5] [--calls 3]"""
import argparse, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ganq_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("ns", nargs="*", type=int, default=[4096])
ap.add_argument("--V", type=int, default=16)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--calls", type=int, default=3)
ap.add_argument("--kmin", type=int, default=1)
args = ap.parse_args()
_lib.selftest()
KERNEL = "onehot_accum_kernel"


def hessian(n, off_log2, k, word, gen):
    """unit diagonal (I = 2^30), off-diagonals uniform below 2^off_log2 in I, k planted symmetric entries of +-word"""
    A = (torch.rand(n, n, generator=gen, device="cuda") * 2 - 1) * 2.0 ** (off_log2 - 30)
    H = torch.triu(A, 1)
    if k:
        u = torch.randint(1, n, (k,), generator=gen, device="cuda")
        v = (torch.rand(k, generator=gen, device="cuda") * u).long().clamp_(max=n - 2)
        sign = torch.randint(0, 2, (k,), generator=gen, device="cuda") * 2.0 - 1.0
        H[v, u] = sign * (word * 2.0 ** -30)
    H = H + H.T
    H.fill_diagonal_(1.0)
    return H.contiguous()


def timed(opts, WH, H, Q, V, calls):
    for name, v in opts.items():
        _lib.debug_option(name, v)
    _lib.profile_enable(True, only=KERNEL)
    for _ in range(calls):
        _lib.update_t(WH, H, Q, V)
    ms, cnt = _lib.profile_report()[KERNEL]
    _lib.profile_enable(False)
    return ms / cnt


for n in args.ns:
    m = n
    _lib.debug_option("GANQ_ACCUM_W4", 1)
    top = _lib.debug_top_rule(m, n, 0, 0)["list_max"]
    gen = torch.Generator(device="cuda").manual_seed(n)
    W = 0.02 * torch.randn(m, n, generator=gen, device="cuda")
    Q = torch.randint(0, args.V, (m, n), generator=gen, device="cuda", dtype=torch.uint8)
    # (sparse form, its partner): options, and the D each must report
    pairs = (("D=3+list vs D=4", 20, 2 ** 30, {"GANQ_T_TOP": -1, "GANQ_T_TOP_CAP": top}, 3, {"GANQ_T_TOP": 0, "GANQ_T_TOP_CAP": top}, 4),
             ("D=2+list vs D=3", 12, 100 * 65536, {"GANQ_T_TOP": -1, "GANQ_T_TOP_CAP": top}, 2, {"GANQ_T_TOP": -1, "GANQ_T_TOP_CAP": 0}, 3))
    for title, off_log2, word, o_sparse, d_sparse, o_dense, d_dense in pairs:
        print(f"# n = m = {n}, V = {args.V}: {title}   (list capacity {top})")
        print(f"{'planted':>8s} {'c3':>8s} {'c2':>9s} {'sparse ms (min med max)':>28s} {'denser ms (min med max)':>28s} {'sparse/denser':>14s}")
        k = 0 if d_dense == 4 else args.kmin
        while k <= top:
            H = hessian(n, off_log2, k, word, gen)
            WH = _lib.matmul_f32(W, H)
            outs = []
            skip = False
            for opts, D in ((o_sparse, d_sparse), (o_dense, d_dense)):
                for name, v in opts.items():
                    _lib.debug_option(name, v)
                got = _lib.debug_top_planes(H, m)
                if got["D"] != D:  # (planted entries fell on each other and the like)
                    skip = True
                    break
                _, A, _ = _lib.update_t(WH, H, Q, args.V, want_ab=True)
                outs.append(A.clone())
            if not skip:
                assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), f"n={n} k={k}: the two forms give different sums"
                t = ([], [])
                for _ in range(args.repeats):
                    t[0].append(timed(o_sparse, WH, H, Q, args.V, args.calls))
                    t[1].append(timed(o_dense, WH, H, Q, args.V, args.calls))
                s = [sorted(x) for x in t]
                f = lambda x: f"{x[0]:8.3f} {x[len(x) // 2]:8.3f} {x[-1]:8.3f}"  # noqa: E731
                print(f"{k:8d} {got['c3']:8d} {got['c2']:9d} {f(s[0]):>28s} {f(s[1]):>28s} {s[0][len(s[0]) // 2] / s[1][len(s[1]) // 2]:14.3f}", flush=True)
            else:
                print(f"{k:8d}  skipped: D = {got['D']} with counts {got['c3']}, {got['c2']}", flush=True)
            k = max(2 * k, args.kmin if k else 1)
            del H, WH
    del W, Q
    torch.cuda.empty_cache()
for name in ("GANQ_ACCUM_W4", "GANQ_T_TOP", "GANQ_T_TOP_CAP"):
    _lib.debug_option(name, None)
