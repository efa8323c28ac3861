"""developer: A/B of the incremental bucket sums, all four digit planes of H (GANQ_MU_TOP=0) against the dense planes only (-1: the
full sum's; 3: those, but at least three), alternating in one process, on synthetic 4096 x 4096 layers: `massive` two features x 1000 (D = 2), `plain` independent features
(D = 3, the benchmark layer's kind), `dense` a common factor in every feature (D = 4: both settings run the same code, the pair shows
the noise).  Per repeat: the wall time of ganq_run_layer (K iterations) and, from a second instrumented call, the time of the
incremental kernels of all iterations (HIP events around q_diff + update, ganq_profile_*) and of the T-update's preparation.  Asserts
that the two settings return the same bytes.
usage: python tools/dev/mu_top_ab.py [kind ...] [--n 4096] [--m 4096] [--K 10] [--repeats 6]"""
import argparse, os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ganq_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("kinds", nargs="*", default=["massive", "dense", "plain"])
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--m", type=int, default=4096)
ap.add_argument("--K", type=int, default=10)
ap.add_argument("--V", type=int, default=16)
ap.add_argument("--repeats", type=int, default=6)
args = ap.parse_args()
_lib.selftest()
SET = (0, 3, -1)
INCR, PREP = "t_incremental_kernels", "t_prepare_kernels"


def layer(kind, m, n, V, gen):
    W = (0.02 * torch.randn(m, n, generator=gen, device="cuda")).half().float()
    scales = 0.1 + torch.rand(n, generator=gen, device="cuda")
    if kind == "massive":
        scales[torch.randperm(n, generator=gen, device="cuda")[:2]] *= 1000.0
    p = 2 * n
    X = torch.randn(p, n, generator=gen, device="cuda", dtype=torch.float64)
    if kind == "dense":
        X += 0.5 * torch.randn(p, 1, generator=gen, device="cuda", dtype=torch.float64)
    X *= scales.double()
    H = (2.0 / p) * (X.T @ X)
    del X
    H += 0.01 * H.diagonal().mean() * torch.eye(n, device="cuda", dtype=torch.float64)
    H = H.float()
    H = (0.5 * (H + H.T)).contiguous()
    Hd = H.double()
    off = (Hd.abs().sum(1) - 2 * Hd.diagonal()).clamp_min(1e-8)
    L = torch.linalg.cholesky(Hd + torch.diag(off)).float().contiguous()
    T0 = _lib.kmeans_init(W, None, V)
    return W, H, L, T0


def once(mu_top, lay, ws, K):
    _lib.debug_option("GANQ_MU_TOP", mu_top)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = _lib.run_layer(*lay, K, alias_q=True, workspace=ws)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    prof = {}
    for name in (INCR, PREP):
        _lib.profile_enable(True, only=name)
        _lib.run_layer(*lay, K, alias_q=True, workspace=ws)
        prof[name] = _lib.profile_report()[name][0]
        _lib.profile_enable(False)
    return wall, prof[INCR], prof[PREP], out


for kind in args.kinds:
    gen = torch.Generator(device="cuda").manual_seed(7)
    lay = layer(kind, args.m, args.n, args.V, gen)
    ws = _lib.run_layer_workspace(args.m, args.n, args.V, lay[0].device)
    tp = _lib.debug_top_planes(lay[1], args.m)
    d = {}
    for mt in SET:
        _lib.debug_option("GANQ_MU_TOP", mt)
        d[mt] = _lib.debug_mu_planes(args.m, args.n, tp["c3"], tp["c2"])["D"]
    print(f"# {kind}: {args.m} x {args.n}, V = {args.V}, K = {args.K}; c3 = {tp['c3']}, c2 = {tp['c2']}, cap = {tp['cap']}; planes read: "
          f"GANQ_MU_TOP " + ", ".join(f"{mt} -> {d[mt]}" for mt in SET), flush=True)
    outs = {mt: once(mt, lay, ws, args.K)[3] for mt in SET}  # warm-up of each, and the bytes
    for mt in SET[1:]:
        for a, b in zip(outs[0][:3], outs[mt][:3]):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"{kind}: the settings return different bytes"
    t = {mt: [] for mt in SET}
    for _ in range(args.repeats):
        for mt in SET:
            t[mt].append(once(mt, lay, ws, args.K)[:3])
    for col, what in enumerate(("run_layer wall ms", "incremental kernels ms per layer", "t_prepare ms")):
        for mt in SET:
            v = sorted(x[col] for x in t[mt])
            print(f"  {what:34s} GANQ_MU_TOP={mt:2d}: " + " ".join(f"{x:.3f}" for x in (r[col] for r in t[mt])) +
                  f"   median {v[len(v) // 2]:.3f}  spread {v[-1] - v[0]:.3f}", flush=True)
    del lay, ws, outs
    torch.cuda.empty_cache()
_lib.debug_option("GANQ_MU_TOP", None)
