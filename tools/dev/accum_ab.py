"""developer: A/B of the T-update's full bucket sum, first kernel (GANQ_ACCUM_W4=0) against the four-wave kernel (=1), alternating
in one process.  Per shape: the kernel's own time (HIP events around the launch, ganq_profile_*) per call for every repeat, and an
assertion that the two give the same A -- bit for bit: the sums behind it are integers.
usage: python tools/dev/accum_ab.py [MxN ...] [--V 8] [--repeats 5] [--calls 3]"""
import argparse, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ganq_amd import _lib

SHAPES = "768x3072 3072x768 2048x8192 8192x2048 14336x4096 4096x14336 4096x11008 4096x4096"
ap = argparse.ArgumentParser()
ap.add_argument("shapes", nargs="*", default=SHAPES.split())
ap.add_argument("--V", type=int, default=8)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--calls", type=int, default=3)
args = ap.parse_args()
_lib.selftest()
KERNEL = "onehot_accum_kernel"


def timed(w4, WH, H, Q, V, calls):
    _lib.debug_option("GANQ_ACCUM_W4", w4)
    _lib.profile_enable(True, only=KERNEL)
    for _ in range(calls):
        _lib.update_t(WH, H, Q, V)
    ms, cnt = _lib.profile_report()[KERNEL]
    _lib.profile_enable(False)
    return ms / cnt


print(f"{'shape':>12s} {'plan':>16s} {'old ms (min med max)':>26s} {'new ms (min med max)':>26s} {'new/old':>8s}")
for shape in args.shapes:
    m, n = map(int, shape.split("x"))
    torch.manual_seed(m + n)
    W = (0.02 * torch.randn(m, n)).cuda()
    X = torch.randn(n, 2 * n, device="cuda") * (0.1 + torch.rand(n, 1, device="cuda"))
    H = (X @ X.T / (2 * n)).contiguous()
    del X
    Q = torch.randint(0, args.V, (m, n), device="cuda", dtype=torch.uint8)
    WH = _lib.matmul_f32(W, H)
    _lib.debug_option("GANQ_ACCUM_W4", None)
    plan = _lib.accum_plan(m, n)
    outs = {}
    for w4 in (0, 1):
        _lib.debug_option("GANQ_ACCUM_W4", w4)
        assert _lib.accum_plan(m, n)["kernel"] == ("onehot_accum_w4" if w4 and plan["supported"] else "onehot_accum")
        _, A, _ = _lib.update_t(WH, H, Q, args.V, want_ab=True)  # (also the warm-up of this kernel at this shape)
        outs[w4] = A.clone()
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), f"{shape}: the two kernels give different sums"
    t = {0: [], 1: []}
    for _ in range(args.repeats):
        for w4 in (0, 1):
            t[w4].append(timed(w4, WH, H, Q, args.V, args.calls))
    _lib.debug_option("GANQ_ACCUM_W4", None)
    s = {k: sorted(v) for k, v in t.items()}
    f = lambda v: f"{v[0]:8.3f} {v[len(v) // 2]:8.3f} {v[-1]:8.3f}"  # noqa: E731
    print(f"{shape:>12s} {plan['kernel']:>16s} {f(s[0])} {f(s[1])} {s[1][len(s[1]) // 2] / s[0][len(s[0]) // 2]:8.3f}", flush=True)
    del W, H, Q, WH, outs
    torch.cuda.empty_cache()
