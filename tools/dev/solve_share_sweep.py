"""developer sweep of the shared helpers' split policies (GANQ_SOLVE_SHARE<k>_XA / _XB: the tile keeps max(XMIN, XA c / 64 - XB) of a
chain of c source panels), one shape per k at n = 4096: 2224 rows (139 tiles, k = 2), 2912 (182, k = 3), 3190 (200, k = 4).
Optional args: k values to sweep (default 2 3 4)."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ganq_amd import _lib
_lib.selftest()
V, n = 16, 4096
shape_of = {2: 2224, 3: 2912, 4: 3190}
torch.manual_seed(0)
L = torch.tril(torch.randn(n, n)).cuda() * 0.01 + torch.eye(n).cuda()
def run(W, T0):
    for _ in range(2): q = _lib.solve_s(W, L, T0)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(5): q = _lib.solve_s(W, L, T0)
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / 5, q
pols = {2: [(37, 0), (41, 0), (43, 0), (45, 0), (47, 0), (49, 0), (51, 0), (53, 0), (57, 0), (44, 6), (48, 8), (52, 12), (50, 2), (54, 4)],
        3: [(45, 0), (49, 0), (53, 0), (55, 0), (57, 0), (59, 0), (61, 0), (63, 0), (56, 8), (60, 8), (62, 2)],
        4: [(50, 0), (54, 0), (58, 0), (60, 0), (61, 0), (62, 0), (63, 0), (60, 6), (63, 2)]}
for k in [int(a) for a in sys.argv[1:]] or [2, 3, 4]:
    m = shape_of[k]
    torch.manual_seed(m)
    W = (0.02 * torch.randn(m, n)).cuda()
    T0 = torch.sort(0.02 * torch.randn(m, V))[0].cuda()
    plan = _lib.debug_solve_plan((m + 15) // 16)
    _lib.debug_option("GANQ_SOLVE_SHARE", 0)
    t0, ref = run(W, T0)
    _lib.debug_option("GANQ_SOLVE_SHARE", None)
    print(f"k={k}: {m}x{n}, planned {plan}; without shared helpers {t0:.3f} ms", flush=True)
    for xa, xb in pols[k]:
        _lib.debug_option(f"GANQ_SOLVE_SHARE{k}_XA", xa)
        _lib.debug_option(f"GANQ_SOLVE_SHARE{k}_XB", xb)
        t, q = run(W, T0)
        assert torch.equal(q, ref)
        print(f"  ({xa:2d}, {xb:2d}): {t:.3f} ms  {t0 / t:.3f}x", flush=True)
    _lib.debug_option(f"GANQ_SOLVE_SHARE{k}_XA", None)
    _lib.debug_option(f"GANQ_SOLVE_SHARE{k}_XB", None)
_lib.debug_option("GANQ_SOLVE_SHARE", 0)
t0, _ = run(W, T0)
print(f"without again ({m}x{n}): {t0:.3f} ms")
_lib.debug_option("GANQ_SOLVE_SHARE", None)
