"""developer A/B: S-solve with shared helper workgroups (one helper for every 2 .. 4 tiles where the launch has more tiles than half
the CUs and idle CUs left over) vs without them (GANQ_SOLVE_SHARE=0), alternating in one process; indices must be identical.
4096 x 4096 (a tile on every CU) and 2048 x 4096 (a helper per tile) are the controls that must not move.
Optional args: rows of further shapes at n = 4096."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ganq_amd import _lib
_lib.selftest()
V, n = 16, 4096
rows = [2224, 2912, 3072, 3584, 4096, 2048] + [int(a) for a in sys.argv[1:]]
torch.manual_seed(0)
L = torch.tril(torch.randn(n, n)).cuda() * 0.01 + torch.eye(n).cuda()
def timed(W, T0, reps=5):
    for _ in range(2): q = _lib.solve_s(W, L, T0)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps): q = _lib.solve_s(W, L, T0)
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / reps, q
for m in rows:
    torch.manual_seed(m)
    W = (0.02 * torch.randn(m, n)).cuda()
    T0 = torch.sort(0.02 * torch.randn(m, V))[0].cuda()
    plan = _lib.debug_solve_plan((m + 15) // 16)
    t = {0: [], 1: []}
    ref = None
    for rnd in range(3):
        for share in (0, 1):
            _lib.debug_option("GANQ_SOLVE_SHARE", share)
            ms, q = timed(W, T0)
            t[share].append(ms)
            ref = q if ref is None else ref
            assert torch.equal(q, ref), f"{m}x{n}: indices differ with GANQ_SOLVE_SHARE={share}"
    _lib.debug_option("GANQ_SOLVE_SHARE", None)
    a, b = sorted(t[0])[1], sorted(t[1])[1]
    print(f"{m}x{n} ({(m + 15) // 16} tiles, {plan['regime']} k={plan['k']}): without {a:.3f} ms ({min(t[0]):.3f} .. {max(t[0]):.3f}), "
          f"shared {b:.3f} ms ({min(t[1]):.3f} .. {max(t[1]):.3f})  {a / b:.3f}x  identical=True", flush=True)
