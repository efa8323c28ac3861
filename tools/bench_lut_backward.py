#!/usr/bin/env python3
"""LUT backward (csrc/lut_backward.hip) against the forward and the library.  Device time per call from HIP-graph replays.
Per (m x n, M): dx = dy @ Wq against the forward lut_linear at the same point and torch dy @ Wq on the pre-dequantised weight;
dlut against torch dy.t() @ x (the library GEMM of the same flops) and the torch composition it replaces (fp32 GEMM +
scatter_add by the codes).  TFLOP/s = 2 M m n / t.  One JSON line per point (--out: also appended to that file).

    python tools/bench_lut_backward.py [--shapes 4096x4096,14336x4096,4096x14336] [--M 1,16,64,512,2048,4096] [--out FILE]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ganq_amd import _lib  # noqa: E402


def graph_time(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(reps):
                fn()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3  # us


def bench(m, n, M, bits=4, dtype=torch.float16):
    g = torch.Generator(device="cuda").manual_seed(0)
    V = 2 ** bits
    Q = torch.randint(0, V, (m, n), device="cuda", generator=g, dtype=torch.int32).to(torch.uint8)
    lut = (0.02 * torch.randn(m, V, device="cuda", generator=g)).to(dtype)
    x = torch.randn(M, n, device="cuda", generator=g).to(dtype)
    dy = torch.randn(M, m, device="cuda", generator=g).to(dtype)
    qw = _lib.pack_indices(Q, bits)
    Wq = _lib.lut_dequant(qw, lut, n, bits)
    Ql = Q.long()
    t_dx = graph_time(lambda: _lib.lut_linear_bwd_input(dy, qw, lut, bits))
    t_fwd = graph_time(lambda: _lib.lut_linear(x, qw, lut, None, bits))
    t_dx_lib = graph_time(lambda: dy @ Wq)
    t_dlut = graph_time(lambda: _lib.lut_linear_bwd_lut(dy, x, qw, bits, m))
    t_dlut_lib = graph_time(lambda: dy.t() @ x)
    t_dlut_torch = graph_time(lambda: torch.zeros(m, V, device="cuda").scatter_add_(1, Ql, dy.float().t() @ x.float()))
    flop = 2.0 * M * m * n
    return {"out_x_in": f"{m}x{n}", "M": M, "bits": bits, "dtype": str(dtype).replace("torch.", ""),
            "dx_us": round(t_dx, 1), "fwd_lut_linear_us": round(t_fwd, 1), "torch_dy_at_Wq_us": round(t_dx_lib, 1),
            "dx_vs_fwd": round(t_dx / t_fwd, 3),
            "dlut_us": round(t_dlut, 1), "torch_dyT_at_x_us": round(t_dlut_lib, 1), "torch_f32_gemm_scatter_us": round(t_dlut_torch, 1),
            "dlut_vs_torch_gemm": round(t_dlut / t_dlut_lib, 3),
            "dx_TFLOPs": round(flop / t_dx / 1e6, 1), "dlut_TFLOPs": round(flop / t_dlut / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x4096,14336x4096,4096x14336")
    ap.add_argument("--M", default="1,16,64,512,2048,4096")
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    for shp in a.shapes.split(","):
        m, n = (int(v) for v in shp.split("x"))
        for M in (int(v) for v in a.M.split(",")):
            r = bench(m, n, M, a.bits)
            line = json.dumps(r)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
