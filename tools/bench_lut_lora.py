#!/usr/bin/env python3
"""LUT forward with a low-rank adapter (`_lib.lut_linear_lora`) against the plain forward and the composition it replaces.
Device time per call from HIP-graph replays; per point, in ONE process and alternating over --rounds rounds:
  (a) fused     _lib.lut_linear_lora(x, ..., lora_A, lora_B)
  (b) plain     _lib.lut_linear(x, ...)                                  no adapter: what the adapter costs on top
  (c) composed  _lib.lut_linear(x, ..., addend=(x @ A.T).float() @ B.T.float())   two library GEMMs + the fp32 [M, m] round trip
Reported: the median of each over the rounds, the spread (max - min) of (b) beside every difference, fused / composed and the
overhead fused - plain.  One JSON line per point (--out: also appended to that file).

--outliers RATIO adds, per point with M <= 64, a layer that also has that share of sparse outliers (CSR): the adapter call with the
outliers handed over (`outliers=`: inside the decode launch at decode sizes), the same with their product as an fp32 addend
(`outlier_matmul` + `addend=`), and the layer without adapter (`lut_linear_outliers`).

    python tools/bench_lut_lora.py [--shapes 4096x4096,14336x4096,4096x14336] [--M 1,16,64,512,2048,4096] [--ranks 32,128]
                                   [--outliers 0.005] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ganq_amd import _lib  # noqa: E402


def make_graph(fn, reps):
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
    return g


def replay_us(g, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def make_csr(m, n, ratio, dtype, g):
    per_row = max(1, int(round(n * ratio)))
    cols = torch.stack([torch.randperm(n, device="cuda", generator=g)[:per_row].sort().values for _ in range(m)]).reshape(-1).to(torch.int32)
    rowptr = (torch.arange(m + 1, device="cuda") * per_row).to(torch.int32)
    vals = (0.1 * torch.randn(m * per_row, device="cuda", generator=g)).to(dtype)
    return rowptr, cols, vals


def bench(m, n, M, r, bits=4, dtype=torch.float16, rounds=7, outliers=0.0):
    g = torch.Generator(device="cuda").manual_seed(0)
    V = 2 ** bits
    Q = torch.randint(0, V, (m, n), device="cuda", generator=g, dtype=torch.int32).to(torch.uint8)
    lut = (0.02 * torch.randn(m, V, device="cuda", generator=g)).to(dtype)
    x = torch.randn(M, n, device="cuda", generator=g).to(dtype)
    A = (torch.randn(r, n, device="cuda", generator=g) / n ** 0.5).to(dtype)
    B = (0.05 * torch.randn(m, r, device="cuda", generator=g)).to(dtype)
    qw = _lib.pack_indices(Q, bits)
    reps = 20 if M <= 512 else 5
    fns = {"fused": lambda: _lib.lut_linear_lora(x, qw, lut, None, bits, A, B),
           "plain": lambda: _lib.lut_linear(x, qw, lut, None, bits),
           "composed": lambda: _lib.lut_linear(x, qw, lut, None, bits, addend=(x @ A.T).float() @ B.T.float())}
    if outliers:
        rowptr, cols, vals = make_csr(m, n, outliers, dtype, g)
        fns = {"fused": lambda: _lib.lut_linear_lora(x, qw, lut, None, bits, A, B, outliers=(rowptr, cols, vals)),
               "plain": lambda: _lib.lut_linear_outliers(x, qw, lut, None, bits, rowptr, cols, vals),
               "composed": lambda: _lib.lut_linear_lora(x, qw, lut, None, bits, A, B, addend=_lib.outlier_matmul(x, rowptr, cols, vals, m))}
    graphs = {k: make_graph(f, reps) for k, f in fns.items()}
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k in fns:  # alternating
            times[k].append(replay_us(graphs[k], reps))
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"out_x_in": f"{m}x{n}", "M": M, "rank": r, **({"outliers": outliers, "composed_is": "adapter call + outlier_matmul addend"} if outliers else {}), "bits": bits, "dtype": str(dtype).replace("torch.", ""), "rounds": rounds,
            "fused_us": round(med["fused"], 2), "plain_us": round(med["plain"], 2), "composed_us": round(med["composed"], 2),
            "plain_spread_us": round(max(times["plain"]) - min(times["plain"]), 2),
            "fused_spread_us": round(max(times["fused"]) - min(times["fused"]), 2),
            "overhead_us": round(med["fused"] - med["plain"], 2), "overhead_rel": round(med["fused"] / med["plain"] - 1, 3),
            "fused_vs_composed": round(med["fused"] / med["composed"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x4096,14336x4096,4096x14336")
    ap.add_argument("--M", default="1,16,64,512,2048,4096")
    ap.add_argument("--ranks", default="32,128")
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--outliers", type=float, default=0.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    for shp in a.shapes.split(","):
        m, n = (int(v) for v in shp.split("x"))
        for M in (int(v) for v in a.M.split(",")):
            for r in (int(v) for v in a.ranks.split(",")):
                lines = [json.dumps(bench(m, n, M, r, a.bits, rounds=a.rounds))]
                if a.outliers and M <= 64:
                    lines.append(json.dumps(bench(m, n, M, r, a.bits, rounds=a.rounds, outliers=a.outliers)))
                for line in lines:
                    print(line, flush=True)
                    if a.out:
                        with open(a.out, "a") as f:
                            f.write(line + "\n")


if __name__ == "__main__":
    main()
