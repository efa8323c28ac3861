#!/usr/bin/env python3
"""Embedding lookup out of a packed LUT head (`_lib.lut_embedding`) against `F.embedding` on the fp16 table, and the head's forward
(`_lib.lut_linear`) against fp16 `F.linear` -- what `QuantizeConfig(lm_head=True)` changes per token.
Device time per call from HIP-graph replays; per point, in ONE process and alternating over --rounds rounds, the median of each and
its spread (max - min).  One JSON line per point (--out: also appended to that file).

  lookup   N ids (random over the vocabulary):   lut_us  _lib.lut_embedding(ids, qweight, lut, n, bits)      fp16_us  F.embedding(ids, W)
  head     x [M, n]:                              lut_us  _lib.lut_linear(x, qweight, lut, None, bits)        fp16_us  F.linear(x, W)

The words of one vocabulary row lie 4 * vocab bytes apart in the packed stream (one cache line each), the fp16 row is contiguous:
the lookup trades 4x fewer bytes held for more lines touched per row.

    python tools/bench_lut_embedding.py [--shapes 128256x2048,50272x768] [--N 1,16,2048] [--M 1,16] [--bits 4] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

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


def alternate(fns, reps, rounds):
    graphs = {k: make_graph(f, reps) for k, f in fns.items()}
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k in fns:  # alternating
            times[k].append(replay_us(graphs[k], reps))
    return {k: (statistics.median(v), max(v) - min(v)) for k, v in times.items()}


def layer(m, n, bits, g):
    V = 2 ** bits
    Q = torch.randint(0, V, (m, n), device="cuda", generator=g, dtype=torch.int32).to(torch.uint8)
    lut = (0.02 * torch.randn(m, V, device="cuda", generator=g)).half()
    qw = _lib.pack_indices(Q, bits)
    del Q
    return qw, lut, _lib.lut_dequant(qw, lut, n, bits)


def result(kind, m, n, size, bits, rounds, t):
    (lut_us, lut_sp), (ref_us, ref_sp) = t["lut"], t["fp16"]
    return {"what": kind, "vocab_x_hidden": f"{m}x{n}", "N" if kind == "lookup" else "M": size, "bits": bits, "rounds": rounds,
            "lut_us": round(lut_us, 2), "lut_spread_us": round(lut_sp, 2), "fp16_us": round(ref_us, 2), "fp16_spread_us": round(ref_sp, 2),
            "lut_vs_fp16": round(lut_us / ref_us, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128256x2048,50272x768")
    ap.add_argument("--N", default="1,16,2048")
    ap.add_argument("--M", default="1,16")
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    for shp in a.shapes.split(","):
        m, n = (int(v) for v in shp.split("x"))
        qw, lut, W = layer(m, n, a.bits, g)
        lines = []
        for N in (int(v) for v in a.N.split(",")):
            ids = torch.randint(0, m, (N,), device="cuda", generator=g)
            out = torch.empty((N, n), dtype=torch.float16, device="cuda")
            assert torch.equal(_lib.lut_embedding(ids, qw, lut, n, a.bits), F.embedding(ids, W))
            t = alternate({"lut": lambda: _lib.lut_embedding(ids, qw, lut, n, a.bits, out=out), "fp16": lambda: F.embedding(ids, W)},
                          20, a.rounds)
            lines.append(result("lookup", m, n, N, a.bits, a.rounds, t))
        for M in (int(v) for v in a.M.split(",")):
            x = torch.randn(M, n, device="cuda", generator=g).half()
            t = alternate({"lut": lambda: _lib.lut_linear(x, qw, lut, None, a.bits), "fp16": lambda: F.linear(x, W)}, 20, a.rounds)
            lines.append(result("head", m, n, M, a.bits, a.rounds, t))
        for rec in lines:
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
        del qw, lut, W


if __name__ == "__main__":
    main()
