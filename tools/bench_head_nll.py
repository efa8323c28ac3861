#!/usr/bin/env python3
"""Per-token negative log-likelihood out of a packed output head: the fused kernel (`GanqHipQuantLinear.nll`, csrc/lut_head_nll.hip)
against the chunked path of the same method and against the composition every caller wrote before,
`F.cross_entropy(head(x).float(), t, reduction="none")`.
Device time per call from HIP-graph replays; per point, in ONE process and alternating over --rounds rounds, the median of each side
and its spread (max - min).  Peak memory per side from an eager call before any graph exists: `torch.cuda.max_memory_allocated`
above what is allocated when the call starts (the inputs and the layer).  One JSON line per point (--out: also appended to that file).

  fused        head.nll(x, t, fused=True)        logits never written: 8 bytes per token and 128-feature tile of partials
  chunked      head.nll(x, t, fused=False)       logits of one row chunk at a time (NLL_CHUNK_BYTES)
  composition  F.cross_entropy(head(x).float(), t, reduction="none")      [M, vocab] logits in fp16 and again in fp32

    python tools/bench_head_nll.py [--shapes 128256x2048,50272x768] [--M 256,2048,4096] [--bits 4] [--reps 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ganq_amd import _lib  # noqa: E402
from ganq_amd.nn_modules.qlinear.ganq_hip import GanqHipQuantLinear  # noqa: E402


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


def peak_mib(fn):
    """peak of the allocator during one eager call, above what was allocated when it started"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak / 2 ** 20


def head(m, n, bits, g):
    V = 2 ** bits
    Q = torch.randint(0, V, (m, n), device="cuda", generator=g, dtype=torch.int32).to(torch.uint8)
    layer = GanqHipQuantLinear(bits=bits, group_size=-1, sym=True, desc_act=False, in_features=n, out_features=m).cuda()
    layer.qweight = _lib.pack_indices(Q, bits)
    layer.lut = (0.02 * torch.randn(m, V, device="cuda", generator=g)).half()
    return layer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128256x2048,50272x768")
    ap.add_argument("--M", default="256,2048,4096")
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    with torch.no_grad():
        for shp in a.shapes.split(","):
            m, n = (int(v) for v in shp.split("x"))
            layer = head(m, n, a.bits, g)
            for M in (int(v) for v in a.M.split(",")):
                x = torch.randn(M, n, device="cuda", generator=g).half()
                t = torch.randint(0, m, (M,), device="cuda", generator=g)
                t[::97] = -100
                fns = {"fused": lambda: layer.nll(x, t, fused=True), "chunked": lambda: layer.nll(x, t, fused=False),
                       "composition": lambda: F.cross_entropy(layer(x).float(), t, reduction="none")}
                want = fns["composition"]()
                diff = {k: float((fns[k]() - want).abs().max()) for k in ("fused", "chunked")}
                del want
                mem = {k: peak_mib(f) for k, f in fns.items()}
                times = alternate(fns, a.reps, a.rounds)
                rec = {"what": "head_nll", "vocab_x_hidden": f"{m}x{n}", "M": M, "bits": a.bits, "dtype": "fp16", "rounds": a.rounds,
                       "reps_per_replay": a.reps}
                for k in fns:
                    rec[f"{k}_us"], rec[f"{k}_spread_us"] = round(times[k][0], 1), round(times[k][1], 1)
                    rec[f"{k}_peak_mib"] = round(mem[k], 1)
                rec["fused_vs_composition_time"] = round(times["fused"][0] / times["composition"][0], 3)
                rec["fused_vs_composition_mem"] = round(mem["fused"] / mem["composition"], 5)
                rec["max_abs_diff_vs_composition"] = {k: round(v, 6) for k, v in diff.items()}
                line = json.dumps(rec)
                print(line, flush=True)
                if a.out:
                    with open(a.out, "a") as f:
                        f.write(line + "\n")
                del times, x, t, fns
                torch.cuda.empty_cache()
            del layer
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
