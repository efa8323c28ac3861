#!/usr/bin/env python3
"""The next token out of a packed output head: the fused kernel (`GanqHipQuantLinear.pick`, csrc/lut_head_pick.hip) against the
head's forward alone and against the compositions every caller wrote before.
Device time per call from HIP-graph replays; per point, in ONE process and alternating over --rounds rounds, the median of each side
and its spread (max - min).  One JSON line per point (--out: also appended to that file).

  fused_greedy    head.pick(x)                                        token + logprob, the logits never written
  fused_sampled   head.pick(x, temperature=0.7)                       ... including the draw of the [M, vocab] noise (four torch launches)
  head            head(x)                                             the logits in fp16, nothing chosen yet
  comp_greedy     l = head(x).float(); argmax; logsumexp; gather
  comp_sampled    s = head(x).float() / T; softmax; exponential_; divide; argmax; gather; logsumexp

    python tools/bench_head_pick.py [--shapes 128256x2048,50272x768] [--M 1,16,64] [--bits 4] [--reps 20] [--out FILE]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_head_nll import alternate, head  # noqa: E402

TEMPERATURE = 0.7


def comp_greedy(layer, x):
    l = layer(x).float()
    t = l.argmax(dim=-1)
    return t, l.gather(1, t.unsqueeze(1)).squeeze(1) - torch.logsumexp(l, dim=-1)


def comp_sampled(layer, x):
    s = layer(x).float() * (1.0 / TEMPERATURE)
    p = torch.softmax(s, dim=-1)
    t = (p / torch.empty_like(p).exponential_()).argmax(dim=-1)
    return t, s.gather(1, t.unsqueeze(1)).squeeze(1) - torch.logsumexp(s, dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128256x2048,50272x768")
    ap.add_argument("--M", default="1,16,64")
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
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
                fns = {"fused_greedy": lambda: layer.pick(x), "fused_sampled": lambda: layer.pick(x, temperature=TEMPERATURE),
                       "head": lambda: layer(x), "comp_greedy": lambda: comp_greedy(layer, x), "comp_sampled": lambda: comp_sampled(layer, x)}
                (tf, lf), (tc, lc) = fns["fused_greedy"](), fns["comp_greedy"]()
                same = tf == tc
                times = alternate(fns, a.reps, a.rounds)
                rec = {"what": "head_pick", "vocab_x_hidden": f"{m}x{n}", "M": M, "bits": a.bits, "dtype": "fp16", "rounds": a.rounds,
                       "reps_per_replay": a.reps}
                for k in fns:
                    rec[f"{k}_us"], rec[f"{k}_spread_us"] = round(times[k][0], 2), round(times[k][1], 2)
                rec["fused_greedy_vs_head"] = round(times["fused_greedy"][0] / times["head"][0], 3)
                rec["fused_greedy_vs_comp_greedy"] = round(times["fused_greedy"][0] / times["comp_greedy"][0], 3)
                rec["fused_sampled_vs_comp_sampled"] = round(times["fused_sampled"][0] / times["comp_sampled"][0], 3)
                rec["greedy_tokens_equal"] = f"{int(same.sum())}/{M}"
                rec["max_abs_logprob_diff_greedy"] = round(float((lf - lc)[same].abs().max()) if bool(same.any()) else 0.0, 6)
                line = json.dumps(rec)
                print(line, flush=True)
                if a.out:
                    with open(a.out, "a") as f:
                        f.write(line + "\n")
                del times, x, fns
                torch.cuda.empty_cache()
            del layer
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
