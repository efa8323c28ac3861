#!/usr/bin/env python3
"""What the draw of the Gumbel noise costs a sampled pick out of a packed output head (`GanqHipQuantLinear.pick`,
csrc/lut_head_pick.hip): drawn by four torch launches into an fp32 [M, vocab] tensor the kernel reads back, or inside the kernel's
epilogue from a PickRng state (Philox4x32-10).  The protocol of tools/bench_head_pick.py: device time per call from HIP-graph
replays; per point, in ONE process and alternating over --rounds rounds, the median of each side and its spread (max - min).
One JSON line per point (--out: also appended to that file).

  greedy          head.pick(x)                                   no noise at all: the floor of both sampled calls
  sampled_torch   head.pick(x, temperature=0.7)                  the noise from torch (empty, exponential_, clamp_min_/log_, neg_)
  sampled_seeded  head.pick(x, temperature=0.7, rng=PickRng(0))  the noise drawn in the epilogue, the state advanced by the merge launch

Reported beside the times: torch_draw_us = sampled_torch - greedy and seeded_draw_us = sampled_seeded - greedy (what each draw adds),
to be read against greedy_spread_us.  A replay of sampled_torch repeats one noise tensor, a replay of sampled_seeded samples afresh.

    python tools/bench_head_pick_rng.py [--shapes 128256x2048,50272x768] [--M 1,16,64] [--bits 4] [--reps 20] [--out FILE]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_head_nll import alternate, head  # noqa: E402
from ganq_amd.nn_modules.qlinear.ganq_hip import PickRng  # noqa: E402

TEMPERATURE = 0.7


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
                rng = PickRng(0)
                fns = {"greedy": lambda: layer.pick(x), "sampled_torch": lambda: layer.pick(x, temperature=TEMPERATURE),
                       "sampled_seeded": lambda: layer.pick(x, temperature=TEMPERATURE, rng=rng)}
                times = alternate(fns, a.reps, a.rounds)
                rec = {"what": "head_pick_rng", "vocab_x_hidden": f"{m}x{n}", "M": M, "bits": a.bits, "dtype": "fp16", "rounds": a.rounds,
                       "reps_per_replay": a.reps}
                for k in fns:
                    rec[f"{k}_us"], rec[f"{k}_spread_us"] = round(times[k][0], 2), round(times[k][1], 2)
                rec["torch_draw_us"] = round(times["sampled_torch"][0] - times["greedy"][0], 2)
                rec["seeded_draw_us"] = round(times["sampled_seeded"][0] - times["greedy"][0], 2)
                rec["seeded_vs_torch"] = round(times["sampled_seeded"][0] / times["sampled_torch"][0], 3)
                rec["picks_drawn"] = rng.offset  # every call of every replay advanced the state by one
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
