#!/usr/bin/env python3
"""EoRA generation time beside the module's quantize() time: one nn.Linear per shape through GANQ.quantize() with and without
`eora_rank` (same synthetic calibration activations, second of two runs each: warm), one JSON line per shape.

    python tools/time_eora.py [--shapes 4096x4096,14336x4096,4096x14336] [--rank 64] [--bits 3] [--out FILE]"""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ganq_amd.looper.named_module import NamedModule  # noqa: E402
from ganq_amd.quantization import GANQ, QuantizeConfig  # noqa: E402


def run(m, n, bits, rank, X, W):
    lin = nn.Linear(n, m, bias=False).half().cuda()
    with torch.no_grad():
        lin.weight.copy_(W)
    q = GANQ(NamedModule(lin, "proj", "model.layers.0.proj", 0), QuantizeConfig(bits=bits))
    q.quantizer.configure(perchannel=True)
    q.eora_rank = rank
    for xb in X:
        q.add_batch(xb, None)
    torch.cuda.synchronize()
    out = q.quantize()
    res = {"quantize_s": round(out[4], 4)}
    if rank:
        res.update({"eora_s": round(q.eora_time, 4), "eora_e_over_e0": round(q.eora_e / q.eora_e0, 4)})
    q.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x4096,14336x4096,4096x14336")
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--bits", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    for shp in a.shapes.split(","):
        m, n = (int(v) for v in shp.split("x"))
        g = torch.Generator(device="cuda").manual_seed(0)
        W = (0.02 * torch.randn(m, n, device="cuda", generator=g)).half()
        scale = torch.ones(n, device="cuda")
        scale[:8] = torch.tensor([30.0, 20.0, 12.0, 8.0, 6.0, 5.0, 4.0, 3.0], device="cuda")
        X = [(torch.randn(1, 2048, n, device="cuda", generator=g) * scale).half() for _ in range(max(4, 2 * n // 2048))]
        plain = [run(m, n, a.bits, 0, X, W) for _ in range(2)][-1]
        with_eora = [run(m, n, a.bits, a.rank, X, W) for _ in range(2)][-1]
        line = json.dumps({"out_x_in": shp, "bits": a.bits, "rank": a.rank, "quantize_s_without": plain["quantize_s"],
                           "quantize_s_with": with_eora["quantize_s"], "eora_s": with_eora["eora_s"],
                           "eora_e_over_e0": with_eora["eora_e_over_e0"]})
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
