#!/usr/bin/env python3
"""Embedding lookup out of a row-packed LUT table (`_lib.lut_table_lookup`, what `QuantizeConfig(ganq_embedding=True)` installs) against
the lookup out of the column layout of the SAME indices (`_lib.lut_embedding`, the packed head's stream) and against `F.embedding` on
the fp16 table.  The protocol of tools/bench_lut_embedding.py: device time per call from HIP-graph replays; per point, in ONE process
and alternating over --rounds rounds, the median of each side and its spread (max - min).  One JSON line per point (--out: also
appended to that file).

  rows_us  _lib.lut_table_lookup(ids, qrows, lut, bits)         a token's row: n * bits / 8 contiguous bytes
  cols_us  _lib.lut_embedding(ids, qweight, lut, n, bits)       the words of a row lie 4 * vocab bytes apart
  fp16_us  F.embedding(ids, W)                                   2 n contiguous bytes

`rows_beats_cols`: rows_us is below cols_us by more than the larger of the two spreads.

    python tools/bench_embedding_table.py [--shapes 128256x2048,50272x768] [--N 1,16,2048] [--bits 4] [--out FILE]
    python tools/bench_embedding_table.py --stage 128256x2048     seconds of quantize_embedding_rows on a table of that shape"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ganq_amd import _lib  # noqa: E402
from bench_lut_embedding import alternate  # noqa: E402


def tables(m, n, bits, g):
    V = 2 ** bits
    Q = torch.randint(0, V, (m, n), device="cuda", generator=g, dtype=torch.int32).to(torch.uint8)
    lut = (0.02 * torch.randn(m, V, device="cuda", generator=g)).half()
    qw = _lib.pack_indices(Q, bits)
    del Q
    return qw, qw.t().contiguous(), lut, _lib.lut_dequant(qw, lut, n, bits)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def stage(shape, bits, out):
    """seconds of the embedding stage's work on a random fp16 table: k-means + assignment, chunked (one warm-up, three timed runs)"""
    from ganq_amd.quantization.embedding import quantize_embedding_rows

    m, n = (int(v) for v in shape.split("x"))
    g = torch.Generator(device="cuda").manual_seed(0)
    W = (0.02 * torch.randn(m, n, device="cuda", generator=g)).half()
    quantize_embedding_rows(W[:1024], bits)
    secs = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        qrows, T, sqerr = quantize_embedding_rows(W, bits)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    rel = float(sqerr.sum() / W.float().pow(2).sum())
    emit({"what": "quantize_embedding_rows", "vocab_x_hidden": shape, "bits": bits, "seconds": [round(s, 3) for s in secs],
          "median_s": round(statistics.median(secs), 3), "relative_squared_error": rel}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128256x2048,50272x768")
    ap.add_argument("--N", default="1,16,2048")
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--stage", default=None, help="VOCABxHIDDEN: time the row quantizer on a random table instead")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.stage:
        stage(a.stage, a.bits, a.out)
        return
    g = torch.Generator(device="cuda").manual_seed(0)
    for shp in a.shapes.split(","):
        m, n = (int(v) for v in shp.split("x"))
        qw, qrows, lut, W = tables(m, n, a.bits, g)
        for N in (int(v) for v in a.N.split(",")):
            ids = torch.randint(0, m, (N,), device="cuda", generator=g)
            o_rows = torch.empty((N, n), dtype=torch.float16, device="cuda")
            o_cols = torch.empty((N, n), dtype=torch.float16, device="cuda")
            want = F.embedding(ids, W)
            assert torch.equal(_lib.lut_table_lookup(ids, qrows, lut, a.bits), want)
            assert torch.equal(_lib.lut_embedding(ids, qw, lut, n, a.bits), want)
            t = alternate({"rows": lambda: _lib.lut_table_lookup(ids, qrows, lut, a.bits, out=o_rows),
                           "cols": lambda: _lib.lut_embedding(ids, qw, lut, n, a.bits, out=o_cols),
                           "fp16": lambda: F.embedding(ids, W)}, 20, a.rounds)
            (r_us, r_sp), (c_us, c_sp), (f_us, f_sp) = t["rows"], t["cols"], t["fp16"]
            emit({"what": "lookup", "vocab_x_hidden": shp, "N": N, "bits": a.bits, "rounds": a.rounds,
                  "rows_us": round(r_us, 2), "rows_spread_us": round(r_sp, 2), "cols_us": round(c_us, 2), "cols_spread_us": round(c_sp, 2),
                  "fp16_us": round(f_us, 2), "fp16_spread_us": round(f_sp, 2), "rows_vs_cols": round(r_us / c_us, 3),
                  "rows_vs_fp16": round(r_us / f_us, 3), "rows_beats_cols": bool(c_us - r_us > max(r_sp, c_sp))}, a.out)
        del qw, qrows, lut, W


if __name__ == "__main__":
    main()
