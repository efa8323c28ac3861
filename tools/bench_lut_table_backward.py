#!/usr/bin/env python3
"""Codebook gradient of the packed embedding lookups (`_lib.lut_table_bwd_lut` on the row-packed table, `_lib.lut_embedding_bwd_lut`
on the column layout of the SAME indices) beside the backward of `F.embedding` into a dense fp16 table of the same size.  The protocol
of tools/bench_lut_embedding.py: device time per call from HIP-graph replays; per point, in ONE process and alternating over --rounds
rounds, the median of each side and its spread (max - min).  One JSON line per point (--out: also appended to that file).

  rows_us   _lib.lut_table_bwd_lut(ids, dy, qrows, bits)             sort of the ids + memset + two launches -> dlut fp32 [m, 2^bits]
  cols_us   _lib.lut_embedding_bwd_lut(ids, dy, qweight, n, bits)    the same with the words of a row 4 * vocab bytes apart
  sort_us   torch.sort(ids, stable=True)                             the share of both calls above that is the caller's sort
  dense_us  aten.embedding_dense_backward(dy, ids, m)                zero-fills and scatters into a dense fp16 [m, n] gradient

ids: `uniform` over the vocabulary, or `half_equal`: every second position holds id 0 (a padding / BOS token in a batch).

    python tools/bench_lut_table_backward.py [--shapes 128256x2048,50272x768] [--N 16,2048] [--bits 4] [--out FILE]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ganq_amd import _lib  # noqa: E402
from bench_lut_embedding import alternate  # noqa: E402


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128256x2048,50272x768")
    ap.add_argument("--N", default="16,2048")
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    V = 2 ** a.bits
    for shp in a.shapes.split(","):
        m, n = (int(v) for v in shp.split("x"))
        Q = torch.randint(0, V, (m, n), device="cuda", generator=g, dtype=torch.int32).to(torch.uint8)
        qw = _lib.pack_indices(Q, a.bits)
        qrows = qw.t().contiguous()
        for N in (int(v) for v in a.N.split(",")):
            for pattern in ("uniform",) + (("half_equal",) if N >= 2048 else ()):
                ids = torch.randint(0, m, (N,), device="cuda", generator=g)
                if pattern == "half_equal":
                    ids[::2] = 0
                dy = torch.randn(N, n, device="cuda", generator=g).half()
                # both layouts give the same bits, and they are the bins of the unpacked indices (fp64, to fp32 rounding)
                got = _lib.lut_table_bwd_lut(ids, dy, qrows, a.bits)
                assert torch.equal(got, _lib.lut_embedding_bwd_lut(ids, dy, qw, n, a.bits))
                uniq, inv = torch.unique(ids, return_inverse=True)
                G = (inv[None, :] == torch.arange(uniq.numel(), device="cuda")[:, None]).double() @ dy.double()  # d loss / d table rows
                ref = torch.stack([(G * (Q[uniq] == v)).sum(1) for v in range(V)], dim=1)
                assert float((got[uniq].double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
                assert int(torch.count_nonzero(got)) == int(torch.count_nonzero(got[uniq]))  # rows no id selects are zero
                del G, ref
                t = alternate({"rows": lambda: _lib.lut_table_bwd_lut(ids, dy, qrows, a.bits),
                               "cols": lambda: _lib.lut_embedding_bwd_lut(ids, dy, qw, n, a.bits),
                               "sort": lambda: torch.sort(ids, stable=True),
                               "dense": lambda: torch.ops.aten.embedding_dense_backward(dy, ids, m, -1, False)}, 20, a.rounds)
                rec = {"what": "lookup_bwd_lut", "vocab_x_hidden": shp, "N": N, "ids": pattern, "bits": a.bits, "rounds": a.rounds}
                for k in ("rows", "cols", "sort", "dense"):
                    rec[f"{k}_us"], rec[f"{k}_spread_us"] = round(t[k][0], 2), round(t[k][1], 2)
                rec["rows_vs_dense"] = round(t["rows"][0] / t["dense"][0], 3)
                rec["cols_vs_dense"] = round(t["cols"][0] / t["dense"][0], 3)
                emit(rec, a.out)
        del Q, qw, qrows


if __name__ == "__main__":
    main()
