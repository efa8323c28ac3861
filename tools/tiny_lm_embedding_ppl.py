#!/usr/bin/env python3
"""GPTQ-style perplexity of the tiny trained model (tests/golden/tiny_lm, tied, vocab 256) with and without the embedding stage
(`QuantizeConfig.ganq_embedding`), in the configuration of tests/test_tiny_lm.py (K = 10): at 4 and 3 bits the body alone, the body +
the embedding, `lm_head` + "untie", and both; then, at 3 bits, the runs that tell which packed table carries the cost (one of them at
4 bits through `dynamic`, the FAKE format, "share" without the stage).  One JSON line per run (--out: also appended to that file).

    python tools/tiny_lm_embedding_ppl.py [--out profiles/embedding_table_v1.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_tiny_lm as tiny  # noqa: E402
from ganq_amd.models.quantize import gptq_style_ppl, quantize_model  # noqa: E402
from ganq_amd.quantization.config import QuantizeConfig  # noqa: E402

EMB = "model.decoder.embed_tokens"
WHAT = "tiny_lm perplexity (tests/golden/tiny_lm, tied, vocab 256)"
WHICH = "tiny_lm perplexity, 3 bits: which table carries the cost"
BOTH = dict(lm_head=True, ganq_embedding=True)
RUNS = [(WHAT, bits, name, kw, None, "ganq_lut") for bits in (4, 3)
        for name, kw in (("body only", {}), ("ganq_embedding", dict(ganq_embedding=True)), ("lm_head untie", dict(lm_head=True)),
                         ("lm_head untie + ganq_embedding", BOTH))]
RUNS += [(WHICH, 3, "3b all (repeat)", BOTH, None, "ganq_lut"),
         (WHICH, 3, "3b all, fake format", BOTH, None, "fake"),
         (WHICH, 3, "3b body+head, embedding 4 bits", BOTH, {EMB: {"bits": 4}}, "ganq_lut"),
         (WHICH, 3, "3b body+embedding, head 4 bits", BOTH, {"lm_head": {"bits": 4}}, "ganq_lut"),
         (WHICH, 3, "3b body+head share", dict(lm_head=True, ganq_tied_embedding="share"), None, "ganq_lut")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    fx = np.load(os.path.join(ROOT, "tests", "golden", "tiny_lm", "fixture.npz"))
    batches = [torch.from_numpy(fx["calib"][i:i + 1].astype(np.int64)).cuda() for i in range(fx["calib"].shape[0])]
    ev = torch.from_numpy(fx["eval_ids"].astype(np.int64))
    for what, bits, name, kw, dyn, fmt in RUNS:
        model = tiny.load_model(torch.float16).cuda()
        qcfg = QuantizeConfig(bits=bits, quant_method="ganq", format=fmt, act_sort="asc", l_damp_style="ganq", dead="mean",
                              desc_act=True, ganq_iterations=10, group_size=128, damp_percent=0.01, dynamic=dyn, **kw)
        proc = quantize_model(model, batches, qcfg)
        ppl = gptq_style_ppl(model, ev, seqlen=int(fx["seq"]))
        rec = {"what": what, "config": name, "bits": bits, "ppl": round(ppl, 4), "head": type(model.get_output_embeddings()).__name__,
               "embedding": type(model.get_input_embeddings()).__name__,
               "log": [r for r in proc.log if r["module"] in (EMB, "lm_head")]}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
