"""EoRA fixtures: the reference's own `eora_process_input` / `eora_compute_lora` (gptqmodel/eora/eora.py) on seeded inputs.
Build container only (the reference tree must be present); runs on the CPU:

    python tests/golden/make_golden_eora.py

Writes tests/golden/eora/<name>.npz (a SUBDIRECTORY: conftest.py parametrises the `golden` fixture over tests/golden/*.npz):
  W          fp16 [m, n]      the weight (generated on the fp16 grid, so the file holds it exactly)
  Wq         fp32 [m, n]      its quantized version (Delta = W - Wq)
  H_triu     fp32 [n(n+1)/2]  the matrix the reference accumulated from the activation batches (raw X^T X / N, no damping), upper
                              triangle row by row -- it is symmetric to the bit, asserted here; tests/eora_fixtures.py unpacks it
  rank       int
  A, B       fp16 [r, n], [m, r]   what eora_compute_lora returned
  E0, E_ref, E_opt  fp64      E(0), E(B A) and the Eckart-Young optimum sum_{i > r} sigma_i^2, with
                              E(M) = tr((Delta - M) H (Delta - M)^T) evaluated in fp64
Cases: heavy-channel activations; iid activations (flat spectrum: the hard case for an iterative method); a wide layer
(m < n) whose Wq is the CPU GANQ of tests/oracle_quantizer.py at 3 bits.  Asserted here, so that the tests cannot pass
vacuously and the reference stays on its main branch: at least 4 n tokens, lambda_min(H) > 0 (neither its negative-eigenvalue
repair nor its 1e-6 I retry runs), (E0 - E_ref) / E0 >= 0.1, and m > rank + 64: the product iterates on a block of rank + 64
vectors, and a case with fewer rows would hand it the exact eigenproblem instead of exercising the iteration.  Shapes are what
keeps every file under the repository's 1 MiB limit for a committed file.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_loader  # noqa: E402

OUT = os.path.join(HERE, "eora")

CASES = [
    dict(name="heavy128x256_r16", m=128, n=256, rank=16, seed=301, batches=8, seq=160, acts="heavy", wq="rtn3"),
    dict(name="iid192x384_r32", m=192, n=384, rank=32, seed=302, batches=8, seq=256, acts="iid", wq="rtn3"),
    dict(name="wide96x512_r16", m=96, n=512, rank=16, seed=303, batches=8, seq=256, acts="heavy", wq="ganq3"),
]


def load_eora():
    ref_loader.load_reference()
    pkg = types.ModuleType("gptqmodel.eora")
    pkg.__path__ = [os.path.join(ref_loader.REF_ROOT, "gptqmodel", "eora")]
    pkg.__package__ = "gptqmodel.eora"
    sys.modules["gptqmodel.eora"] = pkg
    return importlib.import_module("gptqmodel.eora.eora")


def activations(c, gen):
    X = torch.randn((c["batches"], c["seq"], c["n"]), generator=gen)
    if c["acts"] == "heavy":  # a few channels carry most of the energy, a low-rank common component on top
        scale = torch.ones(c["n"])
        scale[torch.randperm(c["n"], generator=gen)[:6]] = torch.tensor([30.0, 20.0, 12.0, 8.0, 6.0, 4.0])
        mix = torch.randn((c["batches"], c["seq"], 4), generator=gen) @ torch.randn((4, c["n"]), generator=gen)
        X = (X + 0.5 * mix) * scale
    return X


def rtn(W, bits):
    """round to nearest on a per-row uniform grid"""
    lo, hi = W.min(dim=1, keepdim=True).values, W.max(dim=1, keepdim=True).values
    step = (hi - lo) / (2 ** bits - 1)
    return (torch.round((W - lo) / step) * step + lo).float()


def ganq_cpu(W, X, bits):
    """Wq by the CPU oracle quantizer of tests/oracle_quantizer.py (desc_act, the default config)"""
    import torch.nn as nn
    from ganq_amd.looper.named_module import NamedModule
    from ganq_amd.quantization.config import QuantizeConfig
    from oracle_quantizer import OracleGANQ

    lin = nn.Linear(W.shape[1], W.shape[0], bias=False)
    lin.weight.data = W.clone()
    g = OracleGANQ(NamedModule(lin, "proj", "layers.0.proj", 0), QuantizeConfig(bits=bits))
    for b in range(X.shape[0]):
        g.add_batch(X[b:b + 1], None)
    return g.quantize()[0].float()


def energy(D, H):
    return float(torch.einsum("ij,jk,ik->", D, H, D))


def run_case(c, eora):
    gen = torch.Generator().manual_seed(c["seed"])
    m, n, r = c["m"], c["n"], c["rank"]
    W = (torch.randn((m, n), generator=gen) * 0.05).half().float()
    X = activations(c, gen)
    assert c["batches"] * c["seq"] >= 4 * n and m > r + 64
    Wq = rtn(W, 3) if c["wq"] == "rtn3" else ganq_cpu(W, X, 3)
    acc = {"m": 0}
    for b in range(c["batches"]):
        eora.eora_process_input(input=(X[b:b + 1],), name="m", eigen_scaling_diag_matrix=acc, sample_size=c["batches"])
    H = acc["m"].float().contiguous()
    assert torch.equal(H, H.T)
    lam_min = float(torch.linalg.eigvalsh(H.double())[0])
    assert lam_min > 0, lam_min
    delta = (W - Wq).float()
    A, B = eora.eora_compute_lora(device=torch.device("cpu"), w_wq_delta=delta.clone(), module=types.SimpleNamespace(name=c["name"]),
                                  eigen_scaling_diag_matrix=H.clone(), rank=r)
    assert A.shape == (r, n) and B.shape == (m, r) and A.dtype == torch.float16
    D, H64 = delta.double(), H.double()
    E0 = energy(D, H64)
    E_ref = energy(D - B.double() @ A.double(), H64)
    lam = torch.linalg.eigvalsh(D @ H64 @ D.T).flip(0)
    E_opt = float(lam[r:].sum())
    assert (E0 - E_ref) / E0 >= 0.1, (E0, E_ref)
    assert E_ref >= E_opt * (1 - 1e-6)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, c["name"] + ".npz")
    iu = np.triu_indices(n)
    np.savez_compressed(path, W=W.half().numpy(), Wq=Wq.numpy(), H_triu=H.numpy()[iu], rank=np.int64(r), A=A.numpy(), B=B.numpy(),
                        E0=np.float64(E0), E_ref=np.float64(E_ref), E_opt=np.float64(E_opt))
    print(f"{c['name']}: lambda_min {lam_min:.3g}  E0 {E0:.6g}  E_ref {E_ref:.6g}  E_opt {E_opt:.6g}  "
          f"reduction {(E0 - E_ref) / E0:.3f}  {os.path.getsize(path)} B")
    assert os.path.getsize(path) <= 1 << 20


if __name__ == "__main__":
    mod = load_eora()
    want = set(sys.argv[1:])
    for case in CASES:
        if not want or case["name"] in want:
            run_case(case, mod)
