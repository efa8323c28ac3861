"""TEST INFRASTRUCTURE: loader of the EoRA fixtures under tests/golden/eora/ (written by tests/golden/make_golden_eora.py)."""
import glob
import os

import numpy as np

from conftest import GOLDEN_DIR

EORA_FIXTURES = sorted(glob.glob(os.path.join(GOLDEN_DIR, "eora", "*.npz")))
EORA_IDS = [os.path.basename(p)[:-4] for p in EORA_FIXTURES]


def load_eora(path):
    """dict with W, Wq, H (fp32, H rebuilt from its stored upper triangle), rank, A, B (fp16), E0, E_ref, E_opt"""
    z = np.load(path)
    n = z["W"].shape[1]
    H = np.zeros((n, n), dtype=np.float32)
    iu = np.triu_indices(n)
    H[iu] = z["H_triu"]
    H = H + np.triu(H, 1).T
    return dict(W=z["W"].astype(np.float32), Wq=z["Wq"], H=H, rank=int(z["rank"]), A=z["A"], B=z["B"], E0=float(z["E0"]),
                E_ref=float(z["E_ref"]), E_opt=float(z["E_opt"]))
