"""EoRA: a training-free low-rank correction B A of the quantization error, weighted by the calibration activations
(the reference's gptqmodel/eora/eora.py:43-102), computed on the device from what the quantizer already holds.

With Delta = W - Wq [m, n] and H the (scaled, damped) second-moment matrix of the module's inputs, the reference takes
H = Q L Q^T, S = Q L^1/2, the SVD Delta S = U Sigma V^T and returns B = U_r Sigma_r^1/2, A = Sigma_r^1/2 V_r^T S^-1.  Because
U_r U_r^T Delta S S^-1 = U_r U_r^T Delta,

    B A = U_r U_r^T Delta,     U_r = the r leading eigenvectors of C = Delta H Delta^T,  sigma_i^2 = their eigenvalues,
    B = U_r diag(sigma_i^1/2),  A = diag(sigma_i^-1/2) U_r^T Delta,
    E(B A) := tr((Delta - B A) H (Delta - B A)^T) = tr(C) - sum_{i <= r} u_i^T C u_i          (any orthonormal U_r)

so neither an eigendecomposition of H nor an inverse is needed, and a positive multiple of H gives the same B A.

U_r comes from block subspace iteration with Rayleigh-Ritz on a block of r + OVERSAMPLE vectors: C is never formed,
C Y = (Delta H) (Delta^T Y) is two thin products by the library's fp32 matrix-core GEMM after the one large product
G = Delta H (also the library's).  The block is re-orthonormalised by a tall-skinny QR and the (r + p)-sized Ritz problem solved
in fp64 (torch.linalg on [m, r + p] / [r + p, r + p] matrices); the iteration stops when the sum of the r leading Ritz values
grows by less than RITZ_TOL relative (activations with a few heavy channels: one or two steps; a flat spectrum: more), or
after MAX_STEPS.  No factorisation of an n x n or m x m matrix anywhere.
"""
from typing import Tuple

import torch

from .. import _lib

OVERSAMPLE = 64
MAX_STEPS = 16
RITZ_TOL = 1e-3


def _orthonormal(Y: torch.Tensor) -> torch.Tensor:
    """orthonormal basis of the columns of the tall-skinny Y [m, k] (k <= m): QR in fp64, back in fp32"""
    Q, _ = torch.linalg.qr(Y.double(), mode="reduced")
    return Q.float().contiguous()


@torch.no_grad()
def eora_generate(delta: torch.Tensor, H: torch.Tensor, rank: int, seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor, float, float]:
    """delta [m, n], H [n, n] symmetric positive (semi-)definite, both fp32 on the GPU -> (A [rank, n], B [m, rank]) in fp16 (the
    layer's lora_A / lora_B), e0 = E(0) = tr(Delta H Delta^T) and e = E(B A) from tr(C) and the Ritz values."""
    delta = _lib._dev_f32(delta, "delta")
    H = _lib._dev_f32(H, "H")
    m, n = delta.shape
    if H.shape != (n, n):
        raise _lib.GanqHipError(f"eora_generate: delta {tuple(delta.shape)} and H {tuple(H.shape)} do not fit")
    r = int(rank)
    if not 0 < r <= min(m, n):
        raise ValueError(f"eora_generate: rank {r} must be in [1, min(out_features, in_features) = {min(m, n)}]")
    k = min(m, r + OVERSAMPLE)
    G = _lib.matmul_f32(delta, H)                       # Delta H  [m, n]
    e0 = float((G.double() * delta.double()).sum())     # tr(C)
    delta_t = delta.t().contiguous()                    # [n, m]
    gen = torch.Generator(device=delta.device)
    gen.manual_seed(seed)
    # start in the range of C: one application to a random block
    Y = _lib.matmul_f32(G, _lib.matmul_f32(delta_t, torch.randn((m, k), generator=gen, device=delta.device, dtype=torch.float32)))
    prev = None
    for step in range(MAX_STEPS):
        Q = _orthonormal(Y)
        Y = _lib.matmul_f32(G, _lib.matmul_f32(delta_t, Q))          # C Q  [m, k]
        T = _lib.matmul_f32(Q.t().contiguous(), Y).double()          # Q^T C Q  [k, k]
        theta, S = torch.linalg.eigh((T + T.t()) * 0.5)              # ascending
        theta, S = theta.flip(0)[:r], S.flip(1)[:, :r]
        captured = float(theta.sum())
        if prev is not None and captured - prev <= RITZ_TOL * abs(captured):
            break
        prev = captured
    U = _lib.matmul_f32(Q, S.float().contiguous())                   # [m, r], orthonormal
    ok = theta > 0                                                   # (rank-deficient Delta: those directions carry nothing)
    quarter = torch.where(ok, theta.clamp(min=1e-300) ** 0.25, torch.zeros_like(theta)).float()
    inv_quarter = torch.where(ok, theta.clamp(min=1e-300) ** -0.25, torch.zeros_like(theta)).float()
    B = U * quarter[None, :]
    A = _lib.matmul_f32(U.t().contiguous(), delta) * inv_quarter[:, None]
    e = e0 - float(theta[ok].sum())
    return A.to(torch.float16).contiguous(), B.to(torch.float16).contiguous(), e0, e


__all__ = ["eora_generate", "OVERSAMPLE", "MAX_STEPS", "RITZ_TOL"]
