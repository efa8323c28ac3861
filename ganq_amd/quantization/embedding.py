"""Quantization of an embedding table on its own (`QuantizeConfig.ganq_embedding`).

A lookup has no activations in front of it, so an embedding row has no Hessian: with H = I the GANQ objective of a row is
sum_j (w_j - T[q_j])^2, and its global optimum is the optimal 1-D k-means of the row's values.  `ganq_kmeans_init` with unit column
weights computes that optimum exactly (the initialisation of the body's codebooks is the whole answer here), and the nearest-code
assignment under the returned codebook is the optimal partition.  Per chunk of rows: one k-means call, one assignment call that
writes the row-packed words directly (csrc/lut_table.hip) -- no alternating iterations, no Cholesky, no calibration data.
"""
from typing import Tuple

import torch

from .. import _lib

# fp32 elements of one chunk of rows: 64 Mi elements = 256 MiB of fp32 beside the table itself (the Llama-3 table of 128256 x 4096
# goes through in 8 chunks).  Nothing else scales with the vocabulary: the k-means workspace depends on the launch grid only.
DEFAULT_MAX_CHUNK_ELEMS = 64 * 1024 * 1024
MAX_EMBEDDING_DIM = 16384  # ganq_kmeans_init sorts a row in LDS


def check_embedding_shape(embedding_dim: int, bits: int) -> None:
    if bits not in (2, 3, 4):
        raise NotImplementedError(f"embedding quantization: bits={bits} not supported (2, 3, 4 are)")
    if embedding_dim % 32 != 0 or embedding_dim > MAX_EMBEDDING_DIM or embedding_dim < 32:
        raise NotImplementedError(f"embedding quantization: embedding_dim={embedding_dim} must be a multiple of 32 and at most "
                                  f"{MAX_EMBEDDING_DIM}")


@torch.no_grad()
def quantize_embedding_rows(W: torch.Tensor, bits: int, max_chunk_elems: int = DEFAULT_MAX_CHUNK_ELEMS
                            ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """W [m, n] (any floating dtype, on the GPU) -> (qrows int32 [m, n*bits/32] in the row-packed layout, T fp32 [m, 2^bits],
    sqerr fp64 [m] = sum_j (w_j - T[q_j])^2 per row).  Rows are independent: the result does not depend on `max_chunk_elems`."""
    if W.dim() != 2:
        raise ValueError(f"quantize_embedding_rows: a [num_embeddings, embedding_dim] table expected, got {tuple(W.shape)}")
    m, n = W.shape
    check_embedding_shape(n, bits)
    if not W.is_cuda:
        raise _lib.GanqHipError(f"quantize_embedding_rows: the table must live on the GPU (got {W.device}); there is no CPU fallback")
    V = 2 ** bits
    rows = max(1, int(max_chunk_elems) // n)
    qrows = torch.empty((m, n * bits // 32), dtype=torch.int32, device=W.device)
    T = torch.empty((m, V), dtype=torch.float32, device=W.device)
    sqerr = torch.empty((m,), dtype=torch.float64, device=W.device)
    for r0 in range(0, m, rows):
        chunk = W[r0:r0 + rows].detach().to(torch.float32).contiguous()
        if not bool(torch.isfinite(chunk).all()):  # (before any kernel sees the chunk; one host synchronisation per chunk)
            raise ValueError("quantize_embedding_rows: the table holds a non-finite weight")
        Tc = _lib.kmeans_init(chunk, None, V)
        qc, ec = _lib.lut_table_assign(chunk, Tc, bits)
        qrows[r0:r0 + rows], T[r0:r0 + rows], sqerr[r0:r0 + rows] = qc, Tc, ec
    return qrows, T, sqerr


__all__ = ["quantize_embedding_rows", "check_embedding_shape", "DEFAULT_MAX_CHUNK_ELEMS", "MAX_EMBEDDING_DIM"]
