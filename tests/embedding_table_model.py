"""Pure-numpy model of the row-packed index layout of a LUT embedding table (csrc/lut_table.hip, GanqHipPackedEmbedding), for the
tests with and without a GPU.  A helper module like tests/lut_arena.py, not a conftest.

Row `id` of `qrows` [m, n * bits / 32] is ONE little-endian bit stream: index j of the row occupies bits [j * bits, (j + 1) * bits)
of it, bit k of the stream being bit k % 32 of word k // 32.  The model expands every index into its bits and re-groups them into
words; `column_stream_words` states the same stream once more with Python integers, for the column layout."""
import numpy as np


def pack_rows(Q, bits):
    """Q [m, n] integers in [0, 2^bits) -> uint32 [m, n * bits / 32]"""
    Q = np.asarray(Q)
    m, n = Q.shape
    assert n % 32 == 0 and int(Q.max(initial=0)) < 2 ** bits and int(Q.min(initial=0)) >= 0
    stream = ((Q[:, :, None].astype(np.uint32) >> np.arange(bits, dtype=np.uint32)) & 1).reshape(m, n * bits)
    words = stream.reshape(m, n * bits // 32, 32).astype(np.uint64)
    return (words << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def unpack_rows(qrows, bits):
    """uint32 / int32 [m, words] -> uint8 [m, words * 32 / bits]"""
    w = np.ascontiguousarray(qrows).view(np.uint32)
    m, words = w.shape
    stream = ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(m, words * 32 // bits, bits)
    return (stream << np.arange(bits, dtype=np.uint32)).sum(axis=2).astype(np.uint8)


def column_stream_words(Q, bits):
    """The column layout [n * bits / 32, m] the LUT layers keep (`qweight`), stated with Python integers: the indices of output
    feature o form ONE number, index j in bits [j * bits, (j + 1) * bits), and word k of column o is bits [32 k, 32 k + 32) of it."""
    Q = np.asarray(Q)
    m, n = Q.shape
    words = n * bits // 32
    out = np.zeros((words, m), dtype=np.uint32)
    for o in range(m):
        number = sum(int(q) << (bits * j) for j, q in enumerate(Q[o]))
        for k in range(words):
            out[k, o] = (number >> (32 * k)) & 0xFFFFFFFF
    return out


def nearest_indices(W, T):
    """the assignment ganq_lut_table_assign defines: the FIRST v minimising |W[o][j] - T[o][v]|, subtraction and comparison in fp32"""
    W, T = np.asarray(W, dtype=np.float32), np.asarray(T, dtype=np.float32)
    return np.argmin(np.abs(W[:, :, None] - T[:, None, :]), axis=2).astype(np.uint8)


def squared_error_rows(W, T, Q):
    """fp64 [m]: sum_j (double)d * d of the fp32 differences d = W[o][j] - T[o][Q[o][j]]"""
    W, T = np.asarray(W, dtype=np.float32), np.asarray(T, dtype=np.float32)
    d = (W - np.take_along_axis(T, np.asarray(Q).astype(np.int64), axis=1)).astype(np.float64)
    return (d * d).sum(axis=1)
