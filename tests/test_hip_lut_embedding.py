"""GPU tests of ganq_lut_embedding (csrc/lut_embedding.hip): rows of the dequantised LUT weight gathered by id out of the packed
stream.  The kernel runs through the C ABI inside a guarded arena (tests/lut_arena.py) with `out` pre-filled with a NaN pattern; the
expected result is F.embedding on the weight the existing `lut_dequant` produces (+ the dense outlier part, added in that dtype).
It is a gather: the comparison is bitwise, there is no tolerance."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lut_arena

pytestmark = pytest.mark.gpu

SHAPES = [(1, 32), (17, 96), (323, 160), (1028, 544), (8200, 2080)]
COUNTS = (1, 63, 64, 65, 1000)
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


def make_ids(rng, N, m):
    """ids with 0, m - 1, repeats, -1 and m (and two far out of range) among random valid ones; N = 1: the last row"""
    ids = rng.integers(0, m, N, dtype=np.int64)
    special = [0, m - 1, m - 1, -1, m, 1 << 40, -(1 << 40), 0]
    if N == 1:
        ids[0] = m - 1
    else:
        pos = rng.permutation(N)[:len(special)]
        ids[pos] = special[:len(pos)]
    return ids


def make_csr(rng, m, n):
    """CSR by vocabulary row: every third row has 1, 2 or 3 entries, the last row 70 (more than one 64-entry chunk of the kernel's
    loop) where the width allows; all other rows have none.  Columns distinct and ascending, the last column among them."""
    counts = np.zeros(m, dtype=np.int64)
    counts[::3] = 1 + (np.arange(0, m, 3) // 3) % 3
    counts[m - 1] = 70
    counts = np.minimum(counts, n)
    rowptr = np.zeros(m + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum(counts)
    cols = np.empty(int(rowptr[-1]), dtype=np.int32)
    for o in np.nonzero(counts)[0]:
        c = np.sort(rng.choice(n, size=int(counts[o]), replace=False))
        if o % 2 == 0:
            c[-1] = n - 1
            c = np.unique(c)
            while c.size < counts[o]:  # (the replaced column was already there)
                c = np.unique(np.append(c, rng.integers(0, n)))
        cols[rowptr[o]:rowptr[o + 1]] = c
    vals = (0.1 * rng.standard_normal(cols.size)).astype(np.float32)
    return rowptr, cols, vals


def dense_weight(hip, qw, lut, n, bits, csr):
    """the parent's dequantised weight: lut_dequant (+ W_sparse, one add in the dtype), as GanqHipQuantLinear.dequantize_weight"""
    W = hip.lut_dequant(qw, lut, n, bits)
    if csr is None:
        return W
    rowptr, cols, vals = csr
    m = lut.shape[0]
    Ws = torch.zeros((m, n), dtype=W.dtype, device=W.device)
    rows = torch.repeat_interleave(torch.arange(m, device=W.device), (rowptr[1:] - rowptr[:-1]).long())
    Ws[rows, cols.long()] = vals
    return W + Ws


def expected(W, ids):
    m = W.shape[0]
    ok = (ids >= 0) & (ids < m)
    out = F.embedding(torch.where(ok, ids, torch.zeros_like(ids)), W)
    return torch.where(ok.unsqueeze(-1), out, torch.zeros_like(out))


def run_in_arena(hip, ids, qw, lut, n, bits, csr):
    """one C ABI call in guarded buffers -> out [N, n] (a clone); asserts the buffer contract"""
    dt = lut.dtype
    m, V = lut.shape
    N = ids.numel()
    specs = [("ids", torch.int64, (N,), ids, False), ("out", torch.int16, (N, n), None, False),
             ("qweight", torch.int32, tuple(qw.shape), qw, False), ("lut", dt, (m, V), lut, True)]
    if csr is not None:
        rowptr, cols, vals = csr
        specs += [("rowptr", torch.int32, (m + 1,), rowptr, False), ("cols", torch.int32, (cols.numel(),), cols, False),
                  ("vals", dt, (vals.numel(),), vals, True)]
    arena = lut_arena.Arena(specs)
    t = arena.t
    t["out"].fill_(lut_arena.Y_PREFILL)
    arena.snapshot(("out",))
    p = {k: v.data_ptr() for k, v in t.items()}
    hip._call("ganq_lut_embedding", tuple(t.values()), p["ids"], N, p["qweight"], p["lut"], 0 if dt == torch.float16 else 1, m, n, bits,
              p.get("rowptr"), p.get("cols"), p.get("vals"), p["out"], hip._ST)
    torch.cuda.synchronize()
    arena.assert_untouched("ganq_lut_embedding")
    kept = int((t["out"] == lut_arena.Y_PREFILL).sum())
    assert kept == 0, f"{kept} of {N * n} elements of out were never written"
    return t["out"].view(dt).clone()


@pytest.mark.parametrize("outliers", [False, True], ids=["plain", "outliers"])
@pytest.mark.parametrize("m,n", SHAPES)
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("bits", [2, 3, 4])
def test_lut_embedding_is_a_bit_exact_gather(bits, dtype, m, n, outliers):
    from ganq_amd import _lib as hip

    dt = DTYPES[dtype]
    rng = np.random.default_rng(1000 * bits + 10 * m + n + (1 if outliers else 0) + (5 if dtype == "bf16" else 0))
    V = 2 ** bits
    Q = torch.from_numpy(rng.integers(0, V, (m, n), dtype=np.uint8)).cuda()
    lut = torch.from_numpy((0.02 * rng.standard_normal((m, V))).astype(np.float32)).to(dt).cuda()
    qw = hip.pack_indices(Q, bits)
    csr = None
    if outliers:
        rowptr, cols, vals = make_csr(rng, m, n)
        csr = (torch.from_numpy(rowptr).cuda(), torch.from_numpy(cols).cuda(), torch.from_numpy(vals).to(dt).cuda())
    W = dense_weight(hip, qw, lut, n, bits, csr)  # the reference: computed once, shared by every N
    assert torch.equal(hip.lut_dequant(qw, lut, n, bits), torch.gather(lut, 1, Q.long()))  # (the reference itself is the plain gather)
    for N in COUNTS:
        ids = torch.from_numpy(make_ids(rng, N, m)).cuda()
        out = run_in_arena(hip, ids, qw, lut, n, bits, csr)
        want = expected(W, ids)
        assert out.shape == want.shape
        same = out.view(torch.int16) == want.view(torch.int16)
        if not bool(same.all()):
            bad = torch.nonzero(~same)
            i, j = (int(v) for v in bad[0])
            raise AssertionError(f"N={N}: {bad.shape[0]} of {out.numel()} elements differ; first out[{i}][{j}] = {float(out[i, j])}, "
                                 f"expected {float(want[i, j])} (id {int(ids[i])})")
        out_of_range = (ids < 0) | (ids >= m)
        assert int(torch.count_nonzero(out[out_of_range].view(torch.int16))) == 0  # rows of (positive) zeros
        # the public binding on ids of another shape gives the same rows
        if N == 64:
            assert torch.equal(hip.lut_embedding(ids.view(4, 16), qw, lut, n, bits, outliers=csr).view(torch.int16).reshape(N, n),
                               want.view(torch.int16))


@pytest.mark.parametrize("outliers", [False, True], ids=["plain", "outliers"])
def test_lut_embedding_replays_in_a_captured_graph_with_new_ids(outliers):
    """no workspace, no host synchronisation, no allocation: the call is captured, and a replay reads the ids as they are THEN"""
    from ganq_amd import _lib as hip

    bits, m, n, N = 4, 1028, 544, 65
    rng = np.random.default_rng(7)
    Q = torch.from_numpy(rng.integers(0, 16, (m, n), dtype=np.uint8)).cuda()
    lut = torch.from_numpy((0.02 * rng.standard_normal((m, 16))).astype(np.float32)).half().cuda()
    qw = hip.pack_indices(Q, bits)
    csr = None
    if outliers:
        rowptr, cols, vals = make_csr(rng, m, n)
        csr = (torch.from_numpy(rowptr).cuda(), torch.from_numpy(cols).cuda(), torch.from_numpy(vals).half().cuda())
    W = dense_weight(hip, qw, lut, n, bits, csr)
    ids = torch.from_numpy(make_ids(rng, N, m)).cuda()
    out = torch.empty((N, n), dtype=torch.float16, device="cuda")
    hip.lut_embedding(ids, qw, lut, n, bits, outliers=csr, out=out)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            hip.lut_embedding(ids, qw, lut, n, bits, outliers=csr, out=out)
    torch.cuda.synchronize()
    for seed in (11, 12):
        ids.copy_(torch.from_numpy(make_ids(np.random.default_rng(seed), N, m)))
        out.view(torch.int16).fill_(lut_arena.Y_PREFILL)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), expected(W, ids).view(torch.int16))


def test_lut_embedding_rejects_bad_arguments():
    from ganq_amd import _lib as hip

    Q = torch.zeros((8, 64), dtype=torch.uint8, device="cuda")
    qw = hip.pack_indices(Q, 4)
    lut = torch.zeros((8, 16), dtype=torch.float16, device="cuda")
    ids = torch.zeros(3, dtype=torch.int64, device="cuda")
    with pytest.raises(hip.GanqHipError):
        hip.lut_embedding(ids.int(), qw, lut, 64, 4)
    with pytest.raises(hip.GanqHipError):
        hip.lut_embedding(ids, qw, lut.float(), 64, 4)
    with pytest.raises(hip.GanqHipError):
        hip.lut_embedding(ids, qw, lut, 96, 4)  # qweight does not fit
    assert hip.lut_embedding(ids[:0], qw, lut, 64, 4).shape == (0, 64)
