"""GPU tests of the row-packed LUT table (csrc/lut_table.hip): `ganq_lut_table_assign` (nearest-code assignment written straight
into the packed rows, with the per-row squared error) and `ganq_lut_table_lookup` (rows gathered by id).  Both are called through
`_lib`; every reference is numpy on the CPU (tests/embedding_table_model.py).  Indices and looked-up rows are compared bit for bit;
the squared error may differ from the fp64 numpy sum only by the order of its fp64 additions."""
import numpy as np
import pytest
import torch

import embedding_table_model as etm
import lut_arena

pytestmark = pytest.mark.gpu

ASSIGN_N = (32, 96, 512, 544, 2080)
ASSIGN_M = (1, 5, 67)
KINDS = ("gauss", "midway", "repeats", "zeros")
LOOKUP_N = (32, 480, 512, 544, 1056)
LOOKUP_M = (1, 300)
LOOKUP_COUNTS = (0, 1, 3, 2053)
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


def make_assign_inputs(kind, rng, m, n, V):
    """(W fp32 [m,n], T fp32 [m,V])"""
    f = np.float32
    if kind == "gauss":
        return (0.02 * rng.standard_normal((m, n))).astype(f), np.sort((0.02 * rng.standard_normal((m, V))).astype(f), axis=1)
    if kind == "midway":  # codes two apart, integer weights: every odd distance lies exactly midway between two codes
        T = (2.0 * np.arange(V)[None, :] + rng.integers(-5, 6, (m, 1))).astype(f)
        W = (T[:, :1] + rng.integers(-3, 2 * V + 2, (m, n))).astype(f)
        W[:, 0] = T[:, 0] + 1.0  # at least one tie per row, between codes 0 and 1
        return W, T
    if kind == "repeats":  # every value of the codebook twice or more; weights on the values and between them
        vals = np.sort((0.02 * rng.standard_normal((m, max(1, V // 4)))).astype(f), axis=1)
        T = np.sort(np.repeat(vals, V // vals.shape[1], axis=1), axis=1)
        W = (0.02 * rng.standard_normal((m, n))).astype(f)
        hit = rng.random((m, n)) < 0.25
        W[hit] = T[np.nonzero(hit)[0], rng.integers(0, V, int(hit.sum()))]
        return W, T
    W = (0.02 * rng.standard_normal((m, n))).astype(f)  # "zeros": a row of zeros, under a codebook with and without a zero
    W[0] = 0.0
    T = np.sort((0.02 * rng.standard_normal((m, V))).astype(f), axis=1)
    if m > 1:
        W[m - 1] = 0.0
        T[m - 1, V // 2] = 0.0
    return W, T


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("bits", [2, 3, 4])
def test_assign_writes_the_first_nearest_code_into_packed_rows(bits, kind):
    from ganq_amd import _lib as hip

    V = 2 ** bits
    for m in ASSIGN_M:
        for n in ASSIGN_N:
            rng = np.random.default_rng([bits, KINDS.index(kind), m, n])
            W, T = make_assign_inputs(kind, rng, m, n, V)
            Q = etm.nearest_indices(W, T)
            tag = (bits, kind, m, n)
            if kind == "midway":  # the lower index wins a tie
                d = (W - T[:, :1]).astype(np.int64)  # code v sits at distance 2 v
                tie = (d % 2 == 1) & (d >= 1) & (d <= 2 * V - 3)
                assert int(tie.sum()) >= m and np.array_equal(Q[tie], (d[tie] - 1) // 2), tag
            if kind == "repeats":  # the first of equal entries wins
                prev = np.take_along_axis(T, np.maximum(Q.astype(np.int64) - 1, 0), 1)
                assert np.all((Q == 0) | (prev != np.take_along_axis(T, Q.astype(np.int64), 1))), tag
            Wd, Td = torch.from_numpy(W).cuda(), torch.from_numpy(T).cuda()
            qrows, sqerr = hip.lut_table_assign(Wd, Td, bits)
            assert qrows.dtype == torch.int32 and tuple(qrows.shape) == (m, n * bits // 32), tag
            got = qrows.cpu().numpy().view(np.uint32)
            want = etm.pack_rows(Q, bits)
            if not np.array_equal(got, want):
                Qg = etm.unpack_rows(got, bits)
                o, j = (int(v[0]) for v in np.nonzero(Qg != Q))
                raise AssertionError(f"{tag}: {int((Qg != Q).sum())} indices differ; first Q[{o}][{j}] = {Qg[o, j]}, expected {Q[o, j]} "
                                     f"(w = {W[o, j]!r}, codebook {T[o]!r})")
            assert torch.equal(qrows, hip.pack_indices(torch.from_numpy(Q).cuda(), bits).t()), tag
            ref = etm.squared_error_rows(W, T, Q)
            err = np.abs(sqerr.cpu().numpy() - ref)
            assert np.all(err <= n * 2.0 ** -52 * ref), (tag, float((err / np.maximum(ref, 1e-300)).max()))
            if kind == "zeros" and m > 1:
                assert float(sqerr[m - 1]) == 0.0  # the row of zeros under a codebook that holds a zero
            q2, e2 = hip.lut_table_assign(Wd, Td, bits)  # the same bytes on a second call
            assert torch.equal(q2, qrows) and torch.equal(e2.view(torch.int64), sqerr.view(torch.int64)), tag
            q3, e3 = hip.lut_table_assign(Wd, Td, bits, want_sqerr=False)  # sqerr_rows = NULL
            assert e3 is None and torch.equal(q3, qrows)


def make_ids(rng, N, m, padding_idx):
    """duplicates, the padding id, both ends and the out-of-range values -1, m and 2^40 among random valid ids"""
    ids = rng.integers(0, m, N, dtype=np.int64)
    if N == 1:
        ids[0] = m - 1
    elif N == 3:
        ids[:] = [m - 1, 1 << 40, -1]
    elif N > 3:
        special = [0, m - 1, m - 1, padding_idx, padding_idx, -1, m, 1 << 40, -(1 << 40), 0]
        ids[rng.permutation(N)[:len(special)]] = special
        ids[N - 1] = m  # the last row of out is a row of zeros: what overruns it is seen in the guard
    return ids


def expected_rows(lut_bits, Q, ids):
    """uint16 [N, n]: lut[id][Q[id]] as bit patterns, zeros for an id outside [0, m)"""
    m = Q.shape[0]
    ok = (ids >= 0) & (ids < m)
    safe = np.where(ok, ids, 0)
    rows = np.take_along_axis(lut_bits[safe], Q[safe].astype(np.int64), axis=1)
    rows[~ok] = 0
    return rows


def lookup_in_arena(hip, ids, qrows, lut, n, bits):
    """one C ABI call in guarded buffers -> out [N, n] as int16 bit patterns (a clone); asserts the buffer contract"""
    dt = lut.dtype
    m, V = lut.shape
    N = ids.numel()
    specs = [("ids", torch.int64, (N,), ids, False), ("out", torch.int16, (N, n), None, False),
             ("qrows", torch.int32, tuple(qrows.shape), qrows, False), ("lut", dt, (m, V), lut, True)]
    arena = lut_arena.Arena(specs)
    t = arena.t
    t["out"].fill_(lut_arena.Y_PREFILL)
    arena.snapshot(("out",))
    p = {k: v.data_ptr() for k, v in t.items()}
    hip._call("ganq_lut_table_lookup", tuple(t.values()), p["ids"], N, p["qrows"], p["lut"], 0 if dt == torch.float16 else 1, m, n, bits,
              p["out"], hip._ST)
    torch.cuda.synchronize()
    arena.assert_untouched("ganq_lut_table_lookup")  # nothing outside the N * n elements of out is written, the inputs are intact
    kept = int((t["out"] == lut_arena.Y_PREFILL).sum())
    assert kept == 0, f"{kept} of {N * n} elements of out were never written"
    return t["out"].clone()


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("bits", [2, 3, 4])
def test_lookup_is_a_bit_exact_gather(bits, dtype):
    from ganq_amd import _lib as hip

    dt = DTYPES[dtype]
    V = 2 ** bits
    for m in LOOKUP_M:
        for n in LOOKUP_N:
            rng = np.random.default_rng([bits, 5 if dtype == "bf16" else 0, m, n])
            Q = rng.integers(0, V, (m, n), dtype=np.uint8)
            Q[m - 1, :] = np.arange(n) % V  # a known pattern in the last row
            lut = torch.from_numpy((0.02 * rng.standard_normal((m, V))).astype(np.float32)).to(dt)
            lut_bits = lut.view(torch.int16).numpy().view(np.uint16)
            qrows = torch.from_numpy(etm.pack_rows(Q, bits).view(np.int32))
            padding_idx = min(1, m - 1)
            for N in LOOKUP_COUNTS:
                ids = make_ids(rng, N, m, padding_idx)
                out = lookup_in_arena(hip, torch.from_numpy(ids), qrows, lut, n, bits).cpu().numpy().view(np.uint16)
                want = expected_rows(lut_bits, Q, ids)
                assert out.shape == want.shape
                if not np.array_equal(out, want):
                    i, j = (int(v[0]) for v in np.nonzero(out != want))
                    raise AssertionError(f"bits={bits} {dtype} m={m} n={n} N={N}: {int((out != want).sum())} of {out.size} elements "
                                         f"differ; first out[{i}][{j}] = {out[i, j]:#06x}, expected {want[i, j]:#06x} (id {ids[i]})")
                bad = (ids < 0) | (ids >= m)
                assert not out[bad].any()  # rows of (positive) zeros
            # the public binding on ids of another shape gives the same rows
            ids = torch.from_numpy(make_ids(rng, 64, m, padding_idx)).cuda()
            got = hip.lut_table_lookup(ids.view(4, 16), qrows.cuda(), lut.cuda(), bits)
            assert got.dtype == dt and tuple(got.shape) == (4, 16, n)
            assert np.array_equal(got.view(torch.int16).cpu().numpy().view(np.uint16).reshape(64, n), expected_rows(lut_bits, Q, ids.cpu().numpy()))


def test_lookup_replays_in_a_captured_graph_with_new_ids():
    """no workspace, no host synchronisation, no allocation: the call is captured, and a replay reads the ids as they are THEN"""
    from ganq_amd import _lib as hip

    bits, m, n, N = 3, 300, 544, 65
    rng = np.random.default_rng(7)
    Q = rng.integers(0, 8, (m, n), dtype=np.uint8)
    lut = torch.from_numpy((0.02 * rng.standard_normal((m, 8))).astype(np.float32)).half()
    lut_bits = lut.view(torch.int16).numpy().view(np.uint16)
    qrows, lut_d = torch.from_numpy(etm.pack_rows(Q, bits).view(np.int32)).cuda(), lut.cuda()
    ids = torch.from_numpy(make_ids(rng, N, m, 1)).cuda()
    out = torch.empty((N, n), dtype=torch.float16, device="cuda")
    hip.lut_table_lookup(ids, qrows, lut_d, bits, out=out)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            hip.lut_table_lookup(ids, qrows, lut_d, bits, out=out)
    torch.cuda.synchronize()
    for seed in (11, 12):
        new = make_ids(np.random.default_rng(seed), N, m, 1)
        ids.copy_(torch.from_numpy(new))
        out.view(torch.int16).fill_(lut_arena.Y_PREFILL)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.view(torch.int16).cpu().numpy().view(np.uint16), expected_rows(lut_bits, Q, new))


def test_bad_arguments_come_back_as_errors_through_the_c_abi():
    from ganq_amd import _lib as hip

    ids = torch.zeros(3, dtype=torch.int64, device="cuda")
    qrows = torch.zeros((8, 8), dtype=torch.int32, device="cuda")
    lut = torch.zeros((8, 16), dtype=torch.float16, device="cuda")
    out = torch.zeros(3 * 64 + 8, dtype=torch.float16, device="cuda")
    W = torch.zeros((8, 64), dtype=torch.float32, device="cuda")
    T = torch.zeros((8, 16), dtype=torch.float32, device="cuda")
    sq = torch.zeros(8, dtype=torch.float64, device="cuda")
    ts = (ids, qrows, lut, out)

    def lookup(n=64, bits=4, out_ptr=None, N=3, m=8, ids_ptr=ids.data_ptr()):
        hip._call("ganq_lut_table_lookup", ts, ids_ptr, N, qrows.data_ptr(), lut.data_ptr(), 0, m, n, bits,
                  out.data_ptr() if out_ptr is None else out_ptr, hip._ST)

    def assign(n=64, bits=4, w_ptr=W.data_ptr(), m=8):
        hip._call("ganq_lut_table_assign", (W, T, qrows, sq), w_ptr, T.data_ptr(), m, n, bits, qrows.data_ptr(), sq.data_ptr(), hip._ST)

    lookup()
    assign()
    for kw in (dict(n=48), dict(bits=5), dict(out_ptr=out.data_ptr() + 2), dict(ids_ptr=None), dict(n=-32), dict(m=1 << 31)):
        with pytest.raises(hip.GanqHipError):
            lookup(**kw)
    for kw in (dict(n=48), dict(bits=5), dict(bits=8), dict(w_ptr=None), dict(m=-1)):
        with pytest.raises(hip.GanqHipError):
            assign(**kw)
    lookup(N=0)  # no-ops
    lookup(m=0)
    assign(m=0)
    torch.cuda.synchronize()
    # the wrappers refuse what does not fit before the library is called
    with pytest.raises(hip.GanqHipError):
        hip.lut_table_lookup(ids.int(), qrows, lut, 4)
    with pytest.raises(hip.GanqHipError):
        hip.lut_table_lookup(ids, qrows, lut.float(), 4)
    with pytest.raises(hip.GanqHipError):
        hip.lut_table_lookup(ids, qrows, lut, 3)
    with pytest.raises(hip.GanqHipError):
        hip.lut_table_lookup(ids, qrows.cpu(), lut, 4)  # a host pointer must not reach the kernel
    with pytest.raises(hip.GanqHipError):
        hip.lut_table_assign(W, T[:, :8], 4)
    # an empty table: every id is out of range, also into a buffer of the caller's
    buf = torch.full((3, 64), 7.0, dtype=torch.float16, device="cuda")
    got = hip.lut_table_lookup(ids, qrows[:0], lut[:0], 4, out=buf)
    assert got.data_ptr() == buf.data_ptr() and int(torch.count_nonzero(buf)) == 0
    assert int(torch.count_nonzero(hip.lut_table_lookup(ids, qrows[:0], lut[:0], 4))) == 0
    assert hip.lut_table_lookup(ids[:0], qrows, lut, 4).shape == (0, 64)
