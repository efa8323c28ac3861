"""GPU tests of the codebook gradient of the packed embedding lookups (csrc/lut_table_backward.hip):
`ganq_lut_table_bwd_lut` (row-packed table) and `ganq_lut_embedding_bwd_lut` (the packed head's column layout) against an fp64 model
built from the unpacked indices -- exactly where every partial sum is exact, within the bound of an fp32 sum otherwise -- and the
modules that train through them: GanqHipPackedEmbedding.train_codebook, the embedding that shares a packed head (whose lookup term
must arrive in head.lut.grad), `train_codebooks` on the tiny language model."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import embedding_table_model as etm

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ENTRIES = ("rows", "cols")
DTYPES = (torch.float16, torch.bfloat16)
U = 2.0 ** -24  # unit roundoff of fp32
GRID_WAVES = 4 * (1 << 15)  # sorted positions one launch covers without looping (TBW_WAVES * TBW_MAX_GRID)


def make_table(bits, m, n, seed):
    """random indices, the lower half of the codes only in the first half of the rows -> (Q int64 [m, n] cuda, qrows, qweight)"""
    from ganq_amd import _lib

    rng = np.random.default_rng(seed)
    Q = rng.integers(0, 1 << bits, (m, n), dtype=np.int64)
    if m > 1:
        Q[: m // 2] %= 1 << (bits - 1)
    Qd = torch.from_numpy(Q).cuda()
    qrows = torch.from_numpy(etm.pack_rows(Q, bits).view(np.int32)).cuda()
    qweight = _lib.pack_indices(Qd.to(torch.uint8), bits)
    assert torch.equal(qweight.t().contiguous(), qrows)  # one table, packed both ways
    return Qd, qrows, qweight


def call(entry, ids, dy, qrows, qweight, n, bits, padding_idx=None):
    from ganq_amd import _lib

    if entry == "rows":
        return _lib.lut_table_bwd_lut(ids, dy, qrows, bits, padding_idx=padding_idx)
    return _lib.lut_embedding_bwd_lut(ids, dy, qweight, n, bits, padding_idx=padding_idx)


def fp64_bins(ids, dy, Q, V, padding_idx=None):
    """(bins, sum of |contributions|, number of contributions) fp64 [m, V] from the unpacked indices, without atomics: the gradient
    of every table element first (a 0/1 matrix of the ids times dy), then per code the masked row sums"""
    m, n = Q.shape
    ids = ids.reshape(-1)
    keep = (ids >= 0) & (ids < m)
    if padding_idx is not None:
        keep &= ids != padding_idx
    rows = ids[keep]
    x = dy.reshape(-1, n)[keep].double()
    every = torch.arange(m, device=Q.device)[:, None]
    out = []
    for vals in (x, x.abs(), torch.ones_like(x)):
        G = torch.zeros(m, n, dtype=torch.float64, device=Q.device)
        for c in range(0, rows.numel(), 1 << 14):
            G += (rows[None, c:c + (1 << 14)] == every).double() @ vals[c:c + (1 << 14)]
        out.append(torch.stack([(G * (Q == v)).sum(1) for v in range(V)], dim=1))
    return out


def quarters(shape, dtype, g):
    """multiples of 1/4 in [-8, 8]: exact in fp16 and bf16, and every fp32 sum of fewer than 2^19 of them is exact in any order"""
    return (torch.randint(-32, 33, shape, device="cuda", generator=g).float() / 4).to(dtype)


def id_patterns(m, n, g, exact):
    """(name, ids, padding_idx) for one table"""
    r = lambda hi, N: torch.randint(0, hi, (N,), device="cuda", generator=g)  # noqa: E731
    pats = [("one", torch.tensor([m - 1], device="cuda"), None),
            ("distinct", torch.randperm(m, device="cuda", generator=g)[:64], None),
            ("equal130", torch.full((130,), m // 2, device="cuda"), None),
            ("scattered257", r(min(m, 7), 257), None),
            ("empty", torch.zeros((0,), dtype=torch.int64, device="cuda"), None)]
    mixed = r(m, 40)
    mixed[::5] = -1
    mixed[1::7] = m
    mixed[2::9] = 1 << 40
    pats.append(("invalid", mixed.view(4, 10), None))
    pad = r(min(m, 7), 257)
    pats.append(("padding", pad, int(pad[0])))
    if n == 32:
        pats.append(("equal5000", torch.full((5000,), m - 1, device="cuda"), None))  # 5000 * 32 * 32 quarter-units < 2^24
    if exact and n == 32 and m == 300:
        pats.append(("beyond_one_grid", r(m, GRID_WAVES + 5), None))  # the waves loop over the sorted positions
    return pats


def bits_of(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("entry", ENTRIES)
def test_bins_are_exact_on_quarter_multiples(entry, bits, dtype):
    """dy drawn from multiples of 1/4: every partial sum is exact, so dlut equals the fp64 model bit for bit.  n: lanes beyond n
    inactive (32), a 3-bit row that is no multiple of 64 columns (96), exactly one slice (512), a slice plus one group (544), two
    slices plus a group (1056); ids: see id_patterns."""
    V = 1 << bits
    g = torch.Generator(device="cuda").manual_seed(100 * bits + (dtype == torch.bfloat16))
    cases = 0
    for n in (32, 96, 512, 544, 1056):
        for m in (1, 5, 300):
            Q, qrows, qweight = make_table(bits, m, n, seed=n + m)
            for name, ids, pad in id_patterns(m, n, g, exact=True):
                dy = quarters(tuple(ids.shape) + (n,), dtype, g)
                got = call(entry, ids, dy, qrows, qweight, n, bits, pad)
                ref, _, cnt = fp64_bins(ids, dy, Q, V, pad)
                assert got.dtype == torch.float32 and tuple(got.shape) == (m, V)
                assert float(ref.abs().max()) < 2 ** 22  # (2^24 quarter-units: the model itself is exact in fp32)
                assert torch.equal(bits_of(got), bits_of(ref.float())), (name, m, n, float((got.double() - ref).abs().max()))
                assert bool((got[cnt == 0] == 0).all()), (name, m, n)  # unused codes, unselected rows, invalid and padding ids
                if m > 1 and ids.numel():
                    assert bool((cnt[: m // 2, V // 2:] == 0).all())  # (the model: the upper codes of those rows are unused)
                cases += 1
    assert cases == 15 * 7 + 3 + 1


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("entry", ENTRIES)
def test_bins_of_gaussian_gradients_within_the_fp32_sum_bound(entry, bits, dtype):
    """dy = randn: a bin is an fp32 sum of c exactly representable terms (exact conversions of fp16 / bf16, no products) in SOME
    order, so |error| <= gamma_c * sum |terms| with gamma_c = c u / (1 - c u), u = 2^-24 -- derived, not measured.  A second call
    returns the same bits."""
    V = 1 << bits
    g = torch.Generator(device="cuda").manual_seed(7 * bits + (dtype == torch.bfloat16))
    worst = 0.0
    for n, m in ((32, 1), (32, 300), (96, 5), (512, 5), (544, 300), (1056, 300)):
        Q, qrows, qweight = make_table(bits, m, n, seed=n + m)
        for name, ids, pad in id_patterns(m, n, g, exact=False):
            if name in ("one", "distinct", "empty"):
                continue
            dy = torch.randn(tuple(ids.shape) + (n,), device="cuda", generator=g).to(dtype)
            got = call(entry, ids, dy, qrows, qweight, n, bits, pad)
            ref, mag, cnt = fp64_bins(ids, dy, Q, V, pad)
            bound = cnt * U / (1 - cnt * U) * mag
            err = (got.double() - ref).abs()
            assert bool(torch.isfinite(got).all()) and bool((got[cnt == 0] == 0).all()), (name, m, n)
            if not bool((cnt > 0).any()):  # (m = 1 with its only row as padding_idx)
                continue
            ratio = float((err / bound.clamp_min(1e-300))[cnt > 0].max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (name, m, n, ratio)
            assert torch.equal(bits_of(got), bits_of(call(entry, ids, dy, qrows, qweight, n, bits, pad))), "not bitwise repeatable"
    print(f"{entry} bits={bits} {dtype}: worst err / bound = {worst:.3g}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("bits", [2, 3, 4])
def test_both_layouts_return_the_same_bits(bits, dtype):
    """one table packed both ways: the two entries differ only in where a word of a row is fetched, the reduction is shared"""
    g = torch.Generator(device="cuda").manual_seed(bits)
    for m, n in ((5, 96), (300, 544), (300, 1056)):
        Q, qrows, qweight = make_table(bits, m, n, seed=m + n)
        ids = torch.randint(0, m, (3, 171), device="cuda", generator=g)
        dy = torch.randn(3, 171, n, device="cuda", generator=g).to(dtype)
        a = call("rows", ids, dy, qrows, qweight, n, bits, 2)
        b = call("cols", ids, dy, qrows, qweight, n, bits, 2)
        assert torch.equal(bits_of(a), bits_of(b))


def test_order_is_not_trusted_and_strided_gradients_are_taken():
    """entries of `order` outside [0, N) are skipped: with every sorted slot of one id replaced by -1, N and 2^40 the result is the
    gradient without that id's occurrences.  The Python entry makes a stride-0 gradient (y.sum().backward()) contiguous."""
    from ganq_amd import _lib

    bits, m, n, N = 4, 20, 96, 300
    V = 1 << bits
    g = torch.Generator(device="cuda").manual_seed(3)
    Q, qrows, _ = make_table(bits, m, n, seed=1)
    ids = torch.randint(0, m, (N,), device="cuda", generator=g)
    dy = quarters((N, n), torch.float16, g)
    order = torch.sort(ids, stable=True).indices
    drop = 7
    bad = torch.tensor([-1, N, 1 << 40], device="cuda")
    slots = (ids[order] == drop).nonzero().reshape(-1)
    assert slots.numel() > 3
    order[slots] = bad[torch.arange(slots.numel(), device="cuda") % 3]
    dlut = torch.full((m, V), float("nan"), dtype=torch.float32, device="cuda")
    ws = _lib._workspace(_lib.lib().ganq_lut_table_bwd_lut_workspace_bytes(N, m, n, bits), dy.device)
    _lib._call("ganq_lut_table_bwd_lut", (ids, order, dy, qrows, dlut, ws), ids.data_ptr(), order.data_ptr(), N, dy.data_ptr(), 0, qrows.data_ptr(),
               m, n, bits, -1, dlut.data_ptr(), ws.data_ptr(), ws.numel(), _lib._ST)
    ref, _, _ = fp64_bins(ids, dy, Q, V, padding_idx=drop)
    assert torch.equal(bits_of(dlut), bits_of(ref.float()))
    # a workspace one byte short of the queried size is refused before anything is written
    need = _lib.lib().ganq_lut_table_bwd_lut_workspace_bytes(N, m, n, bits)
    assert ws.numel() == need
    dlut.fill_(float("nan"))
    with pytest.raises(_lib.GanqHipError, match="workspace"):
        _lib._call("ganq_lut_table_bwd_lut", (ids, order, dy, qrows, dlut, ws), ids.data_ptr(), order.data_ptr(), N, dy.data_ptr(), 0,
                   qrows.data_ptr(), m, n, bits, -1, dlut.data_ptr(), ws.data_ptr(), need - 1, _lib._ST)
    assert bool(torch.isnan(dlut).all())
    ones = torch.ones((), dtype=torch.float16, device="cuda").expand(N, n)
    got = _lib.lut_table_bwd_lut(ids, ones, qrows, bits)
    assert torch.equal(got.double(), fp64_bins(ids, ones, Q, V)[2])  # a gradient of ones counts the contributions
    with pytest.raises(_lib.GanqHipError):
        _lib.lut_table_bwd_lut(ids, dy.float(), qrows, bits)
    with pytest.raises(_lib.GanqHipError):
        _lib.lut_table_bwd_lut(ids.int(), dy, qrows, bits)
    with pytest.raises(_lib.GanqHipError):
        _lib.lut_table_bwd_lut(ids, dy[:, :64], qrows, bits)
    assert int(torch.count_nonzero(_lib.lut_table_bwd_lut(ids, dy, qrows[:0], bits))) == 0  # an empty table: zeros [0, V]


# ---- the modules
def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def packed_embedding(bits, m, n, dtype, padding_idx=None, seed=0):
    from ganq_amd.nn_modules.qlinear.ganq_hip import GanqHipPackedEmbedding

    Q, qrows, _ = make_table(bits, m, n, seed)
    g = torch.Generator(device="cuda").manual_seed(seed)
    emb = GanqHipPackedEmbedding(m, n, bits, dtype=dtype, padding_idx=padding_idx).cuda()
    emb.qweight_rows = qrows
    emb.lut = torch.sort(0.05 * torch.randn(m, 1 << bits, device="cuda", generator=g), dim=1).values.half()
    return emb, Q


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_packed_embedding_trains_its_codebook(dtype):
    from ganq_amd import _lib

    torch.manual_seed(0)
    bits, m, n, pad = 4, 300, 96, 3
    emb, Q = packed_embedding(bits, m, n, dtype, padding_idx=pad)
    lut16 = emb.lut.clone()
    ids = torch.randint(0, m, (4, 150), device="cuda")
    ids[0, :5] = pad
    assert emb(ids).grad_fn is None  # a buffer codebook: today's call
    emb.train_codebook(True)
    assert isinstance(emb.lut, nn.Parameter) and emb.lut.dtype == torch.float32
    assert "lut" in dict(emb.named_parameters()) and list(emb.state_dict()).count("lut") == 1
    dy = torch.randn(4, 150, n, device="cuda").to(dtype)
    out = emb(ids)
    assert out.grad_fn is not None and out.dtype == dtype
    want = _lib.lut_table_lookup(ids, emb.qweight_rows, emb.lut.detach().to(dtype), bits)
    assert torch.equal(out.detach(), want)  # the inference lookup's value, bit for bit
    with torch.no_grad():
        quiet = emb(ids)
    assert quiet.grad_fn is None and torch.equal(quiet, want)
    assert emb.dequantize_weight().grad_fn is None
    out.backward(dy)
    lut64 = emb.lut.detach().double().requires_grad_(True)
    F.embedding(ids, lut64.gather(1, Q), padding_idx=pad).backward(dy.double())
    assert emb.lut.grad.dtype == torch.float32
    assert rel(emb.lut.grad, lut64.grad) < 1e-5, rel(emb.lut.grad, lut64.grad)
    assert bool((emb.lut.grad[pad] == 0).all()) and float(lut64.grad[pad].abs().max()) == 0.0
    emb.lut.grad = None
    emb(ids).sum().backward()  # a stride-0 gradient
    assert torch.equal(emb.lut.grad.double(), fp64_bins(ids, torch.ones_like(dy), Q, 1 << bits, pad)[2])

    # ten SGD steps towards a target table lower the loss.  Eight rows are looked up; the step is the exact minimiser of the
    # stiffest codebook entry (the MSE over N n elements is quadratic in lut[id][v] with curvature 2 c / (N n), c the number of
    # elements that entry feeds), so every entry contracts.
    ids2 = torch.randint(10, 18, (256,), device="cuda")
    target_lut = lut16.float() + 0.01 * torch.randn_like(lut16.float())
    target = F.embedding(ids2, target_lut.gather(1, Q)).to(dtype)
    count = fp64_bins(ids2, torch.ones(256, n, device="cuda"), Q, 1 << bits)[2]
    opt = torch.optim.SGD([emb.lut], lr=256 * n / (2 * float(count.max())))
    losses = []
    for _ in range(10):
        opt.zero_grad()
        loss = F.mse_loss(emb(ids2).float(), target.float())
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print("embedding codebook training losses", [f"{v:.4g}" for v in losses])
    assert losses[-1] < 0.7 * losses[0]

    emb.train_codebook(False)
    assert not isinstance(emb.lut, nn.Parameter) and emb.lut.dtype == torch.float16 and "lut" in dict(emb.named_buffers())
    assert emb(ids).grad_fn is None


def test_save_quantized_of_a_training_embedding_stores_fp16(tmp_path):
    from ganq_amd.models import load_quantized, save_quantized
    from ganq_amd.quantization.config import QuantizeConfig
    from safetensors.torch import load_file

    emb, _ = packed_embedding(3, 40, 64, torch.float16, padding_idx=1, seed=2)
    model = nn.Sequential(emb).cuda()
    qcfg = QuantizeConfig(bits=3, quant_method="ganq", format="ganq_lut", ganq_embedding=True)
    emb.train_codebook(True)
    with torch.no_grad():
        emb.lut.add_(1e-4)
    save_quantized(model, str(tmp_path), qcfg)
    state = load_file(os.path.join(str(tmp_path), "model.safetensors"))
    assert state["0.lut"].dtype == torch.float16 and torch.equal(state["0.lut"].cuda(), emb.lut.detach().half())
    fresh = load_quantized(nn.Sequential(nn.Embedding(40, 64, padding_idx=1)).half().cuda(), str(tmp_path))
    assert fresh[0].lut.dtype == torch.float16 and not isinstance(fresh[0].lut, nn.Parameter)
    assert torch.equal(fresh[0].lut, emb.lut.detach().half()) and torch.equal(fresh[0].qweight_rows, emb.qweight_rows)
    ids = torch.arange(40, device="cuda")
    assert torch.equal(fresh[0](ids), emb(ids).detach())


@pytest.mark.parametrize("outliers", [False, True], ids=["plain", "outliers"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_tied_codebook_gradient_has_the_lookup_term(dtype, outliers):
    """Head and embedding are one table: with W = lut.gather(1, Q) + W_sparse, loss = (head(f(emb(ids))) * g).sum() reaches lut
    through F.linear AND through F.embedding.  head.lut.grad must be the sum of both terms (fp64 reference, the bars of
    test_layer_autograd_against_dequantised_linear for fp16 / bf16 activations), and the head-only term must NOT pass."""
    from ganq_amd.nn_modules.qlinear.ganq_hip import GanqHipQuantEmbedding, GanqHipQuantLinear

    torch.manual_seed(5)
    m, n, bits, N = 300, 64, 4, 600
    tol = 2e-3 if dtype == torch.float16 else 2e-2
    Q, _, _ = make_table(bits, m, n, seed=9)
    lut = torch.sort(0.05 * torch.randn(m, 1 << bits, device="cuda"), dim=1).values
    lut = lut.to(dtype).float()  # (representable in the table dtype: the rounding inside the forward is the identity)
    kw, nnz = {}, 0
    if outliers:
        mask = torch.rand(m, n, device="cuda") < 0.01
        rowptr = torch.zeros(m + 1, dtype=torch.int32, device="cuda")
        rowptr[1:] = torch.cumsum(mask.sum(1), 0).to(torch.int32)
        cols = mask.nonzero()[:, 1].to(torch.int32)
        vals = (0.3 * torch.randn(cols.numel(), device="cuda")).to(dtype).half()  # (exact in fp16 and in `dtype`)
        nnz = cols.numel()
        kw = dict(ganq_outliers=(rowptr, cols, vals))
    head = GanqHipQuantLinear(bits=bits, group_size=-1, sym=True, desc_act=False, in_features=n, out_features=m, outliers=nnz).cuda()
    head.pack(nn.Linear(n, m, bias=False).cuda(), ganq_indices=Q.to(torch.uint8), ganq_codebook=lut.half().float(), **kw)
    emb = GanqHipQuantEmbedding(head, dtype=dtype)
    head.train_codebook(True)
    with torch.no_grad():
        head.lut.copy_(lut)
    f = nn.Linear(n, n).cuda().to(dtype).requires_grad_(False)
    ids = torch.randint(0, m, (2, N // 2), device="cuda")
    g = torch.randn(2, N // 2, m, device="cuda").to(dtype)

    e = emb(ids)
    assert e.grad_fn is not None
    with torch.no_grad():
        assert torch.equal(e.detach(), emb(ids)) and emb(ids).grad_fn is None
    (head(f(e)) * g).sum().backward()
    got = head.lut.grad
    assert got.dtype == torch.float32 and bool(torch.isfinite(got).all())

    Ws = head._sparse_dense(torch.float64) if outliers else 0.0
    refs = {}
    for which in ("both", "head_only"):
        lut64 = lut.double().requires_grad_(True)
        W = lut64.gather(1, Q) + Ws
        e64 = F.embedding(ids, W)
        if which == "head_only":
            e64 = e64.detach()
        (F.linear(F.linear(e64, f.weight.double(), f.bias.double()), W) * g.double()).sum().backward()
        refs[which] = lut64.grad
    err, missing = rel(got, refs["both"]), rel(got, refs["head_only"])
    print(f"tied gradient {dtype} outliers={outliers}: rel. error {err:.3e} (bar {tol}); against the head-only term {missing:.3e}")
    assert err < tol, err
    assert missing > tol and rel(refs["head_only"], refs["both"]) > tol  # the test cannot pass with the lookup term missing


def test_train_codebooks_on_the_tiny_model():
    """the committed tiny OPT with packed body, head and embedding: one LM-loss backward gives every codebook a finite, non-zero
    gradient; train_codebooks(model, False) restores the buffers"""
    sys.path.insert(0, GOLDEN_DIR)
    import make_golden_tiny_lm as tiny
    from ganq_amd.models import quantize_model, train_codebooks
    from ganq_amd.nn_modules.qlinear.ganq_hip import GanqHipPackedEmbedding, GanqHipQuantLinear
    from ganq_amd.quantization.config import QuantizeConfig

    fx = np.load(os.path.join(GOLDEN_DIR, "tiny_lm", "fixture.npz"))
    model = tiny.load_model(torch.float16).cuda().eval()
    qcfg = QuantizeConfig(bits=4, quant_method="ganq", format="ganq_lut", act_sort="asc", l_damp_style="ganq", dead="mean",
                          ganq_iterations=2, ganq_embedding=True, lm_head=True)
    batches = [torch.from_numpy(fx["calib"][i:i + 1].astype(np.int64)).cuda() for i in range(fx["calib"].shape[0])]
    with torch.no_grad():
        quantize_model(model, batches, qcfg)
    packed = {name: mod for name, mod in model.named_modules() if isinstance(mod, (GanqHipQuantLinear, GanqHipPackedEmbedding))}
    assert len(packed) == 26 and sum(isinstance(mod, GanqHipPackedEmbedding) for mod in packed.values()) == 1
    assert isinstance(model.get_output_embeddings(), GanqHipQuantLinear)
    params = train_codebooks(model)
    assert len(params) == 26 and all(isinstance(p, nn.Parameter) and p.dtype == torch.float32 for p in params)
    assert {id(p) for p in params} == {id(mod.lut) for mod in packed.values()}
    seq = int(fx["seq"])
    ids = torch.from_numpy(fx["eval_ids"].astype(np.int64).reshape(-1)[: 2 * seq].reshape(2, seq)).cuda()
    logits = model(ids).logits.float()
    loss = F.cross_entropy(logits[:, :-1].reshape(-1, logits.shape[-1]), ids[:, 1:].reshape(-1))
    (loss * 1024.0).backward()  # (fp16 activations: a static loss scale, as the LoRA test of tests/test_hip_lut_backward.py)
    for name, mod in packed.items():
        grad = mod.lut.grad
        assert grad is not None and grad.dtype == torch.float32, name
        assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0, name
    assert train_codebooks(model, False) == []
    for name, mod in packed.items():
        assert not isinstance(mod.lut, nn.Parameter) and mod.lut.dtype == torch.float16 and "lut" in dict(mod.named_buffers()), name
    assert not any(n.endswith(".lut") for n, _ in model.named_parameters())
