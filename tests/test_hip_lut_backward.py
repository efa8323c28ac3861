"""The LUT backward on the MI355X (csrc/lut_backward.hip) against fp64, and GanqHipQuantLinear trained through autograd:
  dx = dy @ dequant(qweight, lut) on both paths (direct kernel M <= 64, transposed dequant + dense GEMM above), with outliers;
  dlut = the bins of dy^T x by the codes, bounded by (M + n) 2^-24 times each bin's sum of |contributions|;
  the layer against a dequantised nn.Linear; codebook training; a LoRA fine-tune of the tiny OPT model, whose LoRA gradients must
  match those of the same model with nn.Linear(weight=dequantize_weight()) in place of every quantized layer."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def make(bits, m, n, dtype, seed=0):
    from ganq_amd import _lib

    g = torch.Generator(device="cuda").manual_seed(seed)
    V = 1 << bits
    Q = torch.randint(0, V, (m, n), device="cuda", generator=g, dtype=torch.int64).to(torch.uint8)
    lut = torch.sort(0.05 * torch.randn(m, V, device="cuda", generator=g), dim=1).values.to(dtype)
    return Q, lut, _lib.pack_indices(Q, bits)


def check_dx(dx, ref, dtype):  # the forward's tolerance (tests/test_hip_lut_gemm.py check())
    eps = 2 ** -10 if dtype == torch.float16 else 2 ** -7
    assert torch.isfinite(dx).all()
    err = float((dx.double() - ref).abs().max())
    assert torch.allclose(dx.double(), ref, rtol=eps, atol=eps * float(ref.abs().max()) * 0.05 + 1e-6), err


MS = [1, 5, 16, 33, 64, 65, 300, 1024, 2048]
OUTS = [1, 64, 129, 1000, 4096]
INS = [32, 320, 1024, 4096]
GRID = [(bits, dtype, M, OUTS[(i + k) % 5], INS[(i + 2 * k) % 4])
        for k, (bits, dtype) in enumerate([(b, d) for b in (2, 3, 4) for d in (torch.float16, torch.bfloat16)])
        for i, M in enumerate(MS)]
GRID += [(3, torch.float16, 333, 129, 1024), (4, torch.bfloat16, 65, 1000, 320), (2, torch.float16, 1024, 129, 4096),
         (4, torch.float16, 2048, 14336, 4096), (4, torch.bfloat16, 2048, 4096, 14336),
         (2, torch.float16, 512, 4096, 4096), (2, torch.bfloat16, 2048, 4096, 4096),  # 256-row GEMM tiles for every bit width
         (3, torch.bfloat16, 64, 14336, 4096), (4, torch.float16, 16, 4096, 14336), (2, torch.float16, 1, 4096, 4096)]


@pytest.mark.parametrize("bits,dtype,M,m,n", GRID)
def test_dx_against_fp64(bits, dtype, M, m, n):
    from ganq_amd import _lib

    Q, lut, qw = make(bits, m, n, dtype, seed=M + m + n)
    dy = torch.randn(M, m, device="cuda").to(dtype)
    dx = _lib.lut_linear_bwd_input(dy, qw, lut, bits)
    ref = dy.double() @ lut.double().gather(1, Q.long())
    check_dx(dx, ref, dtype)
    assert torch.equal(dx, _lib.lut_linear_bwd_input(dy, qw, lut, bits)), "not bitwise repeatable"


@pytest.mark.parametrize("bits,dtype,M,m,n", GRID)
def test_dlut_against_fp64(bits, dtype, M, m, n):
    from ganq_amd import _lib

    Q, lut, qw = make(bits, m, n, dtype, seed=M + 2 * m + n)
    if m > 1:  # leave some codes unused in some rows
        Q[: m // 2] = Q[: m // 2] % (1 << (bits - 1))
        qw = _lib.pack_indices(Q, bits)
    dy = torch.randn(M, m, device="cuda").to(dtype)
    x = torch.randn(M, n, device="cuda").to(dtype)
    dlut = _lib.lut_linear_bwd_lut(dy, x, qw, bits, m)
    V = 1 << bits
    G = dy.double().T @ x.double()
    ref = torch.zeros(m, V, dtype=torch.float64, device="cuda").scatter_add_(1, Q.long(), G)
    mag = torch.zeros_like(ref).scatter_add_(1, Q.long(), dy.double().abs().T @ x.double().abs())
    used = torch.zeros_like(ref).scatter_add_(1, Q.long(), torch.ones_like(G)) > 0
    err = (dlut.double() - ref).abs()
    bound = (M + n) * 2.0 ** -24 * mag
    ratio = float((err / bound.clamp_min(1e-300))[used].max())
    print(f"dlut bits={bits} {dtype} M={M} m={m} n={n}: max err / bound = {ratio:.3g}")
    assert dlut.dtype == torch.float32 and torch.isfinite(dlut).all()
    assert ratio <= 1.0
    assert (dlut[~used] == 0).all(), "codes no index uses must be exactly 0"
    assert torch.equal(dlut, _lib.lut_linear_bwd_lut(dy, x, qw, bits, m)), "not bitwise repeatable"


def test_python_row_chunks(monkeypatch):
    """activations above the per-call size go in row chunks: dx chunks are independent (bitwise the unchunked result), dlut
    chunk sums are added in chunk order"""
    from ganq_amd import _lib

    bits, m, n, M = 4, 320, 512, 1000
    Q, lut, qw = make(bits, m, n, torch.float16, seed=3)
    dy = torch.randn(M, m, device="cuda").half()
    x = torch.randn(M, n, device="cuda").half()
    dx1 = _lib.lut_linear_bwd_input(dy, qw, lut, bits)
    lut1 = _lib.lut_linear_bwd_lut(dy, x, qw, bits, m)
    monkeypatch.setattr(_lib, "_BWD_CHUNK_BYTES", 2 * n * 513)  # 256-row chunks
    step = _lib._bwd_max_rows(n)
    assert step == 256
    assert torch.equal(_lib.lut_linear_bwd_input(dy, qw, lut, bits), dx1)
    got = _lib.lut_linear_bwd_lut(dy, x, qw, bits, m)
    want = None
    for r in range(0, M, step):
        part = _lib.lut_linear_bwd_lut(dy[r:r + step], x[r:r + step], qw, bits, m)
        want = part if want is None else want + part
    assert torch.equal(got, want)
    assert rel(got, lut1) < 1e-5


def _fp64_bins(dy, x, Q, V, step=1 << 22):
    ref = torch.zeros(Q.shape[0], V, dtype=torch.float64, device="cuda")
    for r in range(0, dy.shape[0], step):
        ref.scatter_add_(1, Q.long(), dy[r:r + step].double().T @ x[r:r + step].double())
    return ref


def test_library_chunks_beyond_32bit_offsets(monkeypatch):
    """More tokens than one GEMM launch addresses (4 GiB of the wider operand): ganq_lut_linear_bwd_lut takes them in chunks whose
    bins it adds in chunk order, the dense dx path in independent row blocks -- bitwise the same as separate calls on the pieces."""
    from ganq_amd import _lib

    monkeypatch.setattr(_lib, "_BWD_CHUNK_BYTES", 1 << 40)  # no chunking in Python: the library's own loops
    bits, m, n = 2, 64, 32
    Q, lut, qw = make(bits, m, n, torch.float16, seed=11)
    cap = ((1 << 32) - 1) // (2 * max(m, n)) // 64 * 64  # tokens per launch of the codebook gradient
    M = cap + 1000
    g = torch.Generator(device="cuda").manual_seed(5)
    dy = torch.randn(M, m, device="cuda", generator=g, dtype=torch.float16)
    x = torch.randn(M, n, device="cuda", generator=g, dtype=torch.float16)
    got = _lib.lut_linear_bwd_lut(dy, x, qw, bits, m)
    want = _lib.lut_linear_bwd_lut(dy[:cap], x[:cap], qw, bits, m) + _lib.lut_linear_bwd_lut(dy[cap:], x[cap:], qw, bits, m)
    assert torch.equal(got, want)
    ref = _fp64_bins(dy, x, Q, 1 << bits)
    mag = _fp64_bins(dy.abs(), x.abs(), Q, 1 << bits)
    assert float(((got.double() - ref).abs() / mag).max()) <= (M + n) * 2.0 ** -24
    del x, got, want
    rows = ((1 << 32) - 1) // (2 * 64)  # rows of dy per dense GEMM launch at ceil64(m) = 64
    assert M > rows
    dx = _lib.lut_linear_bwd_input(dy, qw, lut, bits)
    assert torch.equal(dx[:rows], _lib.lut_linear_bwd_input(dy[:rows], qw, lut, bits))
    assert torch.equal(dx[rows:], _lib.lut_linear_bwd_input(dy[rows:], qw, lut, bits))
    sel = torch.cat([torch.arange(0, 4096, device="cuda"), torch.arange(rows - 2048, M, device="cuda")])
    check_dx(dx[sel], dy[sel].double() @ lut.double().gather(1, Q.long()), torch.float16)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M", [7, 64, 300])
def test_dx_with_outliers(dtype, M):
    from ganq_amd.nn_modules.qlinear.ganq_hip import GanqHipQuantLinear

    m, n, bits = 384, 640, 4
    Q, lut, _ = make(bits, m, n, torch.float16, seed=M)
    g = torch.Generator(device="cuda").manual_seed(7)
    mask = torch.rand(m, n, device="cuda", generator=g) < 0.01
    rowptr = torch.zeros(m + 1, dtype=torch.int32, device="cuda")
    rowptr[1:] = torch.cumsum(mask.sum(1), 0).to(torch.int32)
    nz = mask.nonzero()
    cols = nz[:, 1].to(torch.int32)
    vals = (0.3 * torch.randn(cols.numel(), device="cuda", generator=g)).half()
    layer = GanqHipQuantLinear(bits=bits, group_size=-1, sym=True, desc_act=False, in_features=n, out_features=m,
                               outliers=cols.numel()).cuda()
    lin = nn.Linear(n, m, bias=False).cuda()
    layer.pack(lin, ganq_indices=Q, ganq_codebook=lut.float(), ganq_outliers=(rowptr, cols, vals))
    x = torch.randn(M, n, device="cuda").to(dtype).requires_grad_(True)
    dy = torch.randn(M, m, device="cuda").to(dtype)
    layer(x).backward(dy)
    Wd = lut.to(dtype).double().gather(1, Q.long()) + layer._sparse_dense(dtype).double()  # Wq + W_sparse, values as the layer uses them
    check_dx(x.grad, dy.double() @ Wd, dtype)


def _layer(bits, m, n, dtype, bias=True, seed=0):
    from ganq_amd.nn_modules.qlinear.ganq_hip import GanqHipQuantLinear

    Q, lut, _ = make(bits, m, n, torch.float16, seed=seed)
    layer = GanqHipQuantLinear(bits=bits, group_size=-1, sym=True, desc_act=False, in_features=n, out_features=m, bias=bias).cuda()
    lin = nn.Linear(n, m, bias=bias).cuda()
    layer.pack(lin, ganq_indices=Q, ganq_codebook=lut.float())
    ref = nn.Linear(n, m, bias=bias).cuda().to(dtype)
    with torch.no_grad():
        ref.weight.copy_(layer.dequantize_weight().to(dtype))
        if bias:
            ref.bias.copy_(layer.bias.to(dtype))
    return layer, ref, Q


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("rows", [3, 200])
def test_layer_autograd_against_dequantised_linear(dtype, rows):
    torch.manual_seed(rows)
    m, n = 512, 768
    layer, ref, _ = _layer(4, m, n, dtype)
    tol = 2e-3 if dtype == torch.float16 else 2e-2
    pre = nn.Linear(n, n).cuda().to(dtype)
    pre_ref = copy.deepcopy(pre)
    x = torch.randn(2, rows, n, device="cuda").to(dtype)
    # y.sum().backward(): a stride-0 gradient; then a random non-contiguous one
    for grad in (None, torch.randn(m, 2, rows, device="cuda").to(dtype).permute(1, 2, 0)):
        outs = []
        for lay, p in ((layer, pre), (ref, pre_ref)):
            p.zero_grad(set_to_none=True)
            xi = x.clone().requires_grad_(True)
            y = lay(p(xi))
            (y.sum() if grad is None else (y * grad).sum()).backward()
            outs.append((xi.grad, p.weight.grad, p.bias.grad, y.detach()))
        for a, b in zip(outs[0], outs[1]):
            assert a.dtype == b.dtype and a.shape == b.shape
            assert rel(a, b) < tol, rel(a, b)
    # the forward is the inference path's, bit for bit, and under no_grad it builds no graph
    xi = x.clone().requires_grad_(True)
    y_grad = layer(xi)
    with torch.no_grad():
        y_ng = layer(x)
    assert y_grad.grad_fn is not None and y_ng.grad_fn is None
    assert torch.equal(y_grad.detach(), y_ng)


def test_codebook_training():
    torch.manual_seed(0)
    bits, m, n, M = 4, 256, 512, 96
    layer, _, Q = _layer(bits, m, n, torch.float16, bias=False)
    lut16 = layer.lut.clone()
    layer.train_codebook(True)
    assert isinstance(layer.lut, nn.Parameter) and layer.lut.dtype == torch.float32
    assert "lut" in dict(layer.named_parameters()) and list(layer.state_dict()).count("lut") == 1
    x = torch.randn(M, n, device="cuda").half()
    dy = torch.randn(M, m, device="cuda").half()
    layer(x).backward(dy)
    lut64 = layer.lut.detach().double().requires_grad_(True)
    F.linear(x.double(), lut64.gather(1, Q.long())).backward(dy.double())
    assert layer.lut.grad.dtype == torch.float32
    assert rel(layer.lut.grad, lut64.grad) < 1e-5, rel(layer.lut.grad, lut64.grad)

    # ten SGD steps towards a regression target lower the loss
    target_lut = lut16.float() + 0.01 * torch.randn_like(lut16.float())
    with torch.no_grad():
        target = F.linear(x.float(), target_lut.gather(1, Q.long())).half()
    opt = torch.optim.SGD([layer.lut], lr=1.0)
    losses = []
    for _ in range(10):
        opt.zero_grad()
        loss = F.mse_loss(layer(x).float(), target.float())
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print("codebook training losses", [f"{v:.4g}" for v in losses])
    assert losses[-1] < 0.7 * losses[0]

    # back to an fp16 buffer under the same key; the saved file holds fp16 either way
    layer.train_codebook(False)
    assert not isinstance(layer.lut, nn.Parameter) and layer.lut.dtype == torch.float16 and "lut" in dict(layer.named_buffers())


def test_save_quantized_writes_fp16_codebook(tmp_path):
    from ganq_amd.models.quantize import load_quantized, save_quantized
    from ganq_amd.quantization.config import QuantizeConfig
    from safetensors.torch import load_file

    torch.manual_seed(1)
    layer, _, _ = _layer(4, 128, 256, torch.float16, bias=False)
    model = nn.Sequential(layer).cuda()
    qcfg = QuantizeConfig(bits=4, quant_method="ganq", format="ganq_lut")
    layer.train_codebook(True)
    with torch.no_grad():
        layer.lut.add_(1e-4)
    save_quantized(model, str(tmp_path), qcfg)
    state = load_file(os.path.join(str(tmp_path), "model.safetensors"))
    assert state["0.lut"].dtype == torch.float16
    assert torch.equal(state["0.lut"].cuda(), layer.lut.detach().half())
    layer.train_codebook(False)
    save_quantized(model, str(tmp_path), qcfg)
    fresh = load_quantized(nn.Sequential(nn.Linear(256, 128)).cuda(), str(tmp_path))
    assert fresh[0].lut.dtype == torch.float16 and torch.equal(fresh[0].lut, layer.lut)


class _LoRA(nn.Module):
    """a hand-written rank-4 LoRA branch around a frozen base layer"""

    def __init__(self, base, seed, r=4):
        super().__init__()
        self.base = base
        g = torch.Generator().manual_seed(seed)
        dt = torch.float16
        self.A = nn.Parameter((torch.randn(r, base.in_features, generator=g) / base.in_features ** 0.5).to(dt).cuda())
        self.B = nn.Parameter((0.5 * torch.randn(base.out_features, r, generator=g) / r ** 0.5).to(dt).cuda())

    def forward(self, x):
        return self.base(x) + F.linear(F.linear(x, self.A), self.B)


LORA_BOUND = 2e-2  # relative Frobenius error of a LoRA gradient, fp16 model


def test_tiny_lm_lora_gradients_match_dequantised_model():
    """The LoRA fine-tune of a GANQ-quantized tiny OPT: every LoRA parameter's gradient equals (to fp16 rounding) that of the
    same model with nn.Linear(weight=dequantize_weight()) in place of each quantized layer.  Without the layer's backward, every
    gradient path through a quantized base weight was dropped: the LoRA gradients below the top layer came out wrong (with the forward
    building no graph, 46 of the 48 gradients exceed the bound, the worst by 55 times: relative error 1.1)."""
    errs = lora_grad_errors()
    worst = max(errs, key=errs.get)
    print(f"LoRA gradients: max relative Frobenius error {errs[worst]:.3e} ({worst}); bound {LORA_BOUND}")
    for n, e in errs.items():
        assert e < LORA_BOUND, (n, e)


def lora_grad_errors():
    """{LoRA parameter: relative Frobenius error of its gradient against the dequantised model's}"""
    sys.path.insert(0, GOLDEN_DIR)
    import make_golden_tiny_lm as tiny
    from ganq_amd.models.quantize import quantize_model
    from ganq_amd.nn_modules.qlinear.ganq_hip import GanqHipQuantLinear
    from ganq_amd.quantization.config import QuantizeConfig

    fx = np.load(os.path.join(GOLDEN_DIR, "tiny_lm", "fixture.npz"))
    model = tiny.load_model(torch.float16).cuda()
    qcfg = QuantizeConfig(bits=4, quant_method="ganq", format="ganq_lut", act_sort="asc", l_damp_style="ganq", dead="mean",
                          desc_act=True, ganq_iterations=10, group_size=128, damp_percent=0.01)
    batches = [torch.from_numpy(fx["calib"][i:i + 1].astype(np.int64)).cuda() for i in range(fx["calib"].shape[0])]
    quantize_model(model, batches, qcfg)
    names = [n for n, mod in model.named_modules() if isinstance(mod, GanqHipQuantLinear)]
    assert len(names) == 24

    ref = copy.deepcopy(model)
    for tag, net in (("ganq", model), ("ref", ref)):
        mods = dict(net.named_modules())
        for i, name in enumerate(names):
            q = mods[name]
            base = q
            if tag == "ref":
                base = nn.Linear(q.in_features, q.out_features, bias=q.bias is not None).cuda().half()
                with torch.no_grad():
                    base.weight.copy_(q.dequantize_weight().half())
                    if q.bias is not None:
                        base.bias.copy_(q.bias.half())
            parent, _, child = name.rpartition(".")
            setattr(mods[parent], child, _LoRA(base, seed=i))
        for p_name, p in net.named_parameters():
            p.requires_grad_(p_name.endswith(".A") or p_name.endswith(".B"))
        net.eval()

    seq = int(fx["seq"])  # (the model's position table ends there)
    ids = torch.from_numpy(fx["eval_ids"].astype(np.int64).reshape(-1)[: 2 * seq].reshape(2, seq)).cuda()
    grads = {}
    for tag, net in (("ganq", model), ("ref", ref)):
        logits = net(ids).logits.float()
        loss = F.cross_entropy(logits[:, :-1].reshape(-1, logits.shape[-1]), ids[:, 1:].reshape(-1))
        (loss * 1024.0).backward()  # (fp16 gradients: a static loss scale keeps the small ones out of the subnormals)
        grads[tag] = {n: p.grad.detach().float() / 1024.0 for n, p in net.named_parameters() if p.requires_grad}
    assert grads["ganq"].keys() == grads["ref"].keys() and len(grads["ref"]) == 48
    return {n: rel(grads["ganq"][n], grads["ref"][n]) for n in grads["ref"]}
