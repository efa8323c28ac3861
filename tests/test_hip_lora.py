"""LUT forward with a low-rank adapter (`_lib.lut_linear_lora`, GanqHipQuantLinear(adapter=Lora(...))) on the GPU.

Reference, in fp64 and independent of the code under test: y = x Wq^T + t lora_B^T + bias (+ addend) with t = the fp64 product
x lora_A^T ROUNDED to the activation dtype -- the implementation rounds t once (it is the matrix-core operand of the second
product) and y once.  Bound: the project's own for the LUT kernels (tests/test_hip_lut_gemm.py check(): rtol = atol scale =
2^-10 fp16 / 2^-7 bf16) plus one derived term for the rounding of t.  The implementation rounds an fp32-ACCUMULATED t, and an
element whose exact value lies within the accumulation error of a rounding tie may land on the other side: one step of the
activation dtype away from the reference's t, which moves output o of that row by step(t_j) |lora_B[o][j]|.  (Measured at
2048 x 14336 x 4096, r = 32, fp16: 131 of 65536 elements of t differ by one step; with check()'s bound alone 1 of 29 M outputs
is 4e-5 past it.)  How many: the accumulation error of n products is about sqrt(n) 2^-24 relative (random walk), ties are
2^-mant relative apart (mant = 10 fp16, 7 bf16), so an element flips with probability p <= sqrt(n) 2^(mant - 23) and a row of r
elements has a Poisson number of flips of mean mu = r p.  The bound grants every output F = max(1, ceil(mu + 3 sqrt(mu)))
flips (mean plus three standard deviations), each as large as the LARGEST single one possible for that output,
max_j step(t[row][j]) |lora_B[o][j]|, with step() taken from the reference's own t.  For r = 32, n = 4096, fp16: F = 2 and the
term is about 2e-4 against outputs of RMS 1.3.  The factors are scaled so
that the adapter term is a visible share of y (RMS ratio in [0.1, 1], asserted): a wrong adapter cannot hide in the tolerance."""
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

RANKS = [16, 32, 64, 256]
MS = [1, 5, 16, 33, 64, 65, 300, 1024, 2048]
OUTS = [1, 64, 129, 1000, 4096]      # the lists of tests/test_hip_lut_backward.py
INS = [32, 320, 1024, 4096]
GRID = [(bits, dtype, M, OUTS[(i + k) % 5], INS[(i + 2 * k) % 4], RANKS[(i + k) % 4], (i + k) % 2 == 0)
        for k, (bits, dtype) in enumerate([(b, d) for b in (2, 3, 4) for d in (torch.float16, torch.bfloat16)])
        for i, M in enumerate(MS)]
# every regime at the shapes the README quotes: the 16- and 32-feature decode variants, the split decode variant (few feature
# blocks, long rows), the fused GEMM with and without a split of in_features, the dense path at M = 2048
GRID += [(4, torch.float16, M, m, n, r, True) for (m, n, r) in ((4096, 4096, 64), (14336, 4096, 32), (4096, 14336, 128))
         for M in (1, 2048)]
GRID += [(3, torch.bfloat16, 16, 2048, 8192, 64, False), (2, torch.float16, 64, 14336, 4096, 256, True),
         (4, torch.bfloat16, 512, 4096, 4096, 16, False), (3, torch.float16, 4096, 1000, 1024, 48, True),
         (4, torch.float16, 300, 512, 1056, 32, True)]  # (in_features = 32 mod 64)
# the dense regime (M >= 1024, enough 128 x 256 tiles for every CU, in_features >= 8192): the adapter's second product as the fp32
# addend of the dense path -- and the same row counts below that width, where the fused kernel keeps the adapter
GRID += [(3, torch.bfloat16, 2048, 4096, 8192, 64, True), (2, torch.float16, 1024, 8192, 8192, 16, False),
         (4, torch.bfloat16, 1100, 8200, 8192, 48, True), (3, torch.bfloat16, 2048, 4096, 4096, 64, True)]


@pytest.fixture(scope="module")
def hip():
    from ganq_amd import _lib

    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.selftest()
    return _lib


def make(bits, M, m, n, r, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    V = 2 ** bits
    Q = torch.randint(0, V, (m, n), device="cuda", generator=g, dtype=torch.int32).to(torch.uint8)
    lut = (0.02 * torch.randn(m, V, device="cuda", generator=g)).to(dtype)
    x = torch.randn(M, n, device="cuda", generator=g).to(dtype)
    bias = (0.1 * torch.randn(m, device="cuda", generator=g)).to(dtype)
    # base term: RMS 0.02 sqrt(n).  t = x A^T has RMS 1 with A ~ 1 / sqrt(n); the adapter term then has RMS b sqrt(r): a third of
    # the base term with b = 0.02 sqrt(n) / (3 sqrt(r))
    A = (torch.randn(r, n, device="cuda", generator=g) / n ** 0.5).to(dtype)
    B = (torch.randn(m, r, device="cuda", generator=g) * (0.02 * n ** 0.5 / (3 * r ** 0.5))).to(dtype)
    return Q, lut, x, bias, A, B


def flip_slack(t, B, n, dtype):
    """[M, m] fp32: what F rounding-tie flips of t can move each output by (module docstring)"""
    mant = 10 if dtype == torch.float16 else 7
    r = t.shape[1]
    mu = r * math.sqrt(n) * 2.0 ** (mant - 23)
    F = max(1, math.ceil(mu + 3 * math.sqrt(mu)))
    _, e = torch.frexp(t.float().abs())               # |t| = f 2^e, f in [0.5, 1): one step of the dtype is 2^(e - 1 - mant)
    step = torch.ldexp(torch.ones_like(t, dtype=torch.float32), e - 1 - mant)
    Babs = B.float().abs()
    worst = torch.zeros((t.shape[0], B.shape[0]), dtype=torch.float32, device=t.device)
    for j in range(r):
        worst = torch.maximum(worst, step[:, j:j + 1] * Babs[:, j][None, :])
    return F * worst


def reference(x, Q, lut, bias, A, B, dtype, addend=None):
    Wq = torch.gather(lut.double(), 1, Q.long())
    base = x.double() @ Wq.T
    t = (x.double() @ A.double().T).to(dtype)  # the fp64 product, rounded once to the activation dtype
    ad = t.double() @ B.double().T
    ref = base + ad
    if addend is not None:
        ref = ref + addend.double()
    if bias is not None:
        ref = ref + bias.double()
    return ref, base, ad, flip_slack(t, B, x.shape[1], dtype)


def within(y, ref, dtype, slack=None):
    eps = 2 ** -10 if dtype == torch.float16 else 2 ** -7
    tol = eps * ref.abs() + (eps * float(ref.abs().max()) * 0.05 + 1e-6)
    if slack is not None:
        tol = tol + slack.double()
    return (y.double() - ref).abs() <= tol


def check(y, ref, dtype, slack=None):
    assert torch.isfinite(y).all()
    ok = within(y, ref, dtype, slack)
    assert bool(ok.all()), (int((~ok).sum()), float((y.double() - ref).abs().max()))


def visible(base, ad):
    ratio = float(ad.pow(2).mean().sqrt() / base.pow(2).mean().sqrt().clamp_min(1e-30))
    assert 0.1 <= ratio <= 1.0, ratio


@pytest.mark.parametrize("bits,dtype,M,m,n,r,with_bias", GRID)
def test_lora_forward_against_fp64(hip, bits, dtype, M, m, n, r, with_bias):
    Q, lut, x, bias, A, B = make(bits, M, m, n, r, dtype, seed=bits * 1000 + M + m + n + r)
    if not with_bias:
        bias = None
    qw = hip.pack_indices(Q, bits)
    y = hip.lut_linear_lora(x, qw, lut, bias, bits, A, B)
    ref, base, ad, slack = reference(x, Q, lut, bias, A, B, dtype)
    if M * m >= 64:  # (an RMS over a handful of outputs says nothing)
        visible(base, ad)
    check(y, ref, dtype, slack)
    assert torch.equal(y, hip.lut_linear_lora(x, qw, lut, bias, bits, A, B)), "not bitwise repeatable"
    # without the adapter term the result must NOT pass: the test can see a missing adapter
    if M * m >= 64:
        plain = hip.lut_linear(x, qw, lut, bias, bits)
        assert float(within(plain, ref, dtype, slack).double().mean()) < 0.5


@pytest.mark.parametrize("M", [1, 16, 33, 64, 65, 300, 2048, 8192])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_lora_forward_with_addend(hip, M, dtype):
    bits, m, n, r = 4, 1000, 1024, 32
    Q, lut, x, bias, A, B = make(bits, M, m, n, r, dtype, seed=M)
    qw = hip.pack_indices(Q, bits)
    add = 0.3 * torch.randn(M, m, device="cuda")
    y = hip.lut_linear_lora(x, qw, lut, bias, bits, A, B, addend=add)
    ref, _, _, slack = reference(x, Q, lut, bias, A, B, dtype, addend=add)
    check(y, ref, dtype, slack)
    assert torch.equal(y, hip.lut_linear_lora(x, qw, lut, bias, bits, A, B, addend=add))


def test_lora_workspace_is_left_clean_across_shapes(hip):
    """the ticket counters of the t kernel and of the split decode kernel are shared by every shape that follows: alternate
    shapes whose workspaces overlap differently and compare with the first results"""
    cases = [(4, 1, 4096, 4096, 64), (4, 16, 2048, 8192, 256), (3, 64, 129, 1024, 16), (4, 300, 512, 2048, 128), (2, 5, 14336, 4096, 32)]
    data = [make(b, M, m, n, r, torch.float16, seed=i) for i, (b, M, m, n, r) in enumerate(cases)]
    first = []
    for (b, M, m, n, r), (Q, lut, x, bias, A, B) in zip(cases, data):
        first.append(hip.lut_linear_lora(x, hip.pack_indices(Q, b), lut, bias, b, A, B))
    for _ in range(2):
        for i in reversed(range(len(cases))):
            b = cases[i][0]
            Q, lut, x, bias, A, B = data[i]
            assert torch.equal(first[i], hip.lut_linear_lora(x, hip.pack_indices(Q, b), lut, bias, b, A, B)), cases[i]
            assert torch.equal(hip.lut_linear(x, hip.pack_indices(Q, b), lut, bias, b), hip.lut_linear(x, hip.pack_indices(Q, b), lut, bias, b))


def test_lora_argument_checks(hip):
    Q, lut, x, bias, A, B = make(4, 4, 64, 128, 16, torch.float16, seed=1)
    qw = hip.pack_indices(Q, 4)
    with pytest.raises(hip.GanqHipError):
        hip.lut_linear_lora(x, qw, lut, bias, 4, A[:8], B[:, :8])  # rank 8
    with pytest.raises(hip.GanqHipError):
        hip.lut_linear_lora(x, qw, lut, bias, 4, A, B[:32])        # lora_B rows != out_features
    with pytest.raises(hip.GanqHipError):
        hip.lut_linear_lora(x, qw, lut, bias, 4, A.bfloat16(), B)  # dtype mix
    with pytest.raises(hip.GanqHipError):
        hip.lut_linear_lora(x, qw, lut, bias, 4, A, B, addend=torch.zeros(4, 64, device="cuda", dtype=torch.float16))


def _layer(bits, m, n, r, bias=True, outlier_every=0, seed=0):
    from ganq_amd.adapter import Lora
    from ganq_amd.nn_modules.qlinear.ganq_hip import GanqHipQuantLinear

    Q, lut, _, _, A, B = make(bits, 1, m, n, max(r, 16), torch.float16, seed)
    nnz, outl = 0, None
    if outlier_every:
        rows = torch.arange(0, m, outlier_every, device="cuda")
        cnt = torch.zeros(m, dtype=torch.int32, device="cuda")
        cnt[rows] = 2
        rowptr = torch.zeros(m + 1, dtype=torch.int32, device="cuda")
        rowptr[1:] = torch.cumsum(cnt, 0)
        cols = torch.stack([(rows * 7) % n, (rows * 7) % n + 1], dim=1).clamp(max=n - 1).reshape(-1).to(torch.int32)
        vals = torch.full((cols.numel(),), 0.25, dtype=torch.float32, device="cuda")
        nnz, outl = int(cols.numel()), (rowptr, cols, vals)
    layer = GanqHipQuantLinear(bits=bits, group_size=-1, sym=True, desc_act=False, in_features=n, out_features=m, bias=bias,
                               adapter=Lora(rank=r) if r else None, outliers=nnz).cuda()
    lin = nn.Linear(n, m, bias=bias).cuda()
    layer.pack(lin, ganq_indices=Q, ganq_codebook=lut.float(), ganq_outliers=outl, ganq_lora=(A, B) if r else None)
    return layer, Q, lut


@pytest.mark.parametrize("M", [1, 16, 64, 65, 512])
def test_layer_without_adapter_is_bit_identical_to_plain_call(hip, M):
    layer, Q, lut = _layer(4, 512, 768, 0)
    x = torch.randn(M, 768, device="cuda").half()
    assert layer.adapter_rank == 0 and not hasattr(layer, "lora_A")
    assert torch.equal(layer(x), hip.lut_linear(x, layer.qweight, layer.lut, layer.bias, 4))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("outlier_every", [0, 5])
@pytest.mark.parametrize("M", [1, 16, 40, 64, 65, 300, 1500])
def test_layer_forward_equals_linear_on_merged_weight(hip, M, outlier_every, dtype):
    bits, m, n, r = 3, 512, 1024, 32
    layer, Q, lut = _layer(bits, m, n, r, outlier_every=outlier_every, seed=M)
    x = torch.randn(2, M, n, device="cuda").to(dtype)
    with torch.no_grad():
        y = layer(x)
    assert y.shape == (2, M, m) and y.dtype == dtype and y.grad_fn is None
    W = layer.merged_weight()
    assert W.shape == (m, n) and W.dtype == layer.lut.dtype
    y_lib = F.linear(x.float(), W.float(), layer.bias.float()).detach()
    # fp16: the second bound of test_lut_gemm_baseline_shapes_vs_f_linear; bf16 carries three mantissa bits fewer
    assert float((y.float() - y_lib).abs().max()) <= (2 ** -8 if dtype == torch.float16 else 2 ** -5) * float(y_lib.abs().max())
    # the adapter is a visible share of it, and the fp64 bound of the kernel holds for the layer too (outliers as the addend)
    sparse = None
    if outlier_every:
        sparse = x.reshape(-1, n).double() @ layer._sparse_dense(torch.float64).T
    ref, base, ad, slack = reference(x.reshape(-1, n), Q, layer.lut.to(dtype), layer.bias.to(dtype), layer.lora_A.to(dtype),
                                     layer.lora_B.to(dtype), dtype, addend=sparse)
    visible(base, ad)
    check(y.reshape(-1, m), ref, dtype, slack)
    with torch.no_grad():
        assert torch.equal(y, layer(x))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("rows", [3, 200])
def test_layer_adapter_gradients_against_fp32_torch_lora(dtype, rows):
    """x, lora_A and lora_B gradients after train_adapter(True) against the same model from nn.Linear + torch LoRA in fp32;
    tolerances of tests/test_hip_lut_backward.py's layer test"""
    torch.manual_seed(rows)
    bits, m, n, r = 4, 512, 768, 32
    layer, Q, lut = _layer(bits, m, n, r)
    layer.train_adapter(True)
    assert isinstance(layer.lora_A, nn.Parameter) and layer.lora_A.dtype == torch.float32
    tol = 2e-3 if dtype == torch.float16 else 2e-2
    W = layer.dequantize_weight().float()
    A_ref = layer.lora_A.detach().clone().requires_grad_(True)
    B_ref = layer.lora_B.detach().clone().requires_grad_(True)
    x = torch.randn(2, rows, n, device="cuda").to(dtype)
    dy = torch.randn(2, rows, m, device="cuda").to(dtype)

    def rel(a, b):
        return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))

    xi = x.clone().requires_grad_(True)
    y = layer(xi)
    assert y.grad_fn is not None and y.dtype == dtype
    y.backward(dy)
    xr = x.float().requires_grad_(True)
    y_ref = F.linear(xr, W, layer.bias.float()) + (xr @ A_ref.T) @ B_ref.T
    y_ref.backward(dy.float())
    assert rel(y.detach(), y_ref.detach()) < tol
    assert xi.grad.dtype == dtype and rel(xi.grad, xr.grad) < tol, rel(xi.grad, xr.grad)
    assert layer.lora_A.grad.dtype == torch.float32 and rel(layer.lora_A.grad, A_ref.grad) < tol, rel(layer.lora_A.grad, A_ref.grad)
    assert rel(layer.lora_B.grad, B_ref.grad) < tol, rel(layer.lora_B.grad, B_ref.grad)
    assert layer.qweight.requires_grad is False and layer.lut.grad is None
    # an optimizer step on the adapter changes the inference output, and train_adapter(False) keeps it (fp16 rounding of the factors)
    with torch.no_grad():
        before = layer(x)
        layer.lora_B -= 0.05 * layer.lora_B.grad / layer.lora_B.grad.abs().max()
        after = layer(x)
        assert not torch.equal(before, after)
    layer.train_adapter(False)
    assert layer.lora_A.dtype == torch.float16 and not list(layer.parameters())
    with torch.no_grad():
        assert rel(layer(x), after) < tol
