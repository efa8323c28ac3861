"""Per-token negative log-likelihood straight from a packed head on the MI355X (csrc/lut_head_nll.hip) through every layer: the C
ABI in guarded buffers against fp64, GanqHipQuantLinear.nll (fused, chunked, autograd) and the model-level helpers.

The bound of the Gaussian cases.  ref = fp64 from gather(lut, Q); per row
    E = n 2^-23 max_o sum_j |x_j w_oj|
bounds the error of every fp32 logit whatever the order of its n additions (n roundings of at most 2^-23 relative to the partial
sums, each at most sum_j |x_j w_oj|; 2^-23 and not 2^-24 leaves room for a matrix core that truncates).  tgt_logit is one such
logit: |tgt_logit - ref| <= E.  lse = log sum_o exp(l_o) moves by at most max_o |delta l_o| when the l_o move (its gradient is a
probability vector), so the logits' errors cost lse at most E.  The rest of lse's error is that of forming it from exact fp32
logits, counted in units of u = 2^-24 relative to S = sum_o exp(l_o - max) -- which is an absolute error of lse, log S moving by
dS / S.  With p_i = exp(l_i - max) / S and d_i = max - l_i >= 0:  sum_i p_i d_i <= sum_i p_i (-ln p_i) <= ln m  (d_i <= -ln p_i
because S >= 1), so an error proportional to a term's own distance from the maximum weighs at most ln m in total.
  in a lane      exp(l - mx): the subtraction and the scaling by log2(e) each cost d u, the hardware exp2 2 u; three additions of
                 positive terms, 1 u each:                                                                  2 ln m + 5
  five lane exchanges  S = s1 exp(m1 - M) + s2 exp(m2 - M): one factor is exp(0) = 1 exactly; the other costs (2 d' + 2) u on
                 its side, where the d' of a term telescope over the levels to at most its own d; a product and an addition,
                 1 u each:                                                                                  2 ln m + 20
  combine        sm exp(mx - max) per tile (expf 2 u, subtraction d u, product 1 u), ceil(T / 16) additions in a wave's range and
                 16 across the waves, T = ceil(m / 128):                                                    ln m + 3 + T / 16 + 16
  log and max + log S   2 u of log S and one rounding of lse itself:                                        2 + |lse|
Sum: 5 ln m + 46 + T / 16 + |lse| <= 105 + T / 16 + |lse| for m <= 128256, inside the (T + 192) 2^-24 max(1, |ref|) the test
allows.  nll = lse - tgt_logit (one more rounding, of a number no larger than |lse| + |tgt_logit|) gets the sum of both bounds.
Integer inputs (tests/lut_arena.py) make every logit exact: E = 0, tgt_logit is bit-exact and lse has the second term alone."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import head_nll_model as hm
import lut_arena as la

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -24


@pytest.fixture(scope="module")
def hip():
    from ganq_amd import _lib

    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.selftest()
    return _lib


# ---- the C ABI in guarded buffers
def run_abi(hip, inp, bits, dtype, targets):
    """ganq_lut_head_nll on `inp` (numpy, tests/lut_arena.py) inside an Arena: a workspace of EXACTLY the sizer's bytes, outputs
    pre-filled with NaN between NaN guards -> ((nll, lse, tgt_logit) clones, device tensors)"""
    dt = la._torch_dtype(dtype)
    M, n = inp["x"].shape
    m, V = inp["Q"].shape[0], 2 ** bits

    def as_dt(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dt)

    qw = hip.pack_indices(torch.from_numpy(inp["Q"]).cuda(), bits)
    nbytes = hip.lib().ganq_lut_head_nll_workspace_bytes(M, m, n, bits)
    assert nbytes == hm.workspace_layout(M, m)["total"]
    specs = [("x", dt, (M, n), as_dt(inp["x"]), True),
             ("nll", torch.float32, (M,), None, True), ("lse", torch.float32, (M,), None, True),
             ("tgt_logit", torch.float32, (M,), None, True), ("ws", torch.uint8, (nbytes,), None, False),
             ("qweight", torch.int32, tuple(qw.shape), qw, False), ("lut", dt, (m, V), as_dt(inp["lut"]), True),
             ("targets", torch.int64, (M,), torch.from_numpy(targets), False)]
    if inp["bias"] is not None:
        specs.append(("bias", dt, (m,), as_dt(inp["bias"]), True))
    arena = la.Arena(specs)
    t = arena.t
    outs = ("nll", "lse", "tgt_logit")
    for name in outs:
        t[name].fill_(float("nan"))
    arena.snapshot(outs + ("ws",))
    p = {k: v.data_ptr() for k, v in t.items()}
    hip._call("ganq_lut_head_nll", tuple(t.values()), p["x"], p["qweight"], p["lut"], p.get("bias"), p["targets"],
              0 if dtype == "fp16" else 1, M, m, n, bits, p["nll"], p["lse"], p["tgt_logit"], p["ws"], nbytes, hip._ST)
    torch.cuda.synchronize()
    arena.assert_untouched("ganq_lut_head_nll")
    for name in outs:
        assert not bool(torch.isnan(t[name]).any()), f"{name}: rows never written (or NaN)"
    dev = dict(t)
    dev["Q"] = torch.from_numpy(inp["Q"]).cuda()
    dev["arena"] = arena
    return tuple(t[name].clone() for name in outs), dev


def reference(dev, m):
    """fp64 (nll, lse, tgt_logit, E) [M] on the arena's tensors"""
    x = dev["x"].double()
    W = torch.gather(dev["lut"].double(), 1, dev["Q"].long())
    logits = x @ W.T
    if "bias" in dev:
        logits = logits + dev["bias"].double()
    E = x.shape[1] * 2.0 ** -23 * (x.abs() @ W.abs().T).max(dim=1).values
    t = dev["targets"]
    hit = (t >= 0) & (t < m)
    lse = torch.logsumexp(logits, dim=1)
    tgt = torch.where(hit, logits.gather(1, t.clamp(0, m - 1).unsqueeze(1)).squeeze(1), torch.zeros_like(lse))
    return torch.where(hit, lse - tgt, torch.zeros_like(lse)), lse, tgt, E


def check(got, dev, m, what, exact=False):
    nll, lse, tgt = got
    rnll, rlse, rtgt, E = reference(dev, m)
    if exact:
        E = torch.zeros_like(E)
    t = dev["targets"]
    hit = (t >= 0) & (t < m)
    second = (-(-m // 128) + 192) * U * rlse.abs().clamp_min(1.0)
    e_lse, e_tgt, e_nll = (lse.double() - rlse).abs(), (tgt.double() - rtgt).abs(), (nll.double() - rnll).abs()
    print(f"{what}: max |lse - ref| / bound {float((e_lse / (E + second)).max()):.3g}; lse error beyond E in units of 2^-24 max(1, |ref|) "
          f"{float(((e_lse - E).clamp_min(0) / (U * rlse.abs().clamp_min(1.0))).max()):.3g} of {-(-m // 128) + 192}; "
          f"max |tgt_logit - ref| / E {float((e_tgt / E.clamp_min(1e-300))[hit].max()) if bool(hit.any()) and not exact else 0.0:.3g}")
    assert bool((e_lse <= E + second).all()), what
    if exact:
        assert torch.equal(tgt, rtgt.float()), f"{what}: tgt_logit is not the exact logit"
    else:
        assert bool((e_tgt <= E).all()), what
    assert bool((e_nll <= 2 * E + second).all()), what
    assert bool((nll[~hit] == 0).all()) and bool((tgt[~hit] == 0).all()), f"{what}: an ignored row is not 0"
    assert bool(torch.isfinite(lse).all())


def wrapper(hip, dev, bits):
    return hip.lut_head_nll(dev["x"], dev["qweight"], dev["lut"], dev.get("bias"), bits, dev["targets"])


@pytest.mark.parametrize("case", hm.CASES, ids=hm.case_id)
def test_c_abi_against_fp64(hip, case):
    bits, dtype, M, m, n, with_bias = case
    seed = zlib.crc32(hm.case_id(case).encode())
    targets = hm.make_targets(M, m, seed)
    inp = la.gaussian(bits, M, m, n, "plain" if with_bias else "nobias", seed)
    inp["x"] *= 2.0  # logits of a few units: the softmax is far from flat
    got, dev = run_abi(hip, inp, bits, dtype, targets)
    check(got, dev, m, "gaussian " + hm.case_id(case))
    again = wrapper(hip, dev, bits)
    for a, b in zip(got, again):
        assert torch.equal(a, b), "the public wrapper and the C ABI call on the same tensors differ"
    inp = la.integers(bits, M, m, n, "plain" if with_bias else "nobias", seed, dtype)
    got, dev = run_abi(hip, inp, bits, dtype, targets)
    check(got, dev, m, "integers " + hm.case_id(case), exact=True)


@pytest.mark.parametrize("case", hm.PADDING_CASES, ids=hm.case_id)
def test_padding_features_take_no_part(hip, case):
    """every real logit <= -40 (bias -48, |x w| small): a padding feature of the last tile counted as a logit of 0 would lift lse
    by more than 30"""
    bits, dtype, M, m, n = case
    inp = la.gaussian(bits, M, m, n, "plain", 11 * m + n)
    inp["bias"] = np.full(m, -48.0, dtype=np.float32)
    got, dev = run_abi(hip, inp, bits, dtype, hm.make_targets(M, m, m))
    ref = reference(dev, m)
    assert float(ref[1].max()) < -40 + np.log(m)  # (so every logit is below -40)
    check(got, dev, m, "padding " + hm.case_id(case))
    assert float((got[1].double() - ref[1]).abs().max()) < 1e-3  # (a counted padding feature: > 30)


def test_repeatable_and_capturable(hip):
    """two calls give the same bytes; a call captured in a HIP graph and replayed on changed x and targets gives the bytes of a
    fresh call (no host synchronisation, all scratch in the workspace, nothing left over from the previous replay)"""
    bits, M, m, n = 4, 257, 300, 160
    inp = la.gaussian(bits, M, m, n, "plain", 5)
    qw = hip.pack_indices(torch.from_numpy(inp["Q"]).cuda(), bits)
    lut, bias = torch.from_numpy(inp["lut"]).cuda().half(), torch.from_numpy(inp["bias"]).cuda().half()
    xs = [torch.from_numpy(la.gaussian(bits, M, m, n, "plain", s)["x"]).cuda().half() for s in (5, 6, 7)]
    ts = [torch.from_numpy(hm.make_targets(M, m, s)).cuda() for s in (5, 6, 7)]
    eager = [hip.lut_head_nll(x, qw, lut, bias, bits, t) for x, t in zip(xs, ts)]
    for a, b in zip(eager[0], hip.lut_head_nll(xs[0], qw, lut, bias, bits, ts[0])):
        assert torch.equal(a, b), "not bitwise repeatable"
    torch.cuda.synchronize()
    static_x, static_t = xs[0].clone(), ts[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        hip.lut_head_nll(static_x, qw, lut, bias, bits, static_t)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            static_out = hip.lut_head_nll(static_x, qw, lut, bias, bits, static_t)
    torch.cuda.current_stream().wait_stream(side)
    for x, t, want in list(zip(xs, ts, eager))[1:] + [(xs[0], ts[0], eager[0])]:
        static_x.copy_(x)
        static_t.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(static_out, want):
            assert torch.equal(a, b), "the replay differs from a fresh call"


def test_large_vocabulary(hip):
    """m = 128256 (1002 feature tiles, 63 per wave of the combine kernel): targets around 0, 32768, 65536, 98304 and m - 1"""
    bits, dtype, M, m, n = hm.LARGE_VOCAB
    inp = la.gaussian(bits, M, m, n, "plain", 99)
    inp["x"] *= 2.0
    targets = hm.make_targets(M, m, 3)
    marks = [0, 1, 32767, 32768, 32769, 65535, 65536, 65537, 98303, 98304, 98305, m - 2, m - 1]
    targets[8:8 + len(marks)] = marks
    targets[M - len(marks):] = marks[::-1]  # the same ids in the second row block
    got, dev = run_abi(hip, inp, bits, dtype, targets)
    check(got, dev, m, "large vocabulary")


def test_c_abi_rejects_bad_arguments(hip):
    lib = hip.lib()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    need = lib.ganq_lut_head_nll_workspace_bytes(65, 300, 96, 4)
    args = lambda **kw: (p, p, p, None, p, kw.get("dtype", 0), kw.get("M", 65), kw.get("m", 300), kw.get("n", 96), kw.get("bits", 4),
                         p, p, p, p, kw.get("ws", need), None)
    before = buf.clone()
    assert lib.ganq_lut_head_nll(*args(ws=need - 1)) == -4
    assert lib.ganq_lut_head_nll(*args(bits=5)) == -2 and lib.ganq_lut_head_nll(*args(n=48)) == -2
    assert lib.ganq_lut_head_nll(*args(dtype=2)) == -2 and lib.ganq_lut_head_nll(*args(M=-1)) == -1
    assert lib.ganq_lut_head_nll(*args(M=1 << 24, n=4096, ws=1 << 40)) == -1  # beyond the 2 GB window of the buffer loads
    torch.cuda.synchronize()
    assert torch.equal(buf, before), "a refused call wrote something"


# ---- the module
def make_layer(bits, m, n, dtype=torch.float16, bias=True, seed=0, outliers=False, rank=0, scale=0.05):
    from ganq_amd.adapter import Lora
    from ganq_amd.nn_modules.qlinear.ganq_hip import GanqHipQuantLinear

    g = torch.Generator(device="cuda").manual_seed(seed)
    V = 1 << bits
    Q = torch.randint(0, V, (m, n), device="cuda", generator=g, dtype=torch.int64).to(torch.uint8)
    lut = torch.sort(scale * torch.randn(m, V, device="cuda", generator=g), dim=1).values.half()
    kw, pack = {}, {}
    if outliers:
        mask = torch.rand(m, n, device="cuda", generator=g) < 0.01
        rowptr = torch.zeros(m + 1, dtype=torch.int32, device="cuda")
        rowptr[1:] = torch.cumsum(mask.sum(1), 0).to(torch.int32)
        cols = mask.nonzero()[:, 1].to(torch.int32)
        vals = (0.3 * torch.randn(cols.numel(), device="cuda", generator=g)).half()
        kw["outliers"], pack["ganq_outliers"] = cols.numel(), (rowptr, cols, vals)
    if rank:
        kw["adapter"] = Lora(rank=rank)
        pack["ganq_lora"] = ((torch.randn(rank, n, device="cuda", generator=g) / n ** 0.5).half(),
                             (0.05 * torch.randn(m, rank, device="cuda", generator=g)).half())
    layer = GanqHipQuantLinear(bits=bits, group_size=-1, sym=True, desc_act=False, in_features=n, out_features=m, bias=bias, **kw).cuda()
    lin = nn.Linear(n, m, bias=bias).cuda()
    layer.pack(lin, ganq_indices=Q, ganq_codebook=lut.float(), **pack)
    return layer


@torch.no_grad()
def fp64_nll(W, bias, x, t):
    logits = x.double() @ W.double().T + (0 if bias is None else bias.double())
    return F.cross_entropy(logits, t, reduction="none", ignore_index=-100), logits


def module_targets(shape, m, seed):
    t = torch.from_numpy(hm.make_targets(int(np.prod(shape)), m, seed)).cuda()
    return torch.where((t < 0) | (t >= m), torch.full_like(t, -100), t).reshape(shape)  # (F.cross_entropy knows only -100)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_module_fused_against_chunked(hip, dtype, monkeypatch):
    """the same layer through the kernel and through the chunked path: the chunked path rounds its logits to the layer dtype, an
    error of at most eps |logit| per logit and so of lse and of the target's logit: 2 eps max |logit| per token, on top of the fused
    call's own bound (its E + second term, twice, for nll)"""
    import ganq_amd.nn_modules.qlinear.ganq_hip as gh

    m, n = 300, 160
    layer = make_layer(4, m, n, seed=1, scale=0.1)
    x = torch.randn(3, 43, n, device="cuda").to(dtype)
    t = module_targets((3, 43), m, 4)
    monkeypatch.setattr(gh, "NLL_CHUNK_BYTES", 64 * m * 6)  # 64-row chunks: three of them
    with torch.no_grad():
        fused, chunked, default = layer.nll(x, t, fused=True), layer.nll(x, t, fused=False), layer.nll(x, t)
        logits = torch.cat([layer(xc) for xc in x.reshape(-1, n).split(64)]).float()  # the chunks' own calls
    assert fused.shape == t.shape and fused.dtype == torch.float32 and fused.grad_fn is None
    assert torch.equal(fused, default), "a layer with neither outliers nor an adapter takes the kernel by default"
    want = F.cross_entropy(logits.reshape(-1, m), t.reshape(-1), reduction="none").reshape(t.shape)
    assert torch.allclose(chunked, want, rtol=1e-5, atol=1e-5)  # (torch.logsumexp against F.cross_entropy's log_softmax)
    eps = 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8
    W = layer.dequantize_weight().to(dtype)
    E = n * 2.0 ** -23 * float((x.reshape(-1, n).double().abs() @ W.double().abs().T).max())
    bound = 2 * eps * float(logits.abs().max()) + 2 * E + (3 + 192) * U * max(1.0, float(logits.abs().max()) + np.log(m))
    err = float((fused - chunked).abs().max())
    print(f"fused vs chunked {dtype}: max difference {err:.3g}, bound {bound:.3g}")
    assert err <= bound
    assert bool((fused[t == -100] == 0).all()) and bool((chunked[t == -100] == 0).all())


@pytest.mark.parametrize("kind", ["outliers", "adapter"])
def test_module_chunked_layers_against_fp64(hip, kind, monkeypatch):
    """a layer with outliers and a layer with an adapter take the chunked path (fused=True raises) and match fp64 through
    dequantize_weight() / merged_weight().  Per logit: its rounding to fp16, 2^-11 |logit|; the fp16 rounding of the reference weight
    itself (Wq + W_sparse, Wq + lora_B lora_A), 2^-11 sum_j |x_j W_oj|; with an adapter the forward's rounding of t = x lora_A^T,
    2^-11 sum_k |t_k B_ok|.  lse and the target's logit each move by at most the largest of these sums: twice that per token."""
    import ganq_amd.nn_modules.qlinear.ganq_hip as gh

    m, n = 300, 160
    layer = make_layer(4, m, n, seed=2, outliers=kind == "outliers", rank=16 if kind == "adapter" else 0, scale=0.1)
    x = torch.randn(130, n, device="cuda").half()
    t = module_targets((130,), m, 9)
    monkeypatch.setattr(gh, "NLL_CHUNK_BYTES", 64 * m * 6)
    with torch.no_grad():
        got = layer.nll(x, t)
        assert torch.equal(got, layer.nll(x, t, fused=False))
        with pytest.raises(ValueError, match="fused=True"):
            layer.nll(x, t, fused=True)
    W = layer.merged_weight() if kind == "adapter" else layer.dequantize_weight()
    want, logits = fp64_nll(W, layer.bias, x, t)
    per_logit = logits.abs() + x.double().abs() @ W.double().abs().T
    if kind == "adapter":
        per_logit = per_logit + (x.double() @ layer.lora_A.double().T).abs() @ layer.lora_B.double().abs().T
    bound = 2 * 2.0 ** -11 * float(per_logit.max())
    err = float((got.double() - want).abs().max())
    print(f"chunked {kind}: max error {err:.3g}, bound {bound:.3g}")
    assert err <= bound and bool((got[t == -100] == 0).all())


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


@pytest.mark.parametrize("m,n,M,fused", [(300, 160, 70, True), (129, 512, 257, True), (129, 512, 257, False)])
def test_gradients_against_the_composition(hip, m, n, M, fused, monkeypatch):
    """dx and dlut of nll.sum() and of a random-weighted sum against what autograd gives for
    F.cross_entropy(layer(x).float(), t, reduction="none") through _GanqLutLinearFn, at the tolerances tests/test_hip_lut_backward.py
    uses for these two gradients (relative error of dx below 2e-3 in fp16, of the codebook gradient below 1e-5); 64-row chunks: two
    at M = 70, five at M = 257"""
    import ganq_amd.nn_modules.qlinear.ganq_hip as gh

    monkeypatch.setattr(gh, "NLL_CHUNK_BYTES", 64 * m * 6)
    layer = make_layer(4, m, n, seed=M).train_codebook(True)
    assert layer._nll_chunk_rows(2) == 64
    torch.manual_seed(M)
    x = torch.randn(M, n, device="cuda").half()
    t = module_targets((M,), m, M)
    assert int((t == -100).sum()) >= 3
    for w in (None, torch.rand(M, device="cuda") + 0.5):
        grads = []
        for which in ("nll", "composition"):
            layer.lut.grad = None
            xi = x.clone().requires_grad_(True)
            if which == "nll":
                loss = layer.nll(xi, t, fused=fused)
                assert loss.grad_fn is not None
            else:
                loss = F.cross_entropy(layer(xi).float(), t, reduction="none")
            (loss.sum() if w is None else (loss * w).sum()).backward()
            grads.append((xi.grad, layer.lut.grad.clone(), loss.detach()))
        (dx, dlut, _), (dx_ref, dlut_ref, _) = grads
        e_dx, e_dlut = rel(dx, dx_ref), rel(dlut, dlut_ref)
        print(f"gradients m={m} n={n} M={M} fused={fused} weighted={w is not None}: rel. error dx {e_dx:.3g} (bar 2e-3), dlut {e_dlut:.3g} (bar 1e-5)")
        assert dx.dtype == torch.float16 and dlut.dtype == torch.float32
        assert bool((dx[t == -100] == 0).all()), "an ignored row has a gradient"
        assert e_dx < 2e-3 and e_dlut < 1e-5
        # deterministic
        layer.lut.grad = None
        xi = x.clone().requires_grad_(True)
        loss = layer.nll(xi, t, fused=fused)
        (loss.sum() if w is None else (loss * w).sum()).backward()
        assert torch.equal(xi.grad, dx) and torch.equal(layer.lut.grad, dlut) and torch.equal(loss.detach(), grads[0][2])
    with torch.no_grad():  # the forward under autograd is the inference call
        assert torch.equal(grads[0][2], layer.nll(x, t, fused=fused))


def test_trainable_adapter_raises(hip):
    layer = make_layer(4, 129, 96, seed=3, rank=16).train_adapter(True)
    x = torch.randn(5, 96, device="cuda").half()
    t = torch.arange(5, device="cuda")
    with pytest.raises(NotImplementedError, match="forward"):
        layer.nll(x, t)
    with torch.no_grad():
        assert layer.nll(x, t).shape == (5,)
    with pytest.raises(ValueError):
        layer.nll(x, t[:4])
    with pytest.raises(TypeError):
        layer.nll(x, t.float())


# ---- the model
@pytest.fixture(scope="module")
def tiny_model(hip):
    sys.path.insert(0, GOLDEN_DIR)
    import make_golden_tiny_lm as tiny
    from ganq_amd.models import quantize_model
    from ganq_amd.quantization.config import QuantizeConfig

    fx = np.load(os.path.join(GOLDEN_DIR, "tiny_lm", "fixture.npz"))
    model = tiny.load_model(torch.float16).cuda().eval()
    qcfg = QuantizeConfig(bits=4, quant_method="ganq", format="ganq_lut", act_sort="asc", l_damp_style="ganq", dead="mean",
                          ganq_iterations=2, lm_head=True)
    batches = [torch.from_numpy(fx["calib"][i:i + 1].astype(np.int64)).cuda() for i in range(fx["calib"].shape[0])]
    with torch.no_grad():
        quantize_model(model, batches, qcfg)
    seq = int(fx["seq"])
    ids = torch.from_numpy(fx["eval_ids"].astype(np.int64).reshape(-1)[: 4 * seq]).cuda()
    return model, ids, seq


def test_causal_lm_nll_against_the_logits(tiny_model):
    from ganq_amd.models import causal_lm_nll, gptq_style_ppl
    from ganq_amd.nn_modules.qlinear.ganq_hip import GanqHipQuantLinear

    model, ids, seq = tiny_model
    assert isinstance(model.get_output_embeddings(), GanqHipQuantLinear)
    batch = ids[: 2 * seq].reshape(2, seq)
    with torch.no_grad():
        logits = model(batch).logits.float()
        got = causal_lm_nll(model, batch)
    want = F.cross_entropy(logits[:, :-1].reshape(-1, logits.shape[-1]), batch[:, 1:].reshape(-1), reduction="none").reshape(2, seq - 1)
    bound = 2 * 2.0 ** -11 * float(logits.abs().max())
    err = float((got - want).abs().max())
    print(f"causal_lm_nll: max difference {err:.3g}, bound {bound:.3g}")
    assert got.shape == (2, seq - 1) and got.dtype == torch.float32 and err <= bound
    labels = batch.clone()
    labels[:, 5:9] = -100
    with torch.no_grad():
        masked = causal_lm_nll(model, batch, labels)
    assert bool((masked[:, 4:8] == 0).all()) and torch.equal(masked[:, 8:], got[:, 8:]) and torch.equal(masked[:, :4], got[:, :4])
    plain = gptq_style_ppl(model, ids.reshape(1, -1), seqlen=seq)
    fused = gptq_style_ppl(model, ids.reshape(1, -1), seqlen=seq, fused_head=True)
    print(f"gptq_style_ppl: {plain:.6f} with the logits, {fused:.6f} straight from the head")
    assert abs(np.log(fused) - np.log(plain)) <= bound


def test_causal_lm_nll_refuses_what_it_cannot_serve(tiny_model):
    sys.path.insert(0, GOLDEN_DIR)
    import make_golden_tiny_lm as tiny
    from ganq_amd.models import causal_lm_nll, gptq_style_ppl

    model, ids, seq = tiny_model
    batch = ids[:seq].reshape(1, seq)
    plain = tiny.load_model(torch.float16).cuda().eval()
    with pytest.raises(TypeError, match="GanqHipQuantLinear"):
        causal_lm_nll(plain, batch)
    with pytest.raises(TypeError, match="GanqHipQuantLinear"):
        gptq_style_ppl(plain, ids.reshape(1, -1), seqlen=seq, fused_head=True)
    model.config.final_logit_softcapping = 30.0
    try:
        with pytest.raises(NotImplementedError, match="final_logit_softcapping"):
            causal_lm_nll(model, batch)
    finally:
        del model.config.final_logit_softcapping
