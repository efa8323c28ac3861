"""Next token straight from a packed head on the MI355X (csrc/lut_head_pick.hip) through every layer: the C ABI in guarded buffers
against fp64, GanqHipQuantLinear.pick (fused and composition) and causal_lm_next_token.

The bounds of the Gaussian cases (tests/head_pick_model.py::reference computes them in fp64 on the CPU, from the values the device
tensors hold).  Per row, with E = n 2^-23 max_o sum_j |x_j w_oj| the bound of every fp32 logit (tests/test_hip_head_nll.py):
    E1 = E inv_t + 4 2^-24 max_o |z_o|
bounds the error of every s and z: the logit's error scaled by inv_t, and one rounding each of the sum with the bias, the product
with inv_t and the sum with the noise.  So |score - s64[token]| <= E1, the chosen z is within 2 E1 of the fp64 maximum, and on a row
whose fp64 gap between the best and the second-best z exceeds 2 E1 the token IS the fp64 argmax; the seeds are chosen (and checked
without a GPU, tests/test_head_pick_model.py) so that these are at least 90 % of every case's rows.
lse moves by at most max_o |delta s_o| <= E inv_t when the s_o move (its gradient is a probability vector); the roundings of s itself
weigh sum_i p_i |s_i| <= |lse| + 2 ln m units of u = 2^-24 each (|s_i| <= |max| + d_i, sum_i p_i d_i <= ln m), two of them.  The
rest is the error of forming lse from exact fp32 values, counted as tests/test_hip_head_nll.py counts it, in units of u relative to
S = sum_o exp(s_o - max):
  eight merge levels (four lane exchanges, the two tiles, three waves): S = s1 exp(m1 - M) + s2 exp(m2 - M), one factor exp(0) = 1,
                 the other (2 d' + 2) u with the d' of a term telescoping to its own d; a product and an addition:  2 ln m + 32
  merge kernel   sm exp(mx - max) per block (expf 2 u, subtraction d u, product 1 u), ceil(T / 64) + 6 <= T + 6 additions: ln m + 9 + T
  log and max + log S                                                                                               2 + |lse|
Sum: 7 ln m + 43 + T + 3 |lse| <= 126 + T + 3 |lse| for m <= 128256, inside the (T + 192) 2^-24 max(1, |ref|) the test allows
(T = the number of feature blocks).  logprob is the fp32 difference of the two outputs, bit for bit.
Integer inputs (tests/lut_arena.py, integer or half-integer noise, inv_t = 1) make every z exact: the token is np.argmax's -- the
first maximum -- on every row, score is bit-exact and lse has the last term alone."""
import zlib

import numpy as np
import pytest
import torch

import head_pick_model as hm
import lut_arena as la
from test_hip_head_nll import make_layer

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TOKEN_PREFILL = -7


@pytest.fixture(scope="module")
def hip():
    from ganq_amd import _lib

    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.selftest()
    return _lib


# ---- the C ABI in guarded buffers
def run_abi(hip, inp, bits, dtype, noise, inv_t):
    """ganq_lut_head_pick on `inp` (numpy, tests/lut_arena.py) inside an Arena: a workspace of EXACTLY the sizer's bytes, outputs
    pre-filled (NaN, a negative token) between guards -> ((token, score, lse, logprob) numpy, device tensors)"""
    dt = la._torch_dtype(dtype)
    M, n = inp["x"].shape
    m, V = inp["Q"].shape[0], 2 ** bits

    def as_dt(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dt)

    qw = hip.pack_indices(torch.from_numpy(inp["Q"]).cuda(), bits)
    nbytes = hip.lib().ganq_lut_head_pick_workspace_bytes(M, m, n, bits)
    assert nbytes == hm.workspace_layout(M, m)["total"]
    specs = [("x", dt, (M, n), as_dt(inp["x"]), True), ("token", torch.int64, (M,), None, False),
             ("score", torch.float32, (M,), None, True), ("lse", torch.float32, (M,), None, True),
             ("logprob", torch.float32, (M,), None, True), ("ws", torch.uint8, (nbytes,), None, False),
             ("qweight", torch.int32, tuple(qw.shape), qw, False), ("lut", dt, (m, V), as_dt(inp["lut"]), True)]
    if noise is not None:
        specs.append(("noise", torch.float32, (M, m), torch.from_numpy(noise), True))
    if inp["bias"] is not None:
        specs.append(("bias", dt, (m,), as_dt(inp["bias"]), True))
    arena = la.Arena(specs)
    t = arena.t
    outs = ("token", "score", "lse", "logprob")
    t["token"].fill_(TOKEN_PREFILL)
    for name in outs[1:]:
        t[name].fill_(float("nan"))
    arena.snapshot(outs + ("ws",))
    p = {k: v.data_ptr() for k, v in t.items()}
    hip._call("ganq_lut_head_pick", tuple(t.values()), p["x"], p["qweight"], p["lut"], p.get("bias"), p.get("noise"), float(inv_t),
              0 if dtype == "fp16" else 1, M, m, n, bits, p["token"], p["score"], p["lse"], p["logprob"], p["ws"], nbytes, hip._ST)
    torch.cuda.synchronize()
    arena.assert_untouched("ganq_lut_head_pick")
    for name in outs[1:]:
        assert not bool(torch.isnan(t[name]).any()), f"{name}: rows never written (or NaN)"
    assert bool(((t["token"] >= 0) & (t["token"] < m)).all()), "token: rows never written, or a padding feature chosen"
    dev = dict(t)
    dev["arena"] = arena
    return tuple(t[name].cpu().numpy() for name in outs), dev


def check(got, ref, m, inv_t, what, exact=False):
    token, score, lse, logprob = got
    rows = np.arange(token.shape[0])
    E, E1 = (np.zeros_like(ref["E"]), np.zeros_like(ref["E1"])) if exact else (ref["E"], ref["E1"])
    T = hm.blocks_of(m)
    second = (T + 192) * U * np.maximum(1.0, np.abs(ref["lse"]))
    s_tok, z_tok = ref["s"][rows, token], ref["z"][rows, token]
    e_score, e_lse = np.abs(score.astype(np.float64) - s_tok), np.abs(lse.astype(np.float64) - ref["lse"])
    short = ref["z"].max(axis=1) - z_tok
    decisive = ref["gap"] > 2 * E1
    print(f"{what}: max |score - ref| / E1 {float((e_score / np.maximum(E1, 1e-300)).max()) if not exact else float(e_score.max()):.3g}; "
          f"max |lse - ref| / bound {float((e_lse / (E * inv_t + second)).max()):.3g}; lse error beyond E inv_t in units of "
          f"2^-24 max(1, |ref|) {float((np.maximum(e_lse - E * inv_t, 0) / (U * np.maximum(1.0, np.abs(ref['lse'])))).max()):.3g} of "
          f"{T + 192}; max (max z - z[token]) / 2 E1 {float((short / np.maximum(2 * E1, 1e-300)).max()) if not exact else float(short.max()):.3g}; "
          f"decisive rows {int(decisive.sum())} of {decisive.size}, of them wrong {int((token != ref['token'])[decisive].sum())}")
    assert (e_score <= E1).all(), what
    assert (e_lse <= E * inv_t + second).all(), what
    assert (short <= 2 * E1).all(), what
    assert np.array_equal(token[decisive], ref["token"][decisive]), what
    assert exact or decisive.mean() >= 0.9, what
    assert np.array_equal(logprob, score - lse), f"{what}: logprob is not score - lse in fp32"
    if exact:
        assert np.array_equal(token, ref["token"]), f"{what}: not the first maximum"
        assert np.array_equal(score, s_tok.astype(np.float32)), f"{what}: score is not the exact value"


def wrapper(hip, dev, bits, inv_t):
    return hip.lut_head_pick(dev["x"], dev["qweight"], dev["lut"], dev.get("bias"), bits, dev.get("noise"), inv_t)


def integer_noise(M, m, seed):
    """integers and half-integers in [-2, 2]"""
    return (np.random.default_rng(seed).integers(-4, 5, (M, m)) / 2).astype(np.float32)


@pytest.mark.parametrize("case", hm.CASES, ids=hm.case_id)
def test_c_abi_against_fp64(hip, case):
    bits, dtype, M, m, n, with_bias, with_noise, inv_t = case
    inp, noise, ref = hm.gaussian_case(case)
    got, dev = run_abi(hip, inp, bits, dtype, noise, inv_t)
    check(got, ref, m, inv_t, "gaussian " + hm.case_id(case))
    for a, b in zip(got, wrapper(hip, dev, bits, inv_t)):
        assert np.array_equal(a, b.cpu().numpy()), "the public wrapper and the C ABI call on the same tensors differ"
    seed = zlib.crc32(hm.case_id(case).encode())
    inp = la.integers(bits, M, m, n, "plain" if with_bias else "nobias", seed, dtype)
    noise = integer_noise(M, m, seed) if with_noise else None
    ref = hm.reference(inp, dtype, 1.0, noise)
    got, dev = run_abi(hip, inp, bits, dtype, noise, 1.0)
    ties = int((np.ptp(np.sort(ref["z"], axis=1)[:, -2:], axis=1) == 0).sum()) if m > 1 else 0
    check(got, ref, m, 1.0, f"integers ({ties} of {M} rows with a tied maximum) " + hm.case_id(case), exact=True)


def test_large_vocabulary(hip):
    """m = 128256: 1002 feature blocks, 16 per lane of the merge kernel"""
    bits, dtype, M, m, n, _, _, inv_t = hm.LARGE_VOCAB
    inp, noise, ref = hm.gaussian_case(hm.LARGE_VOCAB)
    got, dev = run_abi(hip, inp, bits, dtype, noise, inv_t)
    check(got, ref, m, inv_t, "large vocabulary")
    noise = np.zeros((M, m), dtype=np.float32)
    marks = [0, 65535, 65536, 128127, m - 1]  # a planted winner in the first and last block and around 2^16
    noise[np.arange(M), marks] = 64.0
    got, dev = run_abi(hip, inp, bits, dtype, noise, inv_t)
    assert got[0].tolist() == marks


def test_planted_ties(hip):
    """features 5, 21, 40 and 133 of m = 300 get the same codes, the same codebook and a bias that makes them the maximum of every
    row: the same wave's other tile, another wave, another workgroup.  The smallest of them is the token; without it the next."""
    bits, dtype, M, m, n = 4, "fp16", 17, 300, 160
    base = la.gaussian(bits, M, m, n, "plain", 77)
    members = list(hm.TIE_FEATURES)
    while members:
        inp = {k: (None if v is None else np.array(v)) for k, v in base.items()}
        inp["Q"][members] = inp["Q"][members[0]]
        inp["lut"][members] = inp["lut"][members[0]]
        inp["bias"][members] = 24.0
        ref = hm.reference(inp, dtype, 1.0, None)
        assert (ref["token"] == members[0]).all() and (ref["gap"] == 0).all() == (len(members) > 1)
        (token, score, lse, logprob), _ = run_abi(hip, inp, bits, dtype, None, 1.0)
        assert (token == members[0]).all(), (members, token)
        assert (np.abs(score - ref["score"]) <= ref["E1"]).all()
        members = members[1:]


@pytest.mark.parametrize("case", [(4, "fp16", 17, 300, 96, True, True, 0.5), (3, "bf16", 65, 129, 160, False, True, 1.0)], ids=hm.case_id)
def test_noise_moves_the_token_not_the_score(hip, case):
    """a noise of +64 at one index per row makes that index the token; score and logprob are the unperturbed values there"""
    bits, dtype, M, m, n, with_bias, _, inv_t = case
    inp = la.gaussian(bits, M, m, n, "plain" if with_bias else "nobias", 31)
    planted = (np.arange(M) * 37 + 5) % m
    noise = np.zeros((M, m), dtype=np.float32)
    noise[np.arange(M), planted] = 64.0
    ref = hm.reference(inp, dtype, inv_t, noise)
    assert np.array_equal(ref["token"], planted)
    (token, score, lse, logprob), _ = run_abi(hip, inp, bits, dtype, noise, inv_t)
    assert np.array_equal(token, planted)
    plain = hm.reference(inp, dtype, inv_t, None)
    s_tok = plain["s"][np.arange(M), planted]
    second = (hm.blocks_of(m) + 192) * U * np.maximum(1.0, np.abs(plain["lse"]))
    assert (np.abs(score - s_tok) <= ref["E1"]).all() and (np.abs(lse - plain["lse"]) <= plain["E"] * inv_t + second).all()
    assert np.array_equal(logprob, score - lse)
    assert (np.abs(logprob - (s_tok - plain["lse"])) <= ref["E1"] + plain["E"] * inv_t + second + U * (np.abs(s_tok) + np.abs(plain["lse"]))).all()


@pytest.mark.parametrize("case", hm.PADDING_CASES, ids=hm.case_id)
def test_padding_features_take_no_part(hip, case):
    """every real logit <= -40 (bias -48, |x w| small): a padding feature of the last block counted as a logit of 0 would lift lse
    by more than 30 and win the pick"""
    bits, dtype, M, m, n = case
    inp = la.gaussian(bits, M, m, n, "plain", 11 * m + n)
    inp["bias"] = np.full(m, -48.0, dtype=np.float32)
    ref = hm.reference(inp, dtype, 1.0, None)
    assert float(ref["lse"].max()) < -40 + np.log(m)  # (so every logit is below -40)
    got, dev = run_abi(hip, inp, bits, dtype, None, 1.0)
    check(got, ref, m, 1.0, "padding " + hm.case_id(case))
    assert float(np.abs(got[2] - ref["lse"]).max()) < 1e-3 and (got[0] < m).all() and (got[1] < -40).all()


def test_repeatable_and_capturable(hip):
    """two calls give the same bytes; a call captured in a HIP graph and replayed on changed x and noise gives the bytes of a fresh
    call (no host synchronisation, all scratch in the workspace, nothing left over from the previous replay)"""
    bits, M, m, n, inv_t = 4, 65, 300, 160, 1 / 0.7
    inp = la.gaussian(bits, M, m, n, "plain", 5)
    qw = hip.pack_indices(torch.from_numpy(inp["Q"]).cuda(), bits)
    lut, bias = torch.from_numpy(inp["lut"]).cuda().half(), torch.from_numpy(inp["bias"]).cuda().half()
    xs = [torch.from_numpy(la.gaussian(bits, M, m, n, "plain", s)["x"]).cuda().half() for s in (5, 6, 7)]
    ns = [torch.from_numpy(hm.gumbel(M, m, s)).cuda() for s in (5, 6, 7)]
    eager = [hip.lut_head_pick(x, qw, lut, bias, bits, nz, inv_t) for x, nz in zip(xs, ns)]
    for a, b in zip(eager[0], hip.lut_head_pick(xs[0], qw, lut, bias, bits, ns[0], inv_t)):
        assert torch.equal(a, b), "not bitwise repeatable"
    assert not torch.equal(eager[0][0], eager[1][0])
    torch.cuda.synchronize()
    static_x, static_n = xs[0].clone(), ns[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        hip.lut_head_pick(static_x, qw, lut, bias, bits, static_n, inv_t)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            static_out = hip.lut_head_pick(static_x, qw, lut, bias, bits, static_n, inv_t)
    torch.cuda.current_stream().wait_stream(side)
    for x, nz, want in list(zip(xs, ns, eager))[1:] + [(xs[0], ns[0], eager[0])] * 2:
        static_x.copy_(x)
        static_n.copy_(nz)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(static_out, want):
            assert torch.equal(a, b), "the replay differs from a fresh call"


def test_c_abi_rejects_bad_arguments(hip):
    lib = hip.lib()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    need = lib.ganq_lut_head_pick_workspace_bytes(65, 300, 96, 4)
    assert need <= buf.numel()

    def args(**kw):
        return (kw.get("x", p), p, p, None, kw.get("noise", p), kw.get("inv_t", 1.0), kw.get("dtype", 0), kw.get("M", 65), kw.get("m", 300),
                kw.get("n", 96), kw.get("bits", 4), kw.get("token", p), p, p, p, p, kw.get("ws", need), None)

    before = buf.clone()
    call = lib.ganq_lut_head_pick
    assert call(*args(ws=need - 1)) == -4
    assert call(*args(bits=5)) == -2 and call(*args(n=48)) == -2 and call(*args(dtype=2)) == -2
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call(*args(inv_t=bad)) == -2, bad
    assert call(*args(M=-1)) == -1
    assert call(*args(M=1 << 24, n=4096, ws=1 << 40)) == -1  # beyond the 2 GB window of the 32-bit offsets
    assert call(*args(x=None)) == -3 and call(*args(token=None)) == -3
    torch.cuda.synchronize()
    assert torch.equal(buf, before), "a refused call wrote something"


# ---- the module
def fp64_logits(W, bias, x):
    return x.double() @ W.double().T + (0 if bias is None else bias.double())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_module_fused_against_composition(hip, dtype, monkeypatch):
    """the same layer through the kernel and through the composition: the composition rounds its logits to the layer dtype, an error
    of at most eps |logit| per logit, so of lse and of the token's logit: 2 eps max |logit| per token, on top of the fused call's own
    bound (tests/test_hip_head_nll.py::test_module_fused_against_chunked).  Where the gap between the composition's two largest fp32
    logits exceeds 2 eps max |logit| + 4 E (the composition's logits are eps max |logit| + E from the exact ones, so the exact gap
    still exceeds the 2 E the kernel's fp32 logits can close), both pick the same token."""
    import ganq_amd.nn_modules.qlinear.ganq_hip as gh

    m, n = 300, 160
    layer = make_layer(4, m, n, seed=1, scale=0.1)
    x = torch.randn(3, 43, n, device="cuda").to(dtype).requires_grad_(True)
    monkeypatch.setattr(gh, "NLL_CHUNK_BYTES", 64 * m * 6)  # 64-row chunks: three of them
    fused, comp, default = layer.pick(x, fused=True), layer.pick(x, fused=False), layer.pick(x)
    with torch.no_grad():
        logits = torch.cat([layer(xc) for xc in x.reshape(-1, n).split(64)]).float()
    for token, logprob in (fused, comp):
        assert token.shape == logprob.shape == (3, 43) and token.dtype == torch.int64 and logprob.dtype == torch.float32
        assert token.grad_fn is None and logprob.grad_fn is None and not logprob.requires_grad
    assert torch.equal(fused[0], default[0]) and torch.equal(fused[1], default[1]), "a plain layer takes the kernel by default"
    assert torch.equal(comp[0].reshape(-1), logits.argmax(-1))
    eps = 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8
    W = layer.dequantize_weight().to(dtype)
    E = n * 2.0 ** -23 * float((x.detach().reshape(-1, n).double().abs() @ W.double().abs().T).max())
    lmax = float(logits.abs().max())
    bound = 2 * eps * lmax + 2 * E + (3 + 192) * U * max(1.0, lmax + np.log(m))
    top2 = logits.topk(2, dim=-1).values
    sure = ((top2[:, 0] - top2[:, 1]) > 2 * eps * lmax + 4 * E).reshape(3, 43)
    same = fused[0] == comp[0]
    err = float((fused[1] - comp[1])[same].abs().max())
    print(f"fused vs composition {dtype}: max logprob difference {err:.3g}, bound {bound:.3g}; {int(sure.sum())} of {sure.numel()} rows sure, "
          f"{int((~same).sum())} tokens differ")
    assert bool(same[sure].all()) and err <= bound and float(sure.float().mean()) >= 0.5


def test_module_sampling_is_the_library_call_on_torch_noise(hip):
    """pick(temperature=0.7, generator=g) is bit for bit _lib.lut_head_pick on the noise the same torch calls give from an equally
    seeded generator; a caller's own noise is passed through; at temperature 1 logprob is -nll(x, token) within both calls' bounds"""
    m, n, M = 300, 160, 70
    layer = make_layer(4, m, n, seed=3, scale=0.1)
    x = torch.randn(M, n, device="cuda").half()
    g = torch.Generator(device="cuda").manual_seed(123)
    token, logprob = layer.pick(x, temperature=0.7, generator=g)
    g2 = torch.Generator(device="cuda").manual_seed(123)
    e = torch.empty(M, m, dtype=torch.float32, device="cuda").exponential_(generator=g2)
    noise = -torch.log(e.clamp_min(torch.finfo(torch.float32).tiny))
    want = hip.lut_head_pick(x, layer.qweight, layer.lut, layer.bias, 4, noise, 1.0 / 0.7)
    assert torch.equal(token, want[0]) and torch.equal(logprob, want[3])
    assert not torch.equal(token, layer.pick(x)[0]), "the noise changed no token of 70"
    own = layer.pick(x.reshape(2, 35, n), temperature=0.7, noise=noise.reshape(2, 35, m))
    assert torch.equal(own[0].reshape(-1), token) and torch.equal(own[1].reshape(-1), logprob)
    # temperature 1: the rollout's logprob and the training pass's -nll are the same number
    token, logprob = layer.pick(x, temperature=1.0, noise=noise)
    with torch.no_grad():
        nll = layer.nll(x, token)
    W = layer.dequantize_weight()
    l64 = fp64_logits(W, layer.bias, x)
    E = n * 2.0 ** -23 * (x.double().abs() @ W.double().abs().T).max(dim=1).values
    lse64 = torch.logsumexp(l64, dim=1)
    second = (3 + 192) * U * lse64.abs().clamp_min(1.0)
    bound = (2 * E + second) + (E + 4 * U * (l64 + noise.double()).abs().max(dim=1).values + E + second)
    err = (logprob.double() + nll.double()).abs()
    print(f"logprob + nll at temperature 1: max {float(err.max()):.3g}, max of err / bound {float((err / bound).max()):.3g}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("kind", ["outliers", "adapter"])
def test_module_composition_layers_against_fp64(hip, kind, monkeypatch):
    """a layer with outliers and a layer with an adapter take the composition (fused=True raises) and match fp64 through
    dequantize_weight() / merged_weight(): per logit the error terms of
    tests/test_hip_head_nll.py::test_module_chunked_layers_against_fp64, B = 2^-11 times their largest sum; logprob within 2 B, and
    the token is the fp64 argmax wherever the fp64 gap exceeds 2 B"""
    import ganq_amd.nn_modules.qlinear.ganq_hip as gh

    m, n = 300, 160
    layer = make_layer(4, m, n, seed=2, outliers=kind == "outliers", rank=16 if kind == "adapter" else 0, scale=0.1)
    x = torch.randn(130, n, device="cuda").half()
    monkeypatch.setattr(gh, "NLL_CHUNK_BYTES", 64 * m * 6)
    token, logprob = layer.pick(x)
    again = layer.pick(x, fused=False)
    assert torch.equal(token, again[0]) and torch.equal(logprob, again[1])
    with pytest.raises(ValueError, match="fused=True"):
        layer.pick(x, fused=True)
    W = layer.merged_weight() if kind == "adapter" else layer.dequantize_weight()
    logits = fp64_logits(W, layer.bias, x)
    per_logit = logits.abs() + x.double().abs() @ W.double().abs().T
    if kind == "adapter":
        per_logit = per_logit + (x.double() @ layer.lora_A.double().T).abs() @ layer.lora_B.double().abs().T
    B = 2.0 ** -11 * float(per_logit.max())
    top2 = logits.topk(2, dim=-1).values
    sure = (top2[:, 0] - top2[:, 1]) > 2 * B
    want = logits.gather(1, token.unsqueeze(1)).squeeze(1) - torch.logsumexp(logits, dim=1)
    err = float((logprob.double() - want).abs().max())
    print(f"composition {kind}: max logprob error {err:.3g}, bound {2 * B:.3g}; {int(sure.sum())} of 130 rows sure")
    assert err <= 2 * B and torch.equal(token[sure], logits.argmax(-1)[sure]) and float(sure.float().mean()) >= 0.5
    # sampled: the composition's own steps on the caller's noise
    noise = torch.from_numpy(hm.gumbel(130, m, 8)).cuda()
    token, logprob = layer.pick(x, temperature=0.5, noise=noise)
    with torch.no_grad():
        s = torch.cat([layer(xc) for xc in x.split(64)]).float() * 2.0
    assert torch.equal(token, (s + noise).argmax(-1))
    assert torch.equal(logprob, s.gather(1, token.unsqueeze(1)).squeeze(1) - torch.logsumexp(s, dim=-1))


def test_module_rejects_bad_arguments(hip):
    layer = make_layer(4, 129, 96, seed=3)
    x = torch.randn(5, 96, device="cuda").half()
    with pytest.raises(hip.GanqHipError):
        layer.pick(x.cpu())
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temperature"):
            layer.pick(x, temperature=bad)
    with pytest.raises(ValueError, match="noise"):
        layer.pick(x, temperature=1.0, noise=torch.zeros(4, 129, device="cuda"))
    with pytest.raises(TypeError, match="noise"):
        layer.pick(x, temperature=1.0, noise=torch.zeros(5, 129, device="cuda", dtype=torch.float16))
    assert layer.pick(x[:0])[0].shape == (0,)


# ---- the model
from test_hip_head_nll import tiny_model  # noqa: E402,F401  (the quantized tests/golden/tiny_lm fixture of the nll tests)


def test_causal_lm_next_token_against_the_logits(tiny_model):  # noqa: F811
    from ganq_amd.models import causal_lm_next_token

    model, ids, seq = tiny_model
    batch = ids[: 4 * seq].reshape(4, seq)
    with torch.no_grad():
        logits = model(batch).logits[:, -1].float()
        hidden = model.base_model(batch)[0]
    token, logprob, outputs = causal_lm_next_token(model, batch)
    assert token.shape == logprob.shape == (4,) and token.dtype == torch.int64 and logprob.grad_fn is None
    assert torch.equal(outputs[0], hidden), "the base model's outputs are handed back"
    bound = 2 * 2.0 ** -11 * float(logits.abs().max())
    top2 = logits.topk(2, dim=-1).values
    sure = (top2[:, 0] - top2[:, 1]) > bound
    want = logits.gather(1, token.unsqueeze(1)).squeeze(1) - torch.logsumexp(logits, dim=-1)
    err = float((logprob - want).abs().max())
    print(f"causal_lm_next_token: {int(sure.sum())} of 4 rows sure, max logprob difference {err:.3g}, bound {bound:.3g}")
    assert torch.equal(token[sure], logits.argmax(-1)[sure]) and bool(sure.any()) and err <= bound
    g = torch.Generator(device="cuda").manual_seed(1)
    t1, lp1, _ = causal_lm_next_token(model, batch, temperature=1.0, generator=g)
    g = torch.Generator(device="cuda").manual_seed(1)
    t2, lp2, _ = causal_lm_next_token(model, batch, temperature=1.0, generator=g)
    assert torch.equal(t1, t2) and torch.equal(lp1, lp2) and bool((lp1 <= 0).all())


def test_causal_lm_next_token_refuses_what_it_cannot_serve(tiny_model):  # noqa: F811
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_tiny_lm as tiny
    from ganq_amd.models import causal_lm_next_token

    model, ids, seq = tiny_model
    batch = ids[:seq].reshape(1, seq)
    plain = tiny.load_model(torch.float16).cuda().eval()
    with pytest.raises(TypeError, match="GanqHipQuantLinear"):
        causal_lm_next_token(plain, batch)
    model.config.final_logit_softcapping = 30.0
    try:
        with pytest.raises(NotImplementedError, match="final_logit_softcapping"):
            causal_lm_next_token(model, batch)
    finally:
        del model.config.final_logit_softcapping
