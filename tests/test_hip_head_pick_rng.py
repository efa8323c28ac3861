"""The sampled pick with the noise drawn inside the head kernel (csrc/lut_head_pick.hip: ganq_lut_head_pick_seeded,
ganq_lut_head_pick_noise) on the MI355X through every layer: the C ABI in guarded buffers against the numpy model
(tests/head_pick_rng_model.py: its own Philox4x32-10, fp64 logs), GanqHipQuantLinear.pick(rng=) fused and composed, a captured
decode step, and causal_lm_next_token.

Bounds.  E, E1 and the bound of lse are those of tests/test_hip_head_pick.py (its docstring derives them), with the noise taking the
part the caller's noise takes there.  The device noise is within Eg = 2^-21 (1 + max |g|) of the model's fp64 noise
(tests/head_pick_rng_model.py), so the chosen z is within 2 (E1 + Eg) of the fp64 maximum and on a row whose fp64 gap exceeds that
the token IS the model's; score carries no noise and keeps E1.  The seeds and offsets are fixed in advance (crc32 of the case id);
tests/test_head_pick_rng_model.py checks without a GPU that at least 90 % of every case's rows are decisive.
Measured on the MI355X: every raw word the model's; the noise at most 0.22 of Eg from the fp64 noise (0.29 of the elementwise
2^-21 (1 + |g|)); every row decisive but one of the 3 x 4096 distribution rows, and no row with another token than the model's; the device chi-squares 9.34, 6.26
and 8.79, exactly the model's."""
import copy
import functools
import pickle

import numpy as np
import pytest
import torch

import head_pick_model as hm
import head_pick_rng_model as rm
import lut_arena as la
from test_hip_head_nll import make_layer
from test_hip_head_pick import run_abi

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TOKEN_PREFILL = -7
WORD_PREFILL = 0x5A5A5A5A
MASK64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def hip():
    from ganq_amd import _lib

    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.selftest()
    return _lib


def signed(v):
    return v - (1 << 64) if v >= (1 << 63) else v


def state_tensor(seed, offset):
    return torch.tensor([signed(seed), signed(offset)], dtype=torch.int64)


gaussian_case = functools.lru_cache(maxsize=None)(rm.gaussian_case)  # computed once, shared, never changed


# ---- the C ABI in guarded buffers
def run_noise(hip, seed, offset, M, m, with_words=True):
    """ganq_lut_head_pick_noise inside an Arena -> (noise fp32 [M, m], words uint32 [M, m] or None); the state must stay"""
    specs = [("rng", torch.int64, (2,), state_tensor(seed, offset), False), ("noise", torch.float32, (M, m), None, True)]
    if with_words:
        specs.append(("words", torch.int32, (M, m), None, False))
    arena = la.Arena(specs)
    t = arena.t
    t["noise"].fill_(float("nan"))
    if with_words:
        t["words"].fill_(WORD_PREFILL)
    arena.snapshot(("noise", "words") if with_words else ("noise",))
    hip._call("ganq_lut_head_pick_noise", tuple(t.values()), t["rng"].data_ptr(), M, m, t["noise"].data_ptr(),
              t["words"].data_ptr() if with_words else None, hip._ST)
    torch.cuda.synchronize()
    arena.assert_untouched("ganq_lut_head_pick_noise")
    noise = t["noise"].cpu().numpy()
    assert not np.isnan(noise).any(), "noise: elements never written (or NaN)"
    return noise, (t["words"].cpu().numpy().view(np.uint32) if with_words else None)


def run_seeded(hip, inp, bits, dtype, seed, offset, inv_t, advance):
    """ganq_lut_head_pick_seeded on `inp` (numpy, tests/lut_arena.py) inside an Arena: a workspace of EXACTLY the sizer's bytes,
    outputs pre-filled between guards; with advance=0 the state belongs to the bytes that must not change
    -> ((token, score, lse, logprob) numpy, (seed, offset) after the call, device tensors)"""
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
             ("rng", torch.int64, (2,), state_tensor(seed, offset), False),
             ("qweight", torch.int32, tuple(qw.shape), qw, False), ("lut", dt, (m, V), as_dt(inp["lut"]), True)]
    if inp["bias"] is not None:
        specs.append(("bias", dt, (m,), as_dt(inp["bias"]), True))
    arena = la.Arena(specs)
    t = arena.t
    outs = ("token", "score", "lse", "logprob")
    t["token"].fill_(TOKEN_PREFILL)
    for name in outs[1:]:
        t[name].fill_(float("nan"))
    arena.snapshot(outs + ("ws",) + (("rng",) if advance else ()))
    p = {k: v.data_ptr() for k, v in t.items()}
    hip._call("ganq_lut_head_pick_seeded", tuple(t.values()), p["x"], p["qweight"], p["lut"], p.get("bias"), p["rng"], int(advance),
              float(inv_t), 0 if dtype == "fp16" else 1, M, m, n, bits, p["token"], p["score"], p["lse"], p["logprob"], p["ws"], nbytes,
              hip._ST)
    torch.cuda.synchronize()
    arena.assert_untouched("ganq_lut_head_pick_seeded")
    for name in outs[1:]:
        assert not bool(torch.isnan(t[name]).any()), f"{name}: rows never written (or NaN)"
    assert bool(((t["token"] >= 0) & (t["token"] < m)).all()), "token: rows never written, or a padding feature chosen"
    after = tuple(int(v) & MASK64 for v in t["rng"].cpu().tolist())
    dev = dict(t)
    dev["arena"] = arena
    return tuple(t[name].cpu().numpy() for name in outs), after, dev


def check_model(got, ref, m, inv_t, what):
    """the seeded pick against the fp64 model: score and lse within the bounds of tests/test_hip_head_pick.py::check, the chosen z
    within 2 (E1 + Eg) of the fp64 maximum, the token the model's on every decisive row"""
    token, score, lse, logprob = got
    rows = np.arange(token.shape[0])
    E, E1, Eg = ref["E"], ref["E1"], ref["Eg"]
    second = (hm.blocks_of(m) + 192) * U * np.maximum(1.0, np.abs(ref["lse"]))
    e_score = np.abs(score.astype(np.float64) - ref["s"][rows, token])
    e_lse = np.abs(lse.astype(np.float64) - ref["lse"])
    short = ref["z"].max(axis=1) - ref["z"][rows, token]
    decisive = ref["decisive"]
    print(f"{what}: max |score - ref| / E1 {float((e_score / np.maximum(E1, 1e-300)).max()):.3g}; max |lse - ref| / bound "
          f"{float((e_lse / (E * inv_t + second)).max()):.3g}; max (max z - z[token]) / 2 (E1 + Eg) {float((short / (2 * (E1 + Eg))).max()):.3g}; "
          f"decisive rows {int(decisive.sum())} of {decisive.size}, of them wrong {int((token != ref['token'])[decisive].sum())}")
    assert (e_score <= E1).all(), what
    assert (e_lse <= E * inv_t + second).all(), what
    assert (short <= 2 * (E1 + Eg)).all(), what
    assert np.array_equal(token[decisive], ref["token"][decisive]), what
    assert decisive.mean() >= 0.9, what
    assert np.array_equal(logprob, score - lse), f"{what}: logprob is not score - lse in fp32"


@pytest.mark.parametrize("m", [1, 129, 300])
@pytest.mark.parametrize("M", [1, 5, 65])
def test_noise_entry_against_the_model(hip, M, m):
    """the raw words are the model's; the noise within Eg of the model's fp64 noise, element by element"""
    seed = 0x9E3779B97F4A7C15
    for offset in rm.OFFSETS:
        noise, words = run_noise(hip, seed, offset, M, m)
        want = rm.words(seed, offset, M, m)
        assert np.array_equal(words, want), f"offset {offset}: {int((words != want).sum())} of {words.size} words differ"
        g = rm.gumbel_from_words(want)
        err = np.abs(noise.astype(np.float64) - g)
        print(f"{M}x{m} offset {offset}: max |g - g64| / Eg {float(err.max() / rm.noise_bound(g)):.3g}, elementwise against "
              f"2^-21 (1 + |g|) {float((err / (2.0 ** -21 * (1 + np.abs(g)))).max()):.3g}")
        assert (err <= rm.noise_bound(g)).all()
        only, _ = run_noise(hip, seed, offset, M, m, with_words=False)
        assert np.array_equal(only, noise), "the noise depends on whether the words are asked for"


def seeded_and_fed(hip, case, inp, seed, offset):
    """the seeded call, and the existing entry fed the noise entry's output for the same state"""
    bits, dtype, M, m, n, _, _, inv_t = case
    got, after, dev = run_seeded(hip, inp, bits, dtype, seed, offset, inv_t, advance=1)
    assert after == (seed, (offset + 1) & MASK64)
    noise, _ = run_noise(hip, seed, offset, M, m, with_words=False)
    fed, _ = run_abi(hip, inp, bits, dtype, noise, inv_t)
    for name, a, b in zip(("token", "score", "lse", "logprob"), got, fed):
        assert np.array_equal(a, b), f"{name}: the seeded pick differs from ganq_lut_head_pick on the noise entry's output"
    return got, dev


@pytest.mark.parametrize("case", rm.CASES, ids=hm.case_id)
def test_seeded_pick(hip, case):
    """bit for bit ganq_lut_head_pick fed ganq_lut_head_pick_noise's output (this pins the draw inside the tile kernel to the tested
    noise entry); against the fp64 model with its own Philox; through the public wrapper"""
    bits, dtype, M, m, n, _, _, inv_t = case
    inp, g, ref, seed, offset = gaussian_case(case)
    got, dev = seeded_and_fed(hip, case, inp, seed, offset)
    check_model(got, ref, m, inv_t, hm.case_id(case))
    state = state_tensor(seed, offset).cuda()
    wrapped = hip.lut_head_pick_seeded(dev["x"], dev["qweight"], dev["lut"], dev.get("bias"), bits, state, inv_t, advance=False)
    for a, b in zip(got, wrapped):
        assert np.array_equal(a, b.cpu().numpy()), "the public wrapper and the C ABI call on the same tensors differ"
    assert state.cpu().tolist() == state_tensor(seed, offset).tolist()


def test_large_vocabulary(hip):
    """m = 128256: 1002 feature blocks, feature indices beyond 2^16 in the counter"""
    case = rm.LARGE_VOCAB
    inp, g, ref, seed, offset = gaussian_case(case)
    got, _ = seeded_and_fed(hip, case, inp, seed, offset)
    check_model(got, ref, case[3], case[7], "large vocabulary")


def test_state(hip):
    """advance=1 leaves the seed and sets the offset to offset + 1, the carry from 2^32 - 1 to 2^32 included; advance=0 leaves all 16
    bytes (run_seeded compares them with every other byte of the arena); the same state gives the same bytes, consecutive offsets
    different noise"""
    bits, dtype, M, m, n, inv_t = 4, "fp16", 65, 300, 96, 1 / 0.7
    inp = la.gaussian(bits, M, m, n, "plain", 41)
    inp["x"] *= 2.0
    seed = 0xFEDCBA9876543210  # (the top bit set: the state is unsigned)
    for offset in (0, 7, (1 << 32) - 1, 1 << 32, MASK64):
        _, after, _ = run_seeded(hip, inp, bits, dtype, seed, offset, inv_t, advance=1)
        assert after == (seed, (offset + 1) & MASK64), (offset, after)
    a, after, _ = run_seeded(hip, inp, bits, dtype, seed, 7, inv_t, advance=0)
    assert after == (seed, 7)
    b, _, _ = run_seeded(hip, inp, bits, dtype, seed, 7, inv_t, advance=1)
    c, _, _ = run_seeded(hip, inp, bits, dtype, seed, 8, inv_t, advance=0)
    for x, y in zip(a, b):
        assert np.array_equal(x, y), "two calls at the same state differ (or advance changes the call's own result)"
    assert not np.array_equal(a[0], c[0]), "consecutive offsets picked the same 65 tokens"
    assert not np.array_equal(run_noise(hip, seed, 7, M, m, False)[0], run_noise(hip, seed, 8, M, m, False)[0])
    # the carry: the noise at 2^32 - 1 and at 2^32 is the model's on both sides
    for offset in ((1 << 32) - 1, 1 << 32):
        assert np.array_equal(run_noise(hip, seed, offset, 5, 129)[1], rm.words(seed, offset, 5, 129))


@pytest.mark.parametrize("case", hm.PADDING_CASES, ids=hm.case_id)
def test_padding_features_are_invisible(hip, case):
    """every real logit <= -40 (bias -48) and every real z below the smallest value the noise takes: a padding feature of the last
    block that took part -- a logit of 0 plus whatever it drew -- would win the pick and lift lse by more than 30.  The result is
    the model's, which knows no feature past m."""
    bits, dtype, M, m, n = case
    inp, g, ref, seed, offset = rm.padding_case(case)
    assert float(ref["lse"].max()) < -40 + np.log(m) and float(ref["z"].max()) < rm.G_MIN
    got, _, _ = run_seeded(hip, inp, bits, dtype, seed, offset, 1.0, advance=0)
    check_model(got, ref, m, 1.0, "padding " + hm.case_id(case))
    assert float(np.abs(got[2] - ref["lse"]).max()) < 1e-3 and (got[0] < m).all() and (got[1] < -40).all()


@pytest.mark.parametrize("seed", rm.DIST_SEEDS)
def test_distribution_on_the_device(hip, seed):
    """the m = 8, 4096-row case of the model test (n = 32, 64 tile launches): the tokens are the model's on decisive rows and their
    chi-square against softmax stays below the 0.999 quantile at 7 degrees of freedom"""
    bits, dtype, M, m, n, _, _, inv_t = rm.DIST_CASE
    inp, logits = rm.dist_inputs()
    ref = rm.reference(inp, dtype, inv_t, rm.noise(seed, 0, M, m))
    got, after, _ = run_seeded(hip, inp, bits, dtype, seed, 0, inv_t, advance=1)
    assert after == (seed, 1)
    check_model(got, ref, m, inv_t, f"distribution seed {seed}")
    chi2 = rm.chi_square(got[0], logits)
    print(f"seed {seed}: device chi-square {chi2:.3f}, model {rm.chi_square(ref['token'], logits):.3f}, bound {rm.CHI2_7_999}")
    assert chi2 < rm.CHI2_7_999


def test_c_abi_rejects_bad_arguments(hip):
    """everything ganq_lut_head_pick rejects, and a null or misaligned state; a refused call writes nothing"""
    lib = hip.lib()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    need = lib.ganq_lut_head_pick_workspace_bytes(65, 300, 96, 4)
    assert need <= buf.numel()

    def args(**kw):
        return (kw.get("x", p), p, p, None, kw.get("rng", p), kw.get("advance", 1), kw.get("inv_t", 1.0), kw.get("dtype", 0), kw.get("M", 65),
                kw.get("m", 300), kw.get("n", 96), kw.get("bits", 4), kw.get("token", p), p, p, p, p, kw.get("ws", need), None)

    before = buf.clone()
    call = lib.ganq_lut_head_pick_seeded
    assert call(*args(ws=need - 1)) == -4
    assert call(*args(bits=5)) == -2 and call(*args(n=48)) == -2 and call(*args(dtype=2)) == -2
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call(*args(inv_t=bad)) == -2, bad
    assert call(*args(M=-1)) == -1
    assert call(*args(M=1 << 24, n=4096, ws=1 << 40)) == -1  # beyond the 2 GB window of the 32-bit offsets
    assert call(*args(x=None)) == -3 and call(*args(token=None)) == -3
    assert call(*args(rng=None)) == -3 and call(*args(rng=p + 4)) == -2
    assert call(*args(M=0, rng=None)) == 0  # (no rows: a no-op, as ganq_lut_head_pick)
    noise = lib.ganq_lut_head_pick_noise
    assert noise(None, 5, 8, p, None, None) == -3 and noise(p, 5, 8, None, None, None) == -3
    assert noise(p + 4, 5, 8, p, None, None) == -2 and noise(p, -1, 8, p, None, None) == -1
    torch.cuda.synchronize()
    assert torch.equal(buf, before), "a refused call wrote something"


# ---- the module
def module_reference(layer, x, inv_t, g):
    """rm.reference for a layer's own tensors: its dequantized weight as a codebook of in_features entries indexed by the column"""
    W = layer.dequantize_weight().detach().float().cpu().numpy()
    m, n = W.shape
    inp = dict(x=x.detach().float().cpu().numpy(), Q=np.broadcast_to(np.arange(n), (m, n)), lut=W,
               bias=None if layer.bias is None else layer.bias.detach().float().cpu().numpy())
    return rm.reference(inp, "fp16", inv_t, g)


def test_capture(hip):
    """one pick(x, 0.7, rng=rng) captured in a HIP graph and replayed three times: replay k is bit for bit an eager call at
    PickRng(seed, offset0 + k), the three samples are not all equal (nor are the model's), and the state ends at offset0 + 3"""
    from ganq_amd.nn_modules.qlinear.ganq_hip import PickRng

    m, n, M, seed, offset0 = 300, 160, 65, 0xC0FFEE1234567, (1 << 32) - 2
    layer = make_layer(4, m, n, seed=5, scale=0.1)
    x = torch.randn(M, n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(50)).half()
    model = [module_reference(layer, x, 1 / 0.7, rm.noise(seed, offset0 + k, M, m)) for k in range(3)]
    assert all(not np.array_equal(model[a]["token"], model[b]["token"]) for a, b in ((0, 1), (1, 2), (0, 2)))
    eager = [layer.pick(x, 0.7, rng=PickRng(seed, offset0 + k)) for k in range(3)]
    torch.cuda.synchronize()
    rng = PickRng(seed, offset0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        layer.pick(x, 0.7, rng=rng)  # (warm-up: advances the state)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            static_out = layer.pick(x, 0.7, rng=rng)
    torch.cuda.current_stream().wait_stream(side)
    rng.state.copy_(PickRng(seed, offset0).state)  # nothing ran during the capture: back to offset0 for the replays
    replays = []
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        replays.append(tuple(t.clone() for t in static_out))
        assert torch.equal(replays[k][0], eager[k][0]) and torch.equal(replays[k][1], eager[k][1]), f"replay {k} differs from a fresh call"
        d = model[k]["decisive"]
        assert np.array_equal(replays[k][0].cpu().numpy()[d], model[k]["token"][d]) and d.mean() >= 0.9
    assert not (torch.equal(replays[0][0], replays[1][0]) and torch.equal(replays[1][0], replays[2][0])), "every replay drew the same sample"
    assert (rng.seed, rng.offset) == (seed, offset0 + 3)


def test_module_fused_and_composition_draw_the_same_noise(hip, monkeypatch):
    """pick(rng=) through the kernel and through the composition (fused=False): the composition's noise buffer IS the noise entry's
    output for the state; both advance the state by one; the tokens agree wherever the composition's gap between its two best
    z exceeds what its rounded logits and the kernel's fp32 logits can differ by (tests/test_hip_head_pick.py::
    test_module_fused_against_composition: 2 eps max |logit| + 4 E, scaled by inv_t)"""
    import ganq_amd.nn_modules.qlinear.ganq_hip as gh

    m, n, M, T = 300, 160, 130, 0.7
    layer = make_layer(4, m, n, seed=1, scale=0.1)
    x = torch.randn(2, M // 2, n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(51)).half()
    monkeypatch.setattr(gh, "NLL_CHUNK_BYTES", 64 * m * 6)  # 64-row chunks: three of them
    drawn = []
    real = hip.lut_head_pick_noise
    monkeypatch.setattr(gh._lib, "lut_head_pick_noise", lambda *a, **k: drawn.append(real(*a, **k)) or drawn[-1])
    rng_f, rng_c = gh.PickRng(77, 5), gh.PickRng(77, 5)
    fused = layer.pick(x, T, rng=rng_f)
    assert not drawn, "the fused path formed a noise tensor"
    comp = layer.pick(x, T, rng=rng_c, fused=False)
    assert len(drawn) == 1 and torch.equal(drawn[0], real(gh.PickRng(77, 5).state, M, m))
    assert (rng_f.seed, rng_f.offset) == (77, 6) and (rng_c.seed, rng_c.offset) == (77, 6)
    assert fused[0].shape == comp[0].shape == (2, M // 2) and fused[1].dtype == torch.float32
    x2 = x.reshape(-1, n)
    want = hip.lut_head_pick(x2, layer.qweight, layer.lut, layer.bias, 4, drawn[0], 1.0 / T)
    assert torch.equal(fused[0].reshape(-1), want[0]) and torch.equal(fused[1].reshape(-1), want[3])
    with torch.no_grad():
        s = torch.cat([layer(xc) for xc in x2.split(64)]).float() * (1.0 / T)
    assert torch.equal(comp[0].reshape(-1), (s + drawn[0]).argmax(-1))
    W = layer.dequantize_weight()
    E = n * 2.0 ** -23 * float((x2.double().abs() @ W.double().abs().T).max())
    top2 = (s + drawn[0]).topk(2, dim=-1).values
    sure = (top2[:, 0] - top2[:, 1]) > (2 * 2.0 ** -11 * float(s.abs().max()) * T + 4 * E) / T + 8 * U * float((s + drawn[0]).abs().max())
    same = fused[0].reshape(-1) == comp[0].reshape(-1)
    print(f"fused vs composition with rng: {int(sure.sum())} of {M} rows sure, {int((~same).sum())} tokens differ")
    assert bool(same[sure].all()) and float(sure.float().mean()) >= 0.9


@pytest.mark.parametrize("kind", ["outliers", "adapter"])
def test_module_composition_layers_take_rng(hip, kind):
    """a layer with outliers and a layer with an adapter take the composition with rng: its own steps on the noise entry's output,
    the state advanced by one"""
    from ganq_amd.nn_modules.qlinear.ganq_hip import PickRng

    m, n, M = 300, 160, 70
    layer = make_layer(4, m, n, seed=2, outliers=kind == "outliers", rank=16 if kind == "adapter" else 0, scale=0.1)
    x = torch.randn(M, n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(52)).half()
    rng = PickRng(9, (1 << 32) - 1)
    token, logprob = layer.pick(x, temperature=0.5, rng=rng)
    assert (rng.seed, rng.offset) == (9, 1 << 32)
    noise = hip.lut_head_pick_noise(PickRng(9, (1 << 32) - 1).state, M, m)
    with torch.no_grad():
        s = layer(x).float() * 2.0
    assert torch.equal(token, (s + noise).argmax(-1))
    assert torch.equal(logprob, s.gather(1, token.unsqueeze(1)).squeeze(1) - torch.logsumexp(s, dim=-1))
    with pytest.raises(ValueError, match="fused=True"):
        layer.pick(x, temperature=0.5, rng=rng, fused=True)
    assert rng.offset == 1 << 32


def test_module_rng_arguments(hip):
    from ganq_amd.nn_modules.qlinear.ganq_hip import PickRng

    layer = make_layer(4, 129, 96, seed=3)
    x = torch.randn(5, 96, device="cuda", generator=torch.Generator(device="cuda").manual_seed(53)).half()
    rng = PickRng((1 << 64) - 1, 3)
    assert rng.state.dtype == torch.int64 and tuple(rng.state.shape) == (2,) and rng.state.is_cuda
    assert (rng.seed, rng.offset) == ((1 << 64) - 1, 3)
    # temperature 0 ignores rng and leaves it untouched
    greedy = layer.pick(x, rng=rng)
    assert torch.equal(greedy[0], layer.pick(x)[0]) and torch.equal(greedy[1], layer.pick(x)[1]) and rng.offset == 3
    assert layer.pick(x[:0], 1.0, rng=rng)[0].shape == (0,) and rng.offset == 3
    with pytest.raises(ValueError, match="rng"):
        layer.pick(x, 1.0, rng=rng, generator=torch.Generator(device="cuda"))
    with pytest.raises(ValueError, match="rng"):
        layer.pick(x, 1.0, rng=rng, noise=torch.zeros(5, 129, device="cuda"))
    with pytest.raises(TypeError, match="PickRng"):
        layer.pick(x, 1.0, rng=torch.Generator(device="cuda"))
    with pytest.raises(ValueError, match="GPU"):
        PickRng(1, device="cpu")
    with pytest.raises(ValueError, match="2\\^64"):
        PickRng(-1)
    stray = PickRng(1)
    stray.state = stray.state.cpu()  # a state that left the device of x
    with pytest.raises(ValueError, match="lives on"):
        layer.pick(x, 1.0, rng=stray)
    assert rng.offset == 3, "a refused call advanced the state"
    # copies own their tensor; pickling keeps the two integers
    a = layer.pick(x, 1.0, rng=copy.deepcopy(rng))
    twin, shallow, back = copy.deepcopy(rng), copy.copy(rng), pickle.loads(pickle.dumps(rng))
    for other in (twin, shallow, back):
        assert other.state.data_ptr() != rng.state.data_ptr() and (other.seed, other.offset) == (rng.seed, 3)
        b = layer.pick(x, 1.0, rng=other)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and other.offset == 4
    assert rng.offset == 3


# ---- the model
from test_hip_head_nll import tiny_model  # noqa: E402,F401  (the quantized tests/golden/tiny_lm fixture of the nll tests)


def test_causal_lm_next_token_with_rng(tiny_model):  # noqa: F811
    from ganq_amd.models import causal_lm_next_token
    from ganq_amd.nn_modules.qlinear.ganq_hip import PickRng

    model, ids, seq = tiny_model
    batch = ids[: 4 * seq].reshape(4, seq)
    rng = PickRng(2024, 11)
    token, logprob, outputs = causal_lm_next_token(model, batch, 0.8, rng=rng)
    assert (rng.seed, rng.offset) == (2024, 12)
    head = model.get_output_embeddings()
    with torch.no_grad():
        hidden = model.base_model(batch)[0]
    want = head.pick(hidden[:, -1, :], 0.8, rng=PickRng(2024, 11))
    assert torch.equal(outputs[0], hidden) and torch.equal(token, want[0]) and torch.equal(logprob, want[1])
    assert token.shape == (4,) and bool((logprob <= 0).all())
    greedy = causal_lm_next_token(model, batch, rng=rng)
    assert torch.equal(greedy[0], causal_lm_next_token(model, batch)[0]) and rng.offset == 12
