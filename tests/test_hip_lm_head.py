"""GPU tests of the head stage of quantize_model (`QuantizeConfig.lm_head`) and of the two ways a tied input embedding is handled
(`ganq_tied_embedding` = "untie" / "share"): two-layer OPT and Llama models, vocabulary 323 (odd), hidden 64, fp16, tied and untied
heads, K = 2; and one run of a head-sized layer (128256 rows) through quantizer, packed forward and embedding lookup."""
import copy
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import lut_arena
from conftest import rel_fro

pytestmark = pytest.mark.gpu

VOCAB = 323
KINDS = ("opt", "llama")
N_LIN = {"opt": 12, "llama": 14}
EMB_NAME = {"opt": "model.decoder.embed_tokens", "llama": "model.embed_tokens"}
# LUT forward against the forward on the dequantised weights: the tolerance of tests/test_hip_models.py::test_quantize_model_save_load_ppl
LOGIT_TOL = dict(rtol=2e-2, atol=2e-2)


def tiny(kind, tied, dtype=torch.float16):
    import transformers

    torch.manual_seed(0)
    if kind == "opt":
        cfg = transformers.OPTConfig(vocab_size=VOCAB, hidden_size=64, ffn_dim=128, num_hidden_layers=2, num_attention_heads=4,
                                     max_position_embeddings=128, word_embed_proj_dim=64, tie_word_embeddings=tied)
        model = transformers.OPTForCausalLM(cfg)
    else:
        cfg = transformers.LlamaConfig(vocab_size=VOCAB, hidden_size=64, intermediate_size=128, num_hidden_layers=2,
                                       num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=128,
                                       tie_word_embeddings=tied)
        model = transformers.LlamaForCausalLM(cfg)
    model = model.to(dtype).cuda().eval()
    assert (model.get_output_embeddings().weight is model.get_input_embeddings().weight) == tied
    return model


def calibration():
    g = torch.Generator().manual_seed(1)
    return [torch.randint(0, VOCAB, (2, 64), generator=g) for _ in range(3)]


def probe_ids():
    return torch.randint(0, VOCAB, (1, 64), generator=torch.Generator().manual_seed(5)).cuda()


def logits_of(model, ids):
    """inference forward; FORMAT.FAKE models hold weights written under inference_mode, which autograd refuses to save"""
    with torch.no_grad():
        return model(ids).logits


def assert_same_dequantised(fake_w, head):
    """the FORMAT.FAKE weight against the packed head's dequantize_weight(): bit-equal wherever no outlier sits.  At an outlier the
    quantizer returns fp16(t + v) of the fp32 codebook value t and outlier v, the packed layer fp16(fp16(t) + fp16(v)) (ganq.py
    `index_put_` / `dequantize_weight`): the inner roundings move the sum by at most 2^-11 (|t| + |v|), each outer rounding its
    result by at most 2^-11 of itself (2^-25 where subnormal)."""
    from ganq_amd import _lib

    W = head.dequantize_weight()
    if not head.outliers:
        assert torch.equal(fake_w, W)
        return
    Wq = _lib.lut_dequant(head.qweight, head.lut, head.in_features, head.bits)
    Ws = head._sparse_dense(Wq.dtype)
    at_outlier = Ws != 0
    assert torch.equal(fake_w[~at_outlier], W[~at_outlier])
    diff = (fake_w.double() - W.double()).abs()
    bound = 2.0 ** -11 * (1 + 2.0 ** -10) * (Wq.double().abs() + Ws.double().abs() + fake_w.double().abs() + W.double().abs()) \
        + 2.0 ** -24
    print(f"fake vs packed at {int(at_outlier.sum())} outliers: {int((diff > 0).sum())} differ, max |difference| = "
          f"{float(diff.max()):.3e}, smallest bound there = {float(bound[at_outlier].min()):.3e}")
    assert bool((diff <= bound).all())


def make_qcfg(**kw):
    from ganq_amd.quantization import QuantizeConfig

    base = dict(bits=4, act_sort="asc", l_damp_style="ganq", dead="mean", ganq_iterations=2)
    base.update(kw)
    return QuantizeConfig(**base)


@functools.lru_cache(maxsize=None)
def quantized(kind, tied, lm_head=True, mode="untie", fmt="ganq_lut", dynamic=None, outlier_ratio=0.0):
    """one quantize_model run, shared by the tests that read it (they do not modify it) -> dict(model, proc, table, head_weight,
    head_inputs): the original embedding table / head weight and what the head's statistics hook was fed, batch by batch"""
    from ganq_amd.looper.gptq_processor import GPTQProcessor
    from ganq_amd.models import quantize_model

    class Recording(GPTQProcessor):
        head_inputs = None

        def preprocess_fwd_hook(self, name):
            hook = super().preprocess_fwd_hook(name)
            if name != "lm_head":
                return hook
            self.head_inputs = []

            def record(mod, inp, out):
                self.head_inputs.append(inp[0].detach().clone())
                hook(mod, inp, out)

            return record

    model = tiny(kind, tied)
    table = model.get_input_embeddings().weight.detach().clone()
    head_weight = model.get_output_embeddings().weight.detach().clone()
    qcfg = make_qcfg(lm_head=lm_head, ganq_tied_embedding=mode, format=fmt, dynamic=json.loads(dynamic) if dynamic else None,
                     ganq_outlier_ratio=outlier_ratio)
    proc = Recording(qcfg)
    with torch.no_grad():
        quantize_model(model, calibration(), qcfg, processor=proc)
    return dict(model=model, proc=proc, table=table, head_weight=head_weight, head_inputs=proc.head_inputs, qcfg=qcfg)


def packed_layers(model):
    from ganq_amd.nn_modules.qlinear.ganq_hip import GanqHipQuantLinear

    return {n: m for n, m in model.named_modules() if isinstance(m, GanqHipQuantLinear)}


@pytest.mark.parametrize("tied", [True, False], ids=["tied", "untied"])
@pytest.mark.parametrize("kind", KINDS)
def test_head_is_packed_and_the_body_is_unchanged(kind, tied):
    from ganq_amd.nn_modules.qlinear.ganq_hip import GanqHipQuantLinear

    run = quantized(kind, tied)
    model, proc = run["model"], run["proc"]
    head = model.get_output_embeddings()
    assert isinstance(head, GanqHipQuantLinear)  # (the parent leaves an nn.Linear here)
    assert (head.out_features, head.in_features, head.bits) == (VOCAB, 64, 4)
    assert len(proc.results()) == N_LIN[kind] + 1 and "lm_head" in proc.results()
    assert proc.log[-1]["module"] == "lm_head" and proc.log[-1]["layer"] == 2 and len(proc.log) == N_LIN[kind] + 1
    assert model.config.tie_word_embeddings is False
    body = packed_layers(quantized(kind, tied, lm_head=False)["model"])
    assert len(body) == N_LIN[kind] and "lm_head" not in body
    mine = packed_layers(model)
    assert set(mine) == set(body) | {"lm_head"}
    for name, mod in body.items():
        assert torch.equal(mine[name].qweight, mod.qweight) and torch.equal(mine[name].lut, mod.lut), name
    logits = logits_of(model, probe_ids())
    assert logits.shape == (1, 64, VOCAB) and bool(torch.isfinite(logits).all())


@pytest.mark.parametrize("kind", KINDS)
def test_head_equals_a_standalone_task_on_the_same_inputs(kind):
    """the head stage adds nothing of its own to the quantizer: a GANQ task of the existing quantizer on the original head weight,
    fed the recorded `pre_head` outputs in the same batches and order, returns the same indices and codebook, bit for bit"""
    from ganq_amd import _lib
    from ganq_amd.quantization.ganq import GANQ

    run = quantized(kind, True)
    head = run["model"].get_output_embeddings()
    inputs = run["head_inputs"]
    assert len(inputs) == len(calibration()) and all(tuple(x.shape) == (2, 64, 64) and x.dtype == torch.float16 for x in inputs)
    lin = nn.Linear(64, VOCAB, bias=False).half().cuda()
    lin.weight.data.copy_(run["head_weight"])
    task = GANQ(module=lin, qcfg=copy.deepcopy(run["qcfg"]))
    task.quantizer.configure(perchannel=True)
    for x in inputs:
        task.add_batch(x, None)
    task.end_of_calibration()
    with torch.no_grad():
        task.quantize()
    assert torch.equal(_lib.pack_indices(task.ganq_indices.to(torch.uint8).contiguous(), 4), head.qweight)
    assert torch.equal(task.ganq_codebook.to(torch.float16), head.lut)


@pytest.mark.parametrize("kind", KINDS)
def test_untie_keeps_the_original_table(kind):
    run = quantized(kind, True)
    model = run["model"]
    emb = model.get_input_embeddings()
    assert type(emb) is nn.Embedding and emb.weight.dtype == torch.float16
    assert torch.equal(emb.weight, run["table"])
    assert model.config.tie_word_embeddings is False
    model.tie_weights()  # must not hang a `weight` onto the packed head
    head = model.get_output_embeddings()
    assert "weight" not in dict(head.named_parameters()) and not isinstance(getattr(head, "weight", None), torch.Tensor)
    assert f"{EMB_NAME[kind]}.weight" in model.state_dict()


@pytest.mark.parametrize("kind,outlier_ratio", [("opt", 0.0), ("llama", 0.0), ("llama", 0.01)])
def test_share_serves_the_embedding_from_the_packed_head(kind, outlier_ratio):
    from ganq_amd.nn_modules.qlinear.ganq_hip import GanqHipQuantEmbedding

    run = quantized(kind, True, mode="share", outlier_ratio=outlier_ratio)
    model = run["model"]
    emb, head = model.get_input_embeddings(), model.get_output_embeddings()
    assert isinstance(emb, GanqHipQuantEmbedding) and emb.head is head
    assert bool(head.outliers) == bool(outlier_ratio)
    assert not [k for k in model.state_dict() if k.startswith(EMB_NAME[kind])]
    assert model.config.tie_word_embeddings is False
    W = head.dequantize_weight()
    ids = torch.cat([torch.arange(VOCAB), torch.tensor([0, VOCAB - 1, 7, 7])]).cuda().view(3, 109)
    out = emb(ids)
    assert out.dtype == torch.float16 and out.shape == (3, 109, 64) and out.grad_fn is None
    assert torch.equal(out.view(torch.int16), W[ids].view(torch.int16))
    assert torch.equal(emb(ids.int()), out)
    # the same run in the FORMAT.FAKE view: the embedding's weight IS the dequantised head weight
    fake = quantized(kind, True, mode="share", fmt="fake", outlier_ratio=outlier_ratio)["model"]
    f_emb, f_head = fake.get_input_embeddings(), fake.get_output_embeddings()
    assert type(f_emb) is nn.Embedding and isinstance(f_head, nn.Linear)
    assert f_emb.weight is f_head.weight and fake.config.tie_word_embeddings is False
    assert_same_dequantised(f_head.weight.detach(), head)
    x = probe_ids()
    a, b = logits_of(model, x).float(), logits_of(fake, x).float()
    print(f"[{kind} outliers={outlier_ratio}] share: max |logit difference| LUT vs dequantised = {float((a - b).abs().max()):.3e}")
    assert torch.allclose(a, b, **LOGIT_TOL)
    # format "fake" + "untie": the embedding keeps the original table, the head its dequantised weight
    if not outlier_ratio:
        fu = quantized(kind, True, mode="untie", fmt="fake")
        assert torch.equal(fu["model"].get_input_embeddings().weight, fu["table"])
        assert torch.equal(fu["model"].get_output_embeddings().weight, W)


@pytest.mark.parametrize("mode", ["untie", "share"])
@pytest.mark.parametrize("kind", KINDS)
def test_save_and_load_reproduce_the_logits(kind, mode, tmp_path):
    from safetensors import safe_open

    from ganq_amd.models import load_quantized, save_quantized
    from ganq_amd.nn_modules.qlinear.ganq_hip import GanqHipQuantEmbedding, GanqHipQuantLinear

    run = quantized(kind, True, mode=mode)
    model = run["model"]
    x = probe_ids()
    before = logits_of(model, x)
    path = os.path.join(tmp_path, "ckpt")
    save_quantized(model, path)
    cfg = json.load(open(os.path.join(path, "quantize_config.json")))
    assert cfg["modules"]["lm_head"]["bits"] == 4 and cfg["modules"]["lm_head"]["out_features"] == VOCAB
    with safe_open(os.path.join(path, "model.safetensors"), "pt") as f:
        keys = set(f.keys())
    assert {"lm_head.qweight", "lm_head.lut"} <= keys and "lm_head.weight" not in keys
    if mode == "share":
        assert cfg["tied_embedding"] == {"module": EMB_NAME[kind], "source": "lm_head"}
        assert not [k for k in keys if k.startswith(EMB_NAME[kind])]  # no fp16 table in the checkpoint
    else:
        assert "tied_embedding" not in cfg and f"{EMB_NAME[kind]}.weight" in keys
    fresh = load_quantized(tiny(kind, True), path)  # a freshly built TIED model: load must not re-tie
    assert isinstance(fresh.get_output_embeddings(), GanqHipQuantLinear)
    assert not isinstance(getattr(fresh.get_output_embeddings(), "weight", None), torch.Tensor)
    if mode == "share":
        assert isinstance(fresh.get_input_embeddings(), GanqHipQuantEmbedding)
        assert fresh.get_input_embeddings().head is fresh.get_output_embeddings()
    else:
        assert torch.equal(fresh.get_input_embeddings().weight, run["table"])
    assert fresh.quantize_config.lm_head is True and fresh.quantize_config.ganq_tied_embedding == mode
    assert torch.equal(logits_of(fresh, x), before)
    assert torch.equal(logits_of(model, x), before)


@pytest.mark.parametrize("kind", KINDS)
def test_checkpoint_without_a_quantized_head_loads_as_before(kind, tmp_path):
    from ganq_amd.models import load_quantized, save_quantized

    model = quantized(kind, True, lm_head=False)["model"]
    assert isinstance(model.get_output_embeddings(), nn.Linear) and model.config.tie_word_embeddings is True
    assert model.get_output_embeddings().weight is model.get_input_embeddings().weight
    x = probe_ids()
    path = os.path.join(tmp_path, "ckpt")
    save_quantized(model, path)
    cfg = json.load(open(os.path.join(path, "quantize_config.json")))
    assert "lm_head" not in cfg["modules"] and "tied_embedding" not in cfg
    del cfg["ganq_tied_embedding"]  # as a checkpoint written before the field existed
    json.dump(cfg, open(os.path.join(path, "quantize_config.json"), "w"))
    fresh = load_quantized(tiny(kind, True), path)
    assert isinstance(fresh.get_output_embeddings(), nn.Linear) and fresh.config.tie_word_embeddings is True
    assert fresh.get_output_embeddings().weight is fresh.get_input_embeddings().weight
    assert fresh.quantize_config.ganq_tied_embedding == "untie"
    assert torch.equal(logits_of(fresh, x), logits_of(model, x))


def test_dynamic_overrides_and_skips_the_head():
    from ganq_amd.nn_modules.qlinear.ganq_hip import GanqHipQuantLinear

    run = quantized("llama", True, dynamic=json.dumps({"lm_head": {"bits": 3}}))
    head = run["model"].get_output_embeddings()
    assert isinstance(head, GanqHipQuantLinear) and head.bits == 3 and tuple(head.lut.shape) == (VOCAB, 8)
    assert tuple(head.qweight.shape) == (64 * 3 // 32, VOCAB)
    assert all(m.bits == 4 for n, m in packed_layers(run["model"]).items() if n != "lm_head")
    assert bool(torch.isfinite(logits_of(run["model"], probe_ids())).all())

    run = quantized("llama", True, mode="share", dynamic=json.dumps({"-:lm_head": {}}))
    model = run["model"]
    head, emb = model.get_output_embeddings(), model.get_input_embeddings()
    assert type(head) is nn.Linear and type(emb) is nn.Embedding and head.weight is emb.weight  # untouched, still tied
    assert torch.equal(head.weight, run["table"]) and model.config.tie_word_embeddings is True
    assert len(run["proc"].results()) == N_LIN["llama"] and run["head_inputs"] is None


def test_share_refuses_what_is_not_a_plain_half_table():
    from ganq_amd.models import quantize_model

    class ScaledEmbedding(nn.Embedding):
        def forward(self, ids):
            return super().forward(ids) * 8.0

    model = tiny("llama", True)
    old = model.get_input_embeddings()
    scaled = ScaledEmbedding(VOCAB, 64).half().cuda()
    scaled.weight = old.weight
    model.set_input_embeddings(scaled)
    assert model.get_output_embeddings().weight is model.get_input_embeddings().weight
    with pytest.raises(NotImplementedError, match="ScaledEmbedding"):
        quantize_model(model, calibration(), make_qcfg(lm_head=True, ganq_tied_embedding="share"))
    assert type(model.get_output_embeddings()) is nn.Linear and not packed_layers(model)  # refused before any work

    model = tiny("llama", True, dtype=torch.float32)
    with pytest.raises(NotImplementedError, match="float32"):
        quantize_model(model, calibration(), make_qcfg(lm_head=True, ganq_tied_embedding="share"))
    assert type(model.get_output_embeddings()) is nn.Linear and not packed_layers(model)

    class NotLinearHead(nn.Module):
        def __init__(self, lin):
            super().__init__()
            self.lin = lin

        def forward(self, x):
            return self.lin(x)

    model = tiny("llama", False)
    model.set_output_embeddings(NotLinearHead(model.get_output_embeddings()))
    with pytest.raises(NotImplementedError, match="NotLinearHead"):
        quantize_model(model, calibration(), make_qcfg(lm_head=True))


# ---- a head-sized layer: 128256 rows (Llama-3 vocabulary), the smallest in_features that keeps it to seconds
BIG_M, BIG_N, BIG_K = 128256, 256, 2
TOL_T = 1e-5  # tests/test_hip_configs.py: codebooks within 1e-5 relative Frobenius


def big_rows():
    """64 rows: the first, the last, and those around 65535 / 65536 and the 131071-adjacent tile edges within range"""
    m = BIG_M
    fixed = [0, 1, 15, 16, 63, 64, 32767, 32768, 65519, 65520, 65534, 65535, 65536, 65537, 65551, 65552, 98303, 98304,
             m - 129, m - 128, m - 65, m - 64, m - 33, m - 32, m - 17, m - 16, m - 2, m - 1]
    rng = np.random.default_rng(3)
    extra = [int(r) for r in rng.choice(m, size=200, replace=False) if int(r) not in fixed]
    rows = sorted(fixed + extra[:64 - len(fixed)])
    assert len(rows) == 64 and len(set(rows)) == 64
    return rows


def test_head_sized_layer_quantizer_forward_and_lookup():
    """row indexing at a vocabulary's row count, one run: k-means, S-solve, T-update, loss (64 sampled rows against the CPU oracle
    given the GPU's own H: indices exact, codebooks within 1e-5), the packed forward at M = 1, 16, 64, 300, 1100 on small-integer
    inputs (bit-exact against fp64) and the embedding lookup on 1000 ids over the whole range (bit-exact)."""
    from ganq_amd import _lib
    from ganq_amd.nn_modules.qlinear.ganq_hip import GanqHipQuantEmbedding, GanqHipQuantLinear
    from ganq_amd.quantization.ganq import GANQ
    from oracle import c_oracle

    m, n, K, V = BIG_M, BIG_N, BIG_K, 16
    seen = {}

    class Recording(GANQ):
        def _initialize_codebook_kmeans(self, W, Hinv, num_bits, device):
            T0 = super()._initialize_codebook_kmeans(W, Hinv, num_bits, device)
            seen.update(W=W.clone(), H=self.Xxt_damped.clone(), L=self.L.clone(), T0=T0.clone(), hinv=Hinv.clone())
            return T0

    g = torch.Generator(device="cuda").manual_seed(11)
    lin = nn.Linear(n, m, bias=False).half().cuda()
    lin.weight.data.copy_((0.02 * torch.randn(m, n, device="cuda", generator=g)).half())
    X = (torch.randn(2048, n, device="cuda", generator=g) * (0.1 + torch.rand(n, device="cuda", generator=g))).half()
    qcfg = make_qcfg(ganq_iterations=K)
    task = Recording(module=lin, qcfg=qcfg)
    task.quantizer.configure(perchannel=True)
    for b in range(4):  # 2048 calibration tokens in 4 batches
        task.add_batch(X[512 * b:512 * (b + 1)].view(1, 512, n), None)
    task.end_of_calibration()
    with torch.no_grad():
        task.quantize()
    torch.cuda.synchronize()
    stats = task.ganq_stats
    bk = int(stats["best_k"])
    T = task.ganq_codebook
    # the loop's own outputs in the loop's column order, from the recorded inputs (deterministic: the same bits)
    T_best, Q_last, dists, best_k = _lib.run_layer(seen["W"], seen["H"], seen["L"], seen["T0"], K, alias_q=True)
    assert int(best_k) == bk and torch.equal(T_best, T)
    Q_perm = Q_last
    rows = big_rows()
    ridx = torch.tensor(rows, device="cuda")
    Wr, T0r = seen["W"][ridx].cpu().numpy(), seen["T0"][ridx].cpu().numpy()
    Hn, Ln = seen["H"].cpu().numpy(), seen["L"].cpu().numpy()
    # k-means at these rows: the oracle's weighted 1-D k-means on the same weights (the tolerance smoke() uses)
    hd = seen["hinv"] if seen["hinv"].dim() == 1 else torch.diagonal(seen["hinv"])
    cw = (hd ** -4).double().cpu().numpy()  # as GANQ._initialize_codebook_kmeans forms the column weights: fp32, then double
    T0o = c_oracle.kmeans_init(Wr, cw, V)
    assert np.allclose(T0r, T0o, rtol=1e-6, atol=1e-8), "k-means init of the sampled rows differs from the oracle"
    tr = c_oracle.run_layer_trace(Wr, Hn, Ln, T0r, K)
    Qg = Q_perm[ridx].cpu().numpy()
    bad = [rows[i] for i in range(len(rows)) if not np.array_equal(Qg[i], tr["Q_all"][K - 1][i])]
    assert not bad, f"indices of rows {bad} differ from the oracle"
    e = rel_fro(T_best[ridx].cpu().numpy(), tr["T_all"][bk])
    print(f"[head-sized layer] best_k {bk}, codebook rel. Frobenius on 64 rows {e:.3e}")
    assert e < TOL_T, f"codebooks of the sampled rows: rel. Frobenius {e:.3e}"
    # the indices the task hands over are the loop's, back in the original column order
    assert tuple(task.ganq_indices.shape) == (m, n)

    # ---- the packed layer: forward on small-integer inputs, bit-exact against fp64 (any regime, any summation order)
    head = GanqHipQuantLinear(bits=4, group_size=128, sym=True, desc_act=True, in_features=n, out_features=m, bias=False).cuda()
    rng = np.random.default_rng(5)
    lut_int = torch.from_numpy(rng.integers(-2, 3, (m, V)).astype(np.float32)).cuda()
    with torch.no_grad():
        head.pack(lin, ganq_indices=task.ganq_indices, ganq_codebook=lut_int)
    Q = task.ganq_indices.long()
    assert torch.equal(_lib.unpack_indices(head.qweight, n, 4), task.ganq_indices.to(torch.uint8))
    Wd = torch.gather(lut_int.double(), 1, Q)  # [m, n] fp64, integers in [-2, 2]
    for M in (1, 16, 64, 300, 1100):
        x = torch.from_numpy((rng.integers(0, 2, (M, n)) * 2 - 1).astype(np.float32)).cuda()
        ref = x.double() @ Wd.T
        assert float(ref.abs().max()) <= lut_arena.INT_LIMIT["fp16"]
        y = head(x.half())
        assert y.shape == (M, m)
        want = ref.half()
        if not torch.equal(y, want):
            nz = torch.nonzero(y != want)
            i, j = (int(v) for v in nz[0])
            raise AssertionError(f"M={M}: {nz.shape[0]} of {y.numel()} outputs differ from the exact result; first y[{i}][{j}] = "
                                 f"{float(y[i, j])}, exact {float(want[i, j])}")
        del ref, y, want

    # ---- the lookup: 1000 ids over the whole range (both ends, the 65535 / 65536 neighbours, out-of-range ids)
    emb = GanqHipQuantEmbedding(head, dtype=torch.float16)
    ids = torch.from_numpy(np.concatenate([rng.integers(0, m, 1000 - len(rows) - 2), np.array(rows), np.array([-1, m])])).cuda()
    assert ids.numel() == 1000
    out = emb(ids)
    ok = (ids >= 0) & (ids < m)
    want = torch.where(ok.unsqueeze(1), Wd[ids.clamp(0, m - 1)], torch.zeros((), dtype=torch.float64, device="cuda")).half()
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))
    assert torch.equal(out[ok], head.dequantize_weight()[ids[ok]])
