"""GPU tests of the embedding stage of quantize_model (`QuantizeConfig.ganq_embedding`): the row quantizer
(quantization/embedding.py) against the exact 1-D k-means optimum, and the stage itself on two-layer OPT and Llama models
(vocabulary 323, hidden 64, fp16, tied and untied; built like the models of tests/test_hip_lm_head.py): FORMAT.GANQ_LUT against
FORMAT.FAKE, what the calibration passes see, ties, both tables packed, refusals, `dynamic`, checkpoints."""
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import embedding_table_model as etm
import kmeans_cases as kc

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52  # tests/test_hip_kmeans.py
VOCAB = 323
KINDS = ("opt", "llama")
N_LIN = {"opt": 12, "llama": 14}
EMB_NAME = {"opt": "model.decoder.embed_tokens", "llama": "model.embed_tokens"}
FIRST_MODULE = "self_attn.k_proj"  # the first module of a layer's first group in both layer maps
# LUT forward against the forward on the dequantised weights: the tolerance of tests/test_hip_lm_head.py
LOGIT_TOL = dict(rtol=2e-2, atol=2e-2)


# ---- the row quantizer
@pytest.mark.parametrize("V", [4, 8, 16])
def test_rows_reach_the_exact_kmeans_optimum(V):
    """rows with ties, repeated values and fewer values than V: the codebook's cost under nearest assignment is the exhaustive
    optimum within the margin tests/test_hip_kmeans.py allows a GPU codebook; rows with at most V distinct values come back exactly;
    a chunk of 7 rows gives the bits of the unchunked call"""
    from ganq_amd.quantization.embedding import quantize_embedding_rows

    n, bits = 512, {4: 2, 8: 3, 16: 4}[V]
    values = kc.VALUE_FAMILIES + ("distinct5", "stair", "coarse", "gauss", "distinctV")  # 16 rows: more than two chunks of 7
    W, w, fams = kc.make_matrix(n, V, 23, weights="unweighted", values=values)
    assert w is None and len(fams) == 16
    Wd = torch.from_numpy(W).cuda()
    qrows, T, sqerr = quantize_embedding_rows(Wd, bits)
    assert qrows.dtype == torch.int32 and tuple(qrows.shape) == (16, n * bits // 32)
    assert T.dtype == torch.float32 and tuple(T.shape) == (16, V) and sqerr.dtype == torch.float64 and tuple(sqerr.shape) == (16,)
    Tn, Q = T.cpu().numpy(), etm.unpack_rows(qrows.cpu().numpy(), bits)
    assert np.array_equal(Q, etm.nearest_indices(W, Tn))
    worst, exact = 0.0, 0
    for r, fam in enumerate(fams):
        best = kc.exhaustive_cost(W[r], None, V, device="cuda")
        got, E = kc.nearest_cost(W[r], None, Tn[r]), kc.total_energy(W[r], None)
        ratio = (got - best) / (EPS * E) if E > 0 else 0.0
        worst = max(worst, ratio)
        assert got - best <= kc.GPU_COST_FACTOR * kc.C_CPU * EPS * E, (fam, got, best, ratio)
        assert abs(float(sqerr[r]) - got) <= 1e-6 * got + 1e-30, (fam, float(sqerr[r]), got)  # (fp32 differences against fp64 ones)
        if kc.distinct_count(W[r]) <= V:
            exact += 1
            assert best == 0.0 and float(sqerr[r]) == 0.0, fam
            assert np.array_equal(np.take_along_axis(Tn[r:r + 1], Q[r:r + 1].astype(np.int64), axis=1)[0], W[r]), fam
    assert exact >= 3
    print(f"V={V}: largest (nearest_cost(T) - exhaustive_cost) / (2^-52 sum x^2) = {worst:.3f}; {exact} rows reconstructed exactly")
    q7, T7, e7 = quantize_embedding_rows(Wd, bits, max_chunk_elems=7 * n)
    assert torch.equal(q7, qrows) and torch.equal(T7.view(torch.int32), T.view(torch.int32))
    assert torch.equal(e7.view(torch.int64), sqerr.view(torch.int64))
    # the table's own dtype goes in: fp16 values are exact in fp32
    qh, Th, eh = quantize_embedding_rows(Wd.half(), bits)
    q32, T32, e32 = quantize_embedding_rows(Wd.half().float(), bits)
    assert torch.equal(qh, q32) and torch.equal(Th, T32) and torch.equal(eh, e32)


def test_row_quantizer_refuses_bad_tables():
    from ganq_amd.quantization.embedding import quantize_embedding_rows

    W = torch.zeros((4, 64), device="cuda")
    W[2, 5] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        quantize_embedding_rows(W, 4)
    W[2, 5] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        quantize_embedding_rows(W, 4)
    with pytest.raises(NotImplementedError):
        quantize_embedding_rows(torch.zeros((4, 48), device="cuda"), 4)
    with pytest.raises(NotImplementedError):
        quantize_embedding_rows(torch.zeros((4, 16384 + 32), device="cuda"), 4)


# ---- the models (the helpers of tests/test_hip_lm_head.py)
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
    with torch.no_grad():
        return model(ids).logits


def make_qcfg(**kw):
    from ganq_amd.quantization import QuantizeConfig

    base = dict(bits=4, act_sort="asc", l_damp_style="ganq", dead="mean", ganq_iterations=2)
    base.update(kw)
    return QuantizeConfig(**base)


@functools.lru_cache(maxsize=None)
def quantized(kind, tied, embedding=True, lm_head=False, mode="untie", fmt="ganq_lut", dynamic=None):
    """one quantize_model run, shared by the tests that read it (they do not modify it) -> dict(model, proc, table, first_inputs):
    the original embedding table and what the statistics hook of the first module was fed, call by call"""
    from ganq_amd.looper.gptq_processor import GPTQProcessor
    from ganq_amd.models import quantize_model

    class Recording(GPTQProcessor):
        def __init__(self, qcfg):
            super().__init__(qcfg)
            self.first_inputs = []

        def preprocess_fwd_hook(self, name):
            hook = super().preprocess_fwd_hook(name)
            if name != FIRST_MODULE:
                return hook

            def record(mod, inp, out):
                self.first_inputs.append(inp[0].detach().clone())
                hook(mod, inp, out)

            return record

    model = tiny(kind, tied)
    table = model.get_input_embeddings().weight.detach().clone()
    qcfg = make_qcfg(ganq_embedding=embedding, lm_head=lm_head, ganq_tied_embedding=mode, format=fmt,
                     dynamic=json.loads(dynamic) if dynamic else None)
    proc = Recording(qcfg)
    with torch.no_grad():
        quantize_model(model, calibration(), qcfg, processor=proc)
    return dict(model=model, proc=proc, table=table, first_inputs=proc.first_inputs, qcfg=qcfg)


def packed_layers(model):
    from ganq_amd.nn_modules.qlinear.ganq_hip import GanqHipQuantLinear

    return {n: m for n, m in model.named_modules() if isinstance(m, GanqHipQuantLinear)}


def all_ids():
    return torch.cat([torch.arange(VOCAB), torch.tensor([0, VOCAB - 1, 7, 7])]).cuda().view(3, 109)


@pytest.mark.parametrize("kind", KINDS)
def test_packed_embedding_against_the_fake_format(kind):
    from ganq_amd.nn_modules.qlinear.ganq_hip import GanqHipPackedEmbedding
    from ganq_amd.quantization.embedding import quantize_embedding_rows

    run = quantized(kind, False)
    model, proc = run["model"], run["proc"]
    emb = model.get_input_embeddings()
    assert isinstance(emb, GanqHipPackedEmbedding)
    assert (emb.num_embeddings, emb.embedding_dim, emb.bits, emb.dtype) == (VOCAB, 64, 4, torch.float16)
    assert emb.padding_idx == run_padding(kind)
    assert tuple(emb.qweight_rows.shape) == (VOCAB, 8) and tuple(emb.lut.shape) == (VOCAB, 16) and emb.lut.dtype == torch.float16
    assert f"{EMB_NAME[kind]}.weight" not in model.state_dict()
    # the module holds what the row quantizer returns for the original table
    qrows, T, sqerr = quantize_embedding_rows(run["table"], 4)
    assert torch.equal(emb.qweight_rows, qrows) and torch.equal(emb.lut, T.half())
    row = proc.log[0]
    assert row["module"] == EMB_NAME[kind] and row["bits"] == 4 and len(proc.log) == N_LIN[kind] + 1
    assert abs(float(row["loss"]) - float(sqerr.sum())) <= 1e-5 + 1e-9 * float(sqerr.sum()) and float(row["time"]) >= 0.0
    assert len(proc.results()) == N_LIN[kind]  # the embedding is no Linear: nothing for pack_model
    ids = all_ids()
    out = emb(ids)
    assert out.dtype == torch.float16 and tuple(out.shape) == (3, 109, 64) and out.grad_fn is None
    assert torch.equal(emb(ids.int()), out)
    assert torch.equal(emb.dequantize_weight(), emb(torch.arange(VOCAB, device="cuda")))
    with pytest.raises(TypeError):
        emb(ids.half())
    with pytest.raises(TypeError):
        emb(ids > 3)
    # FORMAT.FAKE: the same run with the dequantised rows in an nn.Embedding
    fake = quantized(kind, False, fmt="fake")["model"]
    f_emb = fake.get_input_embeddings()
    assert type(f_emb) is nn.Embedding and f_emb.weight.dtype == torch.float16
    assert torch.equal(out.view(torch.int16), f_emb.weight[ids].view(torch.int16))
    assert not torch.equal(f_emb.weight, run["table"])
    # ... and the body calibrated on the same quantized embedding: the same weights, bit for bit
    body = packed_layers(model)
    assert len(body) == N_LIN[kind]
    named = dict(fake.named_modules())
    for name, mod in body.items():
        assert torch.equal(mod.dequantize_weight(), named[name].weight), name
    a, b = logits_of(model, probe_ids()).float(), logits_of(fake, probe_ids()).float()
    print(f"[{kind}] max |logit difference| LUT vs dequantised = {float((a - b).abs().max()):.3e}")
    assert torch.allclose(a, b, **LOGIT_TOL)
    # without the stage the body is calibrated on the exact embedding: other weights
    plain = packed_layers(quantized(kind, False, embedding=False)["model"])
    assert any(not torch.equal(plain[n].qweight, body[n].qweight) for n in body)


def run_padding(kind):
    return 1 if kind == "opt" else None  # OPTConfig's pad_token_id; Llama has none


@pytest.mark.parametrize("kind", KINDS)
def test_calibration_runs_through_the_quantized_embedding(kind):
    """what the first module of layer 0 was calibrated on is what it receives in the finished model on the same batch, bit for bit
    (it would be the exact embedding's output had the stage run after the capture of the layer inputs)"""
    run = quantized(kind, False)
    model = run["model"]
    batches = calibration()
    recorded = run["first_inputs"][:len(batches)]  # the first pass over layer 0
    assert len(recorded) == len(batches)
    first = dict(model.named_modules())[f"{'model.decoder.layers' if kind == 'opt' else 'model.layers'}.0.{FIRST_MODULE}"]
    seen = []
    handle = first.register_forward_pre_hook(lambda mod, args: seen.append(args[0].detach().clone()))
    try:
        for ids in batches:
            logits_of(model, ids.cuda())
    finally:
        handle.remove()
    assert len(seen) == len(batches)
    for got, want in zip(seen, recorded):
        assert torch.equal(got.reshape(want.shape), want)
    # teeth: the exact table gives this module another input
    exact = quantized(kind, False, embedding=False)["first_inputs"][0]
    assert exact.shape == recorded[0].shape and not torch.equal(exact, recorded[0])


@pytest.mark.parametrize("kind", KINDS)
def test_tied_model_keeps_the_original_table_in_the_head(kind, tmp_path):
    from ganq_amd.models import load_quantized, save_quantized
    from ganq_amd.nn_modules.qlinear.ganq_hip import GanqHipPackedEmbedding

    run = quantized(kind, True)
    model = run["model"]
    head, emb = model.get_output_embeddings(), model.get_input_embeddings()
    assert type(head) is nn.Linear and torch.equal(head.weight, run["table"])
    assert isinstance(emb, GanqHipPackedEmbedding)
    assert model.config.tie_word_embeddings is False
    model.tie_weights()
    assert isinstance(model.get_input_embeddings(), GanqHipPackedEmbedding) and torch.equal(head.weight, run["table"])
    x = probe_ids()
    before = logits_of(model, x)
    path = os.path.join(tmp_path, "ckpt")
    save_quantized(model, path)
    cfg = json.load(open(os.path.join(path, "quantize_config.json")))
    assert cfg["embeddings"] == {EMB_NAME[kind]: {"bits": 4, "num_embeddings": VOCAB, "embedding_dim": 64, "padding_idx": run_padding(kind)}}
    assert cfg["ganq_embedding"] is True and "tied_embedding" not in cfg
    fresh = load_quantized(tiny(kind, True), path)  # a freshly built TIED model: load must not re-tie
    f_emb = fresh.get_input_embeddings()
    assert isinstance(f_emb, GanqHipPackedEmbedding) and f_emb.dtype == torch.float16 and f_emb.padding_idx == run_padding(kind)
    assert fresh.config.tie_word_embeddings is False and type(fresh.get_output_embeddings()) is nn.Linear
    assert torch.equal(fresh.get_output_embeddings().weight, run["table"])
    assert torch.equal(f_emb.qweight_rows, emb.qweight_rows) and torch.equal(f_emb.lut, emb.lut)
    assert fresh.quantize_config.ganq_embedding is True
    assert torch.equal(logits_of(fresh, x), before)
    assert torch.equal(logits_of(model, x), before)


@pytest.mark.parametrize("kind", KINDS)
def test_tied_model_with_quantized_head_packs_both_tables(kind, tmp_path):
    from safetensors import safe_open

    from ganq_amd.models import load_quantized, save_quantized
    from ganq_amd.nn_modules.qlinear.ganq_hip import GanqHipPackedEmbedding, GanqHipQuantLinear

    run = quantized(kind, True, lm_head=True, mode="untie")
    model, proc = run["model"], run["proc"]
    head, emb = model.get_output_embeddings(), model.get_input_embeddings()
    assert isinstance(head, GanqHipQuantLinear) and isinstance(emb, GanqHipPackedEmbedding)
    assert model.config.tie_word_embeddings is False
    assert proc.log[0]["module"] == EMB_NAME[kind] and proc.log[-1]["module"] == "lm_head" and len(proc.log) == N_LIN[kind] + 2
    x = probe_ids()
    before = logits_of(model, x)
    assert bool(torch.isfinite(before).all())
    path = os.path.join(tmp_path, "ckpt")
    save_quantized(model, path)
    bits = 4
    with safe_open(os.path.join(path, "model.safetensors"), "pt") as f:
        keys = set(f.keys())
        for k in keys:
            t = f.get_tensor(k)
            if t.is_floating_point() and VOCAB in t.shape:
                assert t.numel() <= VOCAB * 2 ** bits, (k, tuple(t.shape))  # no fp16 table of the vocabulary is left
    assert {f"{EMB_NAME[kind]}.qweight_rows", f"{EMB_NAME[kind]}.lut", "lm_head.qweight", "lm_head.lut"} <= keys
    assert f"{EMB_NAME[kind]}.weight" not in keys and "lm_head.weight" not in keys
    fresh = load_quantized(tiny(kind, True), path)
    assert isinstance(fresh.get_output_embeddings(), GanqHipQuantLinear) and isinstance(fresh.get_input_embeddings(), GanqHipPackedEmbedding)
    assert torch.equal(logits_of(fresh, x), before)


def test_refusals_come_before_any_work():
    from ganq_amd.models import quantize_model

    model = tiny("llama", True)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    with pytest.raises(ValueError, match="share"):
        quantize_model(model, calibration(), make_qcfg(ganq_embedding=True, lm_head=True, ganq_tied_embedding="share"))
    after = model.state_dict()
    assert list(after) == list(state) and all(torch.equal(after[k], state[k]) for k in state)
    assert type(model.get_input_embeddings()) is nn.Embedding and not packed_layers(model)
    assert model.get_output_embeddings().weight is model.get_input_embeddings().weight and model.config.tie_word_embeddings is True

    model = tiny("llama", False)
    model.get_input_embeddings().max_norm = 1.0
    with pytest.raises(NotImplementedError, match="max_norm"):
        quantize_model(model, calibration(), make_qcfg(ganq_embedding=True))
    assert type(model.get_input_embeddings()) is nn.Embedding and not packed_layers(model)

    class ScaledEmbedding(nn.Embedding):
        def forward(self, ids):
            return super().forward(ids) * 8.0

    model = tiny("llama", False)
    model.set_input_embeddings(ScaledEmbedding(VOCAB, 64).half().cuda())
    with pytest.raises(NotImplementedError, match="ScaledEmbedding"):
        quantize_model(model, calibration(), make_qcfg(ganq_embedding=True))
    assert not packed_layers(model)

    model = tiny("llama", False, dtype=torch.float32)
    with pytest.raises(NotImplementedError, match="float32"):
        quantize_model(model, calibration(), make_qcfg(ganq_embedding=True))
    assert not packed_layers(model)


def test_dynamic_overrides_and_skips_the_embedding():
    from ganq_amd.nn_modules.qlinear.ganq_hip import GanqHipPackedEmbedding

    run = quantized("llama", False, dynamic=json.dumps({"model.embed_tokens": {"bits": 3}}))
    emb = run["model"].get_input_embeddings()
    assert isinstance(emb, GanqHipPackedEmbedding) and emb.bits == 3
    assert tuple(emb.lut.shape) == (VOCAB, 8) and tuple(emb.qweight_rows.shape) == (VOCAB, 6)
    assert run["proc"].log[0]["bits"] == 3
    assert all(m.bits == 4 for m in packed_layers(run["model"]).values())
    assert bool(torch.isfinite(logits_of(run["model"], probe_ids())).all())

    run = quantized("llama", True, dynamic=json.dumps({"-:model.embed_tokens": {}}))
    model = run["model"]
    emb, head = model.get_input_embeddings(), model.get_output_embeddings()
    assert type(emb) is nn.Embedding and torch.equal(emb.weight, run["table"])
    assert head.weight is emb.weight and model.config.tie_word_embeddings is True  # untouched, still tied
    assert len(run["proc"].log) == N_LIN["llama"]


def test_fake_format_takes_a_float32_table():
    """the stage alone (models/quantize.py `_Embedding`) on a tied fp32 model: FORMAT.FAKE writes the rows the packed module would
    return, as fp32; FORMAT.GANQ_LUT refuses the table (test_refusals_come_before_any_work)"""
    from ganq_amd.looper.gptq_processor import GPTQProcessor
    from ganq_amd.models.quantize import _Embedding
    from ganq_amd.quantization.embedding import quantize_embedding_rows

    model = tiny("llama", True, dtype=torch.float32)
    emb = model.get_input_embeddings()
    table = emb.weight.detach().clone()
    qcfg = make_qcfg(ganq_embedding=True, format="fake")
    proc = GPTQProcessor(qcfg)
    stage = _Embedding(model, qcfg)
    assert stage.tied and stage.bits == 4 and not stage.skipped
    with torch.no_grad():
        stage.quantize(model, qcfg, proc)
    assert model.get_input_embeddings() is emb and emb.weight.dtype == torch.float32
    assert torch.equal(model.get_output_embeddings().weight, table) and model.config.tie_word_embeddings is False
    qrows, T, _ = quantize_embedding_rows(table, 4)
    Q = torch.from_numpy(etm.unpack_rows(qrows.cpu().numpy(), 4).astype(np.int64)).cuda()
    assert torch.equal(emb.weight, torch.gather(T.half(), 1, Q).float())
    assert len(proc.log) == 1 and proc.log[0]["module"] == "model.embed_tokens"


@pytest.mark.parametrize("kind", KINDS)
def test_checkpoint_without_the_stage_loads_as_before(kind, tmp_path):
    from ganq_amd.models import load_quantized, save_quantized

    model = quantized(kind, True, embedding=False)["model"]
    x = probe_ids()
    path = os.path.join(tmp_path, "ckpt")
    save_quantized(model, path)
    cfg = json.load(open(os.path.join(path, "quantize_config.json")))
    assert "embeddings" not in cfg and cfg["ganq_embedding"] is False
    del cfg["ganq_embedding"]  # as a checkpoint written before the field existed
    json.dump(cfg, open(os.path.join(path, "quantize_config.json"), "w"))
    fresh = load_quantized(tiny(kind, True), path)
    assert type(fresh.get_input_embeddings()) is nn.Embedding and fresh.config.tie_word_embeddings is True
    assert fresh.get_output_embeddings().weight is fresh.get_input_embeddings().weight
    assert fresh.quantize_config.ganq_embedding is False
    assert torch.equal(logits_of(fresh, x), logits_of(model, x))
