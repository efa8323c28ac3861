"""quantize_model / save_quantized / load_quantized / gptq_style_ppl.

quantize_model  == BaseGPTQModel.quantize for quant_method=GANQ (models/base.py:317-459): capture the inputs of
                   decoder layer 0 for every calibration batch (module_looper.py:44-127 `cache_inputs`), then run the
                   device-resident looper over the layers.
save/load       the packed format the reference lacks: it can only save FORMAT.FAKE (dequantised fp16) and refuses to
                   load even that (config.py:369,398-401).  Here: one safetensors file with, per quantized Linear,
                   `<name>.qweight` int32 [in*bits/32, out], `<name>.lut` fp16 [out, 2^bits], `<name>.bias`; every other
                   tensor of the model unchanged; `quantize_config.json` next to it with the per-module bit widths.
                   A layer with an adapter adds `<name>.lora_A` fp16 [r, in] / `<name>.lora_B` fp16 [out, r] to the same
                   file and `"adapter_rank": r` to its entry of `"modules"` (absent in older checkpoints: no adapter).
                   With `QuantizeConfig.lm_head` the output head is one more entry of `"modules"`; an input embedding served from the
                   packed head (`ganq_tied_embedding="share"`) has no tensor in the file and is recorded as
                   `"tied_embedding": {"module": <embedding>, "source": <head>}` (absent in older checkpoints: nothing shared).
                   An input embedding quantized on its own (`QuantizeConfig.ganq_embedding`) is `<name>.qweight_rows` int32
                   [vocab, dim*bits/32] / `<name>.lut` fp16 [vocab, 2^bits] and an entry of `"embeddings"`: {<name>: {"bits",
                   "num_embeddings", "embedding_dim", "padding_idx"}} (absent in older checkpoints: no packed embedding).
gptq_style_ppl  the evaluator behind the README numbers (examples/quantization/basic_usage_wikitext2.py:63-93):
                   non-overlapping windows of `seqlen` tokens, mean token NLL, exp.
"""
import json
import os
import time
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn as nn

from ..looper.gptq_processor import GPTQProcessor
from ..looper.module_looper import ModuleLooper
from ..looper.named_module import NamedModule
from ..adapter import Lora
from .. import _lib
from ..nn_modules.qlinear.ganq_hip import GanqHipPackedEmbedding, GanqHipQuantEmbedding, GanqHipQuantLinear
from ..quantization.config import FORMAT, QuantizeConfig
from ..quantization.embedding import check_embedding_shape, quantize_embedding_rows
from .definitions import LayerMap, layer_map_for


def _get_module(root: nn.Module, path: str) -> nn.Module:
    mod = root
    for part in path.split("."):
        mod = getattr(mod, part)
    return mod


class _StopForward(Exception):
    pass


@torch.no_grad()
def capture_layer_inputs(model: nn.Module, layers: Sequence[nn.Module], batches: Sequence[torch.Tensor]):
    """run the model up to decoder layer 0 for every batch and keep that layer's positional/keyword inputs"""
    hidden, kwargs_list = [], []

    def hook(_, args, kwargs):
        hidden.append(args[0] if args else kwargs["hidden_states"])
        kw = {k: v for k, v in kwargs.items() if k not in ("hidden_states", "past_key_values", "past_key_value", "use_cache")}
        kwargs_list.append(kw)
        raise _StopForward()

    handle = layers[0].register_forward_pre_hook(hook, with_kwargs=True)
    try:
        for ids in batches:
            try:
                model(ids, use_cache=False)
            except _StopForward:
                pass
    finally:
        handle.remove()
    return hidden, kwargs_list


def _set_module(root: nn.Module, path: str, new: nn.Module) -> None:
    parent, _, child = path.rpartition(".")
    setattr(_get_module(root, parent) if parent else root, child, new)


def _name_of(model: nn.Module, module: nn.Module) -> str:
    for name, mod in model.named_modules():
        if mod is module:
            return name
    raise ValueError(f"{type(module).__name__} is not a module of the model")


class _Head:
    """the output head of a model and its tie to the input embedding, as the head stage of quantize_model needs them"""

    def __init__(self, model: nn.Module, qcfg: QuantizeConfig):
        get = getattr(model, "get_output_embeddings", None)
        self.module = get() if get is not None else None
        if self.module is None:
            raise ValueError("QuantizeConfig.lm_head: the model has no output embeddings (get_output_embeddings())")
        if not isinstance(self.module, nn.Linear):
            raise NotImplementedError(f"QuantizeConfig.lm_head: the head is a {type(self.module).__name__}, only nn.Linear is quantized")
        self.name = _name_of(model, self.module)
        self.skipped = qcfg.dynamic_get(layer_name=self.name) is False  # '-:' pattern
        get = getattr(model, "get_input_embeddings", None)
        self.embedding = get() if get is not None else None
        w = getattr(self.embedding, "weight", None)
        self.tied = w is not None and (w is self.module.weight or w.data_ptr() == self.module.weight.data_ptr())
        self.embedding_name = _name_of(model, self.embedding) if self.tied else None
        self.share = self.tied and not self.skipped and qcfg.ganq_tied_embedding == "share"
        if self.share:  # refuse before any work is done
            if type(self.embedding) is not nn.Embedding:
                raise NotImplementedError(f"ganq_tied_embedding=`share`: the input embedding is a {type(self.embedding).__name__}; only "
                                          f"a plain nn.Embedding is a row lookup of the head's table (use `untie`)")
            if qcfg.format == FORMAT.GANQ_LUT and w.dtype not in (torch.float16, torch.bfloat16):
                raise NotImplementedError(f"ganq_tied_embedding=`share`: a {w.dtype} table cannot be served from the packed head "
                                          f"(float16 and bfloat16 can; use `untie`)")
        self.table_dtype = w.dtype if self.tied else None

    def break_tie(self, model: nn.Module, qcfg: QuantizeConfig) -> None:
        """before the head is quantized: GPTQProcessor.process writes the head's weight, which a tied embedding would share"""
        if not self.tied:
            return
        if not self.share:
            w = self.module.weight
            self.embedding.weight = nn.Parameter(w.detach().clone(), requires_grad=w.requires_grad)
        # ("share": FORMAT.FAKE keeps the one Parameter, so the embedding's weight IS the dequantised head weight; FORMAT.GANQ_LUT
        # replaces the embedding after packing)
        cfg = getattr(model, "config", None)
        if cfg is not None and getattr(cfg, "tie_word_embeddings", False):
            cfg.tie_word_embeddings = False  # tie_weights() must not hang a `weight` onto the packed head

    def share_packed(self, model: nn.Module) -> None:
        head_q = _get_module(model, self.name)
        if self.share and isinstance(head_q, GanqHipQuantLinear):
            _set_module(model, self.embedding_name, GanqHipQuantEmbedding(head_q, dtype=self.table_dtype,
                                                                          padding_idx=self.embedding.padding_idx))


class _Embedding:
    """the input embedding as the embedding stage of quantize_model needs it (`QuantizeConfig.ganq_embedding`): every refusal
    happens here, before any work"""

    def __init__(self, model: nn.Module, qcfg: QuantizeConfig):
        get = getattr(model, "get_input_embeddings", None)
        self.module = get() if get is not None else None
        if self.module is None:
            raise ValueError("QuantizeConfig.ganq_embedding: the model has no input embeddings (get_input_embeddings())")
        self.name = _name_of(model, self.module)
        self.skipped = qcfg.dynamic_get(layer_name=self.name) is False  # '-:' pattern
        if self.skipped:
            return
        if type(self.module) is not nn.Embedding:
            raise NotImplementedError(f"QuantizeConfig.ganq_embedding: the input embedding is a {type(self.module).__name__}; only a "
                                      f"plain nn.Embedding is a row lookup of its table")
        if self.module.max_norm is not None:
            raise NotImplementedError("QuantizeConfig.ganq_embedding: an nn.Embedding with max_norm renormalises its rows on every "
                                      "lookup; a packed table cannot")
        w = self.module.weight
        served = (torch.float16, torch.bfloat16) + ((torch.float32,) if qcfg.format == FORMAT.FAKE else ())
        if w.dtype not in served:
            raise NotImplementedError(f"QuantizeConfig.ganq_embedding: a {w.dtype} table cannot be packed for format `{qcfg.format}` "
                                      f"({', '.join(str(d) for d in served)} can)")
        self.bits = int(qcfg.dynamic_get(self.name, "bits", qcfg.bits))
        check_embedding_shape(self.module.embedding_dim, self.bits)
        get = getattr(model, "get_output_embeddings", None)
        head = get() if get is not None else None
        hw = getattr(head, "weight", None)
        self.tied = isinstance(hw, torch.Tensor) and (hw is w or hw.data_ptr() == w.data_ptr())

    def quantize(self, model: nn.Module, qcfg: QuantizeConfig, proc: GPTQProcessor) -> None:
        """quantize the table (quantization/embedding.py) and put the result where the calibration passes will read it.  A tie is
        broken first: the head keeps the original Parameter, the embedding is quantized from its values."""
        emb = self.module
        w = emb.weight
        dev = w.device
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        t0 = time.time()
        qrows, T, sqerr = quantize_embedding_rows(w.detach(), self.bits)
        lut = T.to(torch.float16)
        if self.tied:
            cfg = getattr(model, "config", None)
            if cfg is not None and getattr(cfg, "tie_word_embeddings", False):
                cfg.tie_word_embeddings = False  # tie_weights() must not hand the head's table back to the embedding
        if qcfg.format == FORMAT.GANQ_LUT:
            packed = GanqHipPackedEmbedding(emb.num_embeddings, emb.embedding_dim, self.bits, dtype=w.dtype, padding_idx=emb.padding_idx)
            packed.qweight_rows, packed.lut = qrows, lut
            packed.train(emb.training)
            _set_module(model, self.name, packed)
        else:  # FORMAT.FAKE: the rows the packed module would return, in the table's dtype
            served = w.dtype if w.dtype in (torch.float16, torch.bfloat16) else torch.float16
            deq = _lib.lut_table_lookup(torch.arange(emb.num_embeddings, device=dev), qrows, lut.to(served), self.bits).to(w.dtype)
            if self.tied:
                emb.weight = nn.Parameter(deq, requires_grad=w.requires_grad)
            else:
                w.data = deq
        total = float(sqerr.sum())
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        proc.embedding_stage_seconds = time.time() - t0
        proc.log.append({"layer": -1, "module": self.name, "bits": self.bits, "loss": f"{total:.5f}",
                         "time": f"{proc.embedding_stage_seconds:.3f}"})


def _quantize_head(proc: GPTQProcessor, model: nn.Module, lm: LayerMap, head: _Head, hidden, layer_index: int, progress=None):
    """the head as one one-module group of the same processor, under its real module name, on `pre_head` of the hidden states
    leaving the last decoder layer (the looper's outputs: what the quantized body feeds it)"""
    pre = [m for m in (_get_module(model, p) for p in lm.pre_head) if m is not None]
    named = NamedModule(head.module, name=head.name, full_name=head.name, layer_index=layer_index)
    proc.preprocess(named, buffered_fwd=False)
    if proc.is_skipped(named):
        return
    hook = proc.preprocess_fwd_hook(head.name)
    for x in hidden:
        for mod in pre:
            x = mod(x)
        hook(head.module, (x,), None)  # the statistics hook alone: the logits of the calibration batches are not needed
    task = proc.tasks[head.name]
    end = getattr(task, "end_of_calibration", None)
    if end is not None:
        end()
    proc.process(named)
    if progress:
        progress(named)


@torch.no_grad()
def quantize_model(model: nn.Module, calibration: Sequence[torch.Tensor], qcfg: QuantizeConfig,
                   layer_map: Optional[LayerMap] = None, progress=None, processor: Optional[GPTQProcessor] = None,
                   **looper_options) -> GPTQProcessor:
    """Quantize every Linear the layer map names, layer by layer, on the device the model lives on (with `qcfg.lm_head` also the
    output head, last, on the normalised hidden states the quantized body produces; a tied input embedding follows
    `qcfg.ganq_tied_embedding`; with `qcfg.ganq_embedding` the input embedding itself, FIRST, so that every calibration pass runs
    through the quantized embedding).  `calibration`:
    token-id tensors [b, seq].  Returns the processor (per-module log, results); the model is modified in place
    (GanqHipQuantLinear / GanqHipPackedEmbedding modules for FORMAT.GANQ_LUT, dequantised weights for FORMAT.FAKE).
    looper_options: `early_exit=` / `cache_outputs=` / `share_group_hessian=` of ModuleLooper (results do not depend on
    them).  processor: a GPTQProcessor (subclass) to drive instead of a fresh one -- the reference's LoopProcessor slot."""
    lm = layer_map or layer_map_for(model)
    layers = _get_module(model, lm.layers_node)
    dev = next(model.parameters()).device
    from .. import distributed as gdist

    dist = gdist.Dist.current()
    # several ranks, dist_mode="rows" (the default): calibration is data-parallel -- this rank embeds and forwards only the
    # batches rank, rank + world, ...
    local = dist.world > 1 and looper_options.get("dist_mode", "rows") == "rows"
    if qcfg.adapter is not None and dist.world > 1:
        raise NotImplementedError("QuantizeConfig.adapter with several ranks: the row shards would have to exchange the "
                                  "quantization error (and the layer mode the adapters); quantize on one GPU")
    head = None
    if qcfg.lm_head:
        if dist.world > 1:
            raise NotImplementedError("QuantizeConfig.lm_head with several ranks: the head's rows would have to be sharded like the "
                                      "body's and its calibration inputs gathered; quantize on one GPU")
        head = _Head(model, qcfg)
        if head.skipped:
            head = None
    embedding = None
    if qcfg.ganq_embedding:
        if dist.world > 1:
            raise NotImplementedError("QuantizeConfig.ganq_embedding with several ranks: every rank would quantize the whole table; "
                                      "quantize on one GPU")
        embedding = _Embedding(model, qcfg)
        if embedding.skipped:
            embedding = None
        elif head is not None and head.share:
            raise ValueError("QuantizeConfig: ganq_embedding=True with lm_head=True and ganq_tied_embedding=`share`: `share` already "
                             "serves the embedding from the head's packed table (use `untie` to pack both)")
    batches = [b.to(dev) for b in (calibration[dist.rank::dist.world] if local else calibration)]
    was_training = model.training
    model.eval()
    proc = processor if processor is not None else GPTQProcessor(qcfg)
    if embedding is not None:
        embedding.quantize(model, qcfg, proc)
        if head is not None and embedding.tied:
            head = _Head(model, qcfg)  # the tie is gone: the head stage finds a head of its own
    hidden, kwargs_list = capture_layer_inputs(model, layers, batches)
    looper_options.setdefault("share_group_hessian", lm.shared_group_inputs)

    def fwd(layer, x, kw):
        return layer(x, **kw)

    hidden = ModuleLooper(proc, layers, lm.layer_modules, layers_prefix=lm.layers_node, **looper_options).loop(
        hidden, kwargs_list, forward=fwd, progress=progress, inputs_are_local=local)
    if head is not None:
        if dev.type == "cuda":  # (once per model: the stage's seconds are reported, so they should be the stage's)
            torch.cuda.synchronize(dev)
        t0 = time.time()
        head.break_tie(model, qcfg)
        _quantize_head(proc, model, lm, head, hidden, len(layers), progress)
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        proc.head_stage_seconds = time.time() - t0
    del hidden
    proc.finalize(model, lm_head_name=head.name if head is not None else None)
    if head is not None:
        head.share_packed(model)
    model.quantize_config = qcfg
    model.train(was_training)
    return proc


def save_quantized(model: nn.Module, path: str, qcfg: Optional[QuantizeConfig] = None) -> None:
    from safetensors.torch import save_file

    qcfg = qcfg or getattr(model, "quantize_config", None)
    if qcfg is None:
        raise ValueError("save_quantized: no QuantizeConfig given and the model carries none")
    os.makedirs(path, exist_ok=True)
    modules = {n: {"bits": m.bits, "in_features": m.in_features, "out_features": m.out_features,
                   "bias": m.bias is not None, "outliers": int(getattr(m, "outliers", 0)),
                   **({"adapter_rank": int(m.adapter_rank)} if getattr(m, "adapter_rank", 0) else {})}
               for n, m in model.named_modules() if isinstance(m, GanqHipQuantLinear)}
    # the codebook is stored as fp16 also while it trains as an fp32 parameter (train_codebook): the format does not change
    # (likewise the adapter while it trains, train_adapter)
    embeddings = {n: {"bits": m.bits, "num_embeddings": m.num_embeddings, "embedding_dim": m.embedding_dim, "padding_idx": m.padding_idx}
                  for n, m in model.named_modules() if isinstance(m, GanqHipPackedEmbedding)}
    luts = {f"{n}.{k}" for n in modules for k in ("lut", "lora_A", "lora_B")} | {f"{n}.lut" for n in embeddings}
    state = {k: (v.detach().to(torch.float16) if k in luts else v.detach()).contiguous().cpu() for k, v in model.state_dict().items()}
    # tied weights (lm_head <-> embeddings) share storage: safetensors wants each tensor once
    seen, out = {}, {}
    for k, v in state.items():
        key = (v.data_ptr(), tuple(v.shape), v.dtype)
        if key in seen and v.numel() > 0:
            continue
        seen[key] = k
        out[k] = v
    save_file(out, os.path.join(path, "model.safetensors"), metadata={"format": "pt", "ganq_format": FORMAT.GANQ_LUT})
    cfg = qcfg.to_dict()
    cfg["modules"] = modules
    if embeddings:
        cfg["embeddings"] = embeddings
    for n, m in model.named_modules():  # an embedding served from the packed head: the checkpoint holds no table for it
        if isinstance(m, GanqHipQuantEmbedding):
            cfg["tied_embedding"] = {"module": n, "source": _name_of(model, m.head)}
    with open(os.path.join(path, "quantize_config.json"), "w") as f:
        json.dump(cfg, f, indent=2, default=str)


def load_quantized(model: nn.Module, path: str) -> nn.Module:
    """`model`: a freshly constructed (unquantized, any weights) instance of the same architecture.  Replaces the
    recorded Linear modules by GanqHipQuantLinear (the output head among them if it was quantized; an embedding recorded as
    `"tied_embedding"` by a GanqHipQuantEmbedding on the rebuilt head; one recorded under `"embeddings"` by a
    GanqHipPackedEmbedding), then loads every tensor of the checkpoint."""
    from safetensors.torch import load_file

    with open(os.path.join(path, "quantize_config.json")) as f:
        cfg = json.load(f)
    modules: Dict[str, dict] = cfg.pop("modules")
    tied = cfg.pop("tied_embedding", None)
    embeddings: Dict[str, dict] = cfg.pop("embeddings", None) or {}
    qcfg = QuantizeConfig.from_dict(cfg)
    named = dict(model.named_modules())
    get_head = getattr(model, "get_output_embeddings", None)
    head = get_head() if get_head is not None else None
    head_packed = head is not None and any(named[n] is head for n in modules)
    table_dtype = named[tied["module"]].weight.dtype if tied else None
    for name, info in modules.items():
        lin = named[name]
        q = GanqHipQuantLinear(bits=info["bits"], group_size=qcfg.group_size, sym=qcfg.sym, desc_act=qcfg.desc_act,
                               in_features=info["in_features"], out_features=info["out_features"], bias=info["bias"],
                               pack_dtype=torch.int32, name=name, outliers=info.get("outliers", 0),
                               adapter=Lora(rank=info["adapter_rank"]) if info.get("adapter_rank") else None).to(lin.weight.device)
        parent, _, child = name.rpartition(".")
        setattr(named[parent] if parent else model, child, q)
    if tied:  # the shared embedding reads the rebuilt head: no table of its own is expected in the checkpoint
        emb = named[tied["module"]]
        _set_module(model, tied["module"], GanqHipQuantEmbedding(_get_module(model, tied["source"]), dtype=table_dtype,
                                                                 padding_idx=getattr(emb, "padding_idx", None)))
    for name, info in embeddings.items():  # built before load_state_dict: the checkpoint's tensors find their buffers
        emb = named[name]
        _set_module(model, name, GanqHipPackedEmbedding(info["num_embeddings"], info["embedding_dim"], info["bits"], dtype=emb.weight.dtype,
                                                        padding_idx=info.get("padding_idx")).to(emb.weight.device))
    if (head_packed or embeddings) and getattr(getattr(model, "config", None), "tie_word_embeddings", False):
        # a packed head / a packed embedding has no `weight`: tie_weights() below must not reach for it
        model.config.tie_word_embeddings = False
    state = load_file(os.path.join(path, "model.safetensors"))
    missing, unexpected = model.load_state_dict(state, strict=False)
    missing = [k for k in missing if k not in ("lm_head.weight",)]  # tied to the embeddings
    if missing or unexpected:
        raise RuntimeError(f"load_quantized: missing {missing[:5]} unexpected {list(unexpected)[:5]}")
    if hasattr(model, "tie_weights"):
        model.tie_weights()
    model.quantize_config = qcfg
    return model


def train_codebooks(model: nn.Module, enabled: bool = True) -> List[nn.Parameter]:
    """Switch the codebook of every packed module of `model` (GanqHipQuantLinear, GanqHipPackedEmbedding) with its
    `train_codebook(enabled)` and return the codebook parameters (an empty list for enabled=False), in `named_modules()` order.  An
    embedding that shares a packed head (GanqHipQuantEmbedding) owns no tensor: it trains through its head's `lut`, which then
    collects the gradient of both the output projection and the lookup."""
    params = []
    for m in model.modules():
        if isinstance(m, (GanqHipQuantLinear, GanqHipPackedEmbedding)):
            m.train_codebook(enabled)
            if enabled:
                params.append(m.lut)
    return params


_POST_HEAD_LOGIT_ATTRS = ("final_logit_softcapping", "logit_scale", "logits_scaling")  # config entries that change the logits after the head


def causal_lm_nll(model: nn.Module, input_ids: torch.Tensor, labels: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-token negative log-likelihood [batch, seq - 1] of a causal LM whose output head is a packed GanqHipQuantLinear, without
    the [batch, seq, vocab] logits: the hidden states of `model.base_model(input_ids)[0]` go through `head.nll` (the fused HIP
    kernel, or the chunked path of a head with outliers or an adapter).  Position t is scored against labels[:, t + 1]; labels
    default to input_ids; a label outside the vocabulary (-100) gives 0.  Gradients follow `GanqHipQuantLinear.nll`.
    Raises for a head that is not packed and for a config that scales or caps the logits after the head."""
    head = model.get_output_embeddings() if hasattr(model, "get_output_embeddings") else None
    if not isinstance(head, GanqHipQuantLinear):
        raise TypeError(f"causal_lm_nll: the output head is {type(head).__name__}, not a GanqHipQuantLinear (quantize with "
                        f"QuantizeConfig.lm_head=True)")
    cfg = getattr(model, "config", None)
    for attr in _POST_HEAD_LOGIT_ATTRS:
        v = getattr(cfg, attr, None)
        if v is not None and v != 1.0:
            raise NotImplementedError(f"causal_lm_nll: the model's config sets {attr}={v}, applied to the logits after the head; "
                                      f"the loss straight from the head would miss it")
    labels = input_ids if labels is None else labels
    if tuple(labels.shape) != tuple(input_ids.shape):
        raise ValueError(f"causal_lm_nll: labels {tuple(labels.shape)} do not fit input_ids {tuple(input_ids.shape)}")
    hidden = model.base_model(input_ids)[0]
    return head.nll(hidden[:, :-1, :], labels[:, 1:].to(hidden.device))


def causal_lm_next_token(model: nn.Module, input_ids: torch.Tensor, temperature: float = 0.0, generator=None, rng=None, **base_model_kwargs):
    """The next token of a causal LM whose output head is a packed GanqHipQuantLinear, without the [batch, vocab] logits:
    `model.base_model(input_ids, **base_model_kwargs)` runs and the hidden state of the last position goes through `head.pick`
    (greedy at temperature 0, a sample from softmax(logits / temperature) drawn with `generator` otherwise -- or, with
    rng=PickRng(seed), inside the head's kernel from that state, which the call advances by one: no [batch, vocab] noise either).
    -> (token int64 [batch], logprob fp32 [batch], the base model's outputs -- so a caller can carry `past_key_values`).  No graph is
    built; the gradient of logprob is taken in the training pass, through `causal_lm_nll`.
    Raises for a head that is not packed and for a config that scales or caps the logits after the head."""
    head = model.get_output_embeddings() if hasattr(model, "get_output_embeddings") else None
    if not isinstance(head, GanqHipQuantLinear):
        raise TypeError(f"causal_lm_next_token: the output head is {type(head).__name__}, not a GanqHipQuantLinear (quantize with "
                        f"QuantizeConfig.lm_head=True)")
    cfg = getattr(model, "config", None)
    for attr in _POST_HEAD_LOGIT_ATTRS:
        v = getattr(cfg, attr, None)
        if v is not None and v != 1.0:
            raise NotImplementedError(f"causal_lm_next_token: the model's config sets {attr}={v}, applied to the logits after the head; "
                                      f"the token straight from the head would miss it")
    with torch.no_grad():
        outputs = model.base_model(input_ids, **base_model_kwargs)
        token, logprob = head.pick(outputs[0][:, -1, :], temperature=temperature, generator=generator, rng=rng)
    return token, logprob, outputs


@torch.no_grad()
def gptq_style_ppl(model: nn.Module, token_ids: torch.Tensor, seqlen: int = 2048, fused_head: bool = False) -> float:
    """token_ids: [1, total] (e.g. the wikitext-2-raw-v1 test split joined with "\\n\\n" and tokenized).
    fused_head: the loss of every window straight from the packed head (`causal_lm_nll`): no [seqlen, vocab] logits."""
    dev = next(model.parameters()).device
    ids = token_ids.to(dev)
    nsamples = ids.numel() // seqlen
    if nsamples == 0:
        raise ValueError("gptq_style_ppl: fewer tokens than one window")
    model.eval()
    nlls = []
    loss_fct = nn.CrossEntropyLoss()
    for i in range(nsamples):
        batch = ids[:, i * seqlen:(i + 1) * seqlen]
        if fused_head:
            nlls.append(causal_lm_nll(model, batch).mean() * seqlen)
            continue
        logits = model(batch).logits
        shift_logits = logits[:, :-1, :].contiguous().float()
        shift_labels = batch[:, 1:]
        loss = loss_fct(shift_logits.view(-1, shift_logits.size(-1)), shift_labels.reshape(-1))
        nlls.append(loss.float() * seqlen)
    return float(torch.exp(torch.stack(nlls).sum() / (nsamples * seqlen)))
