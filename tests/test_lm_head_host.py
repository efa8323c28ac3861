"""Host-side checks of the head stage (no GPU): the `ganq_tied_embedding` field, the `pre_head` entries of every layer map
against a real forward of the family's model, and the presence of `ganq_lut_embedding` in header, binding and library."""
import os
import re

import pytest
import torch

from test_hip_models import FAMILIES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ALL_FAMILIES = dict(FAMILIES)
ALL_FAMILIES["opt"] = ("OPTConfig", "OPTForCausalLM", dict(vocab_size=320, hidden_size=64, ffn_dim=128, num_hidden_layers=2,
                                                           num_attention_heads=4, max_position_embeddings=128, word_embed_proj_dim=64), 6)
# a projection between the decoder width and the embedding width: the second entry of OPT's pre_head is a module here
ALL_FAMILIES["opt_project_out"] = ("OPTConfig", "OPTForCausalLM", dict(vocab_size=320, hidden_size=64, ffn_dim=128, num_hidden_layers=2,
                                                                       num_attention_heads=4, max_position_embeddings=128,
                                                                       word_embed_proj_dim=32), 6)
ALL_FAMILIES["llama"] = ("LlamaConfig", "LlamaForCausalLM", dict(vocab_size=320, hidden_size=64, intermediate_size=128,
                                                                 num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                                                                 max_position_embeddings=128), 7)


def test_tied_embedding_field_validates_and_round_trips():
    from ganq_amd.quantization import QuantizeConfig

    assert QuantizeConfig().ganq_tied_embedding == "untie"
    for mode in ("untie", "share"):
        q = QuantizeConfig(lm_head=True, ganq_tied_embedding=mode)
        d = q.to_dict()
        assert d["ganq_tied_embedding"] == mode and d["lm_head"] is True
        back = QuantizeConfig.from_dict(d)
        assert back.ganq_tied_embedding == mode and back.lm_head is True
    with pytest.raises(ValueError):
        QuantizeConfig(ganq_tied_embedding="copy")
    old = QuantizeConfig().to_dict()
    del old["ganq_tied_embedding"]  # a checkpoint written before the field existed
    assert QuantizeConfig.from_dict(old).ganq_tied_embedding == "untie"


def test_every_layer_map_has_pre_head():
    from ganq_amd.models.definitions import LAYER_MAPS

    for name, lm in LAYER_MAPS.items():
        assert isinstance(lm.pre_head, tuple) and len(lm.pre_head) >= 1, name
    assert set(ALL_FAMILIES) - {"opt_project_out"} <= set(LAYER_MAPS)


@pytest.mark.parametrize("kind", sorted(ALL_FAMILIES))
@torch.no_grad()
def test_pre_head_maps_last_layer_output_to_head_input(kind):
    import transformers

    from ganq_amd.models.definitions import layer_map_for
    from ganq_amd.models.quantize import _get_module

    cfg_name, cls_name, kwargs, _ = ALL_FAMILIES[kind]
    torch.manual_seed(0)
    model = getattr(transformers, cls_name)(getattr(transformers, cfg_name)(**kwargs)).float().eval()
    lm = layer_map_for(model)
    layers = _get_module(model, lm.layers_node)
    head = model.get_output_embeddings()
    assert isinstance(head, torch.nn.Linear)
    seen = {}

    def layer_hook(_mod, _inp, out):
        seen["layer"] = out[0] if isinstance(out, (tuple, list)) else out

    def head_hook(_mod, inp):
        seen["head"] = inp[0]

    handles = [layers[len(layers) - 1].register_forward_hook(layer_hook), head.register_forward_pre_hook(head_hook)]
    ids = torch.randint(1, 320, (2, 24), generator=torch.Generator().manual_seed(3))
    model(ids, use_cache=False)
    for h in handles:
        h.remove()
    x = seen["layer"]
    applied = 0
    for path in lm.pre_head:
        mod = _get_module(model, path)
        if mod is not None:
            x = mod(x)
            applied += 1
    assert applied >= 1
    if kind == "opt_project_out":
        assert applied == 2 and x.shape[-1] == 32
    assert torch.equal(x, seen["head"])


def test_header_binding_and_library_carry_lut_embedding():
    from ganq_amd import _lib

    text = open(os.path.join(ROOT, "include", "ganq_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+ganq_lut_embedding\s*\(", text)
    assert len(_lib.SIGNATURES["ganq_lut_embedding"][1]) == 13
    _lib.build()
    assert hasattr(_lib.lib(), "ganq_lut_embedding")
    assert callable(_lib.lut_embedding)
    assert "lut_embedding.hip" in open(os.path.join(ROOT, "ganq_amd", "csrc", "Makefile")).read()


def test_shared_embedding_owns_no_tensor():
    """built on the CPU (no kernel call): the module registers nothing, so a model's state_dict gains no key"""
    from ganq_amd.nn_modules.qlinear.ganq_hip import GanqHipQuantEmbedding, GanqHipQuantLinear

    head = GanqHipQuantLinear(bits=4, group_size=128, sym=True, desc_act=True, in_features=64, out_features=323, bias=False)
    emb = GanqHipQuantEmbedding(head, dtype=torch.bfloat16, padding_idx=1)
    assert len(emb.state_dict()) == 0 and list(emb.parameters()) == [] and list(emb.buffers()) == [] and list(emb.children()) == []
    assert (emb.num_embeddings, emb.embedding_dim, emb.head) == (323, 64, head)
    holder = torch.nn.ModuleDict({"embed": emb, "lm_head": head})
    assert sorted(holder.state_dict()) == ["lm_head.lut", "lm_head.qweight"]
    with pytest.raises(NotImplementedError):
        GanqHipQuantEmbedding(head, dtype=torch.float32)
    with pytest.raises(_lib_error()):
        emb(torch.zeros(3, dtype=torch.int64))  # no CPU fallback


def _lib_error():
    from ganq_amd import _lib

    return _lib.GanqHipError
