"""Host side of the adapter feature (no GPU): the adapter objects, QuantizeConfig.adapter with its `dynamic` overrides, the
layer's buffers and state_dict keys, the checkpoint round trip on CPU tensors, and the identity the device-side EoRA generation
rests on -- B A = U_r U_r^T Delta with U_r the leading eigenvectors of Delta H Delta^T -- against the fixtures the reference's
own eora_compute_lora produced (tests/golden/eora/, make_golden_eora.py)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from eora_fixtures import EORA_FIXTURES, EORA_IDS, load_eora


def test_normalize_adapter_and_lora_contract(tmp_path):
    from ganq_amd.adapter import Adapter, Lora, normalize_adapter

    assert normalize_adapter(None) is None
    src = {"name": "lora", "rank": 64}
    a = normalize_adapter(src)
    assert isinstance(a, Lora) and isinstance(a, Adapter) and a.rank == 64 and a.path is None
    assert src == {"name": "lora", "rank": 64}  # the caller's dict is not consumed
    assert normalize_adapter(a) is a
    assert Lora.name() == "lora" and Lora.parameter_keys() == ["lora_A", "lora_B"]
    assert a.to_dict() == {"name": "lora", "path": None, "rank": 64}
    for bad in ({"rank": 64}, {"name": "dora", "rank": 64}, {"name": "lora", "rnk": 64}, "lora"):
        with pytest.raises(ValueError):
            normalize_adapter(bad)
    # a path must be an existing local directory: nothing is ever fetched
    assert Lora(rank=16, path=str(tmp_path)).path == str(tmp_path)
    for bad in ("https://example.invalid/adapter", "org/some-repo", str(tmp_path / "adapter_model.safetensors")):
        with pytest.raises(ValueError):
            Lora(rank=16, path=bad)


def test_config_adapter_field_validation_and_round_trip():
    from ganq_amd.adapter import Lora
    from ganq_amd.quantization.config import QuantizeConfig

    assert QuantizeConfig().adapter is None and QuantizeConfig().to_dict()["adapter"] is None
    c = QuantizeConfig(bits=3, adapter={"name": "lora", "rank": 64})
    assert isinstance(c.adapter, Lora) and c.adapter.rank == 64
    assert QuantizeConfig(bits=3, adapter=Lora(rank=256)).adapter.rank == 256
    d = c.to_dict()
    assert d["adapter"] == {"name": "lora", "path": None, "rank": 64}
    json.dumps(d, default=str)
    back = QuantizeConfig.from_dict(json.loads(json.dumps(d, default=str)))
    assert isinstance(back.adapter, Lora) and back.adapter.rank == 64 and back.bits == 3
    for rank in (0, -16, 8, 24, 272, 512, 16.0, None):
        with pytest.raises(ValueError):
            QuantizeConfig(adapter={"name": "lora", "rank": rank})
    with pytest.raises(ValueError):
        QuantizeConfig(adapter={"name": "lora", "rank": 32}, format="fake")
    # a config saved before the field existed loads unchanged
    old = {k: v for k, v in d.items() if k != "adapter"}
    assert QuantizeConfig.from_dict(old).adapter is None


def test_config_dynamic_rank_override_and_switch_off():
    from ganq_amd.quantization.config import QuantizeConfig

    c = QuantizeConfig(bits=3, adapter={"name": "lora", "rank": 64},
                       dynamic={"+:.*down_proj": {"adapter": {"rank": 128}}, r"+:.*\.k_proj": {"adapter": {}},
                                r".*\.v_proj": {"adapter": {"rank": 0}}, r"-:.*\.gate": {}})
    assert c.adapter_rank("model.layers.3.mlp.down_proj") == 128
    assert c.adapter_rank("model.layers.3.self_attn.k_proj") == 0
    assert c.adapter_rank("model.layers.3.self_attn.v_proj") == 0
    assert c.adapter_rank("model.layers.3.self_attn.q_proj") == 64
    assert c.adapter_rank("model.layers.3.mlp.gate") == 0
    assert QuantizeConfig(bits=3, dynamic={"+:.*down_proj": {"adapter": {"rank": 128}}}).adapter_rank("x.down_proj") == 0
    for bad in ({"rank": 40}, {"rank": 512}, 64):
        with pytest.raises(ValueError):
            QuantizeConfig(adapter={"name": "lora", "rank": 64}, dynamic={"+:.*down_proj": {"adapter": bad}})


def test_layer_accepts_lora_and_registers_buffers():
    from ganq_amd.adapter import Adapter, Lora
    from ganq_amd.nn_modules.backend import select_quant_linear
    from ganq_amd.nn_modules.qlinear.ganq_hip import GanqHipQuantLinear

    kw = dict(bits=3, group_size=128, desc_act=True, sym=True, pack_dtype=torch.int32)
    assert GanqHipQuantLinear.SUPPORTS_ADAPTERS == [Lora]
    ok, err = GanqHipQuantLinear.validate(adapter=Lora(rank=32), **kw)
    assert ok and err is None

    class Other(Adapter):
        pass

    ok, err = GanqHipQuantLinear.validate(adapter=Other(rank=32), **kw)
    assert not ok and isinstance(err, NotImplementedError)
    assert select_quant_linear(bits=3, group_size=128, desc_act=True, sym=True, adapter=Lora(rank=32)) is GanqHipQuantLinear
    with pytest.raises(NotImplementedError):
        select_quant_linear(bits=3, group_size=128, desc_act=True, sym=True, adapter=Other(rank=32))

    m, n = 48, 96
    plain = GanqHipQuantLinear(in_features=n, out_features=m, bias=True, **kw)
    assert plain.adapter_rank == 0 and sorted(plain.state_dict()) == ["bias", "lut", "qweight"]
    layer = GanqHipQuantLinear(in_features=n, out_features=m, bias=True, adapter=Lora(rank=32), **kw)
    assert layer.adapter_rank == 32
    assert layer.lora_A.shape == (32, n) and layer.lora_B.shape == (m, 32)
    assert layer.lora_A.dtype == layer.lora_B.dtype == torch.float16 and layer.lora_A.is_contiguous() and layer.lora_B.is_contiguous()
    assert sorted(layer.state_dict()) == ["bias", "lora_A", "lora_B", "lut", "qweight"]
    with pytest.raises(ValueError):
        GanqHipQuantLinear(in_features=n, out_features=m, bias=False, adapter=Lora(rank=24), **kw)
    # tensors on the adapter object use the reference's attribute orientation (the transposes of the buffers)
    A, B = torch.randn(32, n), torch.randn(m, 32)
    seeded = GanqHipQuantLinear(in_features=n, out_features=m, bias=False, adapter=Lora(rank=32, lora_A=A.t(), lora_B=B.t()), **kw)
    assert torch.equal(seeded.lora_A, A.half()) and torch.equal(seeded.lora_B, B.half())
    # train_adapter: fp32 parameters under the same keys, and back
    layer.train_adapter(True)
    assert isinstance(layer.lora_A, nn.Parameter) and layer.lora_B.dtype == torch.float32
    assert sorted(layer.state_dict()) == ["bias", "lora_A", "lora_B", "lut", "qweight"]
    assert {"lora_A", "lora_B"} <= set(dict(layer.named_parameters()))
    layer.train_adapter(False)
    assert not isinstance(layer.lora_A, nn.Parameter) and layer.lora_A.dtype == torch.float16 and not list(layer.parameters())
    with pytest.raises(ValueError):
        plain.train_adapter(True)


class _Tiny(nn.Module):
    def __init__(self):
        super().__init__()
        self.fc1 = nn.Linear(64, 96)
        self.fc2 = nn.Linear(96, 32, bias=False)
        self.head = nn.Linear(32, 8)


def test_save_load_round_trip_with_adapters_on_cpu(tmp_path):
    from ganq_amd.adapter import Lora
    from ganq_amd.models.quantize import load_quantized, save_quantized
    from ganq_amd.nn_modules.qlinear.ganq_hip import GanqHipQuantLinear
    from ganq_amd.quantization.config import QuantizeConfig

    torch.manual_seed(0)
    kw = dict(bits=3, group_size=128, desc_act=True, sym=True)
    model = _Tiny()
    model.fc1 = GanqHipQuantLinear(in_features=64, out_features=96, bias=True, adapter=Lora(rank=32), **kw)
    model.fc2 = GanqHipQuantLinear(in_features=96, out_features=32, bias=False, **kw)  # switched off for this module
    for q in (model.fc1, model.fc2):
        q.qweight.random_(-2 ** 31, 2 ** 31 - 1)
        q.lut.normal_()
    model.fc1.lora_A.normal_()
    model.fc1.lora_B.normal_()
    model.fc1.train_adapter(True)  # saved as fp16 whatever the training state
    qcfg = QuantizeConfig(bits=3, adapter={"name": "lora", "rank": 32}, dynamic={"+:fc2": {"adapter": {}}})
    save_quantized(model, str(tmp_path), qcfg)
    with open(tmp_path / "quantize_config.json") as f:
        cfg = json.load(f)
    assert cfg["adapter"] == {"name": "lora", "path": None, "rank": 32}
    assert cfg["modules"]["fc1"]["adapter_rank"] == 32 and "adapter_rank" not in cfg["modules"]["fc2"]
    loaded = load_quantized(_Tiny(), str(tmp_path))
    assert loaded.fc1.adapter_rank == 32 and loaded.fc2.adapter_rank == 0
    assert loaded.fc1.lora_A.dtype == torch.float16
    assert torch.equal(loaded.fc1.lora_A, model.fc1.lora_A.detach().half()) and torch.equal(loaded.fc1.lora_B, model.fc1.lora_B.detach().half())
    assert torch.equal(loaded.fc1.qweight, model.fc1.qweight) and torch.equal(loaded.fc2.lut, model.fc2.lut)
    assert loaded.quantize_config.adapter.rank == 32
    # a checkpoint written before adapters existed: no "adapter" in the config, no "adapter_rank" per module
    del cfg["adapter"]
    del cfg["modules"]["fc1"]["adapter_rank"]
    with open(tmp_path / "quantize_config.json", "w") as f:
        json.dump(cfg, f)
    with pytest.raises(RuntimeError):  # ... and then the adapter tensors of THIS file are unexpected: nothing is dropped silently
        load_quantized(_Tiny(), str(tmp_path))
    plain = _Tiny()
    plain.fc1 = GanqHipQuantLinear(in_features=64, out_features=96, bias=True, **kw)
    plain.fc2 = model.fc2
    old_dir = tmp_path / "old"
    save_quantized(plain, str(old_dir), QuantizeConfig(bits=3))
    with open(old_dir / "quantize_config.json") as f:
        old_cfg = json.load(f)
    old_cfg.pop("adapter")
    with open(old_dir / "quantize_config.json", "w") as f:
        json.dump(old_cfg, f)
    old = load_quantized(_Tiny(), str(old_dir))
    assert old.fc1.adapter_rank == 0 and "fc1.lora_A" not in old.state_dict() and old.quantize_config.adapter is None


def test_eora_fixtures_present():
    from ganq_amd.quantization.eora import OVERSAMPLE

    assert len(EORA_FIXTURES) >= 3
    for path in EORA_FIXTURES:
        assert os.path.getsize(path) <= 1 << 20  # the repository's limit for a committed file
        z = load_eora(path)
        r, (m, n) = z["rank"], z["W"].shape
        assert z["A"].shape == (r, n) and z["B"].shape == (m, r) and z["A"].dtype == np.float16
        assert z["H"].shape == (n, n) and np.array_equal(z["H"], z["H"].T)
        assert (z["E0"] - z["E_ref"]) / z["E0"] >= 0.1
        # the product iterates on a block of r + OVERSAMPLE vectors: with fewer rows it would solve the exact eigenproblem and
        # the fixture would not exercise the iteration, its stopping rule or its cap
        assert m > r + OVERSAMPLE, (m, r)
    assert any(load_eora(p)["W"].shape[0] < load_eora(p)["W"].shape[1] // 2 for p in EORA_FIXTURES)  # the wide one


@pytest.mark.parametrize("path", EORA_FIXTURES, ids=EORA_IDS)
def test_closed_form_reproduces_reference_product(path):
    """fp64 restatement of the closed form (quantization/eora.py docstring) against the reference's SVD route: same B A to the
    fp16 rounding of the reference's stored factors, same optimum E"""
    z = load_eora(path)
    D = torch.from_numpy(z["W"]).double() - torch.from_numpy(z["Wq"]).double()
    H = torch.from_numpy(z["H"]).double()
    r = z["rank"]
    lam, U = torch.linalg.eigh(D @ H @ D.T)
    lam, U = lam.flip(0), U.flip(1)
    Ur = U[:, :r]
    B = Ur * lam[:r] ** 0.25
    A = (Ur.T @ D) / (lam[:r] ** 0.25)[:, None]
    BA_ref = torch.from_numpy(z["B"]).double() @ torch.from_numpy(z["A"]).double()
    err = float((B @ A - BA_ref).norm() / BA_ref.norm())
    print(f"[eora identity] {os.path.basename(path)}: |BA - BA_ref| / |BA_ref| = 2^{np.log2(err):.2f}")
    assert err <= 2 ** -9
    R = D - B @ A
    E = float(torch.einsum("ij,jk,ik->", R, H, R))
    assert abs(E - z["E_opt"]) <= 1e-9 * z["E_opt"]
    assert abs(float(lam.sum()) - z["E0"]) <= 1e-9 * z["E0"]
    assert abs(float(lam[r:].sum()) - z["E_opt"]) <= 1e-9 * z["E_opt"]
    # the balancing: both factors carry sigma^1/2 -- B in the Euclidean norm (orthonormal U_r), A in the H-norm
    # (a_i H a_i^T = sigma_i^-1 u_i^T Delta H Delta^T u_i = sigma_i)
    half = lam[:r] ** 0.25
    assert torch.allclose(B.norm(dim=0), half)
    assert torch.allclose(torch.einsum("ij,jk,ik->i", A, H, A).sqrt(), half)
