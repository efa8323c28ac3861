"""Adapter description objects -- the contract of the reference's gptqmodel/adapter/adapter.py (`Adapter`, `Lora`,
`normalize_adapter`, `name()`, `parameter_keys()`, `to_dict()`), reduced to what the GANQ path uses.

An adapter object only DESCRIBES the adapter (its kind, its rank, optionally a local directory and tensors to start from): the
tensors that run live in the QuantLinear as `lora_A [rank, in_features]` / `lora_B [out_features, rank]` buffers and are saved
with the model (models/quantize.py).  Not carried: hub / URL loading, PEFT `LoraConfig` files, `apply()` in Python (the HIP
forward adds the adapter inside the LUT kernels).

`Lora.lora_A` / `Lora.lora_B`, when given, use the reference's attribute orientation -- `lora_A [in_features, rank]`,
`lora_B [rank, out_features]`, the transposes of the layer's buffers.
"""
import os
from typing import Dict, List, Optional, Union

import torch

RANK_MULTIPLE = 16  # matrix-core K granularity of the adapter steps in the LUT kernels
MAX_RANK = 256


def validate_rank(rank, what: str = "Adapter") -> int:
    """a rank the HIP forward serves: a positive multiple of 16, at most 256"""
    if isinstance(rank, bool) or not isinstance(rank, int):
        raise ValueError(f"{what}: `rank` must be an int, got {rank!r}")
    if rank <= 0 or rank % RANK_MULTIPLE != 0 or rank > MAX_RANK:
        raise ValueError(f"{what}: `rank` must be a positive multiple of {RANK_MULTIPLE} and at most {MAX_RANK}, got {rank}")
    return rank


class Adapter:
    def __init__(self, rank: int = None, path: str = None):
        self.rank = rank
        self.path = path.strip() if isinstance(path, str) else path

    def validate_path(self, local: bool = True):
        """`path` names a local directory; nothing is ever fetched"""
        if not self.path or not isinstance(self.path, str):
            raise ValueError("Adapter: `path` str is required.")
        if self.path.endswith(".safetensors"):
            raise ValueError(f"Adapter: `path` must be a directory, not a file: `{self.path}`")
        if not os.path.isdir(self.path):
            raise ValueError(f"Adapter: `path` must be an existing local directory (no remote loading): `{self.path}`")

    @classmethod
    def name(cls) -> str:
        raise NotImplementedError

    @classmethod
    def parameter_keys(cls) -> List[str]:
        raise NotImplementedError

    def to_dict(self) -> Dict:
        return {"name": self.name(), "path": self.path, "rank": self.rank}

    def __eq__(self, other):
        return type(other) is type(self) and other.to_dict() == self.to_dict()

    def __repr__(self):
        return f"{type(self).__name__}(rank={self.rank}, path={self.path!r})"


class Lora(Adapter):
    def __init__(self, rank: int, path: str = None, lora_A: Optional[torch.Tensor] = None, lora_B: Optional[torch.Tensor] = None):
        super().__init__(rank, path)
        if self.path is not None:
            self.validate_path()
        self.lora_A = lora_A
        self.lora_B = lora_B

    @classmethod
    def name(cls) -> str:
        return "lora"

    @classmethod
    def parameter_keys(cls) -> List[str]:
        return ["lora_A", "lora_B"]


ADAPTER_MAPPING = {Lora.name(): Lora}


def normalize_adapter(adapter: Union[Dict, Adapter, None]) -> Optional[Adapter]:
    """dict (`{"name": "lora", "rank": 64}`) or Adapter instance or None -> Adapter instance or None"""
    if adapter is None:
        return None
    if isinstance(adapter, Adapter):
        return adapter
    if not isinstance(adapter, dict):
        raise ValueError("Adapter: Invalid adapter config: `adapter`.")
    cfg = dict(adapter)  # the caller's dict is left as it is
    kind = cfg.pop("name", None)
    cls = ADAPTER_MAPPING.get(kind)
    if cls is None:
        raise ValueError(f"Adapter: compatible adapters are {sorted(ADAPTER_MAPPING)}: actual `{kind}`.")
    try:
        return cls(**cfg)
    except TypeError as e:
        raise ValueError(f"Adapter: Invalid adapter config: `{adapter}`.") from e
