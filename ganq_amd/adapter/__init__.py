from .adapter import ADAPTER_MAPPING, MAX_RANK, RANK_MULTIPLE, Adapter, Lora, normalize_adapter, validate_rank

__all__ = ["ADAPTER_MAPPING", "MAX_RANK", "RANK_MULTIPLE", "Adapter", "Lora", "normalize_adapter", "validate_rank"]
