from .config import FORMAT, QUANT_METHOD, QuantizeConfig
from .embedding import quantize_embedding_rows
from .ganq import GANQ
from .gptq import GPTQ
from .quantizer import Quantizer

__all__ = ["FORMAT", "QUANT_METHOD", "QuantizeConfig", "GANQ", "GPTQ", "Quantizer", "quantize_embedding_rows"]
