"""Model-level entry points around the hot path (SURVEY.md section 8(f) "next" rows): per-architecture layer maps
(the two the BASELINE configs need), `quantize_model`, a packed LUT checkpoint format and the GPTQ-style
perplexity evaluator.  The reference's model zoo / loader / writer (models/base.py, loader.py, writer.py, 52
definitions) are NOT rebuilt: these helpers operate on any Hugging Face style decoder the caller has built."""
from .calibration import as_batches, get_c4, get_wikitext2, load_text_split, wikitext2_test_ids
from .definitions import LAYER_MAPS, layer_map_for
from .quantize import causal_lm_next_token, causal_lm_nll, gptq_style_ppl, load_quantized, quantize_model, save_quantized, train_codebooks

__all__ = ["LAYER_MAPS", "layer_map_for", "quantize_model", "save_quantized", "load_quantized", "train_codebooks", "gptq_style_ppl", "causal_lm_nll",
           "causal_lm_next_token", "get_wikitext2", "get_c4", "wikitext2_test_ids", "load_text_split", "as_batches"]
