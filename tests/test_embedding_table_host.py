"""Host-side checks of the embedding-table feature (`QuantizeConfig.ganq_embedding`): the config field, the numpy model of the
row-packed layout (tests/embedding_table_model.py) against the column layout's bit stream and against words worked out by hand,
and the two new symbols in header, binding and library.  No GPU."""
import os
import re

import numpy as np
import pytest

import embedding_table_model as etm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_config_field_round_trips():
    from ganq_amd.quantization import QuantizeConfig

    assert QuantizeConfig().ganq_embedding is False
    cfg = QuantizeConfig(ganq_embedding=True, dynamic={"model.embed_tokens": {"bits": 3}})
    d = cfg.to_dict()
    assert d["ganq_embedding"] is True
    back = QuantizeConfig.from_dict(d)
    assert back.ganq_embedding is True and back.dynamic_get("model.embed_tokens", "bits", 4) == 3
    d.pop("ganq_embedding")  # a config written before the field existed
    assert QuantizeConfig.from_dict(d).ganq_embedding is False


@pytest.mark.parametrize("bits", [2, 3, 4])
@pytest.mark.parametrize("m,n", [(1, 32), (5, 96), (7, 544)])
def test_row_stream_model_is_the_transposed_column_layout(bits, m, n):
    rng = np.random.default_rng(100 * bits + n)
    Q = rng.integers(0, 2 ** bits, (m, n), dtype=np.uint8)
    Q[0, :] = 2 ** bits - 1  # every bit set: a bit dropped at a word boundary shows
    if m > 1:
        Q[1, :] = np.arange(n) % 2 ** bits
    rows = etm.pack_rows(Q, bits)
    assert rows.shape == (m, n * bits // 32) and rows.dtype == np.uint32
    assert np.array_equal(rows, etm.column_stream_words(Q, bits).T)
    assert np.array_equal(etm.unpack_rows(rows, bits), Q)


def test_three_bit_indices_straddle_word_boundaries():
    """index 10 of a group lies in bits 30..32 (two in word 0, one in word 1), index 21 in bits 63..65: set alone, each must light
    exactly those bits"""
    for j, want in ((10, {0: 0b11 << 30, 1: 0b1}), (21, {1: 0b1 << 31, 2: 0b11}), (42, {3: 0b11 << 30, 4: 0b1})):
        Q = np.zeros((1, 64), dtype=np.uint8)
        Q[0, j] = 7
        rows = etm.pack_rows(Q, 3)[0]
        for w in range(6):
            assert int(rows[w]) == want.get(w, 0), (j, w, hex(int(rows[w])))
        assert np.array_equal(rows, etm.column_stream_words(Q, 3)[:, 0])


def test_layout_words_worked_out_by_hand():
    """the layout the header documents for `qrows`, as literal words: 4 bits -- eight nibbles a word, the first index lowest;
    2 bits -- 0, 1, 2, 3 make the byte 0b11100100; 3 bits -- 0 .. 7 make the 24 bits 0o76543210 = 0xFAC688, four of them three words"""
    want = {4: [0x76543210, 0xFEDCBA98, 0x76543210, 0xFEDCBA98], 2: [0xE4E4E4E4, 0xE4E4E4E4], 3: [0x88FAC688, 0xC688FAC6, 0xFAC688FA]}
    for bits, words in want.items():
        Q = (np.arange(32) % 2 ** bits).astype(np.uint8)[None, :]
        assert [int(w) for w in etm.pack_rows(Q, bits)[0]] == words, bits
        assert np.array_equal(etm.unpack_rows(np.array([words], dtype=np.uint32), bits), Q)
    # what the module and the C ABI size their buffers by
    from ganq_amd.nn_modules.qlinear.ganq_hip import GanqHipPackedEmbedding

    for bits, words in want.items():
        assert tuple(GanqHipPackedEmbedding(5, 32, bits).qweight_rows.shape) == (5, len(words))


def test_nearest_indices_break_ties_downwards():
    T = np.array([[-1.0, 0.0, 0.0, 2.0]], dtype=np.float32)
    W = np.array([[-0.5, 0.0, 1.0, 5.0] * 8], dtype=np.float32)  # midway -1 | 0: index 0; the repeated 0: index 1; midway 0 | 2: 1
    assert np.array_equal(etm.nearest_indices(W, T)[0, :4], [0, 1, 1, 3])


def test_new_symbols_in_header_binding_and_library():
    from ganq_amd import _lib

    text = open(os.path.join(ROOT, "include", "ganq_hip.h")).read()
    for name, nargs in (("ganq_lut_table_assign", 8), ("ganq_lut_table_lookup", 10)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(_lib.lib(), name)
    assert re.search(r"#define\s+GANQ_HIP_ABI_VERSION\s+4\b", text)
    assert "lut_table.hip" in open(os.path.join(ROOT, "ganq_amd", "csrc", "Makefile")).read()


def test_packed_embedding_module_owns_two_buffers_and_refuses_bad_shapes():
    import torch

    from ganq_amd._lib import GanqHipError
    from ganq_amd.nn_modules.qlinear.ganq_hip import GanqHipPackedEmbedding
    from ganq_amd.quantization.embedding import quantize_embedding_rows

    emb = GanqHipPackedEmbedding(323, 96, 3, dtype=torch.bfloat16, padding_idx=1)
    assert sorted(emb.state_dict()) == ["lut", "qweight_rows"] and not list(emb.parameters())
    assert tuple(emb.qweight_rows.shape) == (323, 9) and emb.qweight_rows.dtype == torch.int32
    assert tuple(emb.lut.shape) == (323, 8) and emb.lut.dtype == torch.float16
    assert (emb.num_embeddings, emb.embedding_dim, emb.bits, emb.dtype, emb.padding_idx) == (323, 96, 3, torch.bfloat16, 1)
    with pytest.raises(GanqHipError):
        emb(torch.zeros(3, dtype=torch.int64))  # ids on the CPU: no fallback
    with pytest.raises(NotImplementedError):
        GanqHipPackedEmbedding(10, 48, 4)
    with pytest.raises(NotImplementedError):
        GanqHipPackedEmbedding(10, 64, 4, dtype=torch.float32)
    # the quantizer refuses shapes before any work (also without a GPU)
    with pytest.raises(NotImplementedError):
        quantize_embedding_rows(torch.zeros(4, 48), 4)
    with pytest.raises(NotImplementedError):
        quantize_embedding_rows(torch.zeros(4, 16384 + 32), 4)
