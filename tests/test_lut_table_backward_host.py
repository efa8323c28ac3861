"""Host-side checks of the lookup codebook gradient (no GPU): ABI presence, workspace sizes, the argument checks that return before
anything touches a device, and the Python surface (`train_codebook` on the packed embedding, `train_codebooks`)."""
import os
import re

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ganq_lut_table_bwd_lut", "ganq_lut_embedding_bwd_lut")


def test_header_binding_library_and_makefile_carry_the_entries():
    from ganq_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ganq_hip.h")).read(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text) and re.search(r"\bsize_t\s+%s_workspace_bytes\s*\(" % name, text)
        assert len(_lib.SIGNATURES[name][1]) == 14 and len(_lib.SIGNATURES[name + "_workspace_bytes"][1]) == 4
        assert hasattr(_lib.lib(), name) and hasattr(_lib.lib(), name + "_workspace_bytes")
    assert callable(_lib.lut_table_bwd_lut) and callable(_lib.lut_embedding_bwd_lut)
    assert "lut_table_backward.hip" in open(os.path.join(ROOT, "ganq_amd", "csrc", "Makefile")).read()


def test_workspace_sizes_depend_on_the_arguments_alone():
    from ganq_amd import _lib

    h = _lib.lib()
    for name in ENTRIES:
        size = getattr(h, name + "_workspace_bytes")
        for bits in (2, 3, 4):
            assert size(0, 300, 64, bits) == 0 and size(16, 0, 64, bits) == 0 and size(16, 300, 0, bits) == 0
            for N in (1, 16, 2048, 5000):
                need = size(N, 300, 64, bits)
                # N partial rows of 2^bits fp32 bins and N int64 keys, each region rounded up to 256 bytes
                assert N * (4 << bits) + 8 * N <= need <= N * (4 << bits) + 8 * N + 512
                assert need == size(N, 128256, 2048, bits)  # neither the table's size nor the width enters
        assert size(16, 300, 64, 5) == 0
    assert h.ganq_lut_table_bwd_lut_workspace_bytes(2048, 300, 64, 4) == h.ganq_lut_embedding_bwd_lut_workspace_bytes(2048, 300, 64, 4)


def test_argument_checks_come_before_any_device_work():
    """shape and pointer checks in the style of the neighbouring entries: -1 negative / too large, -2 unsupported, -3 null pointer"""
    from ganq_amd import _lib

    h = _lib.lib()
    for name in ENTRIES:
        fn = getattr(h, name)
        args = lambda N, m, n, bits, dtype=0: (None, None, N, None, dtype, None, m, n, bits, -1, None, None, 0, None)  # noqa: E731
        assert fn(*args(-1, 300, 64, 4)) == -1 and fn(*args(4, -1, 64, 4)) == -1
        assert fn(*args(4, 1 << 31, 64, 4)) == -1 and b"too large" in h.ganq_hip_last_error()
        assert fn(*args(4, 300, 48, 4)) == -2 and b"multiple of 32" in h.ganq_hip_last_error()
        assert fn(*args(4, 300, 64, 5)) == -2 and fn(*args(4, 300, 64, 1)) == -2
        assert fn(*args(4, 300, 64, 4, dtype=2)) == -2
        assert fn(*args(4, 0, 64, 4)) == 0  # an empty table: nothing to write
        assert fn(*args(4, 300, 64, 4)) == -3 and name.encode() in h.ganq_hip_last_error()


def test_train_codebook_of_the_packed_embedding_on_the_host():
    from ganq_amd.models import train_codebooks
    from ganq_amd.nn_modules.qlinear.ganq_hip import GanqHipPackedEmbedding, GanqHipQuantEmbedding, GanqHipQuantLinear

    emb = GanqHipPackedEmbedding(40, 64, 3, padding_idx=-1)
    emb.lut = torch.randn(40, 8).half()
    lut16 = emb.lut.clone()
    assert emb.train_codebook(True) is emb
    assert isinstance(emb.lut, nn.Parameter) and emb.lut.dtype == torch.float32 and torch.equal(emb.lut.detach().half(), lut16)
    assert sorted(emb.state_dict()) == ["lut", "qweight_rows"] and "lut" in dict(emb.named_parameters())
    emb.train_codebook(False)
    assert not isinstance(emb.lut, nn.Parameter) and emb.lut.dtype == torch.float16 and torch.equal(emb.lut, lut16)
    assert emb._padding_id() == 39 and GanqHipPackedEmbedding(40, 64, 3)._padding_id() is None
    assert GanqHipPackedEmbedding(40, 64, 3, padding_idx=7)._padding_id() == 7
    for bad in (40, -41):  # nn.Embedding refuses these at construction
        with pytest.raises(ValueError, match="padding_idx"):
            GanqHipPackedEmbedding(40, 64, 3, padding_idx=bad)._padding_id()

    head = GanqHipQuantLinear(bits=4, group_size=-1, sym=True, desc_act=False, in_features=64, out_features=40)
    model = nn.ModuleDict({"embed": emb, "head": head, "tied": GanqHipQuantEmbedding(head), "norm": nn.LayerNorm(64)})
    params = train_codebooks(model)
    assert len(params) == 2 and params[0] is emb.lut and params[1] is head.lut  # the shared embedding trains through its head
    assert all(isinstance(p, nn.Parameter) and p.dtype == torch.float32 for p in params)
    assert train_codebooks(model, False) == []
    assert emb.lut.dtype == torch.float16 and head.lut.dtype == torch.float16 and not list(emb.parameters()) + list(head.parameters())
