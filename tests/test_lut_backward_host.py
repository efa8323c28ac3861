"""CPU-side checks of the LUT backward (csrc/lut_backward.hip): the layer declares itself trainable, the four C-ABI entries are
declared and bound, and their workspace queries are pure host functions of their arguments (no GPU needed)."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BWD = ["ganq_lut_linear_bwd_input_workspace_bytes", "ganq_lut_linear_bwd_input", "ganq_lut_linear_bwd_lut_workspace_bytes",
       "ganq_lut_linear_bwd_lut"]


def test_layer_validates_as_trainable():
    from ganq_amd.nn_modules.qlinear.ganq_hip import GanqHipQuantLinear

    for bits in (2, 3, 4):
        ok, err = GanqHipQuantLinear.validate(bits=bits, group_size=-1, desc_act=False, sym=True, in_features=4096, out_features=4096,
                                              pack_dtype=__import__("torch").int32, trainable=True)
        assert (ok, err) == (True, None), err
    assert GanqHipQuantLinear.SUPPORTS_TRAINING


def test_backward_symbols_declared_and_bound():
    from ganq_amd import _lib

    header = open(os.path.join(ROOT, "include", "ganq_hip.h")).read()
    for name in BWD:
        assert name + "(" in header, name
        assert name in _lib.SIGNATURES, name
    handle = _lib.lib()
    for name in BWD:
        assert hasattr(handle, name), name


def test_backward_workspace_queries_are_host_functions():
    from ganq_amd import _lib

    h = _lib.lib()
    for bits in (2, 3, 4):
        for m, n in [(1, 32), (129, 320), (4096, 4096), (14336, 4096), (4096, 14336)]:
            assert h.ganq_lut_linear_bwd_input_workspace_bytes(0, m, n, bits) == 0
            assert h.ganq_lut_linear_bwd_input_workspace_bytes(128, m, n, 5) == 0  # invalid arguments: 0 from both queries
            assert h.ganq_lut_linear_bwd_lut_workspace_bytes(128, m, n, 5) == 0
            assert h.ganq_lut_linear_bwd_lut_workspace_bytes(0, m, n, bits) == 0
            for M in (1, 16, 64, 65, 333, 2048):
                a = h.ganq_lut_linear_bwd_input_workspace_bytes(M, m, n, bits)
                b = h.ganq_lut_linear_bwd_lut_workspace_bytes(M, m, n, bits)
                assert a == h.ganq_lut_linear_bwd_input_workspace_bytes(M, m, n, bits)
                assert b == h.ganq_lut_linear_bwd_lut_workspace_bytes(M, m, n, bits)
                mp = (m + 63) // 64 * 64
                if M > 64:  # the transposed dequantised layer Wq^T [n][ceil64(m)] lives in the workspace
                    assert a >= n * mp * 2
                    if m % 64:  # ... and the zero-padded copy of dy
                        assert a >= n * mp * 2 + M * mp * 2
                Mp = (M + 63) // 64 * 64  # dy^T, x^T staged over whole tiles of 64 tokens, one fp32 bin set per 256 columns
                assert b >= (m + n) * Mp * 2 + ((n + 255) // 256) * m * (1 << bits) * 4
