"""The LUT forward under HIP-graph replay, on concurrent streams and across a growth of the binding's workspace.

Every device time the README quotes comes from graph replays and real decode loops run captured graphs; these tests look at the
OUTPUT of a replay.  All kernels involved take a ticket and return (the last workgroup of a feature block reduces); none waits
for another workgroup."""
import weakref

import pytest
import torch

from test_hip_lora import _layer, check, reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from ganq_amd import _lib

    assert torch.cuda.is_available(), "these tests need the MI355X"
    _lib.selftest()
    return _lib


# a decoder block's five projections: (bits, out_features, in_features, adapter rank, outliers); the fourth has few feature blocks
# and long rows, so its decode plan splits in_features across workgroups
BLOCK = [(4, 1536, 1024, 0, 4), (4, 1024, 1536, 32, 0), (3, 8192, 1024, 0, 0), (4, 1024, 8192, 0, 0), (2, 640, 1024, 16, 0)]


def build_block():
    layers = [_layer(bits, m, n, r, bias=(i % 2 == 0), outlier_every=every, seed=40 + i) for i, (bits, m, n, r, every) in enumerate(BLOCK)]
    cols = layers[0][0].outlier_cols.view(-1, 2)  # two entries per outlier feature: distinct columns, or the dense reference would drop one
    assert bool((cols[:, 0] < cols[:, 1]).all())
    return layers


def run_block(layers, x):
    outs, h = [], x
    with torch.no_grad():
        for layer, _, _ in layers:
            h = layer(h)
            outs.append(h)
    return outs


def check_layer(layer, Q, h_in, y, dtype):
    """the fp64 bound of the kernel tests for one layer of the block on its actual input"""
    n, m = layer.in_features, layer.out_features
    bias = None if layer.bias is None else layer.bias.to(dtype)
    sparse = h_in.double() @ layer._sparse_dense(torch.float64).T if layer.outliers else None
    if layer.adapter_rank:
        ref, _, _, slack = reference(h_in, Q, layer.lut.to(dtype), bias, layer.lora_A.to(dtype), layer.lora_B.to(dtype), dtype, addend=sparse)
        check(y, ref, dtype, slack)
    else:
        ref = h_in.double() @ torch.gather(layer.lut.to(dtype).double(), 1, Q.long()).T
        if sparse is not None:
            ref = ref + sparse
        if bias is not None:
            ref = ref + bias.double()
        check(y, ref, dtype)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M", [1, 16])
def test_block_replay_is_bit_identical_to_eager(hip, M, dtype):
    layers = build_block()
    assert hip.debug_lut_plan(M, 1024, 8192, 4)["KS"] > 1 and hip.debug_lut_plan(M, 1024, 8192, 4)["regime"] == "decode16"
    g = torch.Generator(device="cuda").manual_seed(M)
    xs = [torch.randn(M, 1024, device="cuda", generator=g).to(dtype) for _ in range(5)]
    eager = [run_block(layers, x) for x in xs]
    for x, outs in zip(xs, eager):
        h = x
        for (layer, Q, _), y in zip(layers, outs):
            check_layer(layer, Q, h, y, dtype)
            h = y
    torch.cuda.synchronize()
    static_x = xs[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        for _ in range(2):  # warm-up on the capturing stream: its workspace exists before the capture
            run_block(layers, static_x)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            static_outs = run_block(layers, static_x)
    torch.cuda.current_stream().wait_stream(side)
    for x, outs in list(zip(xs, eager))[1:]:  # four replays, each on a new input
        static_x.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        for i, (got, want) in enumerate(zip(static_outs, outs)):
            assert torch.equal(got, want), f"layer {i} of the replay differs from eager"


def test_two_streams_run_different_layers_concurrently(hip):
    """each stream gets its own workspace (_LUT_WS is keyed by device and stream); both layers split in_features, so shared tickets
    or partial tiles would show"""
    (la_, _, _), (lb, _, _) = _layer(4, 1024, 8192, 0, seed=1), _layer(4, 640, 4096, 0, seed=2)
    xa = torch.randn(16, 8192, device="cuda").half()
    xb = torch.randn(300, 4096, device="cuda").half()
    assert hip.debug_lut_plan(16, 1024, 8192, 4)["KS"] > 1 and hip.debug_lut_plan(300, 640, 4096, 4)["regime"] == "gemm_splitk"
    with torch.no_grad():
        ya, yb = la_(xa), lb(xb)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    got_a, got_b = [], []
    with torch.no_grad():
        for _ in range(10):
            with torch.cuda.stream(s1):
                got_a.append(la_(xa))
            with torch.cuda.stream(s2):
                got_b.append(lb(xb))
    torch.cuda.synchronize()
    dev = torch.cuda.current_device()
    w1, w2 = hip._LUT_WS[(dev, s1.cuda_stream)], hip._LUT_WS[(dev, s2.cuda_stream)]
    assert w1.data_ptr() != w2.data_ptr()
    assert all(torch.equal(y, ya) for y in got_a) and all(torch.equal(y, yb) for y in got_b)


def test_graph_survives_the_growth_of_the_workspace(hip):
    """a graph captured on a stream keeps the pointer of that stream's workspace; a larger layer on the same stream makes the
    binding allocate a bigger one.  The superseded workspace has to stay allocated (`_lib._LUT_WS_RETIRED`): otherwise the replay's
    tickets and partial tiles land in whatever the allocator handed the block to"""
    small, _, _ = _layer(4, 512, 512, 0, seed=3)
    big, _, _ = _layer(4, 8192, 512, 0, seed=4)
    x = torch.randn(40, 512, device="cuda").half()
    xg = torch.randn(64, 512, device="cuda").half()
    assert hip.debug_lut_plan(40, 512, 512, 4)["regime"] == "mfma_small" and hip.debug_lut_plan(40, 512, 512, 4)["KS"] > 1
    assert hip.lib().ganq_lut_linear_workspace_bytes(64, 8192, 512, 4) > 1 << 20  # (the binding's smallest workspace)
    with torch.no_grad():
        want = small(x)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    key = (torch.cuda.current_device(), side.cuda_stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side), torch.no_grad():
        small(x)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            got = small(x)
        old = weakref.ref(hip._LUT_WS[key])
        old_ptr, old_bytes = old().data_ptr(), old().numel()
        big(xg)  # grows the workspace of this stream
        side.synchronize()
    assert hip._LUT_WS[key].data_ptr() != old_ptr and hip._LUT_WS[key].numel() > old_bytes
    assert old() is not None, "the superseded workspace was released while a captured graph may still point into it"
    # fresh tensors of the old workspace's size: the allocator would hand them the released block
    fresh = [torch.full((old_bytes,), 0x5A, dtype=torch.uint8, device="cuda") for _ in range(4)]
    assert all(f.data_ptr() != old_ptr for f in fresh)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert all(bool((f == 0x5A).all()) for f in fresh)
