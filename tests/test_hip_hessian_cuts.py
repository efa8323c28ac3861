"""GPU tests of the Hessian's token cuts against float64: the transposed staging path (hessian_w4.hip, 256 x 256 tiles cut stream-K,
partial tiles summed by hessian_w4_fix_kernel) at the short staged groups and workgroup counts where the cut changes shape, the
quantizer's staging path that reaches them, and the row-major token-split launches.

Every call is set up so that a wrong read shows: H holds 7.0 before a first group and a symmetric H0 before a decayed one, the
workspace is filled with 0xFF bytes (fp32 NaN) so that reading a partial tile nobody wrote this call fails every time, and the
staging buffer holds stale tokens behind the group.  Every result is checked finite, exactly symmetric, against the float64
2/N sum X^T X (+ decay H0) in the relative Frobenius norm overall AND in every 256 x 256 tile (one bad tile out of hundreds does
not move the global norm), and for the same bits over three repeats."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TILE = 256


@pytest.fixture(scope="module")
def hip():
    from ganq_amd import _lib

    assert torch.cuda.is_available()
    _lib.lib()
    return _lib


def poisoned(nbytes):
    """a workspace of `nbytes` filled with 0xFF bytes: every fp32 word in it is NaN"""
    return torch.full((max(int(nbytes), 256),), 0xFF, dtype=torch.uint8, device="cuda")


def check_vs_fp64(H, ref, what):
    """H (fp32, cuda) against ref (fp64, cuda): finite, exactly symmetric, rel. Frobenius < 1e-6 overall and < 1e-5 per 256 x 256 tile"""
    assert bool(torch.isfinite(H).all()), f"{what}: {int((~torch.isfinite(H)).sum())} non-finite entries"
    assert torch.equal(H, H.T), f"{what}: not exactly symmetric"
    D = H.double() - ref
    err = float(D.norm() / ref.norm())
    assert err < 1e-6, f"{what}: rel. Frobenius {err:.3g}"
    n = H.shape[0]
    nt = -(-n // TILE)
    pad = nt * TILE - n

    def tile_norms(A):
        A = torch.nn.functional.pad(A, (0, pad, 0, pad))
        return A.view(nt, TILE, nt, TILE).pow(2).sum(dim=(1, 3)).sqrt()

    rel = tile_norms(D) / tile_norms(ref).clamp_min(1e-300)
    worst = int(torch.argmax(rel))
    assert float(rel.max()) < 1e-5, f"{what}: tile {divmod(worst, nt)} rel. Frobenius {float(rel.max()):.3g} (overall {err:.3g})"


def make_group(n, rows, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, n, generator=g) * 0.5).to(dtype).cuda()


def make_h0(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    A = torch.randn(n, n, device="cuda", generator=g)
    return (0.25 * (A + A.T)).contiguous()  # (exactly symmetric)


def run_transposed(hip, X, before, batch, H0):
    """one staged group through the product's calls: hessian_stage_t batch by batch into a buffer with stale tokens behind the group,
    the ragged last slice zero-filled, hessian_accum_t with a NaN-poisoned workspace; H starts as H0 (decayed group) or 7.0"""
    rows, n = X.shape
    pad = -(-rows // 32) * 32
    cap = pad + 64
    assert hip.hessian_t_supported(n, cap)
    H = H0.clone() if H0 is not None else torch.full((n, n), 7.0, device="cuda")
    Xt = torch.full((n, cap), 3.0, dtype=X.dtype, device="cuda")  # stale tokens behind the group must not count
    step = max(8, rows // 3 // 8 * 8)
    for t0 in range(0, rows, step):
        hip.hessian_stage_t(Xt, X[t0:t0 + step], t0)
    Xt[:, rows:pad].zero_()
    ws = poisoned(hip.lib().ganq_hessian_t_workspace_bytes(n))
    hip.hessian_accum_t(H, Xt, pad, before, batch, workspace=ws)
    return H


def reference(X, before, batch, H0):
    """float64 H <- H0 * N/(N+b) + (2/(N+b)) X^T X (N = sequences before, b = sequences of the group)"""
    Xd = X.double()
    total = before + batch
    ref = (2.0 / total) * (Xd.T @ Xd)
    if H0 is not None and before > 0:
        ref += (before / total) * H0.double()
    return ref


def cut_of(hip, n, rows, G):
    """the launch's cut on the host, by the kernels' own code: header + the number of parts of every left-over tile + the largest
    number of left-over segments of one workgroup"""
    h = hip.lib()
    hdr = (ctypes.c_int * 7)()
    assert h.ganq_debug_hessian_t_cut(n, rows, G, hdr, None, 0, None, 0) == 0
    Ks, _, W, R, nprim, P, Sh = list(hdr)
    per = W + 3
    segs = (ctypes.c_int * (G * per * 5))()
    assert h.ganq_debug_hessian_t_cut(n, rows, G, hdr, segs, len(segs), None, 0) == 0
    S = np.frombuffer(segs, dtype=np.int32).reshape(G, per, 5)[:, W:, :]
    parts = np.zeros(max(R, 1), dtype=np.int64)
    for t in S[..., 0][S[..., 0] >= 0]:
        parts[t - W * G] += 1
    return dict(W=W, R=R, nprim=nprim, P=P, Sh=Sh, Ks=Ks, parts=parts[:R], max_left=int((S[..., 0] >= 0).sum(1).max()))


def regime_holds(c, regime):
    if regime == "R=0":
        return c["R"] == 0
    if regime == "whole+left-over":
        return c["W"] > 0 and c["R"] > 0
    if regime == "plain, one part each":
        return c["R"] > 0 and c["P"] == 0 and bool((c["parts"] == 1).all())
    if regime == "plain, several parts each":
        return c["R"] > 0 and c["P"] == 0 and bool((c["parts"] >= 2).all())
    if regime == "primary+helpers":
        return c["nprim"] > 0 and c["P"] > 0
    if regime == "helper with three segments":
        return c["max_left"] == 3
    raise AssertionError(regime)


# ------------------------------------------------------------------------------------------ 1. short staged groups
@pytest.mark.parametrize("mode", ["first", "decayed"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("rows", [32, 64, 96, 160, 256])
@pytest.mark.parametrize("n", [3072, 4096, 5120, 11008])
def test_short_staged_groups_vs_fp64(hip, n, rows, dtype, mode):
    """The staged groups a calibration ends with (the last group, a group cut short by a ragged batch or a dtype change, a
    mixture-of-experts expert with few tokens) at default options: on 256 CUs these are the plain cuts where left-over tiles are
    in ONE part (n = 4096 at 32 / 64 tokens: the whole H), finished by the main kernel alone, next to primary cuts of 2-3 parts."""
    X = make_group(n, rows, dtype, seed=n + rows)
    before, batch = (0, 2) if mode == "first" else (5, 2)
    H0 = make_h0(n, seed=n) if mode == "decayed" else None
    H = run_transposed(hip, X, before, batch, H0)
    check_vs_fp64(H, reference(X, before, batch, H0), f"n={n} rows={rows} {dtype} {mode}")
    for _ in range(3):  # deterministic: the same bits
        assert torch.equal(run_transposed(hip, X, before, batch, H0), H)


# ------------------------------------------------------------------------------------------ 2. cuts of other workgroup counts
# (G, in_features, tokens, regime): chosen with the host export, each asserted below.  n < 3072 needs GANQ_HESS_W4=2.
REGIMES = [
    (32, 16384, 32, "R=0"),
    (80, 16384, 32, "R=0"),
    (64, 3072, 32, "whole+left-over"),
    (304, 8192, 32, "whole+left-over"),
    (32, 1024, 32, "plain, one part each"),
    (304, 1024, 32, "plain, one part each"),
    (80, 1024, 64, "primary+helpers"),
    (128, 1024, 64, "primary+helpers"),
    (32, 5120, 384, "helper with three segments"),
    (64, 2048, 384, "helper with three segments"),
    (128, 3072, 256, "helper with three segments"),
    (304, 5120, 128, "plain, several parts each"),
    (64, 6144, 128, "plain, several parts each"),
]


@pytest.mark.parametrize("G,n,rows,regime", REGIMES, ids=[f"G{g}-n{n}-r{r}" for g, n, r, _ in REGIMES])
def test_cut_regimes_by_workgroup_count(hip, lib_options, G, n, rows, regime):
    """GANQ_HESS_W4_WGS runs the cut of a part with G CUs (MI300X's 304, partition modes) on this one: each regime of the cut --
    no left-over tiles, whole tiles plus left-overs, a plain cut of one-part tiles, a plain cut of multi-part tiles, primaries with
    helpers, a helper range over three tiles -- against float64 and against the launch at the default workgroup count (the fp32
    sums grouped differently: equal to 1e-5)."""
    c = cut_of(hip, n, rows, G)
    assert regime_holds(c, regime), (regime, {k: v for k, v in c.items() if k != "parts"}, c["parts"][:8])
    if n < 3072:
        lib_options(GANQ_HESS_W4=2)
    dtype = torch.bfloat16 if (G // 16) % 2 else torch.float16
    X = make_group(n, rows, dtype, seed=G + n + rows)
    H0 = make_h0(n, seed=G)
    ref = reference(X, 3, 1, H0)
    lib_options(GANQ_HESS_W4_WGS=G)
    assert hip.debug_option_get("GANQ_HESS_W4_WGS") == G
    H = run_transposed(hip, X, 3, 1, H0)
    check_vs_fp64(H, ref, f"G={G} n={n} rows={rows}")
    for _ in range(3):
        assert torch.equal(run_transposed(hip, X, 3, 1, H0), H)
    lib_options(GANQ_HESS_W4_WGS=0)
    Hd = run_transposed(hip, X, 3, 1, H0)
    check_vs_fp64(Hd, ref, f"default G, n={n} rows={rows}")
    assert float((H - Hd).norm() / Hd.norm()) < 1e-5


def test_workspace_is_sized_for_the_forced_workgroup_count(hip, lib_options):
    """the partial-tile area follows GANQ_HESS_W4_WGS, and a workspace sized for fewer workgroups is refused before any launch"""
    n = 4096
    small = hip.lib().ganq_hessian_t_workspace_bytes(n)
    lib_options(GANQ_HESS_W4_WGS=2 * torch.cuda.get_device_properties(0).multi_processor_count)
    big = hip.lib().ganq_hessian_t_workspace_bytes(n)
    assert big - small == torch.cuda.get_device_properties(0).multi_processor_count * 3 * TILE * TILE * 4
    X = make_group(n, 64, torch.float16, seed=1)
    Xt = X.t().contiguous()
    H = torch.zeros(n, n, device="cuda")
    ws = poisoned(small)
    with pytest.raises(hip.GanqHipError):
        hip.hessian_accum_t(H, Xt, 64, 0, 1, workspace=ws)
    with pytest.raises(hip.GanqHipError):  # (the library's own check, past the binding's)
        hip._call("ganq_hessian_accum_t", (H, Xt, ws), H.data_ptr(), Xt.data_ptr(), 64, 0, 64, n, 0, 1, ws.data_ptr(), small, hip._ST)
    torch.cuda.synchronize()
    assert bool((H == 0).all())  # refused before any launch


# ------------------------------------------------------------------------------------------ 3. the quantizer's staging path
def _poisoned_workspaces(monkeypatch, hip):
    monkeypatch.setattr(hip, "_workspace", lambda nbytes, device: poisoned(nbytes).to(device))


@pytest.mark.parametrize("case", ["40+ragged36", "full16384+tail32", "fp16-to-bf16", "expert24"])
@pytest.mark.parametrize("n", [4096, 5120])
def test_quantizer_short_and_ragged_groups_vs_fp64(hip, monkeypatch, n, case):
    """GPTQ.add_batch at default options, through the transposed staging path, with every scratch buffer NaN-poisoned: a group
    flushed by a ragged batch, a full group followed by a short tail, a group flushed by a dtype change, and a module that sees one
    short batch (a mixture-of-experts expert).  Against the float64 running average with N = sequences (gptq.py:96-131)."""
    from ganq_amd.looper.named_module import NamedModule
    from ganq_amd.quantization import GANQ, QuantizeConfig

    _poisoned_workspaces(monkeypatch, hip)
    g = torch.Generator().manual_seed(n + len(case))

    def batch(seqs, tokens, dtype=torch.float16):
        return (torch.randn(seqs, tokens, n, generator=g) * 0.5).to(dtype).cuda()

    if case == "40+ragged36":
        xs = [batch(1, 40), batch(2, 18)]  # 40 tokens staged, then 36: ragged, flushes a 64-token group and goes alone
    elif case == "full16384+tail32":
        xs = [batch(1, 2048) for _ in range(8)] + [batch(1, 32)]  # a full group of 16384 tokens, then a 32-token tail
    elif case == "fp16-to-bf16":
        xs = [batch(1, 48), batch(2, 20), batch(1, 56, torch.bfloat16), batch(1, 32, torch.bfloat16)]
    else:
        xs = [batch(1, 24)]
    lin = torch.nn.Linear(n, 32, bias=False).half().cuda()
    q = GANQ(NamedModule(lin, "fc", "layers.0.fc", 0), QuantizeConfig(bits=4))
    q.quantizer.configure(perchannel=True)
    ref = torch.zeros(n, n, dtype=torch.float64, device="cuda")
    N = 0
    for x in xs:
        q.add_batch(x, None)
        assert q._stage_t, "the layer must take the transposed staging path"
        b = x.shape[0]
        xd = x.reshape(-1, n).double()
        ref = ref * (N / (N + b)) + (2.0 / (N + b)) * (xd.T @ xd)
        N += b
    q.end_of_calibration()
    assert q.nsamples == N
    check_vs_fp64(q.hessian, ref, f"n={n} {case}")


# ------------------------------------------------------------------------------------------ 4. row-major token-split launches
@pytest.mark.parametrize("rows,n,dtype", [(4096, 768, torch.float16), (5000, 1280, torch.bfloat16), (16384, 2048, torch.float16),
                                          (4101, 3072, torch.float16), (4096, 5120, torch.float16)])
def test_hessian_token_split_launches_poisoned_workspace(hip, rows, n, dtype, lib_options):
    """hessian_sk_kernel + hessian_fix_kernel (hessian.hip) with a NaN-poisoned workspace: every partial tile the fix kernel reads
    is one this call wrote (parts >= 2 per cut tile), for the 128 x 128 and 256 x 128 tiles and a cap of 3 parts."""
    X1 = make_group(n, rows, dtype, seed=rows + n)
    X2 = make_group(n, rows, dtype, seed=rows + n + 1)
    H0 = make_h0(n, seed=n)
    ref = (3.0 / 5.0) * H0.double() + (2.0 / 5.0) * (X1.double().T @ X1.double() + X2.double().T @ X2.double())
    ref1 = (2.0 / 3.0) * (X1.double().T @ X1.double())
    for wide, split in ((0, 1), (0, 3), (2, 1), (2, 3)):
        lib_options(GANQ_HESS_WIDE=wide, GANQ_HESS_SPLIT=split)

        def run():
            H = torch.full((n, n), 7.0, device="cuda")  # stale contents must be ignored on the first batch
            hip.hessian_accum(H, X1, 0, 3, workspace=poisoned(hip.lib().ganq_hessian_workspace_bytes(rows, n)))
            first = H.clone()
            H = H0.clone()
            hip.hessian_accum(H, X1, 3, 1, workspace=poisoned(hip.lib().ganq_hessian_workspace_bytes(rows, n)))
            hip.hessian_accum(H, X2, 4, 1, workspace=poisoned(hip.lib().ganq_hessian_workspace_bytes(rows, n)))
            return first, H

        first, H = run()
        check_vs_fp64(first, ref1, f"first batch, wide={wide} split={split}")
        check_vs_fp64(H, ref, f"decayed, wide={wide} split={split}")
        for _ in range(2):
            f2, h2 = run()
            assert torch.equal(f2, first) and torch.equal(h2, H)
