"""Guarded buffers, inputs and the case list for the LUT-forward regime tests (tests/test_hip_lut_regimes.py on the GPU,
tests/test_lut_regime_cases.py without one).  A helper module like tests/eora_fixtures.py, not a conftest.

* `Arena`: ONE uint8 cuda allocation carved into 256-byte aligned tensors, every tensor between two guard bands of 4 KB of its own.
  Guards of floating inputs hold NaNs of the tensor's dtype (a value read past a ragged edge poisons the accumulator it enters), all
  others a fixed byte pattern.  `forward()` calls the C ABI entry itself with a workspace of EXACTLY the sizer's bytes and a y of
  exactly M * m elements pre-filled with a NaN pattern, and asserts afterwards that every byte outside y and the workspace is what
  it was, that no element of y kept the pre-fill and that the 64 KB counter region at the head of the workspace is zero again.
* inputs from numpy on the CPU by seed: `gaussian()` (the distributions of tests/test_hip_lora.py::make) and `integers()`
  (small integers: every fp64 reference value and every element of t = x lora_A^T is an integer of magnitude <= 2048 for fp16,
  <= 256 for bf16 -- the exact result is representable and every fp32 partial sum exact, so ANY regime, split factor or
  summation order has to return the reference bit for bit).
* `CASES`: the covering list of (regime and the developer options that force it, bits, dtype, M, m, n, variant)."""
import zlib
from collections import namedtuple

import numpy as np

REGIMES = ("decode16", "decode32", "mfma_small", "gemm", "gemm_splitk", "gemm_pipe", "dense128", "dense256")
VARIANTS = ("plain", "nobias", "addend", "outliers", "adapter16", "adapter48_outliers")
PAIRS = [(b, d) for b in (2, 3, 4) for d in ("fp16", "bf16")]
# every developer switch that steers the forward's plan: a case resets all of them and sets its own
PLAN_OPTIONS = ("GANQ_LUT_INWG", "GANQ_LUT_NT", "GANQ_LUT_KS", "GANQ_LUT_WGS", "GANQ_LUT_DENSE_M", "GANQ_LUT_GEMM_RM",
                "GANQ_LUT_GEMM_PIPE", "GANQ_GEMM_H16_BM")

M_SMALL = (1, 15, 16, 17, 31, 32, 33, 63, 64)
M_LARGE = (65, 127, 128, 129, 255, 256, 257, 300, 1100)
M_EDGES = M_SMALL + M_LARGE
OUT_EDGES = (1, 4, 15, 16, 17, 31, 33, 64, 127, 128, 129, 130, 255, 257, 1028, 8200)
IN_EDGES = (32, 64, 96, 160, 192, 512, 544, 1056, 2080, 8192)
MAX_SHAPE = (2048, 8200, 8192)
LARGE_PRODUCT = 1100 * 1028 * 2080  # at most four cases may lie above it
INT_LIMIT = {"fp16": 2048, "bf16": 256}

Case = namedtuple("Case", "regime opts bits dtype M m n variant KS")


def case_id(c):
    ks = "-".join(f"{k[5:]}{v}" for k, v in sorted(c.opts.items()))
    return f"{c.regime}-b{c.bits}-{c.dtype}-{c.M}x{c.m}x{c.n}-{c.variant}-{ks}"


def case_seed(c):
    return zlib.crc32(case_id(c).encode())


def rank_of(variant):
    return {"adapter16": 16, "adapter48_outliers": 48}.get(variant, 0)


def has_outliers(variant):
    return variant in ("outliers", "adapter48_outliers")


# ---- what each regime supports (the checks of csrc/lut_linear.hip, lut_gemm.hip, gemm_h16.hip that bound it)
def regime_axes(regime):
    """(M values, m values, n values, variants) a regime can be forced on.
    decode16 / decode32: lut_plan() takes the in-workgroup kernel for M <= 32 only; the 32-feature variant needs an even m and
    M <= 16.  gemm_splitk: a split needs two stages of 64 columns (n >= 96).  gemm_pipe: lut_gemm_pipe() never serves an adapter.
    dense*: gemm_h16_supported() wants m a multiple of 4 and n a multiple of 64; lut_lora_dense() keeps an adapter on the dense
    path from n = 8192 only (below it the adapter layer takes the fused GEMM, which is the gemm regime)."""
    if regime == "decode16":
        return tuple(M for M in M_SMALL if M <= 32), OUT_EDGES, IN_EDGES, VARIANTS
    if regime == "decode32":
        return tuple(M for M in M_SMALL if M <= 16), tuple(m for m in OUT_EDGES if m % 2 == 0), IN_EDGES, VARIANTS
    if regime == "mfma_small":
        return M_SMALL, OUT_EDGES, IN_EDGES, VARIANTS
    if regime == "gemm":
        return M_LARGE, OUT_EDGES, IN_EDGES, VARIANTS
    if regime == "gemm_splitk":
        return M_LARGE, OUT_EDGES, tuple(n for n in IN_EDGES if n >= 96), VARIANTS
    if regime == "gemm_pipe":
        return M_LARGE, OUT_EDGES, IN_EDGES, tuple(v for v in VARIANTS if not rank_of(v))
    return M_LARGE, tuple(m for m in OUT_EDGES if m % 4 == 0), tuple(n for n in IN_EDGES if n % 64 == 0), VARIANTS


def regime_options(regime, ks):
    if regime == "decode16":
        return dict(GANQ_LUT_INWG=1, GANQ_LUT_NT=1, GANQ_LUT_KS=ks)
    if regime == "decode32":
        return dict(GANQ_LUT_INWG=1, GANQ_LUT_NT=2, GANQ_LUT_KS=ks)
    if regime == "mfma_small":  # a workgroup target no shape reaches: GANQ_LUT_KS alone caps the split
        return dict(GANQ_LUT_INWG=0, GANQ_LUT_WGS=1 << 20, GANQ_LUT_KS=ks)
    if regime == "gemm":
        return dict(GANQ_LUT_DENSE_M=0, GANQ_LUT_GEMM_RM=1, GANQ_LUT_GEMM_PIPE=0)
    if regime == "gemm_splitk":
        return dict(GANQ_LUT_DENSE_M=0, GANQ_LUT_GEMM_RM=ks)
    if regime == "gemm_pipe":
        return dict(GANQ_LUT_DENSE_M=0, GANQ_LUT_GEMM_RM=1, GANQ_LUT_GEMM_PIPE=1)
    return dict(GANQ_LUT_DENSE_M=1, GANQ_GEMM_H16_BM=128 if regime == "dense128" else 256)


def expected_ks(regime, n, ks):
    """the split of in_features a forced factor `ks` gives: groups of 32 columns (stages of 64 for the GEMM) are dealt in equal
    shares, so the number of non-empty shares can be smaller than the factor"""
    nkb = n // 32
    if regime in ("decode16", "decode32"):
        units, ks = nkb, max(1, min(ks, nkb))
    elif regime == "mfma_small":
        units, ks = nkb, max(1, min(ks, nkb // 2))
    elif regime == "gemm_splitk":
        units = (nkb + 1) // 2
        ks = min(ks, units)
    else:
        return 1
    per = -(-units // ks)
    return -(-units // per)


KS_FORCED = {"decode16": (1, 2, 3, 5), "decode32": (1, 3, 2, 5), "mfma_small": (1, 3, 5, 2, 8), "gemm_splitk": (2, 3, 8)}


def _case(regime, i, M, m, n, variant, ks=None):
    bits, dtype = PAIRS[i % len(PAIRS)]
    if ks is None:
        forced = KS_FORCED.get(regime, (1,))
        ks = forced[i % len(forced)]
    return Case(regime, regime_options(regime, ks), bits, dtype, M, m, n, variant, expected_ks(regime, n, ks))


def build_cases():
    cases = []
    for regime in REGIMES:
        Ms, ms, ns, variants = regime_axes(regime)
        ms_s = tuple(m for m in ms if m != 8200)  # the two long edges go with short partners below
        ns_s = tuple(n for n in ns if n != 8192)
        plain = tuple(v for v in variants if not rank_of(v)) if regime.startswith("dense") else variants
        L = max(len(Ms), len(ms_s), len(ns_s), len(PAIRS), len(plain))
        # two passes over every axis with different strides: each edge value, (bits, dtype) pair and variant is met, in changing company
        for i in range(L):
            cases.append(_case(regime, i, Ms[i % len(Ms)], ms_s[i % len(ms_s)], ns_s[i % len(ns_s)], plain[i % len(plain)]))
        for i in range(L):
            cases.append(_case(regime, i + 1, Ms[(2 * i + 1) % len(Ms)], ms_s[(i + 5) % len(ms_s)], ns_s[(3 * i + 2) % len(ns_s)],
                               plain[(i + 3) % len(plain)]))
        # the long edges: m = 8200 on short rows of the weight, n = 8192 on few features
        ragged_m = 130 if regime == "decode32" else (128 if regime.startswith("dense") else 129)
        cases.append(_case(regime, 2, Ms[-1], 8200, ns_s[1 if regime.startswith("dense") else 2], plain[0]))
        cases.append(_case(regime, 3, Ms[1], 8200, ns_s[0], plain[1 % len(plain)]))
        for j, v in enumerate(v for v in variants if rank_of(v)):  # (the dense regimes keep an adapter from n = 8192 on only)
            cases.append(_case(regime, 4 + j, Ms[(3 + 4 * j) % len(Ms)], ragged_m if j else 64, 8192, v))
        cases.append(_case(regime, 5, Ms[0], ms_s[2 % len(ms_s)], 8192, plain[2 % len(plain)]))
        # ragged M x ragged m x (n = 32 mod 64) together (the dense regimes need n = 0 mod 64: gemm_h16_supported)
        if not regime.startswith("dense"):
            Mr = 15 if regime in ("decode16", "decode32") else (33 if regime == "mfma_small" else 257)
            for j, n in enumerate((544, 2080, 1056)):
                if n in ns:
                    cases.append(_case(regime, j, Mr, ragged_m, n, variants[(3 + j) % len(variants)],
                                       ks=None if regime not in KS_FORCED else (3, 5, 3)[j]))
    seen, out = set(), []
    for c in cases:
        if case_id(c) not in seen:
            seen.add(case_id(c))
            out.append(c)
    return out


CASES = build_cases()


# ---- inputs (numpy, CPU): dict(x [M,n], Q uint8 [m,n], lut [m,V], bias [m] | None, addend fp32 [M,m] | None,
#      outliers (rowptr, cols, vals) | None, A [r,n] | None, B [m,r] | None); floating arrays are fp32 holding the values to round
def _outlier_csr(rng, m, n, draw):
    """CSR by output feature: every third feature has 1, 2 or 3 entries at distinct ascending columns"""
    counts = np.zeros(m, dtype=np.int64)
    counts[::3] = 1 + (np.arange(0, m, 3) // 3) % 3
    counts = np.minimum(counts, n)
    rowptr = np.zeros(m + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum(counts)
    cols = np.empty(int(rowptr[-1]), dtype=np.int32)
    for o in np.nonzero(counts)[0]:
        cols[rowptr[o]:rowptr[o + 1]] = np.sort(rng.choice(n, size=int(counts[o]), replace=False))
    return rowptr, cols, draw(cols.size).astype(np.float32)


def _variant_parts(inp, rng, variant, M, m, n, addend, outl_vals, lora):
    if variant == "nobias":
        inp["bias"] = None
    if variant == "addend":
        inp["addend"] = addend().astype(np.float32)
    if has_outliers(variant):
        inp["outliers"] = _outlier_csr(rng, m, n, outl_vals)
    r = rank_of(variant)
    if r:
        inp["A"], inp["B"] = lora(r)
    return inp


def gaussian(bits, M, m, n, variant, seed):
    """tests/test_hip_lora.py::make's distributions: the adapter term is about a third of the base term in RMS"""
    rng = np.random.default_rng(seed)
    V = 2 ** bits
    f = np.float32
    inp = dict(Q=rng.integers(0, V, (m, n), dtype=np.uint8), lut=(0.02 * rng.standard_normal((m, V))).astype(f),
               x=rng.standard_normal((M, n)).astype(f), bias=(0.1 * rng.standard_normal(m)).astype(f), addend=None, outliers=None,
               A=None, B=None)
    return _variant_parts(inp, rng, variant, M, m, n, lambda: 0.3 * rng.standard_normal((M, m)),
                          lambda k: 0.1 * rng.standard_normal(k),
                          lambda r: ((rng.standard_normal((r, n)) / n ** 0.5).astype(f),
                                     (rng.standard_normal((m, r)) * (0.02 * n ** 0.5 / (3 * r ** 0.5))).astype(f)))


def integers(bits, M, m, n, variant, seed, dtype):
    """x in {-1, 0, 1}; codebook, bias, addend, outlier values, lora_A and lora_B small integers.  Densities: the base term is a sum
    of n dx products of variance E[w^2] (2 for a codebook in [-2, 2], 2/3 in [-1, 1]): n dx <= 8192 (fp16) keeps its standard
    deviation at 128, n dx <= 1200 (bf16) at 28 -- six to seven of them stay below 2048 / 256 with room for the other terms;
    t = x lora_A^T has variance n dx dA = 4 and the adapter term 2 r."""
    rng = np.random.default_rng(seed)
    V = 2 ** bits
    f = np.float32
    c = 2 if dtype == "fp16" else 1
    dx = min(1.0, (8192 if dtype == "fp16" else 1200) / n)

    def sparse_signs(shape, density):
        return (rng.integers(0, 2, shape) * 2 - 1).astype(f) * (rng.random(shape) < density)

    inp = dict(Q=rng.integers(0, V, (m, n), dtype=np.uint8), lut=rng.integers(-c, c + 1, (m, V)).astype(f), x=sparse_signs((M, n), dx),
               bias=rng.integers(-2, 3, m).astype(f), addend=None, outliers=None, A=None, B=None)
    return _variant_parts(inp, rng, variant, M, m, n, lambda: rng.integers(-3, 4, (M, m)),
                          lambda k: rng.integers(1, 3, k) * (rng.integers(0, 2, k) * 2 - 1),
                          lambda r: (sparse_signs((r, n), min(1.0, 4.0 / (n * dx))), sparse_signs((m, r), 0.5)))


def sparse_dense(inp, m, n):
    Ws = np.zeros((m, n), dtype=np.float32)
    if inp["outliers"] is not None:
        rowptr, cols, vals = inp["outliers"]
        rows = np.repeat(np.arange(m), np.diff(rowptr))
        Ws[rows, cols] = vals
    return Ws


def integer_reference_cpu(inp):
    """(ref [M,m], t [M,r] or None) of integer inputs in fp32: every product and partial sum is an integer below 2^24, so fp32 is
    exact and equals the fp64 reference"""
    Wq = np.take_along_axis(inp["lut"], inp["Q"].astype(np.int64), axis=1)
    m, n = Wq.shape
    ref = inp["x"] @ (Wq + sparse_dense(inp, m, n)).T
    t = None
    if inp["A"] is not None:
        t = inp["x"] @ inp["A"].T
        ref = ref + t @ inp["B"].T
    if inp["addend"] is not None:
        ref = ref + inp["addend"]
    if inp["bias"] is not None:
        ref = ref + inp["bias"]
    return ref, t


# ---- the GPU side
GUARD = 4096
Y_PREFILL = 0x7FFF      # a NaN of fp16 and of bf16 that no arithmetic produces
BYTE_PATTERN = 0xA5
COUNTER_BYTES = 64 * 1024  # LUT_COUNTER_BYTES of csrc/lut_linear.hip: tickets of the LUT kernels, the adapter's in its last 1024 ints


def _torch_dtype(dtype):
    import torch

    return torch.float16 if dtype == "fp16" else torch.bfloat16


class Arena:
    """specs: list of (name, torch dtype, shape, cpu tensor or None, nan_guard).  `t[name]` are views into one allocation."""

    def __init__(self, specs, device="cuda"):
        import torch

        off, self.place = 0, {}
        for name, dt, shape, _, _ in specs:
            nbytes = int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
            start = off + GUARD
            end = -(-(start + nbytes) // 256) * 256 + GUARD
            self.place[name] = (off, start, nbytes, end)
            off = end
        self.buf = torch.empty(off, dtype=torch.uint8, device=device)
        assert self.buf.data_ptr() % 256 == 0
        self.t = {}
        for name, dt, shape, src, nan_guard in specs:
            lo, start, nbytes, hi = self.place[name]
            block = self.buf[lo:hi]
            if nan_guard:  # quiet NaNs of the tensor's own dtype on both sides (4-byte aligned blocks: fp32 patterns fit)
                block.view(dt).fill_(float("nan"))
            else:
                block.fill_(BYTE_PATTERN)
            view = self.buf[start:start + nbytes].view(dt).reshape(shape)
            if src is not None:
                view.copy_(src)
            self.t[name] = view
        self.outputs = ()

    def snapshot(self, outputs):
        """remember every byte outside the data of `outputs`"""
        self.outputs = tuple(outputs)
        self.before = self._masked()

    def _masked(self):
        c = self.buf.clone()
        for name in self.outputs:
            _, start, nbytes, _ = self.place[name]
            c[start:start + nbytes] = 0
        return c

    def assert_untouched(self, what):
        import torch

        after = self._masked()
        if not torch.equal(after, self.before):
            bad = torch.nonzero(after != self.before).flatten()
            first = int(bad[0])
            owner = [n for n, (lo, s, nb, hi) in self.place.items() if lo <= first < hi]
            lo, s, nb, hi = self.place[owner[0]]
            raise AssertionError(f"{what}: {bad.numel()} bytes outside y and the workspace changed; first at byte {first - s} relative "
                                 f"to `{owner[0]}` ({nb} bytes of data)")


def forward(hip, inp, bits, dtype):
    """the C ABI forward of `inp` (dict of numpy arrays) inside an Arena -> (y, device tensors).  Asserts the buffer contract."""
    import torch

    dt = _torch_dtype(dtype)
    M, n = inp["x"].shape
    m = inp["Q"].shape[0]
    V = 2 ** bits
    r = 0 if inp["A"] is None else inp["A"].shape[0]
    lib = hip.lib()
    code = 0 if dtype == "fp16" else 1

    def as_dt(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dt)

    qw = hip.pack_indices(torch.from_numpy(inp["Q"]).cuda(), bits)
    specs = [("x", dt, (M, n), as_dt(inp["x"]), True), ("qweight", torch.int32, tuple(qw.shape), qw, False),
             ("lut", dt, (m, V), as_dt(inp["lut"]), True)]
    if inp["bias"] is not None:
        specs.append(("bias", dt, (m,), as_dt(inp["bias"]), True))
    if inp["addend"] is not None:
        specs.append(("addend", torch.float32, (M, m), torch.from_numpy(inp["addend"]), True))
    if r:
        specs += [("lora_A", dt, (r, n), as_dt(inp["A"]), True), ("lora_B", dt, (m, r), as_dt(inp["B"]), True)]
    if inp["outliers"] is not None:
        rowptr, cols, vals = inp["outliers"]
        specs += [("rowptr", torch.int32, (m + 1,), torch.from_numpy(rowptr), False),
                  ("cols", torch.int32, (max(cols.size, 1),), torch.from_numpy(cols) if cols.size else None, False),
                  ("vals", dt, (max(vals.size, 1),), as_dt(vals) if vals.size else None, True)]
    outl = inp["outliers"] is not None
    if r and outl:
        entry, nbytes = "ganq_lut_linear_fwd_lora_outliers", lib.ganq_lut_linear_lora_outliers_workspace_bytes(M, m, n, bits, r)
    elif r:
        entry, nbytes = "ganq_lut_linear_fwd_lora", lib.ganq_lut_linear_lora_workspace_bytes(M, m, n, bits, r)
    elif outl:
        entry, nbytes = "ganq_lut_linear_fwd_outliers", lib.ganq_lut_linear_outliers_workspace_bytes(M, m, n, bits)
    else:
        entry = "ganq_lut_linear_fwd_add" if inp["addend"] is not None else "ganq_lut_linear_fwd"
        nbytes = lib.ganq_lut_linear_workspace_bytes(M, m, n, bits)
    assert nbytes >= COUNTER_BYTES, (entry, nbytes)
    # y and the workspace in the middle of the arena: what overruns them lands in the guards and the inputs behind, which are compared
    specs[1:1] = [("y", torch.int16, (M, m), None, False), ("ws", torch.uint8, (nbytes,), None, False)]
    arena = Arena(specs)
    t = arena.t
    t["y"].fill_(Y_PREFILL)
    ws = t["ws"]
    hip._call("ganq_lut_linear_workspace_init", (ws,), ws.data_ptr(), nbytes, hip._ST)
    arena.snapshot(("y", "ws"))
    p = {k: v.data_ptr() for k, v in t.items()}
    bias, addend = p.get("bias"), p.get("addend")
    csr = (p["rowptr"], p["cols"] if outl and inp["outliers"][1].size else None, p["vals"] if outl and inp["outliers"][2].size else None) if outl else ()
    tail = (code, M, m, n, bits, p["y"], p["ws"], nbytes, hip._ST)
    tensors = tuple(t.values())
    if r and outl:
        hip._call(entry, tensors, p["x"], p["qweight"], p["lut"], bias, p["lora_A"], p["lora_B"], r, *csr, *tail)
    elif r:
        hip._call(entry, tensors, p["x"], p["qweight"], p["lut"], bias, p["lora_A"], p["lora_B"], r, addend, *tail)
    elif outl:
        hip._call(entry, tensors, p["x"], p["qweight"], p["lut"], bias, *csr, *tail)
    elif inp["addend"] is not None:
        hip._call(entry, tensors, p["x"], p["qweight"], p["lut"], bias, addend, *tail)
    else:
        hip._call(entry, tensors, p["x"], p["qweight"], p["lut"], bias, *tail)
    torch.cuda.synchronize()
    arena.assert_untouched(entry)
    kept = int((t["y"] == Y_PREFILL).sum())
    assert kept == 0, f"{entry}: {kept} of {M * m} elements of y were never written"
    dirty = int(torch.count_nonzero(ws[:COUNTER_BYTES]))
    assert dirty == 0, f"{entry}: {dirty} non-zero bytes left in the 64 KB counter region of the workspace"
    dev = dict(t)
    dev["Q"] = torch.from_numpy(inp["Q"]).cuda()
    dev["outliers"] = (t["rowptr"], t["cols"][:inp["outliers"][1].size], t["vals"][:inp["outliers"][2].size]) if outl else None
    dev["arena"] = arena  # (keeps the allocation the views live in)
    return t["y"].view(dt).clone(), dev


def wrapper(hip, dev, bits):
    """the public binding on the arena's own tensors"""
    x, qw, lut, bias = dev["x"], dev["qweight"], dev["lut"], dev.get("bias")
    if "lora_A" in dev:
        return hip.lut_linear_lora(x, qw, lut, bias, bits, dev["lora_A"], dev["lora_B"], addend=dev.get("addend"), outliers=dev["outliers"])
    if dev["outliers"] is not None:
        return hip.lut_linear_outliers(x, qw, lut, bias, bits, *dev["outliers"])
    return hip.lut_linear(x, qw, lut, bias, bits, addend=dev.get("addend"))


def sparse_product(dev):
    """fp64 [M, m]: x @ W_sparse^T (+ the addend): what the reference functions of the older tests take as `addend`"""
    import torch

    x = dev["x"]
    m, n = dev["Q"].shape
    add = dev["addend"].double() if "addend" in dev else None
    if dev["outliers"] is not None:
        rowptr, cols, vals = dev["outliers"]
        Ws = torch.zeros((m, n), dtype=torch.float64, device=x.device)
        rows = torch.repeat_interleave(torch.arange(m, device=x.device), (rowptr[1:] - rowptr[:-1]).long())
        Ws[rows, cols.long()] = vals.double()
        sp = x.double() @ Ws.T
        add = sp if add is None else add + sp
    return add


def check_gaussian(y, dev, dtype):
    """the project's own fp64 bound: check() of tests/test_hip_lut_gemm.py; with an adapter reference() / flip_slack() / check() of
    tests/test_hip_lora.py"""
    import test_hip_lora
    import test_hip_lut_gemm

    dt = _torch_dtype(dtype)
    add = sparse_product(dev)
    if "lora_A" in dev:
        ref, base, ad, slack = test_hip_lora.reference(dev["x"], dev["Q"], dev["lut"], dev.get("bias"), dev["lora_A"], dev["lora_B"], dt, addend=add)
        if y.numel() >= 4096:  # (an RMS over a handful of outputs says nothing)
            test_hip_lora.visible(base, ad)
        test_hip_lora.check(y, ref, dt, slack)
    else:
        test_hip_lut_gemm.check(y, dev["x"], dev["Q"], dev["lut"], dev.get("bias"), dt, addend=add)


def reference_fp64(dev, dtype):
    """fp64 reference of the forward on the arena's tensors (t rounded once to the activation dtype, as the forward defines it)"""
    import test_hip_lora
    import torch

    dt = _torch_dtype(dtype)
    add = sparse_product(dev)
    if "lora_A" in dev:
        return test_hip_lora.reference(dev["x"], dev["Q"], dev["lut"], dev.get("bias"), dev["lora_A"], dev["lora_B"], dt, addend=add)[0]
    ref = dev["x"].double() @ torch.gather(dev["lut"].double(), 1, dev["Q"].long()).T
    if add is not None:
        ref = ref + add
    if "bias" in dev:
        ref = ref + dev["bias"].double()
    return ref


def run_case(hip, bits, dtype, M, m, n, variant, seed):
    """steps 2 and 3 of the regime tests under whatever options are set: Gaussian inputs inside the fp64 bound and bit-identical
    through the public wrapper, integer inputs bit-exact"""
    import torch

    y, dev = forward(hip, gaussian(bits, M, m, n, variant, seed), bits, dtype)
    check_gaussian(y, dev, dtype)
    assert torch.equal(y, wrapper(hip, dev, bits)), "the public wrapper and the C ABI call on the same tensors differ"
    y, dev = forward(hip, integers(bits, M, m, n, variant, seed, dtype), bits, dtype)
    ref = reference_fp64(dev, dtype)
    assert float(ref.abs().max()) <= INT_LIMIT[dtype]
    want = ref.to(_torch_dtype(dtype))
    if not torch.equal(y, want):
        bad = torch.nonzero(y != want)
        i, j = (int(v) for v in bad[0])
        raise AssertionError(f"integer inputs: {bad.shape[0]} of {y.numel()} outputs differ from the exact result; first y[{i}][{j}] = "
                             f"{float(y[i, j])}, exact {float(want[i, j])}")
