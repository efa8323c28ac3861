"""GanqHipQuantLinear -- LUT-dequant QuantLinear for GANQ on MI355X.

Supersedes the reference's FakeQuantLinear for this path (gptqmodel/nn_modules/qlinear/fake.py:15-89, which
stores the dequantised fp16 weight and runs F.linear): here the layer stores what GANQ actually produced,
  qweight  int32 [in_features * bits / 32, out_features]   bits-wide indices, GPTQ int32 packing along
                                                           in_features (qlinear/__init__.py:508-538)
  lut      fp16  [out_features, 2^bits]                    per-output-channel codebook
  bias     fp16  [out_features] (optional)
and `forward` == `F.linear(x, lut.gather(1, Q), bias)` == FakeQuantLinear.forward on T.gather(1,Q).half().
With the outlier split (`QuantizeConfig.ganq_outlier_ratio`, paper section 3.3) it also stores the exact outliers,
  outlier_rowptr int32 [out_features + 1], outlier_cols int32 [nnz], outlier_vals fp16 [nnz]   (CSR by output feature)
and `forward` == `F.linear(x, lut.gather(1, Q) + W_sparse, bias)`.

With a low-rank adapter (`adapter=Lora(rank=r)`: LoRA / the EoRA adapters `quantize_model` generates) the layer owns two more
fp16 buffers in PEFT orientation, both contiguous along the dimension the kernels reduce over,
  lora_A   fp16  [r, in_features]      lora_B   fp16  [out_features, r]      (r a multiple of 16, at most 256)
and `forward` == round(x Wq^T + x W_sparse^T + t lora_B^T + bias) with t = round(x lora_A^T): fp32 accumulation, ONE rounding of
y; the intermediate t IS rounded once to the activation dtype (it is the matrix-core operand of the second product; the
reference rounds it too).  One library call (`_lib.lut_linear_lora`): t by a small HIP kernel, then the LUT kernel of the
regime runs r / 32 further matrix-core steps on (t, lora_B) -- no library GEMM beside the layer.  A layer without an adapter
makes exactly the calls it made before.

Training (the reference's FakeQuantLinear is an F.linear on a buffer, so autograd reaches its input): with grad mode on and
`x` or `lut` requiring grad, `forward` goes through `_GanqLutLinearFn`, whose backward runs the HIP kernels of
csrc/lut_backward.hip -- dx = dy @ (Wq + W_sparse) (one rounding) and, after `train_codebook(True)`,
dlut[o][v] = sum of dy[b][o] x[b][j] over the j with Q[o][j] == v.  `qweight` (the indices), `bias` and the outlier values
are frozen buffers: they never receive a gradient.  With an adapter the training forward is composed in autograd,
`_GanqLutLinearFn(x) + ((x lora_A^T) lora_B^T)` with the rank-r products as fp32 torch ops (so y is rounded twice there), and
`train_adapter(True)` turns `lora_A` / `lora_B` into fp32 parameters under the same state_dict keys.  Otherwise (inference, no_grad) `forward` makes exactly the call it
always made: same launches, no grad_fn.

`pack()` keeps the reference signature `(linear, scales, zeros, g_idx)` (utils/model.py:552-570): because that
call only carries the dequantised nn.Linear, the indices/codebook are either passed by keyword
(`ganq_indices=`, `ganq_codebook=`, what ganq_amd's processor does) or recovered from the weight itself -- a
GANQ weight row has at most 2^bits distinct values, so sorted-unique values are the codebook.
"""
import math

import torch
import torch.nn as nn

from ... import _lib
from ...adapter import Lora, validate_rank
from . import BaseQuantLinear

BACKEND_GANQ_HIP = "ganq_hip"
GEMV_MAX_ROWS = 64
NLL_CHUNK_BYTES = 256 << 20  # logits (and their fp32 copy) a chunk of GanqHipQuantLinear.nll's chunked path may form; tests lower it


class PickRng:
    """The state of the counter-based generator `GanqHipQuantLinear.pick(..., rng=)` draws its Gumbel noise from inside the kernel
    (Philox4x32-10, csrc/lut_head_pick.hip): an int64 [2] device tensor {seed, offset}, both read as unsigned 64-bit.  A pick is a
    pure function of (inputs, seed, offset) and consumes one unit of offset whatever its shape; the kernel itself advances the
    offset, so a pick captured in a HIP graph samples afresh on every replay.
      .state          the tensor (the kernels read and advance it in place)
      .seed .offset   read it back (a device synchronisation)
    copy / deepcopy give a generator with a tensor of its own at the same state; pickling stores the two integers (and the device)."""
    _MASK = (1 << 64) - 1

    def __init__(self, seed: int, offset: int = 0, device=None):
        seed, offset = int(seed), int(offset)
        if not (0 <= seed <= self._MASK and 0 <= offset <= self._MASK):
            raise ValueError(f"PickRng: seed and offset must lie in [0, 2^64), got {seed}, {offset}")
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"PickRng: the state lives on the GPU, got device {device}")
        signed = [v - (1 << 64) if v >= (1 << 63) else v for v in (seed, offset)]
        self.state = torch.tensor(signed, dtype=torch.int64, device=device)

    @property
    def seed(self) -> int:
        return int(self.state[0].item()) & self._MASK

    @property
    def offset(self) -> int:
        return int(self.state[1].item()) & self._MASK

    @property
    def device(self):
        return self.state.device

    def __reduce__(self):
        return (PickRng, (self.seed, self.offset, str(self.state.device)))

    def __repr__(self):
        return f"PickRng(seed={self.seed}, offset={self.offset}, device='{self.state.device}')"


class GanqHipQuantLinear(BaseQuantLinear):
    SUPPORTS_BITS = [2, 3, 4]
    SUPPORTS_GROUP_SIZE = [-1, 16, 32, 64, 128]  # accepted and ignored, as GANQ ignores it (ganq.py:489-495)
    SUPPORTS_DESC_ACT = [True, False]
    SUPPORTS_SYM = [True, False]
    SUPPORTS_SHARDS = True
    SUPPORTS_TRAINING = True
    SUPPORTS_AUTO_PADDING = False
    SUPPORTS_IN_FEATURES_DIVISIBLE_BY = [32]
    SUPPORTS_OUT_FEATURES_DIVISIBLE_BY = [1]
    SUPPORTS_DEVICES = ["cuda"]  # ROCm presents as "cuda" in torch (models/_const.py:34,46)
    SUPPORTS_PLATFORM = ["linux"]
    SUPPORTS_PACK_DTYPES = [torch.int32]
    SUPPORTS_ADAPTERS = [Lora]
    SUPPORTS_DTYPES = [torch.float16, torch.bfloat16]

    QUANT_TYPE = "ganq_hip"

    def __init__(self, bits: int, group_size: int, sym: bool, desc_act: bool, in_features: int, out_features: int,
                 bias: bool = False, pack_dtype: torch.dtype = torch.int32, adapter=None, outliers: int = 0, **kwargs):
        super().__init__(bits=bits, group_size=group_size, sym=sym, desc_act=desc_act, in_features=in_features,
                         out_features=out_features, bias=bias, pack_dtype=pack_dtype,
                         backend=kwargs.pop("backend", BACKEND_GANQ_HIP), adapter=adapter, **kwargs)
        self.register_buffer("qweight", torch.zeros((in_features * bits // 32, out_features), dtype=torch.int32))
        self.register_buffer("lut", torch.zeros((out_features, 2 ** bits), dtype=torch.float16))
        if bias:
            self.register_buffer("bias", torch.zeros(out_features, dtype=torch.float16))
        else:
            self.bias = None
        self.outliers = int(outliers)  # number of stored outliers (0: plain GANQ layer, no extra buffers)
        if self.outliers:
            self.register_buffer("outlier_rowptr", torch.zeros(out_features + 1, dtype=torch.int32))
            self.register_buffer("outlier_cols", torch.zeros(self.outliers, dtype=torch.int32))
            self.register_buffer("outlier_vals", torch.zeros(self.outliers, dtype=torch.float16))
        self.adapter_rank = 0  # 0: no adapter, no extra buffers
        if adapter is not None:
            self.adapter_rank = validate_rank(adapter.rank, "GanqHipQuantLinear: `adapter`")
            self.register_buffer("lora_A", torch.zeros((self.adapter_rank, in_features), dtype=torch.float16))
            self.register_buffer("lora_B", torch.zeros((out_features, self.adapter_rank), dtype=torch.float16))
            if adapter.lora_A is not None and adapter.lora_B is not None:  # reference attribute orientation: the transposes
                self._set_lora(adapter.lora_A.t(), adapter.lora_B.t())

    def _set_lora(self, A: torch.Tensor, B: torch.Tensor):
        r = self.adapter_rank
        if tuple(A.shape) != (r, self.in_features) or tuple(B.shape) != (self.out_features, r):
            raise ValueError(f"adapter tensors {tuple(A.shape)} / {tuple(B.shape)} do not fit lora_A [{r}, {self.in_features}] / "
                             f"lora_B [{self.out_features}, {r}]")
        self.lora_A = A.detach().to(device=self.lora_A.device, dtype=torch.float16).contiguous()
        self.lora_B = B.detach().to(device=self.lora_B.device, dtype=torch.float16).contiguous()

    def post_init(self):
        pass

    @staticmethod
    def codebook_from_weight(W: torch.Tensor, bits: int):
        """Recover (Q uint8 [m,n], T [m,V]) from a GANQ-quantised weight: per row, the sorted distinct values.
        Raises if a row has more than 2^bits distinct values (then it is not a GANQ weight)."""
        V = 2 ** bits
        m, n = W.shape
        vals, order = torch.sort(W.float(), dim=1)
        new = torch.ones_like(vals, dtype=torch.bool)
        new[:, 1:] = vals[:, 1:] != vals[:, :-1]
        rank = torch.cumsum(new.to(torch.int64), dim=1) - 1
        if int(rank.max()) >= V:
            raise ValueError(f"weight has more than {V} distinct values in a row: not a {bits}-bit GANQ weight")
        T = torch.zeros((m, V), dtype=torch.float32, device=W.device)
        T.scatter_(1, rank, vals)
        Q = torch.empty((m, n), dtype=torch.uint8, device=W.device)
        Q.scatter_(1, order, rank.to(torch.uint8))
        return Q, T

    def pack(self, linear: nn.Module, scales: torch.Tensor = None, zeros: torch.Tensor = None,
             g_idx: torch.Tensor = None, ganq_indices: torch.Tensor = None, ganq_codebook: torch.Tensor = None,
             ganq_outliers=None, ganq_lora=None):
        """ganq_lora: (lora_A [r, in_features], lora_B [out_features, r]) of a layer built with `adapter=Lora(rank=r)`"""
        if self.adapter_rank and ganq_lora is None and getattr(self.adapter, "lora_A", None) is None:
            raise ValueError("a layer with an adapter cannot be recovered from its weight: pass ganq_lora= (or build the layer "
                             "from an adapter object that carries lora_A / lora_B)")
        if ganq_lora is not None:
            if not self.adapter_rank:
                raise ValueError("ganq_lora= given to a layer that was built without an adapter")
            self._set_lora(*ganq_lora)
        W = linear.weight.data
        if type(linear).__name__ == "Conv1D":
            W = W.t()
        dev = self.qweight.device  # the packing kernel runs where the layer lives
        if dev.type != "cuda":
            dev = W.device if W.is_cuda else torch.device("cuda", torch.cuda.current_device())
        if self.outliers and ganq_outliers is None:
            raise ValueError("a layer with outliers cannot be recovered from its weight: pass ganq_outliers=")
        if ganq_indices is None or ganq_codebook is None:
            ganq_indices, ganq_codebook = self.codebook_from_weight(W.to(dev), self.bits)
        Q = ganq_indices.to(device=dev, dtype=torch.uint8).contiguous()
        if Q.shape != (self.out_features, self.in_features):
            raise ValueError(f"indices shape {tuple(Q.shape)} != ({self.out_features}, {self.in_features})")
        self.qweight = _lib.pack_indices(Q, self.bits).to(self.qweight.device)
        self.lut = ganq_codebook.to(dtype=torch.float16).to(self.lut.device).contiguous()
        if self.bias is not None:
            self.bias[:] = linear.bias.to(self.bias.device, dtype=self.bias.dtype)
        else:
            assert linear.bias is None
        if self.outliers:
            rowptr, cols, vals = ganq_outliers
            if cols.numel() != self.outliers or rowptr.numel() != self.out_features + 1:
                raise ValueError("ganq_outliers do not match the layer's outlier count / out_features")
            self.outlier_rowptr = rowptr.to(device=self.qweight.device, dtype=torch.int32).contiguous()
            self.outlier_cols = cols.to(device=self.qweight.device, dtype=torch.int32).contiguous()
            self.outlier_vals = vals.to(device=self.qweight.device, dtype=torch.float16).contiguous()

    def _sparse_dense(self, dtype) -> torch.Tensor:
        """W_sparse as a dense [out_features, in_features] matrix (prefill path / dequantize_weight)"""
        Ws = torch.zeros((self.out_features, self.in_features), dtype=dtype, device=self.outlier_cols.device)
        rows = torch.repeat_interleave(torch.arange(self.out_features, device=Ws.device),
                                       (self.outlier_rowptr[1:] - self.outlier_rowptr[:-1]).long())
        Ws[rows, self.outlier_cols.long()] = self.outlier_vals.to(dtype)
        return Ws

    def dequantize_weight(self) -> torch.Tensor:
        """[out_features, in_features] in the lut dtype == the FakeQuantLinear weight"""
        Wq = _lib.lut_dequant(self.qweight, self.lut, self.in_features, self.bits)
        return Wq + self._sparse_dense(Wq.dtype) if self.outliers else Wq

    def merged_weight(self) -> torch.Tensor:
        """dequantize_weight() + lora_B @ lora_A: the dense weight the layer's forward is equivalent to (tests, export)"""
        W = self.dequantize_weight()
        if not self.adapter_rank:
            return W
        return (W.float() + self.lora_B.detach().float() @ self.lora_A.detach().float()).to(W.dtype)

    def train_adapter(self, enabled: bool = True):
        """enabled: `lora_A` / `lora_B` become fp32 nn.Parameters (master copies; the training forward uses them in fp32).
        False: back to fp16 buffers, rounded once.  Names and so the state_dict keys stay `lora_A` / `lora_B`."""
        if not self.adapter_rank:
            raise ValueError("train_adapter: the layer has no adapter")
        for name in ("lora_A", "lora_B"):
            t = getattr(self, name).detach()
            delattr(self, name)
            if enabled:
                setattr(self, name, nn.Parameter(t.to(torch.float32).clone()))
            else:
                self.register_buffer(name, t.to(torch.float16).contiguous())
        return self

    def train_codebook(self, enabled: bool = True):
        """enabled: `lut` becomes an fp32 nn.Parameter (the master copy; each forward rounds it to the activation dtype and
        its gradient passes straight through that rounding).  False: back to an fp16 buffer, rounded once.  The name and so
        the state_dict key stay `lut`."""
        lut = self.lut.detach()
        delattr(self, "lut")
        if enabled:
            self.lut = nn.Parameter(lut.to(torch.float32).clone())
        else:
            self.register_buffer("lut", lut.to(torch.float16).contiguous())
        return self

    def _outliers_t(self, dtype):
        """W_sparse^T as CSR by input feature (rowptr [n+1], cols = output features, vals in `dtype`), built once on the device
        (nnz = self.outliers is known: no host read) and cached; vals follow the buffer if it is replaced"""
        cache = getattr(self, "_csr_t", None)
        key = (self.outlier_cols.data_ptr(), self.outlier_vals.data_ptr(), self.outlier_rowptr.data_ptr())
        if cache is None or cache[0] != key:
            dev = self.outlier_cols.device
            m, n, nnz = self.out_features, self.in_features, self.outliers
            counts = (self.outlier_rowptr[1:] - self.outlier_rowptr[:-1]).long()
            rows = torch.repeat_interleave(torch.arange(m, device=dev), counts, output_size=nnz)
            cols = self.outlier_cols.long()
            order = torch.argsort(cols * m + rows)
            rowptr_t = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            rowptr_t.index_add_(0, cols + 1, torch.ones_like(cols))
            rowptr_t = torch.cumsum(rowptr_t, 0).to(torch.int32)
            cache = (key, rowptr_t, rows[order].to(torch.int32).contiguous(), order, {})
            self._csr_t = cache
        _, rowptr_t, cols_t, order, vals_by_dtype = cache
        if dtype not in vals_by_dtype:
            vals_by_dtype[dtype] = self.outlier_vals[order].to(dtype).contiguous()
        return rowptr_t, cols_t, vals_by_dtype[dtype]

    def _lora_as(self, dtype):
        """(lora_A, lora_B) in the activation dtype for the inference call: the buffers themselves when they have it, else a copy
        converted once and kept until a factor is replaced or written in place (bf16 activations, train_adapter's fp32 masters)"""
        A, B = self.lora_A.detach(), self.lora_B.detach()
        if A.dtype == dtype and B.dtype == dtype:
            return A, B
        key = (dtype, A.data_ptr(), A._version, B.data_ptr(), B._version)
        cache = getattr(self, "_lora_cache", None)
        if cache is None or cache[0] != key:
            cache = (key, A.to(dtype).contiguous(), B.to(dtype).contiguous())
            object.__setattr__(self, "_lora_cache", cache)
        return cache[1], cache[2]

    def _lut_forward(self, x2: torch.Tensor, lut: torch.Tensor, bias, lora=None):
        if lora is not None:
            # adapter: t = x lora_A^T and the r / 32 further steps of the LUT kernel in one library call; the outliers of a layer go
            # with it (inside the decode launch at decode sizes, as the fp32 addend otherwise)
            outl = None
            if self.outliers:
                vals = self.outlier_vals if self.outlier_vals.dtype == x2.dtype else self.outlier_vals.to(x2.dtype)
                outl = (self.outlier_rowptr, self.outlier_cols, vals)
            return _lib.lut_linear_lora(x2, self.qweight, lut, bias, self.bits, lora[0], lora[1], outliers=outl)
        # one C-ABI entry for every batch size: the decode kernels up to 64 rows, the fused LUT-dequant GEMM above
        # (csrc/lut_gemm.hip) -- the dequantised weight is never materialised and no library GEMM is called
        if self.outliers:  # x @ W_sparse^T in fp32, added inside the LUT kernel before its one rounding
            vals = self.outlier_vals if self.outlier_vals.dtype == x2.dtype else self.outlier_vals.to(x2.dtype)
            return _lib.lut_linear_outliers(x2, self.qweight, lut, bias, self.bits, self.outlier_rowptr, self.outlier_cols, vals)
        return _lib.lut_linear(x2, self.qweight, lut, bias, self.bits)

    def _inference_forward(self, x2: torch.Tensor, lut: torch.Tensor = None):
        """the inference call on x2 [M, in_features]: no grad_fn; the codebook (default: the layer's) rounded to the activation dtype"""
        lut, bias = self.lut if lut is None else lut, self.bias
        if lut.dtype != x2.dtype:
            lut = lut.to(x2.dtype)
            bias = None if bias is None else bias.to(x2.dtype)
        if not self.adapter_rank:
            return self._lut_forward(x2, lut, bias)
        return self._lut_forward(x2, lut.detach(), bias, self._lora_as(x2.dtype))

    def forward(self, x: torch.Tensor):
        if not x.is_cuda:
            raise _lib.GanqHipError("GanqHipQuantLinear runs on the GPU only (no CPU fallback)")
        out_shape = x.shape[:-1] + (self.out_features,)
        x2 = x.reshape(-1, self.in_features)
        if not self.adapter_rank:
            if torch.is_grad_enabled() and (x.requires_grad or self.lut.requires_grad):
                return _GanqLutLinearFn.apply(x2, self.lut, self).reshape(out_shape)
            return self._inference_forward(x2).reshape(out_shape)
        if torch.is_grad_enabled() and (x.requires_grad or self.lut.requires_grad or self.lora_A.requires_grad
                                        or self.lora_B.requires_grad):
            # training: the adapter term in autograd around the LUT function (rank-r products, fp32)
            y = _GanqLutLinearFn.apply(x2, self.lut, self)
            t = x2.float() @ self.lora_A.float().t()
            return (y + (t @ self.lora_B.float().t()).to(y.dtype)).reshape(out_shape)
        return self._inference_forward(x2).reshape(out_shape)

    # ---- per-token negative log-likelihood of the layer as an output head, without the full logits
    def _nll_chunk_rows(self, itemsize: int) -> int:
        """rows per chunk of the chunked path: the chunk's logits and their fp32 copy stay under NLL_CHUNK_BYTES, at least 64 rows"""
        return max(64, NLL_CHUNK_BYTES // (self.out_features * (itemsize + 4)))

    def _nll_forward(self, x2: torch.Tensor, targets: torch.Tensor, fused: bool, lut: torch.Tensor = None):
        """(nll, lse) fp32 [M] of x2 [M, in_features] and int64 targets [M]; no graph is built"""
        with torch.no_grad():
            if fused:
                lut, bias = self.lut if lut is None else lut, self.bias
                if lut.dtype != x2.dtype:
                    lut = lut.to(x2.dtype)
                    bias = None if bias is None else bias.to(x2.dtype)
                nll, lse, _ = _lib.lut_head_nll(x2, self.qweight, lut.detach(), bias, self.bits, targets)
                return nll, lse
            M = x2.shape[0]
            nll = torch.empty(M, dtype=torch.float32, device=x2.device)
            lse = torch.empty(M, dtype=torch.float32, device=x2.device)
            step = self._nll_chunk_rows(x2.element_size())
            for r in range(0, M, step):
                logits = self._inference_forward(x2[r:r + step], lut).float()
                t = targets[r:r + step]
                hit = (t >= 0) & (t < self.out_features)
                l = torch.logsumexp(logits, dim=-1)
                tl = logits.gather(1, t.clamp(0, self.out_features - 1).unsqueeze(1)).squeeze(1)
                lse[r:r + step] = l
                nll[r:r + step] = torch.where(hit, l - tl, torch.zeros_like(l))
            return nll, lse

    def nll(self, x: torch.Tensor, targets: torch.Tensor, fused=None):
        """Per-token negative log-likelihood -log softmax(layer(x))[target] of the layer as an output head: x [..., in_features],
        integer targets of shape x.shape[:-1] -> fp32 of that shape.  A target outside [0, out_features) (-100 included) marks an
        ignored token: 0.  The [tokens, out_features] logits are never formed:
          fused (the default of a layer with neither outliers nor an adapter; True on any other layer raises): one library call
            (csrc/lut_head_nll.hip) reduces the fp32 logits tile by tile, nothing of them is written;
          chunked (fused=False, and the default of every other layer): rows go through the ordinary forward in chunks whose logits
            stay under NLL_CHUNK_BYTES, torch.logsumexp on the fp32 chunk.
        With grad mode on and x or lut requiring grad the call goes through `_GanqLutNllFn`: dx and dlut from the HIP gradients of
        the ordinary forward, the logits recomputed chunk by chunk.  An adapter in training raises: train it through forward()."""
        if not x.is_cuda:
            raise _lib.GanqHipError("GanqHipQuantLinear runs on the GPU only (no CPU fallback)")
        if targets.is_floating_point() or targets.dtype == torch.bool:
            raise TypeError(f"GanqHipQuantLinear.nll: targets must be integers, got {targets.dtype}")
        if tuple(targets.shape) != tuple(x.shape[:-1]):
            raise ValueError(f"GanqHipQuantLinear.nll: targets {tuple(targets.shape)} do not fit x {tuple(x.shape)}")
        can_fuse = not self.outliers and not self.adapter_rank
        if fused is None:
            fused = can_fuse
        elif fused and not can_fuse:
            raise ValueError("GanqHipQuantLinear.nll: fused=True serves a layer with neither outliers nor an adapter; this layer takes "
                             "the chunked path (fused=False or None)")
        x2 = x.reshape(-1, self.in_features)
        t1 = targets.reshape(-1).to(device=x.device, dtype=torch.int64)
        if torch.is_grad_enabled():
            if self.adapter_rank and (self.lora_A.requires_grad or self.lora_B.requires_grad):
                raise NotImplementedError("GanqHipQuantLinear.nll has no gradient for a trainable adapter: train lora_A / lora_B through "
                                          "the ordinary forward, F.cross_entropy(layer(x).float(), targets)")
            if x.requires_grad or self.lut.requires_grad:
                return _GanqLutNllFn.apply(x2, self.lut, t1, self, bool(fused)).reshape(targets.shape)
        return self._nll_forward(x2, t1, bool(fused))[0].reshape(targets.shape)

    # ---- the next token of the layer as an output head, without the full logits
    @torch.no_grad()
    def pick(self, x: torch.Tensor, temperature: float = 0.0, generator=None, noise: torch.Tensor = None, fused=None, rng: PickRng = None):
        """The next token of the layer as an output head: x [..., in_features] -> (token int64, logprob fp32) of shape x.shape[:-1].
          temperature == 0: greedy, token = argmax of the logits (the smallest index among equals in the fused path), logprob its
            plain log-softmax value;
          temperature > 0: a token sampled from softmax(logits / temperature) by the Gumbel-max rule, token = argmax of
            logits / temperature + noise, logprob = log_softmax(logits / temperature)[token].  noise: fp32 [..., out_features]; by
            default -log(E) with E = torch.empty(M, out_features).exponential_(generator=generator), clamped away from 0.
          rng (a PickRng on x's device, instead of generator / noise): the noise is a function of (rng.seed, rng.offset, row,
            feature) and the call advances rng.offset by one, on the device.  In the fused path the kernel draws it in its epilogue
            -- no [M, out_features] tensor exists and the call can be captured in a HIP graph, every replay a fresh sample; the
            composition fills a buffer with the same noise (`_lib.lut_head_pick_noise`) and advances the state with one torch op.
            temperature == 0 ignores rng and leaves it untouched.
          fused (the default of a layer with neither outliers nor an adapter; True on any other layer raises): one library call
            (csrc/lut_head_pick.hip) reduces the unrounded fp32 logits tile by tile, the same logits `nll` uses: at temperature 1
            logprob and -nll(x, token) are the same number up to the order of the sums;
          composition (fused=False, and the default of every other layer): rows go through the ordinary forward in chunks whose
            logits stay under NLL_CHUNK_BYTES, torch.logsumexp / torch.argmax on the fp32 chunk; ties are torch.argmax's.
        The call always runs under torch.no_grad() and its outputs carry no graph: the gradient of a rollout's logprob is taken in
        the training pass, through nll(x, token)."""
        if not x.is_cuda:
            raise _lib.GanqHipError("GanqHipQuantLinear runs on the GPU only (no CPU fallback)")
        temperature = float(temperature)
        if not math.isfinite(temperature) or temperature < 0:
            raise ValueError(f"GanqHipQuantLinear.pick: temperature must be finite and >= 0, got {temperature}")
        can_fuse = not self.outliers and not self.adapter_rank
        if fused is None:
            fused = can_fuse
        elif fused and not can_fuse:
            raise ValueError("GanqHipQuantLinear.pick: fused=True serves a layer with neither outliers nor an adapter; this layer takes "
                             "the composition (fused=False or None)")
        if rng is not None:
            if not isinstance(rng, PickRng):
                raise TypeError(f"GanqHipQuantLinear.pick: rng must be a PickRng, got {type(rng).__name__}")
            if generator is not None or noise is not None:
                raise ValueError("GanqHipQuantLinear.pick: rng draws the noise itself; pass it without generator and noise")
            if rng.state.device != x.device:
                raise ValueError(f"GanqHipQuantLinear.pick: the rng state lives on {rng.state.device}, x on {x.device}")
        shape = tuple(x.shape[:-1])
        x2 = x.detach().reshape(-1, self.in_features)
        M, m = x2.shape[0], self.out_features
        seeded = rng is not None and temperature > 0 and M > 0
        if noise is not None:
            if noise.dtype != torch.float32:
                raise TypeError(f"GanqHipQuantLinear.pick: noise must be float32, got {noise.dtype}")
            if tuple(noise.shape) != shape + (m,):
                raise ValueError(f"GanqHipQuantLinear.pick: noise {tuple(noise.shape)} does not fit x {tuple(x.shape)} and {m} out_features")
            noise = noise.detach().to(x.device).reshape(M, m)
        inv_t = 1.0
        if temperature > 0:
            inv_t = 1.0 / temperature
            if seeded:
                if not fused:
                    noise = _lib.lut_head_pick_noise(rng.state, M, m)
            elif noise is None:
                e = torch.empty(M, m, dtype=torch.float32, device=x.device).exponential_(generator=generator)
                noise = e.clamp_min_(torch.finfo(torch.float32).tiny).log_().neg_()
        if fused:
            lut, bias = self.lut.detach(), self.bias
            if lut.dtype != x2.dtype:
                lut = lut.to(x2.dtype)
                bias = None if bias is None else bias.to(x2.dtype)
            if seeded:
                token, _, _, logprob = _lib.lut_head_pick_seeded(x2, self.qweight, lut, bias, self.bits, rng.state, inv_t, advance=True)
            else:
                token, _, _, logprob = _lib.lut_head_pick(x2, self.qweight, lut, bias, self.bits, noise, inv_t)
            return token.reshape(shape), logprob.reshape(shape)
        token = torch.empty(M, dtype=torch.int64, device=x2.device)
        logprob = torch.empty(M, dtype=torch.float32, device=x2.device)
        step = self._nll_chunk_rows(x2.element_size())
        for r in range(0, M, step):
            s = self._inference_forward(x2[r:r + step]).float() * inv_t
            t = torch.argmax(s if noise is None else s + noise[r:r + step], dim=-1)
            token[r:r + step] = t
            logprob[r:r + step] = s.gather(1, t.unsqueeze(1)).squeeze(1) - torch.logsumexp(s, dim=-1)
        if seeded:
            rng.state[1:].add_(1)  # one call, one unit of offset (two's complement: the unsigned sum)
        return token.reshape(shape), logprob.reshape(shape)


class _GanqLutLinearFn(torch.autograd.Function):
    """y = F.linear(x, lut.gather(1, Q) + W_sparse, bias) with HIP gradients for x and lut; x is [M, in_features]"""

    @staticmethod
    def forward(ctx, x2, lut_in, layer):
        lut, bias = lut_in, layer.bias
        if lut.dtype != x2.dtype:
            lut = lut.to(x2.dtype)
            bias = None if bias is None else bias.to(x2.dtype)
        y = layer._lut_forward(x2, lut, bias)
        ctx.layer = layer
        ctx.lut_dtype = lut_in.dtype
        ctx.save_for_backward(lut, x2 if ctx.needs_input_grad[1] else None)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        lut, x2 = ctx.saved_tensors
        dx, dlut = _lut_linear_backward(ctx.layer, dy, lut, x2, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        if dlut is not None and dlut.dtype != ctx.lut_dtype:
            dlut = dlut.to(ctx.lut_dtype)
        return dx, dlut, None


def _lut_linear_backward(layer, dy, lut, x2, need_dx: bool, need_dlut: bool):
    """the HIP gradients of y = F.linear(x, lut.gather(1, Q) + W_sparse) for dy [M, out_features]: dx in lut's dtype (one rounding)
    and dlut fp32 [out_features, V]; `lut` in the activation dtype, x2 [M, in_features] (only read for dlut)"""
    dy = dy.contiguous()  # (y.sum().backward() hands over a stride-0 gradient)
    if dy.dtype != lut.dtype:
        dy = dy.to(lut.dtype)
    dx = dlut = None
    if need_dx:
        addend = None
        if layer.outliers:  # dy @ W_sparse in fp32, added before the kernel's one rounding
            rowptr_t, cols_t, vals_t = layer._outliers_t(dy.dtype)
            addend = _lib.outlier_matmul(dy, rowptr_t, cols_t, vals_t, layer.in_features)
        dx = _lib.lut_linear_bwd_input(dy, layer.qweight, lut, layer.bits, addend)
    if need_dlut:
        dlut = _lib.lut_linear_bwd_lut(dy, x2, layer.qweight, layer.bits, layer.out_features)
    return dx, dlut


class _GanqLutNllFn(torch.autograd.Function):
    """nll = layer.nll(x, targets) for x2 [M, in_features] with the HIP gradients of the ordinary forward for x and lut.  The forward
    is the inference call (fused or chunked); the backward walks the row chunks of the chunked path in ascending order: it recomputes a
    chunk's logits with the inference forward, forms g = (softmax - onehot(target)) * dnll in fp32 (0 for ignored rows), rounds it once
    to the activation dtype and hands it to `_lut_linear_backward`; dlut accumulates in fp32 over the chunks.  Deterministic.
    The softmax is normalised by the recomputed chunk itself, not by the forward's lse: the fused forward reduces UNROUNDED logits,
    the recomputed ones are rounded to the activation dtype, and exp(rounded - lse of the unrounded) misses a row sum of 1 by the
    averaged rounding error (1e-4 relative, measured) -- a gradient component along the all-ones direction that is not there."""

    @staticmethod
    def forward(ctx, x2, lut_in, targets, layer, fused):
        nll, _ = layer._nll_forward(x2, targets, fused, lut_in)
        ctx.layer = layer
        ctx.save_for_backward(x2, lut_in, targets)
        return nll

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dnll):
        layer = ctx.layer
        x2, lut_in, targets = ctx.saved_tensors
        need_dx, need_dlut = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        lut = lut_in.detach() if lut_in.dtype == x2.dtype else lut_in.detach().to(x2.dtype)
        m, M = layer.out_features, x2.shape[0]
        dnll = dnll.float()
        step = layer._nll_chunk_rows(x2.element_size())
        dxs, dlut = [], None
        for r in range(0, M, step):
            xc, t = x2[r:r + step], targets[r:r + step]
            g = torch.softmax(layer._inference_forward(xc, lut).float(), dim=-1)
            hit = (t >= 0) & (t < m)
            g.scatter_add_(1, t.clamp(0, m - 1).unsqueeze(1), -hit.to(g.dtype).unsqueeze(1))
            g = (g * torch.where(hit, dnll[r:r + step], torch.zeros_like(dnll[r:r + step])).unsqueeze(1)).to(x2.dtype)
            dx_c, dlut_c = _lut_linear_backward(layer, g, lut, xc, need_dx, need_dlut)
            if need_dx:
                if layer.adapter_rank:  # a frozen adapter: its rank-r products in fp32, as the training forward composes them
                    gf = g.float()
                    dx_c = (dx_c.float() + (gf @ layer.lora_B.detach().float()) @ layer.lora_A.detach().float()).to(dx_c.dtype)
                dxs.append(dx_c)
            if need_dlut:
                dlut = dlut_c if dlut is None else dlut.add_(dlut_c)
        dx = torch.cat(dxs, dim=0) if need_dx else None
        if dlut is not None and dlut.dtype != lut_in.dtype:
            dlut = dlut.to(lut_in.dtype)
        return dx, dlut, None, None, None


class _PackedLookup:
    """What the two packed embedding modules share.  A module provides `dtype`, `padding_idx`, `num_embeddings`, `_codebook()` (the
    tensor that trains), `_lookup(ids)` (the inference launch) and `_lookup_bwd_lut(ids, dy)` (the codebook gradient of that launch)."""

    def _as_dtype(self, slot: str, t: torch.Tensor) -> torch.Tensor:
        """`t` in the output dtype: the buffer itself when it has it, else a copy converted once and kept until the buffer is
        replaced or written in place (like GanqHipQuantLinear._lora_as)"""
        t = t.detach()
        if t.dtype == self.dtype:
            return t
        key = (self.dtype, t.data_ptr(), t._version)
        cache = self.__dict__.get(slot)
        if cache is None or cache[0] != key:
            cache = (key, t.to(self.dtype).contiguous())
            object.__setattr__(self, slot, cache)
        return cache[1]

    def _int64_ids(self, ids: torch.Tensor) -> torch.Tensor:
        if not ids.is_cuda:
            raise _lib.GanqHipError(f"{type(self).__name__} runs on the GPU only (no CPU fallback)")
        if ids.dtype != torch.int64:
            if ids.is_floating_point() or ids.dtype == torch.bool:
                raise TypeError(f"{type(self).__name__}: ids must be integers, got {ids.dtype}")
            ids = ids.long()
        return ids

    def _padding_id(self):
        """`padding_idx` as an id in [0, num_embeddings), or None.  A negative one counts from the end and one outside the table is
        refused, both as nn.Embedding does at construction."""
        pad = self.padding_idx
        if pad is None:
            return None
        pad = int(pad)
        if not -self.num_embeddings <= pad < self.num_embeddings:
            raise ValueError(f"{type(self).__name__}: padding_idx={pad} is outside a table of {self.num_embeddings} rows")
        return pad + self.num_embeddings if pad < 0 else pad

    def forward(self, ids: torch.Tensor):
        ids = self._int64_ids(ids)
        lut = self._codebook()
        if torch.is_grad_enabled() and lut.requires_grad:
            return _GanqLutLookupFn.apply(lut, ids, self)
        return self._lookup(ids)


class GanqHipQuantEmbedding(_PackedLookup, nn.Module):
    """The input embedding of a model whose embedding table is tied to a quantized output head (`QuantizeConfig.lm_head` with
    `ganq_tied_embedding="share"`): `forward(ids)` is row `id` of `head.dequantize_weight()`, gathered out of the head's packed
    stream by one HIP launch (csrc/lut_embedding.hip).  The head's outliers are part of the row; its adapter is not -- an adapter
    corrects the head's OUTPUT under the head's inputs and has no meaning for a lookup.

    The module owns no tensor: it keeps an unregistered reference to the head and reads `qweight`, `lut` and the outlier CSR when it
    is called, so `state_dict()` gains no key, `.to()` of the model moves everything once and a checkpoint holds one table.  Ids of
    any shape give `[..., in_features]` in `dtype` (the dtype of the table this module replaced: fp16 or bf16); an id outside the
    vocabulary gives a row of zeros.

    Training: after `head.train_codebook(True)`, with grad mode on, `forward` goes through `_GanqLutLookupFn`: the same launch, the
    same bits, and a backward (csrc/lut_table_backward.hip) that bins the incoming gradient of every occurrence of a row by the row's
    own codes.  That gradient arrives in `head.lut.grad`, where autograd adds it to the term of the head's own forward: head and
    embedding are one table.  The row `padding_idx` gets none (as in nn.Embedding); the indices and the head's outliers are frozen.
    In every other case (inference, no_grad, a buffer codebook) the output has no grad_fn."""

    def __init__(self, head: GanqHipQuantLinear, dtype: torch.dtype = torch.float16, padding_idx=None):
        super().__init__()
        if not isinstance(head, GanqHipQuantLinear):
            raise TypeError(f"GanqHipQuantEmbedding reads a GanqHipQuantLinear, got {type(head).__name__}")
        if dtype not in (torch.float16, torch.bfloat16):
            raise NotImplementedError(f"GanqHipQuantEmbedding: a table of {dtype} cannot be shared with the packed head "
                                      f"(float16 and bfloat16 can)")
        object.__setattr__(self, "_head", head)  # not a submodule: nothing of the head is registered twice
        self.num_embeddings, self.embedding_dim = head.out_features, head.in_features
        self.dtype = dtype
        self.padding_idx = padding_idx  # (nn.Embedding's forward does not read it either: it only masks the gradient)

    @property
    def head(self) -> GanqHipQuantLinear:
        return self._head

    def _codebook(self) -> torch.Tensor:
        return self._head.lut

    def _lookup(self, ids: torch.Tensor) -> torch.Tensor:
        head = self._head
        outl = None
        if head.outliers:
            outl = (head.outlier_rowptr, head.outlier_cols, self._as_dtype("_vals_cache", head.outlier_vals))
        return _lib.lut_embedding(ids, head.qweight, self._as_dtype("_lut_cache", head.lut), head.in_features, head.bits, outliers=outl)

    def _lookup_bwd_lut(self, ids: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
        head = self._head
        return _lib.lut_embedding_bwd_lut(ids, dy, head.qweight, head.in_features, head.bits, padding_idx=self._padding_id())

    def extra_repr(self) -> str:
        return f"{self.num_embeddings}, {self.embedding_dim}, bits={self._head.bits}, dtype={self.dtype}"


class GanqHipPackedEmbedding(_PackedLookup, nn.Module):
    """An input embedding quantized on its own (`QuantizeConfig.ganq_embedding`): it owns
      qweight_rows  int32 [num_embeddings, embedding_dim * bits / 32]   the row-packed indices: row `id` is the bit stream column `id`
                                                                        of a GanqHipQuantLinear's `qweight` would hold, so a
                                                                        token's row is embedding_dim * bits / 8 contiguous bytes
      lut           fp16  [num_embeddings, 2^bits]                      per-row codebook
    and `forward(ids)` is `lut[id][Q[id][:]]`, one HIP launch (csrc/lut_table.hip).  Ids of any shape give `[..., embedding_dim]` in
    `dtype` (the dtype of the table this module replaced: fp16 or bf16; the codebook is converted once and kept); an id outside the
    vocabulary gives a row of zeros.  `padding_idx` is kept for the record and not read (nn.Embedding's forward does not read it
    either: it only masks the gradient).

    Training: `train_codebook(True)` turns `lut` into an fp32 nn.Parameter; with grad mode on `forward` then goes through
    `_GanqLutLookupFn`: the same launch and the same bits (the codebook rounded to `dtype`, its gradient passing straight through that
    rounding), and a backward (csrc/lut_table_backward.hip) that bins the incoming gradient of every occurrence of a row by the row's
    own codes; the row `padding_idx` gets none, as in nn.Embedding.  The indices are frozen.  In every other case (inference, no_grad,
    a buffer codebook) the output has no grad_fn.

    It has no adapter (an adapter corrects a layer's output under its inputs; a lookup has none) and no outliers: the outlier split of
    `ganq_outlier_ratio` is not applied to embeddings."""

    SUPPORTS_BITS = [2, 3, 4]

    def __init__(self, num_embeddings: int, embedding_dim: int, bits: int, dtype: torch.dtype = torch.float16, padding_idx=None):
        super().__init__()
        if bits not in self.SUPPORTS_BITS:
            raise NotImplementedError(f"GanqHipPackedEmbedding: bits={bits} not supported ({self.SUPPORTS_BITS} are)")
        if embedding_dim % 32 != 0:
            raise NotImplementedError(f"GanqHipPackedEmbedding: embedding_dim={embedding_dim} must be a multiple of 32")
        if dtype not in (torch.float16, torch.bfloat16):
            raise NotImplementedError(f"GanqHipPackedEmbedding: a table of {dtype} cannot be served (float16 and bfloat16 can)")
        self.num_embeddings, self.embedding_dim, self.bits = int(num_embeddings), int(embedding_dim), int(bits)
        self.dtype = dtype
        self.padding_idx = padding_idx
        self.register_buffer("qweight_rows", torch.zeros((self.num_embeddings, self.embedding_dim * self.bits // 32), dtype=torch.int32))
        self.register_buffer("lut", torch.zeros((self.num_embeddings, 2 ** self.bits), dtype=torch.float16))

    def train_codebook(self, enabled: bool = True):
        """enabled: `lut` becomes an fp32 nn.Parameter (the master copy; each forward rounds it to `dtype` and its gradient passes
        straight through that rounding).  False: back to an fp16 buffer, rounded once.  The name and so the state_dict key stay
        `lut` (the semantics of GanqHipQuantLinear.train_codebook)."""
        lut = self.lut.detach()
        delattr(self, "lut")
        if enabled:
            self.lut = nn.Parameter(lut.to(torch.float32).clone())
        else:
            self.register_buffer("lut", lut.to(torch.float16).contiguous())
        return self

    def _codebook(self) -> torch.Tensor:
        return self.lut

    def _lookup(self, ids: torch.Tensor) -> torch.Tensor:
        return _lib.lut_table_lookup(ids, self.qweight_rows, self._as_dtype("_lut_cache", self.lut), self.bits)

    def _lookup_bwd_lut(self, ids: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
        return _lib.lut_table_bwd_lut(ids, dy, self.qweight_rows, self.bits, padding_idx=self._padding_id())

    def dequantize_weight(self) -> torch.Tensor:
        """the table [num_embeddings, embedding_dim] in `dtype`: a lookup of every id (no gradient)"""
        return self._lookup(torch.arange(self.num_embeddings, device=self.qweight_rows.device))

    def extra_repr(self) -> str:
        return f"{self.num_embeddings}, {self.embedding_dim}, bits={self.bits}, dtype={self.dtype}"


class _GanqLutLookupFn(torch.autograd.Function):
    """out = F.embedding(ids, lut.gather(1, Q) (+ W_sparse)) of a packed embedding module with a HIP gradient for lut.  The forward is
    the module's inference lookup (the codebook rounded to the table dtype); the gradient passes straight through that rounding."""

    @staticmethod
    def forward(ctx, lut_in, ids, module):
        ctx.module = module
        ctx.lut_dtype = lut_in.dtype
        ctx.save_for_backward(ids)
        return module._lookup(ids)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        module = ctx.module
        (ids,) = ctx.saved_tensors
        if dy.dtype != module.dtype:
            dy = dy.to(module.dtype)
        dlut = module._lookup_bwd_lut(ids, dy)
        if dlut.dtype != ctx.lut_dtype:
            dlut = dlut.to(ctx.lut_dtype)
        return dlut, None, None


__all__ = ["GanqHipQuantLinear", "GanqHipQuantEmbedding", "GanqHipPackedEmbedding", "BACKEND_GANQ_HIP"]
