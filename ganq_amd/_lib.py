"""ctypes binding of libganq_hip.so (C-ABI declared in include/ganq_hip.h).

The library is the product: there is no CPU or PyTorch fallback.  If the shared object is
missing, fails to load or lacks a symbol, importing a compute entry point raises
``GanqHipError`` -- loudly, by design.

Tensors are torch-owned; this layer only borrows ``data_ptr()`` for the duration of a call
and passes the current torch stream of the tensors' device, with that device made current (reference boundary: the tensors that
``GANQ._perform_quantization_loop`` receives, gptqmodel/quantization/ganq.py:456).
"""
import ctypes
import os
import subprocess
import threading

import torch

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GANQ_HIP_LIB") or os.path.join(_PKG_DIR, "libganq_hip.so")  # override: developer builds
CSRC_DIR = os.path.join(_PKG_DIR, "csrc")

FLAG_ALIAS_Q = 1
FLAG_NO_HELPERS = 2

_c_i64 = ctypes.c_int64
_c_vp = ctypes.c_void_p
_c_sz = ctypes.c_size_t

# name -> (restype, argtypes); mirrors include/ganq_hip.h one to one
SIGNATURES = {
    "ganq_hip_version": (ctypes.c_int, []),
    "ganq_hip_last_error": (ctypes.c_char_p, []),
    "ganq_hip_selftest": (ctypes.c_int, [_c_vp]),
    "ganq_debug_div_check": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_uint32, _c_vp, _c_vp, _c_vp]),
    "ganq_debug_wh_product": (ctypes.c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp]),
    "ganq_debug_t_sums": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_i64, _c_i64, ctypes.c_int, ctypes.c_int, ctypes.c_double] + [_c_vp] * 16),
    "ganq_debug_gemm_h16": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_vp, ctypes.c_int, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp]),
    "ganq_hessian_workspace_bytes": (_c_sz, [_c_i64, _c_i64]),
    "ganq_hessian_accum": (ctypes.c_int, [_c_vp, _c_vp, ctypes.c_int, _c_i64, _c_i64, _c_i64, _c_i64, _c_vp, _c_sz, _c_vp]),
    "ganq_debug_hessian_t_cut": (ctypes.c_int, [_c_i64, _c_i64, ctypes.c_int, _c_vp, _c_vp, ctypes.c_int, _c_vp, ctypes.c_int]),
    "ganq_debug_hessian_t_check": (ctypes.c_int, [_c_i64, _c_i64, ctypes.c_int]),
    "ganq_hessian_t_supported": (ctypes.c_int, [_c_i64, _c_i64]),
    "ganq_hessian_t_workspace_bytes": (_c_sz, [_c_i64]),
    "ganq_hessian_stage_t": (ctypes.c_int, [_c_vp, _c_i64, _c_vp, _c_i64, _c_i64, _c_i64, _c_vp]),
    "ganq_hessian_accum_t": (ctypes.c_int, [_c_vp, _c_vp, _c_i64, ctypes.c_int, _c_i64, _c_i64, _c_i64, _c_i64, _c_vp, _c_sz, _c_vp]),
    "ganq_cholesky_workspace_bytes": (_c_sz, [_c_i64]),
    "ganq_cholesky": (ctypes.c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_sz, _c_vp]),
    "ganq_prologue_rowstats": (ctypes.c_int, [_c_vp, _c_i64, _c_vp, _c_vp, _c_vp]),
    "ganq_prologue_gather": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_i64, _c_vp, _c_vp, ctypes.c_int, _c_vp, _c_vp, ctypes.c_int, _c_vp,
                                            _c_vp, ctypes.c_int, _c_vp]),
    "ganq_prologue_weights": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_i64, _c_i64, ctypes.c_int, _c_vp, _c_vp]),
    "ganq_kmeans_workspace_bytes": (_c_sz, [_c_i64, _c_i64, ctypes.c_int]),
    "ganq_kmeans_init": (ctypes.c_int, [_c_vp, _c_vp, _c_i64, _c_i64, ctypes.c_int, _c_vp, _c_vp, _c_sz, _c_vp]),
    "ganq_debug_kmeans_plan": (ctypes.c_int, [_c_i64, _c_i64, ctypes.c_int, _c_vp]),
    "ganq_solve_s_workspace_bytes": (_c_sz, [_c_i64, _c_i64, ctypes.c_int]),
    "ganq_debug_solve_plan": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_vp]),
    "ganq_debug_accum_plan": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, _c_vp]),
    "ganq_debug_top_rule": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, ctypes.c_longlong, ctypes.c_longlong, _c_vp]),
    "ganq_debug_top_planes": (ctypes.c_int, [_c_vp, ctypes.c_int64, ctypes.c_int64, _c_vp, _c_vp]),
    "ganq_debug_mu_planes": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, ctypes.c_longlong, ctypes.c_longlong, _c_vp]),
    "ganq_debug_solve_role": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_vp]),
    "ganq_solve_s": (ctypes.c_int, [_c_vp, _c_vp, _c_i64, _c_vp, _c_i64, _c_i64, ctypes.c_int, _c_vp, _c_vp, _c_vp,
                                    _c_sz, _c_vp]),
    "ganq_matmul_f32": (ctypes.c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp]),
    "ganq_update_t_workspace_bytes": (_c_sz, [_c_i64, _c_i64, ctypes.c_int]),
    "ganq_update_t": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_i64, _c_i64, ctypes.c_int, ctypes.c_double, _c_vp, _c_vp,
                                     _c_vp, _c_vp, _c_sz, _c_vp]),
    "ganq_quad_loss_workspace_bytes": (_c_sz, [_c_i64, _c_i64, ctypes.c_int]),
    "ganq_quad_loss": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_i64, _c_i64, ctypes.c_int, _c_vp, _c_vp, _c_sz,
                                      _c_vp]),
    "ganq_dequant_losses": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_i64, _c_i64, ctypes.c_int, _c_vp, _c_vp,
                                           _c_vp]),
    "ganq_run_layer_workspace_bytes": (_c_sz, [_c_i64, _c_i64, ctypes.c_int]),
    "ganq_run_layer": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_i64, _c_vp, _c_i64, _c_i64, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_uint32, ctypes.c_double, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_sz,
                                      _c_vp]),
    "ganq_run_layer_rows": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_i64, _c_vp, _c_i64, _c_i64, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_uint32, ctypes.c_double, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp,
                                           _c_vp, _c_sz, _c_vp]),
    "ganq_select_best": (ctypes.c_int, [_c_vp, _c_i64, ctypes.c_int, _c_vp, _c_vp, _c_vp]),
    "ganq_debug_set_option": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_longlong]),
    "ganq_debug_get_option": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_longlong)]),
    "ganq_debug_reset_option": (ctypes.c_int, [ctypes.c_char_p]),
    "ganq_lut_linear_workspace_bytes": (_c_sz, [_c_i64, _c_i64, _c_i64, ctypes.c_int]),
    "ganq_lut_linear_workspace_init": (ctypes.c_int, [_c_vp, _c_sz, _c_vp]),
    "ganq_lut_linear_fwd": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_vp, ctypes.c_int, _c_i64, _c_i64, _c_i64,
                                           ctypes.c_int, _c_vp, _c_vp, _c_sz, _c_vp]),
    "ganq_lut_linear_fwd_add": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_vp, ctypes.c_int, _c_i64, _c_i64, _c_i64,
                                               ctypes.c_int, _c_vp, _c_vp, _c_sz, _c_vp]),
    "ganq_lut_linear_outliers_workspace_bytes": (_c_sz, [_c_i64, _c_i64, _c_i64, ctypes.c_int]),
    "ganq_lut_linear_fwd_outliers": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, ctypes.c_int, _c_i64, _c_i64,
                                                    _c_i64, ctypes.c_int, _c_vp, _c_vp, _c_sz, _c_vp]),
    "ganq_lut_linear_lora_workspace_bytes": (_c_sz, [_c_i64, _c_i64, _c_i64, ctypes.c_int, ctypes.c_int]),
    "ganq_lut_linear_fwd_lora": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, ctypes.c_int, _c_vp, ctypes.c_int, _c_i64, _c_i64,
                                                _c_i64, ctypes.c_int, _c_vp, _c_vp, _c_sz, _c_vp]),
    "ganq_lut_linear_lora_outliers_workspace_bytes": (_c_sz, [_c_i64, _c_i64, _c_i64, ctypes.c_int, ctypes.c_int]),
    "ganq_lut_linear_fwd_lora_outliers": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, ctypes.c_int, _c_vp, _c_vp, _c_vp, ctypes.c_int,
                                                         _c_i64, _c_i64, _c_i64, ctypes.c_int, _c_vp, _c_vp, _c_sz, _c_vp]),
    "ganq_lut_linear_bwd_input_workspace_bytes": (_c_sz, [_c_i64, _c_i64, _c_i64, ctypes.c_int]),
    "ganq_lut_linear_bwd_input": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_vp, ctypes.c_int, _c_i64, _c_i64, _c_i64, ctypes.c_int, _c_vp,
                                                 _c_vp, _c_sz, _c_vp]),
    "ganq_lut_linear_bwd_lut_workspace_bytes": (_c_sz, [_c_i64, _c_i64, _c_i64, ctypes.c_int]),
    "ganq_lut_linear_bwd_lut": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, ctypes.c_int, _c_i64, _c_i64, _c_i64, ctypes.c_int, _c_vp, _c_vp,
                                               _c_sz, _c_vp]),
    "ganq_lut_head_nll_workspace_bytes": (_c_sz, [_c_i64, _c_i64, _c_i64, ctypes.c_int]),
    "ganq_lut_head_nll": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_vp, ctypes.c_int, _c_i64, _c_i64, _c_i64, ctypes.c_int, _c_vp, _c_vp,
                                         _c_vp, _c_vp, _c_sz, _c_vp]),
    "ganq_lut_head_pick_workspace_bytes": (_c_sz, [_c_i64, _c_i64, _c_i64, ctypes.c_int]),
    "ganq_lut_head_pick": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_vp, ctypes.c_float, ctypes.c_int, _c_i64, _c_i64, _c_i64, ctypes.c_int,
                                          _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_sz, _c_vp]),
    "ganq_debug_head_pick_plan": (ctypes.c_int, [_c_i64, _c_i64, _c_i64, ctypes.c_int, _c_vp, ctypes.c_int]),
    "ganq_lut_head_pick_seeded": (ctypes.c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_vp, ctypes.c_int, ctypes.c_float, ctypes.c_int, _c_i64, _c_i64,
                                                 _c_i64, ctypes.c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_sz, _c_vp]),
    "ganq_lut_head_pick_noise": (ctypes.c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp]),
    "ganq_debug_lut_plan": (ctypes.c_int, [_c_i64, _c_i64, _c_i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_vp, ctypes.c_int]),
    "ganq_lut_dequant": (ctypes.c_int, [_c_vp, _c_vp, ctypes.c_int, _c_i64, _c_i64, ctypes.c_int, _c_vp, _c_vp]),
    "ganq_lut_embedding": (ctypes.c_int, [_c_vp, _c_i64, _c_vp, _c_vp, ctypes.c_int, _c_i64, _c_i64, ctypes.c_int, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    "ganq_lut_table_assign": (ctypes.c_int, [_c_vp, _c_vp, _c_i64, _c_i64, ctypes.c_int, _c_vp, _c_vp, _c_vp]),
    "ganq_lut_table_lookup": (ctypes.c_int, [_c_vp, _c_i64, _c_vp, _c_vp, ctypes.c_int, _c_i64, _c_i64, ctypes.c_int, _c_vp, _c_vp]),
    "ganq_lut_table_bwd_lut_workspace_bytes": (_c_sz, [_c_i64, _c_i64, _c_i64, ctypes.c_int]),
    "ganq_lut_table_bwd_lut": (ctypes.c_int, [_c_vp, _c_vp, _c_i64, _c_vp, ctypes.c_int, _c_vp, _c_i64, _c_i64, ctypes.c_int, _c_i64, _c_vp,
                                              _c_vp, _c_sz, _c_vp]),
    "ganq_lut_embedding_bwd_lut_workspace_bytes": (_c_sz, [_c_i64, _c_i64, _c_i64, ctypes.c_int]),
    "ganq_lut_embedding_bwd_lut": (ctypes.c_int, [_c_vp, _c_vp, _c_i64, _c_vp, ctypes.c_int, _c_vp, _c_i64, _c_i64, ctypes.c_int, _c_i64, _c_vp,
                                                  _c_vp, _c_sz, _c_vp]),
    "ganq_outlier_cutoffs": (ctypes.c_int, [_c_vp, _c_i64, _c_i64, ctypes.c_double, _c_vp, _c_vp, _c_vp, _c_vp]),
    "ganq_outlier_extract": (ctypes.c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    "ganq_outlier_matmul": (ctypes.c_int, [_c_vp, ctypes.c_int, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    "ganq_pack_indices": (ctypes.c_int, [_c_vp, _c_i64, _c_i64, ctypes.c_int, _c_vp, _c_vp]),
    "ganq_unpack_indices": (ctypes.c_int, [_c_vp, _c_i64, _c_i64, ctypes.c_int, _c_vp, _c_vp]),
    "ganq_profile_enable": (ctypes.c_int, [ctypes.c_int]),
    "ganq_profile_reset": (ctypes.c_int, []),
    "ganq_profile_select": (ctypes.c_int, [ctypes.c_int]),
    "ganq_profile_num_kernels": (ctypes.c_int, []),
    "ganq_profile_kernel_name": (ctypes.c_char_p, [ctypes.c_int]),
    "ganq_profile_get": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_c_i64)]),
}


class GanqHipError(RuntimeError):
    pass


_lib = None
_lock = threading.Lock()


def build(force: bool = False) -> str:
    """Compile libganq_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC_DIR, "-j8"] + (["-B"] if force else [])
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if proc.returncode != 0:
        raise GanqHipError("building libganq_hip.so failed:\n" + proc.stdout[-4000:])
    return LIB_PATH


def lib():
    """Load the shared library and bind every symbol the header declares."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise GanqHipError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; "
                                   f"g.build()'` (or `make -C ganq_amd/csrc`). There is no CPU fallback.")
            try:
                handle = ctypes.CDLL(LIB_PATH)
            except OSError as e:
                raise GanqHipError(f"cannot load {LIB_PATH}: {e}") from e
            for name, (res, args) in SIGNATURES.items():
                try:
                    fn = getattr(handle, name)
                except AttributeError as e:
                    raise GanqHipError(f"{LIB_PATH} does not export {name}") from e
                fn.restype = res
                fn.argtypes = args
            _lib = handle
    return _lib


def _check(rc: int, what: str):
    if rc != 0:
        msg = lib().ganq_hip_last_error()
        raise GanqHipError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")


def _stream(device=None) -> int:
    """hipStream_t of torch's current stream ON `device` (default: the current device)"""
    return torch.cuda.current_stream(device).cuda_stream


class _on:
    """Make the device of `t` the current HIP device for the duration of a library call: the library launches on the
    current device (kernel attributes, probe results and helper streams are kept per device), and the stream handed
    over must be that device's.  All tensors of a call must live on ONE device."""

    def __init__(self, *tensors):
        devs = {t.device for t in tensors if t is not None and hasattr(t, "device")}
        if len(devs) != 1:
            raise GanqHipError(f"all tensors of a call must live on one GPU, got {sorted(map(str, devs))}")
        self.device = devs.pop()
        if self.device.type != "cuda":
            raise GanqHipError(f"tensors must live on the GPU (got {self.device}); the HIP path has no CPU fallback")
        self._guard = torch.cuda.device(self.device)

    def __enter__(self):
        self._guard.__enter__()
        return _stream(self.device)

    def __exit__(self, *exc):
        return self._guard.__exit__(*exc)


_ST = object()  # placeholder for the stream argument of a library call


def _call(name: str, tensors, *args):
    """one library call on the device of `tensors` (all on one GPU) with that device current and its current stream"""
    with _on(*tensors) as st:
        rc = getattr(lib(), name)(*[st if a is _ST else a for a in args])
    _check(rc, name)


def debug_option(name: str, value=None):
    """developer / test switches of the library (include/ganq_hip.h); value None resets to the default"""
    if value is None:
        _check(lib().ganq_debug_reset_option(name.encode()), "ganq_debug_reset_option")
    else:
        _check(lib().ganq_debug_set_option(name.encode(), int(value)), "ganq_debug_set_option")


def debug_option_get(name: str) -> int:
    v = ctypes.c_longlong(0)
    _check(lib().ganq_debug_get_option(name.encode(), ctypes.byref(v)), "ganq_debug_get_option")
    return v.value


def _ptr(t):
    return None if t is None else t.data_ptr()


def _dev_f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise GanqHipError(f"{name} must live on the GPU (got {t.device}); the HIP path has no CPU fallback")
    if t.dtype != torch.float32:
        raise GanqHipError(f"{name} must be float32, got {t.dtype}")
    return t.contiguous()


def _workspace(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def selftest(device=None):
    """MFMA accumulation-order probe on `device` (default: the current device); cached per device by the library"""
    with torch.cuda.device(device if device is not None else torch.cuda.current_device()):
        _check(lib().ganq_hip_selftest(_stream()), "ganq_hip_selftest")


def debug_div_check(count: int, seed: int = 1):
    """(mismatches, (a, b)) of the reciprocal-based quotient vs IEEE division over `count` pseudo-random pairs"""
    bad = torch.zeros((), dtype=torch.int64, device="cuda")
    first = torch.zeros(2, dtype=torch.float32, device="cuda")
    _call("ganq_debug_div_check", (bad, first), int(count), int(seed), bad.data_ptr(), first.data_ptr(), _ST)
    return int(bad), tuple(first.tolist())


def debug_wh_product(W, H):
    """(WH, H_fixed) in fp64: the product the fused driver feeds to the T-update and the fixed-point H behind it"""
    W, H = _dev_f32(W, "W"), _dev_f32(H, "H")
    m, n = W.shape
    WH = torch.empty((m, n), dtype=torch.float64, device=W.device)
    Hf = torch.empty((n, n), dtype=torch.float64, device=W.device)
    _call("ganq_debug_wh_product", (W, H, WH, Hf), W.data_ptr(), H.data_ptr(), m, n, WH.data_ptr(), Hf.data_ptr(), _ST)
    return WH, Hf


def debug_t_sums(W, H, Qseq, V, rcond=-1.0):
    """The fused loop's T-update on the index sequence Qseq [K,m,n] (uint8) and the integers behind it (ganq_debug_t_sums):
    a dict of cuda tensors -- scale (fp64), ext, Hint / J [n,n] int32, hdiag_int / hdiag_j [n], F_hi / F_lo [K,m,16,16] int64,
    chgcnt [K,m], Qprev [K,m,n] (None with GANQ_T_FULL=1), T_all [K,m,V], loss_rows_all [K,m], active_rows [K,m] /
    active_count [K] (-1: no list built), full_ran [K]."""
    W, H = _dev_f32(W, "W"), _dev_f32(H, "H")
    if Qseq.dtype != torch.uint8 or not Qseq.is_cuda or Qseq.dim() != 3:
        raise GanqHipError("Qseq must be a uint8 cuda tensor [K,m,n]")
    Qseq = Qseq.contiguous()
    K, m, n = Qseq.shape
    if W.shape != (m, n) or H.shape != (n, n):
        raise GanqHipError(f"shape mismatch W{tuple(W.shape)} H{tuple(H.shape)} Qseq{tuple(Qseq.shape)}")
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=W.device)  # noqa: E731
    out = {"scale": new((), torch.float64), "ext": new((), torch.int32), "Hint": new((n, n), torch.int32),
           "J": new((n, n), torch.int32), "hdiag_int": new((n,), torch.int32), "hdiag_j": new((n,), torch.int32),
           "F_hi": new((K, m, 16, 16), torch.int64), "F_lo": new((K, m, 16, 16), torch.int64), "chgcnt": new((K, m), torch.int32),
           "Qprev": None if debug_option_get("GANQ_T_FULL") == 1 else new((K, m, n), torch.uint8),
           "T_all": new((K, m, V), torch.float32), "loss_rows_all": new((K, m), torch.float64),
           "active_rows": new((K, m), torch.int32), "active_count": new((K,), torch.int32), "full_ran": new((K,), torch.int32)}
    order = ("scale", "ext", "Hint", "J", "hdiag_int", "hdiag_j", "F_hi", "F_lo", "chgcnt", "Qprev", "T_all", "loss_rows_all",
             "active_rows", "active_count", "full_ran")
    _call("ganq_debug_t_sums", (W, H, Qseq), W.data_ptr(), H.data_ptr(), Qseq.data_ptr(), m, n, int(V), K, float(rcond),
          *[_ptr(out[k]) for k in order], _ST)
    return out


def solve_s(W, L, T, want_err=False):
    """ganq.py:533-565.  W [m,n], L [n,n] lower, T [m,V] (fp32, cuda) -> Q uint8 [m,n] (, Err fp32 [m,n])."""
    W, T = _dev_f32(W, "W"), _dev_f32(T, "T")
    if not (L.is_cuda and L.dtype == torch.float32 and L.stride(1) == 1):
        L = _dev_f32(L, "L")
    m, n = W.shape
    V = T.shape[1]
    if L.shape != (n, n) or T.shape[0] != m:
        raise GanqHipError(f"shape mismatch W{tuple(W.shape)} L{tuple(L.shape)} T{tuple(T.shape)}")
    Q = torch.empty((m, n), dtype=torch.uint8, device=W.device)
    Err = torch.empty((m, n), dtype=torch.float32, device=W.device) if want_err else None
    ws = _workspace(lib().ganq_solve_s_workspace_bytes(m, n, V), W.device)
    _call("ganq_solve_s", (W, L, T, Q, Err, ws), W.data_ptr(), L.data_ptr(), L.stride(0), T.data_ptr(), m, n, V, Q.data_ptr(), _ptr(Err),
                              ws.data_ptr(), ws.numel(), _ST)
    return (Q, Err) if want_err else Q


def matmul_f32(A, B):
    A, B = _dev_f32(A, "A"), _dev_f32(B, "B")
    m, k = A.shape
    if B.shape[0] != k:
        raise GanqHipError(f"shape mismatch A{tuple(A.shape)} B{tuple(B.shape)}")
    n = B.shape[1]
    C = torch.empty((m, n), dtype=torch.float32, device=A.device)
    _call("ganq_matmul_f32", (A, B, C), A.data_ptr(), B.data_ptr(), m, k, n, C.data_ptr(), _ST)
    return C


def update_t(WH, H, Q, V, rcond=-1.0, want_ab=False):
    """ganq.py:570-591 (gelsd branch).  -> T [m,V] (, A [m,V,V], b [m,V])."""
    WH, H = _dev_f32(WH, "WH"), _dev_f32(H, "H")
    if Q.dtype != torch.uint8 or not Q.is_cuda:
        raise GanqHipError("Q must be a uint8 cuda tensor")
    Q = Q.contiguous()
    m, n = WH.shape
    T = torch.empty((m, V), dtype=torch.float32, device=WH.device)
    A = torch.empty((m, V, V), dtype=torch.float32, device=WH.device) if want_ab else None
    b = torch.empty((m, V), dtype=torch.float32, device=WH.device) if want_ab else None
    ws = _workspace(lib().ganq_update_t_workspace_bytes(m, n, V), WH.device)
    _call("ganq_update_t", (WH, H, Q, T, A, b, ws), WH.data_ptr(), H.data_ptr(), Q.data_ptr(), m, n, V, float(rcond), T.data_ptr(), _ptr(A),
                               _ptr(b), ws.data_ptr(), ws.numel(), _ST)
    return (T, A, b) if want_ab else T


def quad_loss(W, H, T, Q):
    """ganq.py:392-395 on Wq = T.gather(1,Q).  Returns a 0-dim float64 cuda tensor (no sync)."""
    W, H, T = _dev_f32(W, "W"), _dev_f32(H, "H"), _dev_f32(T, "T")
    Q = Q.contiguous()
    m, n = W.shape
    out = torch.empty((), dtype=torch.float64, device=W.device)
    ws = _workspace(lib().ganq_quad_loss_workspace_bytes(m, n, T.shape[1]), W.device)
    _call("ganq_quad_loss", (W, H, T, Q, out, ws), W.data_ptr(), H.data_ptr(), T.data_ptr(), Q.data_ptr(), m, n, T.shape[1],
                                out.data_ptr(), ws.data_ptr(), ws.numel(), _ST)
    return out


def dequant_losses(W, T, Q, hinv_diag, want_losses=True):
    """ganq.py:633-638.  -> (Wq [m,n], Losses [m,n] or None)."""
    W, T = _dev_f32(W, "W"), _dev_f32(T, "T")
    Q = Q.contiguous()
    m, n = W.shape
    Wq = torch.empty((m, n), dtype=torch.float32, device=W.device)
    Lo = torch.empty((m, n), dtype=torch.float32, device=W.device) if want_losses else None
    hd = _dev_f32(hinv_diag, "hinv_diag") if want_losses else None
    _call("ganq_dequant_losses", (W, T, Q, hd, Wq, Lo), W.data_ptr(), T.data_ptr(), Q.data_ptr(), _ptr(hd), m, n, T.shape[1],
                                     Wq.data_ptr(), _ptr(Lo), _ST)
    return Wq, Lo


def run_layer_workspace(m, n, V, device):
    return _workspace(lib().ganq_run_layer_workspace_bytes(m, n, V), device)


def run_layer(W, H, L, T0, K, alias_q=True, rcond=-1.0, workspace=None, helpers=True):
    """ganq.py:516-634.  -> (T_best [m,V], Q uint8 [m,n], dists float64 [K], best_k int32 0-dim); all on the GPU."""
    W, H, T0 = _dev_f32(W, "W"), _dev_f32(H, "H"), _dev_f32(T0, "T0")
    if not (L.is_cuda and L.dtype == torch.float32 and L.stride(1) == 1):
        L = _dev_f32(L, "L")
    m, n = W.shape
    V = T0.shape[1]
    if H.shape != (n, n) or L.shape != (n, n) or T0.shape[0] != m:
        raise GanqHipError(f"shape mismatch W{tuple(W.shape)} H{tuple(H.shape)} L{tuple(L.shape)} T0{tuple(T0.shape)}")
    T = torch.empty((m, V), dtype=torch.float32, device=W.device)
    Q = torch.empty((m, n), dtype=torch.uint8, device=W.device)
    dists = torch.zeros((max(K, 1),), dtype=torch.float64, device=W.device)
    best_k = torch.full((), -1, dtype=torch.int32, device=W.device)
    ws = workspace if workspace is not None else run_layer_workspace(m, n, V, W.device)
    _call("ganq_run_layer", (W, H, L, T0, T, Q, dists, best_k, ws), W.data_ptr(), H.data_ptr(), L.data_ptr(), L.stride(0), T0.data_ptr(), m, n, V, int(K),
          (FLAG_ALIAS_Q if alias_q else 0) | (0 if helpers else FLAG_NO_HELPERS), float(rcond), T.data_ptr(), Q.data_ptr(),
          dists.data_ptr(), best_k.data_ptr(), ws.data_ptr(), ws.numel(), _ST)
    return T, Q, dists[:K], best_k


def run_layer_rows(W, H, L, T0, K, alias_q=True, rcond=-1.0, workspace=None, want_q_all=None, helpers=True):
    """ganq_run_layer_rows: the fused loop on a slice of a layer's rows with the per-iteration records the owner of the
    whole layer needs.  -> dict(T_all [K,m,V], loss_rows_all [K,m] fp64, Q_last [m,n] uint8 (indices of the last
    iteration), Q_all [K,m,n] or None, dists [K] / best_k / T_best of the slice alone)."""
    W, H, T0 = _dev_f32(W, "W"), _dev_f32(H, "H"), _dev_f32(T0, "T0")
    if not (L.is_cuda and L.dtype == torch.float32 and L.stride(1) == 1):
        L = _dev_f32(L, "L")
    m, n = W.shape
    V = T0.shape[1]
    if H.shape != (n, n) or L.shape != (n, n) or T0.shape[0] != m:
        raise GanqHipError(f"shape mismatch W{tuple(W.shape)} H{tuple(H.shape)} L{tuple(L.shape)} T0{tuple(T0.shape)}")
    if want_q_all is None:
        want_q_all = not alias_q
    K = int(K)
    dev = W.device
    T = torch.empty((m, V), dtype=torch.float32, device=dev)
    Q = torch.empty((m, n), dtype=torch.uint8, device=dev)
    dists = torch.zeros((max(K, 1),), dtype=torch.float64, device=dev)
    best_k = torch.full((), -1, dtype=torch.int32, device=dev)
    T_all = torch.empty((K, m, V), dtype=torch.float32, device=dev)
    loss_all = torch.empty((K, m), dtype=torch.float64, device=dev)
    Q_all = torch.empty((K, m, n), dtype=torch.uint8, device=dev) if want_q_all else None
    ws = workspace if workspace is not None else run_layer_workspace(m, n, V, dev)
    # always run the aliasing variant inside the slice: Q then holds the LAST iteration's indices, which is what the
    # reference's torch branch returns; the per-iteration indices (if wanted) come back in Q_all
    _call("ganq_run_layer_rows", (W, H, L, T0, T, Q, dists, best_k, T_all, loss_all, Q_all, ws), W.data_ptr(), H.data_ptr(),
          L.data_ptr(), L.stride(0), T0.data_ptr(), m, n, V, K, FLAG_ALIAS_Q | (0 if helpers else FLAG_NO_HELPERS), float(rcond),
          T.data_ptr(), Q.data_ptr(),
          dists.data_ptr(), best_k.data_ptr(), T_all.data_ptr(), loss_all.data_ptr(), _ptr(Q_all), ws.data_ptr(), ws.numel(),
          _ST)
    return dict(T_all=T_all, loss_rows_all=loss_all, Q_last=Q, Q_all=Q_all, dists=dists[:K], best_k=best_k, T_best=T)


def select_best(loss_rows_all):
    """ganq_select_best: loss_rows_all [K,m] fp64 (all rows of the layer, row order) -> (dists [K] fp64, best_k int32 0-dim)"""
    if loss_rows_all.dtype != torch.float64 or not loss_rows_all.is_cuda or loss_rows_all.dim() != 2:
        raise GanqHipError("select_best: loss_rows_all must be a [K, m] float64 cuda tensor")
    la = loss_rows_all.contiguous()
    K, m = la.shape
    dists = torch.zeros((max(K, 1),), dtype=torch.float64, device=la.device)
    best_k = torch.full((), -1, dtype=torch.int32, device=la.device)
    _call("ganq_select_best", (la, dists, best_k), la.data_ptr(), m, K, dists.data_ptr(), best_k.data_ptr(), _ST)
    return dists[:K], best_k


def profile_enable(on: bool = True, only: str = None):
    """HIP-event timing of the library's kernels; `only`: instrument just this kernel (the events of a fully
    instrumented run leave idle gaps between the dependent launches)."""
    lib().ganq_profile_reset()
    kid = -1
    if only is not None:
        names = [lib().ganq_profile_kernel_name(i).decode() for i in range(lib().ganq_profile_num_kernels())]
        kid = names.index(only)
    lib().ganq_profile_select(kid)
    lib().ganq_profile_enable(1 if on else 0)


def profile_report():
    """{kernel name: (total_ms, launches)} for everything recorded since profile_enable(); synchronises first."""
    torch.cuda.synchronize()
    out = {}
    for kid in range(lib().ganq_profile_num_kernels()):
        ms, cnt = ctypes.c_double(0.0), _c_i64(0)
        _check(lib().ganq_profile_get(kid, ctypes.byref(ms), ctypes.byref(cnt)), "ganq_profile_get")
        if cnt.value:
            out[lib().ganq_profile_kernel_name(kid).decode()] = (ms.value, cnt.value)
    return out


_DTYPE_CODE = {torch.float16: 0, torch.bfloat16: 1}


def _act_dtype(t, name):
    if t.dtype not in _DTYPE_CODE:
        raise GanqHipError(f"{name} must be float16 or bfloat16, got {t.dtype}")
    if not t.is_cuda:
        raise GanqHipError(f"{name} must live on the GPU; the HIP path has no CPU fallback")
    return _DTYPE_CODE[t.dtype]


def debug_gemm_h16(x, w, bias=None, addend=None):
    """developer / tests: y = x @ w.T (+ bias) (+ addend) by csrc/gemm_h16.hip; x [M,K], w [N,K] fp16 / bf16"""
    code = _act_dtype(x, "x")
    if w.dtype != x.dtype or not w.is_cuda:
        raise GanqHipError("w must have x's dtype and live on the GPU")
    x, w = x.contiguous(), w.contiguous()
    M, K = x.shape
    N = w.shape[0]
    y = torch.empty((M, N), dtype=x.dtype, device=x.device)
    _call("ganq_debug_gemm_h16", (x, w, y), x.data_ptr(), w.data_ptr(), _ptr(bias), _ptr(addend), code, M, N, K, y.data_ptr(), _ST)
    return y


def _caller_workspace(ws, nbytes: int, what: str):
    """a workspace the caller passed (tests fill it with a pattern): contiguous, on the GPU, at least `nbytes` -> (ws, its bytes)"""
    if not (ws.is_cuda and ws.is_contiguous()):
        raise GanqHipError(f"{what}: the workspace must be a contiguous cuda tensor")
    have = ws.numel() * ws.element_size()
    if have < nbytes:
        raise GanqHipError(f"{what}: workspace of {have} B < the {nbytes} B required")
    return ws, have


def hessian_accum(H, X, nsamples_before: int, batch: int, workspace=None):
    """gptq.py:96-131.  H [n,n] fp32 (updated in place), X [rows, n] fp16/bf16 (one calibration batch of
    `batch` sequences, flattened).  workspace: optional caller-owned scratch of at least ganq_hessian_workspace_bytes."""
    if not (H.is_cuda and H.dtype == torch.float32 and H.is_contiguous()):
        raise GanqHipError("H must be a contiguous float32 cuda tensor")
    code = _act_dtype(X, "X")
    X = X.contiguous()
    rows, n = X.shape
    if H.shape != (n, n):
        raise GanqHipError(f"shape mismatch H{tuple(H.shape)} X{tuple(X.shape)}")
    # partial tiles of the token-split launches: torch-owned scratch on the current stream (the caching allocator
    # re-uses it from call to call; nothing outlives the call on the library's side)
    with torch.cuda.device(H.device):
        nbytes = lib().ganq_hessian_workspace_bytes(rows, n)
    if workspace is not None:
        ws, nbytes = _caller_workspace(workspace, nbytes, "hessian_accum")
    else:
        ws = _workspace(nbytes, H.device) if nbytes else None
    _call("ganq_hessian_accum", (H, X, ws), H.data_ptr(), X.data_ptr(), code, rows, n, int(nsamples_before), int(batch),
          ws.data_ptr() if ws is not None else None, int(nbytes), _ST)
    return H


def hessian_t_supported(n: int, stage_tokens: int, device=None) -> bool:
    """whether a layer of n in_features is served by the transposed staging path (staging buffer Xt [n, stage_tokens])"""
    with torch.cuda.device(device if device is not None else torch.cuda.current_device()):
        return bool(lib().ganq_hessian_t_supported(int(n), int(stage_tokens)))


def hessian_stage_t(Xt, X, tok0: int):
    """the transposing staging copy of one calibration batch: Xt[:, tok0 : tok0 + rows] = X^T  (X [rows, n], Xt [n, ldt], fp16 / bf16)"""
    code = _act_dtype(X, "X")
    if not (Xt.is_cuda and Xt.dtype == X.dtype and Xt.dim() == 2 and Xt.is_contiguous()) or _act_dtype(Xt, "Xt") != code:
        raise GanqHipError("Xt must be a contiguous cuda tensor [in_features, tokens] of X's dtype")
    X = X.contiguous()
    rows, n = X.shape
    if Xt.shape[0] != n or tok0 < 0 or tok0 + rows > Xt.shape[1]:
        raise GanqHipError(f"hessian_stage_t: batch {tuple(X.shape)} at token {tok0} does not fit Xt{tuple(Xt.shape)}")
    _call("ganq_hessian_stage_t", (Xt, X), Xt.data_ptr(), Xt.shape[1], X.data_ptr(), rows, n, int(tok0), _ST)
    return Xt


def hessian_accum_t(H, Xt, rows: int, nsamples_before: int, batch: int, workspace=None):
    """gptq.py:96-131 for a staged group in transposed layout: H [n,n] fp32 (in place), Xt [n, ldt], its first `rows` tokens
    (a multiple of 32) = `batch` sequences.  workspace: optional caller-owned scratch of at least ganq_hessian_t_workspace_bytes."""
    if not (H.is_cuda and H.dtype == torch.float32 and H.is_contiguous()):
        raise GanqHipError("H must be a contiguous float32 cuda tensor")
    code = _act_dtype(Xt, "Xt")
    if not (Xt.dim() == 2 and Xt.is_contiguous() and H.shape == (Xt.shape[0], Xt.shape[0])):
        raise GanqHipError(f"shape mismatch H{tuple(H.shape)} Xt{tuple(Xt.shape)}")
    n, ldt = Xt.shape
    with torch.cuda.device(H.device):
        nbytes = lib().ganq_hessian_t_workspace_bytes(n)
    if workspace is not None:
        ws, nbytes = _caller_workspace(workspace, nbytes, "hessian_accum_t")
    else:
        ws = _workspace(nbytes, H.device)
    _call("ganq_hessian_accum_t", (H, Xt, ws), H.data_ptr(), Xt.data_ptr(), ldt, code, int(rows), n, int(nsamples_before), int(batch),
          ws.data_ptr(), int(nbytes), _ST)
    return H


def cholesky(H, check: bool = True):
    """torch.linalg.cholesky(H) for a symmetric fp32 matrix on the GPU (lower factor, new tensor).  With check=True a
    non-positive pivot raises torch.linalg.LinAlgError like torch does (one host sync); otherwise -> (L, info tensor)."""
    H = _dev_f32(H, "H")
    n = H.shape[0]
    if H.shape != (n, n):
        raise GanqHipError(f"cholesky: square matrix expected, got {tuple(H.shape)}")
    L = H.clone()
    info = torch.zeros((), dtype=torch.int32, device=H.device)
    ws = _workspace(lib().ganq_cholesky_workspace_bytes(n), H.device)
    _call("ganq_cholesky", (L, info, ws), L.data_ptr(), n, L.stride(0) if n else 0, info.data_ptr(), ws.data_ptr(), ws.numel(), _ST)
    if not check:
        return L, info
    bad = int(info)
    if bad:
        raise torch.linalg.LinAlgError(f"ganq_cholesky: the input is not positive-definite (leading minor of order {bad})")
    return L


def cholesky_inplace(A, check: bool = True):
    """ganq_cholesky on A itself (fp32 [n,n], contiguous rows): the lower factor replaces A, the strict upper part is zeroed.
    -> A, or (A, info tensor) with check=False"""
    if not (A.is_cuda and A.dtype == torch.float32 and A.dim() == 2 and A.shape[0] == A.shape[1] and A.stride(1) == 1):
        raise GanqHipError("cholesky_inplace: a square fp32 cuda matrix with contiguous rows expected")
    n = A.shape[0]
    info = torch.zeros((), dtype=torch.int32, device=A.device)
    ws = _workspace(lib().ganq_cholesky_workspace_bytes(n), A.device)
    _call("ganq_cholesky", (A, info, ws), A.data_ptr(), n, A.stride(0) if n else 0, info.data_ptr(), ws.data_ptr(), ws.numel(), _ST)
    if not check:
        return A, info
    bad = int(info)
    if bad:
        raise torch.linalg.LinAlgError(f"ganq_cholesky: the input is not positive-definite (leading minor of order {bad})")
    return A


def prologue_rowstats(H):
    """gptq.py:267-269,289-291 in one read of H -> (diag [n], rowabs [n] = sum_j |H[i][j]|), fp32"""
    H = _dev_f32(H, "H")
    n = H.shape[0]
    diag = torch.empty((n,), dtype=torch.float32, device=H.device)
    rowabs = torch.empty((n,), dtype=torch.float32, device=H.device)
    _call("ganq_prologue_rowstats", (H, diag, rowabs), H.data_ptr(), n, diag.data_ptr(), rowabs.data_ptr(), _ST)
    return diag, rowabs


def prologue_gather(H, perm, diag_fixed, outputs):
    """One read of H, every output written directly: outputs = [(add [n] fp32 or None, flip: bool), ...] (up to three) ->
    list of new [n,n] fp32 tensors, out[i][j] = H'[perm i][perm j] + (i == j ? add[i] : 0), index-reversed when flip;
    H' = H with diag_fixed on its diagonal; perm int64 [n] or None."""
    H = _dev_f32(H, "H")
    n = H.shape[0]
    if not 1 <= len(outputs) <= 3:
        raise GanqHipError("prologue_gather: one to three outputs")
    diag_fixed = _dev_f32(diag_fixed, "diag_fixed")
    perm_c = None if perm is None else perm.to(device=H.device, dtype=torch.int64).contiguous()
    outs, args, keep = [], [], [H, perm_c, diag_fixed]
    for k in range(3):
        if k < len(outputs):
            add, flip = outputs[k]
            add_c = None if add is None else _dev_f32(add, "add")
            o = torch.empty((n, n), dtype=torch.float32, device=H.device)
            outs.append(o)
            keep += [o, add_c]
            args += [o.data_ptr(), _ptr(add_c), 1 if flip else 0]
        else:
            args += [None, None, 0]
    _call("ganq_prologue_gather", tuple(keep), H.data_ptr(), _ptr(perm_c), diag_fixed.data_ptr(), n, *args, _ST)
    return outs


def prologue_weights(W, perm, dead, mean_fill: bool):
    """gptq.py:270-276,283: W_out[r][c] = dead[perm c] ? fill_r : W[r][perm c] (fill: 0, or the row mean over the live columns)"""
    W = _dev_f32(W, "W")
    m, n = W.shape
    dead_c = dead.to(device=W.device, dtype=torch.uint8).contiguous()
    perm_c = None if perm is None else perm.to(device=W.device, dtype=torch.int64).contiguous()
    out = torch.empty((m, n), dtype=torch.float32, device=W.device)
    _call("ganq_prologue_weights", (W, perm_c, dead_c, out), W.data_ptr(), _ptr(perm_c), dead_c.data_ptr(), m, n, 1 if mean_fill else 0,
          out.data_ptr(), _ST)
    return out


def kmeans_init(W, col_weight, V: int):
    """ganq.py:423-438.  W [m,n] fp32, col_weight [n] float64 (diag(Hinv)^-4) or None -> T0 [m,V] fp32."""
    W = _dev_f32(W, "W")
    m, n = W.shape
    cw = None
    if col_weight is not None:
        cw = col_weight.to(device=W.device, dtype=torch.float64).contiguous()
        if cw.shape != (n,):
            raise GanqHipError("col_weight must have shape [n]")
    T0 = torch.empty((m, V), dtype=torch.float32, device=W.device)
    ws = _workspace(lib().ganq_kmeans_workspace_bytes(m, n, V), W.device)
    _call("ganq_kmeans_init", (W, cw, T0, ws), W.data_ptr(), _ptr(cw), m, n, V, T0.data_ptr(), ws.data_ptr(), ws.numel(), _ST)
    return T0


def debug_kmeans_plan(m: int, n: int, V: int) -> dict:
    """what kmeans_init launches for W [m,n] under the current developer options (ganq_debug_kmeans_plan; host only, no GPU
    needed).  resident: the LDS-resident kernel (else the windowed one); per_cu: workgroups per CU; qcap: queued ranges per balanced
    level (resident); Wcap: the window in candidates (windowed); span: node spacing from which the windowed kernel may solve its
    levels span by span (0: never)."""
    out = (ctypes.c_int * 8)()
    _check(lib().ganq_debug_kmeans_plan(int(m), int(n), int(V), ctypes.cast(out, _c_vp)), "ganq_debug_kmeans_plan")
    return dict(resident=bool(out[0]), per_cu=out[1], P=out[2], qcap=out[3], Wcap=out[4], grid=out[5], lds_bytes=out[6], span=out[7])


def pack_indices(Q, bits: int):
    """Q uint8 [m,n] (original column order) -> qweight int32 [n*bits/32, m] (GPTQ layout)."""
    if Q.dtype != torch.uint8 or not Q.is_cuda:
        raise GanqHipError("Q must be a uint8 cuda tensor")
    Q = Q.contiguous()
    m, n = Q.shape
    qw = torch.empty((n * bits // 32, m), dtype=torch.int32, device=Q.device)
    _call("ganq_pack_indices", (Q, qw), Q.data_ptr(), m, n, bits, qw.data_ptr(), _ST)
    return qw


def unpack_indices(qweight, n: int, bits: int):
    if qweight.dtype != torch.int32 or not qweight.is_cuda:
        raise GanqHipError("qweight must be an int32 cuda tensor")
    qweight = qweight.contiguous()
    m = qweight.shape[1]
    Q = torch.empty((m, n), dtype=torch.uint8, device=qweight.device)
    _call("ganq_unpack_indices", (qweight, Q), qweight.data_ptr(), m, n, bits, Q.data_ptr(), _ST)
    return Q


def lut_dequant(qweight, lut, n: int, bits: int):
    code = _act_dtype(lut, "lut")
    qweight, lut = qweight.contiguous(), lut.contiguous()
    m = lut.shape[0]
    Wq = torch.empty((m, n), dtype=lut.dtype, device=lut.device)
    _call("ganq_lut_dequant", (qweight, lut, Wq), qweight.data_ptr(), lut.data_ptr(), code, m, n, bits, Wq.data_ptr(), _ST)
    return Wq


def lut_embedding(ids, qweight, lut, in_features: int, bits: int, outliers=None, out=None):
    """rows of the dequantised LUT weight by id: ids int64 (any shape), qweight int32 [n*bits/32, m], lut [m, V] fp16 / bf16 ->
    [..., n] in lut's dtype; outliers: (rowptr, cols, vals in lut's dtype) of the layer, added with one rounding.  An id outside
    [0, m) gives a row of zeros.  One launch, nothing else: capturable in a HIP graph (pass `out` to keep the address fixed)."""
    code = _act_dtype(lut, "lut")
    if ids.dtype != torch.int64 or not ids.is_cuda:
        raise GanqHipError("lut_embedding: ids must be an int64 cuda tensor")
    if qweight.dtype != torch.int32:
        raise GanqHipError("lut_embedding: qweight must be int32")
    ids, qweight, lut = ids.contiguous(), qweight.contiguous(), lut.contiguous()
    m, n = lut.shape[0], int(in_features)
    if tuple(qweight.shape) != (n * bits // 32, m) or lut.shape[1] != 2 ** bits:
        raise GanqHipError(f"lut_embedding: qweight {tuple(qweight.shape)} / lut {tuple(lut.shape)} do not fit [{m}, {n}] at {bits} bits")
    rowptr = cols = vals = None
    if outliers is not None:
        rowptr, cols, vals = outliers
        if vals.dtype != lut.dtype or rowptr.dtype != torch.int32 or cols.dtype != torch.int32 or rowptr.numel() != m + 1:
            raise GanqHipError("lut_embedding: outlier vals must have lut's dtype, rowptr [m + 1] / cols must be int32")
    N = ids.numel()
    if out is None:
        out = torch.empty(tuple(ids.shape) + (n,), dtype=lut.dtype, device=lut.device)
    elif out.dtype != lut.dtype or out.numel() != N * n or not out.is_contiguous():
        raise GanqHipError("lut_embedding: out must be contiguous, of lut's dtype, with ids.numel() * in_features elements")
    _call("ganq_lut_embedding", (ids, qweight, lut, rowptr, cols, vals, out), ids.data_ptr(), N, qweight.data_ptr(), lut.data_ptr(), code, m, n,
          bits, _ptr(rowptr), _ptr(cols) if cols is not None and cols.numel() else None,
          _ptr(vals) if vals is not None and vals.numel() else None, out.data_ptr(), _ST)
    return out


def lut_table_assign(W, T, bits: int, want_sqerr: bool = True):
    """nearest-code assignment of a table's rows into the row-packed layout: W [m,n] fp32, T [m, 2^bits] fp32 ->
    (qrows int32 [m, n*bits/32] == pack_indices(Q, bits).t(), sqerr fp64 [m] or None); ties go to the lower index"""
    W, T = _dev_f32(W, "W"), _dev_f32(T, "T")
    m, n = W.shape
    if tuple(T.shape) != (m, 2 ** bits):
        raise GanqHipError(f"lut_table_assign: T {tuple(T.shape)} does not fit W {tuple(W.shape)} at {bits} bits")
    qrows = torch.empty((m, n * bits // 32), dtype=torch.int32, device=W.device)
    sqerr = torch.empty((m,), dtype=torch.float64, device=W.device) if want_sqerr else None
    _call("ganq_lut_table_assign", (W, T, qrows, sqerr), W.data_ptr(), T.data_ptr(), m, n, int(bits), qrows.data_ptr(), _ptr(sqerr), _ST)
    return qrows, sqerr


def lut_table_lookup(ids, qrows, lut, bits: int, out=None):
    """rows of a row-packed LUT table by id: ids int64 (any shape), qrows int32 [m, n*bits/32], lut [m, 2^bits] fp16 / bf16 ->
    [..., n] in lut's dtype.  An id outside [0, m) gives a row of zeros.  One launch, nothing else: capturable in a HIP graph
    (pass `out` to keep the address fixed)."""
    code = _act_dtype(lut, "lut")
    if ids.dtype != torch.int64 or not ids.is_cuda:
        raise GanqHipError("lut_table_lookup: ids must be an int64 cuda tensor")
    if qrows.dtype != torch.int32 or qrows.dim() != 2 or not qrows.is_cuda:
        raise GanqHipError("lut_table_lookup: qrows must be a 2-d int32 cuda tensor")
    ids, qrows, lut = ids.contiguous(), qrows.contiguous(), lut.contiguous()
    m = lut.shape[0]
    n = qrows.shape[1] * 32 // bits
    if qrows.shape[0] != m or n * bits != qrows.shape[1] * 32 or lut.shape[1] != 2 ** bits:
        raise GanqHipError(f"lut_table_lookup: qrows {tuple(qrows.shape)} / lut {tuple(lut.shape)} do not fit one table at {bits} bits")
    N = ids.numel()
    if out is None:
        out = torch.empty(tuple(ids.shape) + (n,), dtype=lut.dtype, device=lut.device)
    elif out.dtype != lut.dtype or out.numel() != N * n or not out.is_contiguous() or not out.is_cuda:
        raise GanqHipError("lut_table_lookup: out must be a contiguous cuda tensor of lut's dtype with ids.numel() * embedding_dim elements")
    if m == 0:  # (the library leaves `out` alone for an empty table; every id is out of range: rows of zeros)
        return out.zero_()
    _call("ganq_lut_table_lookup", (ids, qrows, lut, out), ids.data_ptr(), N, qrows.data_ptr(), lut.data_ptr(), code, m, n, int(bits),
          out.data_ptr(), _ST)
    return out


def _lookup_bwd_lut(entry: str, ids, dy, q, m: int, n: int, bits: int, padding_idx):
    """the shared host side of the two lookup gradients: flatten, sort, size the workspace, call `ganq_<entry>`"""
    code = _act_dtype(dy, "dy")
    if ids.dtype != torch.int64 or not ids.is_cuda:
        raise GanqHipError(f"{entry}: ids must be an int64 cuda tensor")
    if q.dtype != torch.int32 or q.dim() != 2 or not q.is_cuda:
        raise GanqHipError(f"{entry}: the packed indices must be a 2-d int32 cuda tensor")
    N = ids.numel()
    if dy.numel() != N * n or (N and dy.shape[-1] != n):
        raise GanqHipError(f"{entry}: dy {tuple(dy.shape)} does not fit ids {tuple(ids.shape)} x {n} columns")
    dlut = torch.empty((m, 2 ** bits), dtype=torch.float32, device=dy.device)
    if m == 0 or N == 0:  # (an empty sum; the library is not called, as lut_table_lookup does for an empty table)
        return dlut.zero_()
    ids = ids.reshape(-1).contiguous()
    dy = dy.reshape(N, n).contiguous()  # (y.sum().backward() hands over a stride-0 gradient)
    order = torch.sort(ids, stable=True).indices
    pad = -1 if padding_idx is None else int(padding_idx)
    if pad < -1:
        raise GanqHipError(f"{entry}: padding_idx must be None or an id >= 0")
    ws = _workspace(getattr(lib(), f"ganq_{entry}_workspace_bytes")(N, m, n, int(bits)), dy.device)
    _call(f"ganq_{entry}", (ids, order, dy, q, dlut, ws), ids.data_ptr(), order.data_ptr(), N, dy.data_ptr(), code, q.data_ptr(), m, n, int(bits),
          pad, dlut.data_ptr(), ws.data_ptr(), ws.numel(), _ST)
    return dlut


def lut_table_bwd_lut(ids, dy, qrows, bits: int, padding_idx=None):
    """codebook gradient of `lut_table_lookup`: ids int64 (any shape), dy [..., n] fp16 / bf16, qrows int32 [m, n*bits/32] ->
    dlut fp32 [m, 2^bits], dlut[id][v] = the sum of dy[p][j] over the positions p with ids[p] == id and the columns j with
    Q[id][j] == v.  Ids outside [0, m) and the id `padding_idx` contribute nothing; rows and codes nothing selects are exactly 0.
    Bitwise repeatable (no atomics); a sort, a memset and two launches, no host synchronisation."""
    qrows = qrows.contiguous()
    m = qrows.shape[0]
    n = qrows.shape[1] * 32 // bits
    if bits not in (2, 3, 4) or n * bits != qrows.shape[1] * 32:
        raise GanqHipError(f"lut_table_bwd_lut: qrows {tuple(qrows.shape)} is no row-packed table at {bits} bits")
    return _lookup_bwd_lut("lut_table_bwd_lut", ids, dy, qrows, m, n, bits, padding_idx)


def lut_embedding_bwd_lut(ids, dy, qweight, in_features: int, bits: int, padding_idx=None):
    """codebook gradient of `lut_embedding` (the lookup out of a packed head's stream): as `lut_table_bwd_lut` with
    qweight int32 [n*bits/32, m] in the GPTQ column layout.  The head's outliers are frozen and get no gradient; the codes at
    outlier positions count, as in `lut_linear_bwd_lut`."""
    qweight = qweight.contiguous()
    n = int(in_features)
    m = qweight.shape[1]
    if bits not in (2, 3, 4) or qweight.shape[0] * 32 != n * bits:
        raise GanqHipError(f"lut_embedding_bwd_lut: qweight {tuple(qweight.shape)} does not fit {n} columns at {bits} bits")
    return _lookup_bwd_lut("lut_embedding_bwd_lut", ids, dy, qweight, m, n, bits, padding_idx)


SOLVE_REGIMES = ("none", "shared", "duo", "trio")  # GANQ_SOLVE_PLAN_*


def debug_solve_plan(active_tiles: int, grid: int = 0, ncu: int = 0) -> dict:
    """which helper workgroups an S-solve launch with `active_tiles` 16-row tiles still to solve gets under the current developer
    options (ganq_debug_solve_plan: the function the kernel evaluates).  grid 0: what the host launches for a layer of that many
    tiles; ncu > 0: plan for that many compute units, no GPU needed; 0: those of the current device."""
    out = (ctypes.c_int * 4)()
    _check(lib().ganq_debug_solve_plan(int(active_tiles), int(grid), int(ncu), ctypes.cast(out, _c_vp)), "ganq_debug_solve_plan")
    return dict(regime=SOLVE_REGIMES[out[0]], k=out[1], helpers=out[2], grid=out[3])


def debug_solve_role(active_tiles: int, cls: int, ticket: int, grid: int = 0, ncu: int = 0) -> dict:
    """what ticket `ticket` of ticket class `cls` (blockIdx mod 8) makes a workgroup of that launch (ganq_debug_solve_role):
    tile None = no role; stage 0 the tile, 1 / 2 a first / second helper serving `serves` tiles: tile, tile + 8, .."""
    out = (ctypes.c_int * 3)()
    _check(lib().ganq_debug_solve_role(int(active_tiles), int(grid), int(ncu), int(cls), int(ticket), ctypes.cast(out, _c_vp)),
           "ganq_debug_solve_role")
    return dict(tile=None if out[0] < 0 else out[0], stage=out[1], serves=out[2])


ACCUM_KERNELS = ("onehot_accum", "onehot_accum_w4")


def accum_plan(m: int, n: int) -> dict:
    """which kernel the T-update's full bucket sum of an [m, n] layer runs under the current developer options
    (ganq_debug_accum_plan: the function the launch evaluates; no GPU needed).  supported: the four-wave kernel serves the shape."""
    out = (ctypes.c_int * 2)()
    _check(lib().ganq_debug_accum_plan(int(m), int(n), ctypes.cast(out, _c_vp)), "ganq_debug_accum_plan")
    return dict(kernel=ACCUM_KERNELS[out[0]], supported=bool(out[1]))


def debug_top_rule(m: int, n: int, c3: int, c2: int) -> dict:
    """how many digit planes of H the four-wave full bucket sum of an [m, n] layer multiplies when c3 / c2 entries have a non-zero
    digit 3 / digit 2 or 3, under the current developer options (ganq_debug_top_rule; no GPU needed).  cap < 0: no list is wanted."""
    out = (ctypes.c_int * 3)()
    _check(lib().ganq_debug_top_rule(int(m), int(n), int(c3), int(c2), ctypes.cast(out, _c_vp)), "ganq_debug_top_rule")
    return dict(D=out[0], cap=out[1], list_max=out[2])


def debug_top_planes(H, m: int) -> dict:
    """the exception counts of the fixed-point H [n,n] as the T-update's preparation forms them, and the number of dense digit
    planes D of an [m, n] layer under the current developer options (ganq_debug_top_planes)"""
    H = _dev_f32(H, "H")
    n = H.shape[0]
    if H.shape != (n, n):
        raise GanqHipError(f"H must be square, got {tuple(H.shape)}")
    out = (ctypes.c_longlong * 5)()
    _call("ganq_debug_top_planes", (H,), H.data_ptr(), n, int(m), ctypes.cast(out, _c_vp), _ST)
    return dict(c3=out[0], c2=out[1], cap=out[2], list_max=out[3], D=out[4])


def debug_mu_planes(m: int, n: int, c3: int, c2: int) -> dict:
    """how many digit planes of H the incremental bucket sums of an [m, n] layer read on the matrix cores when c3 / c2 entries have
    a non-zero digit 3 / digit 2 or 3, under the current developer options (ganq_debug_mu_planes; no GPU needed); D_full: the full sum's"""
    out = (ctypes.c_int * 2)()
    _check(lib().ganq_debug_mu_planes(int(m), int(n), int(c3), int(c2), ctypes.cast(out, _c_vp)), "ganq_debug_mu_planes")
    return dict(D=out[0], D_full=out[1])


LUT_REGIMES = ("decode16", "decode32", "mfma_small", "gemm", "gemm_splitk", "gemm_pipe", "dense128", "dense256")  # GANQ_LUT_REGIME_*


def debug_lut_plan(M: int, m: int, n: int, bits: int, r: int = 0, outliers: bool = False, ncu: int = 0, device=None) -> dict:
    """which kernels the LUT forward launches for x [M,n] on a layer [m,n] under the current developer options
    (ganq_debug_lut_plan).  ncu > 0: plan for that many compute units, no GPU needed; 0: those of `device` (default: the current
    one).  outliers / adapter: None without them, "fused" inside the LUT launch, "addend" as an fp32 product added by it."""
    out = (ctypes.c_int * 8)()
    args = (int(M), int(m), int(n), int(bits), int(r), 1 if outliers else 0, int(ncu), ctypes.cast(out, _c_vp), 8)
    if ncu > 0:
        _check(lib().ganq_debug_lut_plan(*args), "ganq_debug_lut_plan")
    else:
        with torch.cuda.device(device if device is not None else torch.cuda.current_device()):
            _check(lib().ganq_debug_lut_plan(*args), "ganq_debug_lut_plan")
    mode = {-1: None, 1: "fused", 0: "addend"}
    return dict(regime=LUT_REGIMES[out[0]], row_tiles=out[1], KS=out[2], outliers=mode[out[3]], adapter=mode[out[4]], t_KS=out[5],
                workgroups=out[6], ncu=out[7])


_LUT_WS = {}  # (device index, stream) -> zero-initialised workspace, kept across calls (the kernel leaves it clean)
_LUT_WS_RETIRED = []  # workspaces a larger one superseded: a captured HIP graph may still point into them, so they live as long as the process


def _lut_workspace(nbytes: int, device):
    key = (device.index if device.index is not None else torch.cuda.current_device(), _stream(device))
    ws = _LUT_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        if ws is not None:
            _LUT_WS_RETIRED.append(ws)
        ws = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _call("ganq_lut_linear_workspace_init", (ws,), ws.data_ptr(), ws.numel(), _ST)
        _LUT_WS[key] = ws
    return ws


def outlier_split(W, ratio: float):
    """Algorithm 2 of the paper on the device.  W [m,n] fp32 is overwritten by W_dense (outliers zeroed); returns the
    outliers as CSR (rowptr int32 [m+1], cols int32 [nnz] ascending per row, vals fp32 [nnz]) and the cut-offs [m,2]."""
    W = _dev_f32(W, "W")
    m, n = W.shape
    cut = torch.empty((m, 2), dtype=torch.float32, device=W.device)
    counts = torch.empty((m,), dtype=torch.int32, device=W.device)
    rowptr = torch.empty((m + 1,), dtype=torch.int32, device=W.device)
    _call("ganq_outlier_cutoffs", (W, cut, counts, rowptr), W.data_ptr(), m, n, float(ratio), cut.data_ptr(), counts.data_ptr(), rowptr.data_ptr(),
                                      _ST)
    nnz = int(rowptr[m])  # the one host read: sizes of the CSR arrays
    cols = torch.empty((nnz,), dtype=torch.int32, device=W.device)
    vals = torch.empty((nnz,), dtype=torch.float32, device=W.device)
    if nnz:
        _call("ganq_outlier_extract", (W, cut, rowptr, cols, vals), W.data_ptr(), m, n, cut.data_ptr(), rowptr.data_ptr(), cols.data_ptr(), vals.data_ptr(),
                                          _ST)
    return rowptr, cols, vals, cut


def outlier_matmul(x, rowptr, cols, vals, m: int):
    """x [M,n] fp16/bf16, CSR outliers of a [m,n] weight (vals in x's dtype) -> fp32 [M,m] = x @ W_sparse^T"""
    code = _act_dtype(x, "x")
    if vals.dtype != x.dtype or rowptr.dtype != torch.int32 or cols.dtype != torch.int32:
        raise GanqHipError("outlier_matmul: vals must have x's dtype, rowptr / cols must be int32")
    if rowptr.numel() != m + 1:
        raise GanqHipError("outlier_matmul: rowptr must have out_features + 1 entries")
    x = x.contiguous()
    M, n = x.shape
    out = torch.empty((M, m), dtype=torch.float32, device=x.device)
    _call("ganq_outlier_matmul", (x, rowptr, cols, vals, out), x.data_ptr(), code, M, m, n, rowptr.data_ptr(), _ptr(cols) if cols.numel() else None,
                                     _ptr(vals) if vals.numel() else None, out.data_ptr(), _ST)
    return out


def lut_linear_outliers(x, qweight, lut, bias, bits: int, rowptr, cols, vals):
    """LUT forward of a layer with sparse outliers (CSR by output feature, vals in x's dtype) in one library call."""
    code = _act_dtype(x, "x")
    if lut.dtype != x.dtype or (bias is not None and bias.dtype != x.dtype) or vals.dtype != x.dtype:
        raise GanqHipError("x, lut, bias and outlier values must share one dtype")
    if rowptr.dtype != torch.int32 or cols.dtype != torch.int32 or rowptr.numel() != lut.shape[0] + 1:
        raise GanqHipError("lut_linear_outliers: rowptr / cols must be int32, rowptr of length out_features + 1")
    x, qweight, lut = x.contiguous(), qweight.contiguous(), lut.contiguous()
    M, n = x.shape
    m = lut.shape[0]
    max_rows = ((1 << 31) - 1) // (2 * max(n, 1)) - 256  # see lut_linear
    if M > max_rows:
        step = max(256, max_rows // 256 * 256)
        return torch.cat([lut_linear_outliers(x[r:r + step], qweight, lut, bias, bits, rowptr, cols, vals) for r in range(0, M, step)], dim=0)
    y = torch.empty((M, m), dtype=x.dtype, device=x.device)
    ws = _lut_workspace(lib().ganq_lut_linear_outliers_workspace_bytes(M, m, n, bits), x.device)
    _call("ganq_lut_linear_fwd_outliers", (x, qweight, lut, bias, rowptr, cols, vals, y, ws), x.data_ptr(), qweight.data_ptr(), lut.data_ptr(), _ptr(bias), rowptr.data_ptr(),
                                              cols.data_ptr() if cols.numel() else None,
                                              vals.data_ptr() if vals.numel() else None, code, M, m, n, bits, y.data_ptr(),
                                              ws.data_ptr(), ws.numel(), _ST)
    return y


def lut_linear(x, qweight, lut, bias, bits: int, addend=None):
    """x [M,n] fp16/bf16 (any M: decode kernels up to 64 rows, the fused LUT-dequant GEMM above), qweight int32 [n*bits/32, m],
    lut [m,V], bias [m] or None -> y [M,m].
    addend: optional fp32 [M,m] added before the rounding to x's dtype (the sparse-outlier product)."""
    code = _act_dtype(x, "x")
    if lut.dtype != x.dtype or (bias is not None and bias.dtype != x.dtype):
        raise GanqHipError("x, lut and bias must share one dtype")
    x, qweight, lut = x.contiguous(), qweight.contiguous(), lut.contiguous()
    M, n = x.shape
    m = lut.shape[0]
    # the GEMM kernels address x through 32-bit buffer offsets: more than ~2 GB of activations go in row chunks
    max_rows = ((1 << 31) - 1) // (2 * max(n, 1)) - 256
    if M > max_rows:
        step = max(256, max_rows // 256 * 256)
        return torch.cat([lut_linear(x[r:r + step], qweight, lut, bias, bits, None if addend is None else addend[r:r + step].contiguous())
                          for r in range(0, M, step)], dim=0)
    y = torch.empty((M, m), dtype=x.dtype, device=x.device)
    ws = _lut_workspace(lib().ganq_lut_linear_workspace_bytes(M, m, n, bits), x.device)
    if addend is not None:
        if addend.dtype != torch.float32 or tuple(addend.shape) != (M, m) or not addend.is_contiguous():
            raise GanqHipError("lut_linear: addend must be a contiguous fp32 [M, out_features] tensor")
        _call("ganq_lut_linear_fwd_add", (x, qweight, lut, bias, addend, y, ws), x.data_ptr(), qweight.data_ptr(), lut.data_ptr(), _ptr(bias), addend.data_ptr(), code,
                                             M, m, n, bits, y.data_ptr(), ws.data_ptr(), ws.numel(), _ST)
        return y
    _call("ganq_lut_linear_fwd", (x, qweight, lut, bias, y, ws), x.data_ptr(), qweight.data_ptr(), lut.data_ptr(), _ptr(bias), code, M, m, n, bits,
                                     y.data_ptr(), ws.data_ptr(), ws.numel(), _ST)
    return y


def lut_head_nll(x, qweight, lut, bias, bits: int, targets):
    """per-token negative log-likelihood straight from a packed head, the logits never written (csrc/lut_head_nll.hip):
    x [M,n] fp16/bf16, qweight int32 [n*bits/32, m], lut [m,V], bias [m] or None, targets integer [M]
    -> (nll, lse, tgt_logit), fp32 [M] each.  A row whose target lies outside [0, m) is ignored: nll = tgt_logit = 0."""
    code = _act_dtype(x, "x")
    if lut.dtype != x.dtype or (bias is not None and bias.dtype != x.dtype):
        raise GanqHipError("x, lut and bias must share one dtype")
    if targets.is_floating_point() or targets.dtype == torch.bool or targets.dim() != 1 or targets.shape[0] != x.shape[0]:
        raise GanqHipError(f"lut_head_nll: targets must be an integer tensor [M], got {targets.dtype} {tuple(targets.shape)}")
    x, qweight, lut, targets = x.contiguous(), qweight.contiguous(), lut.contiguous(), targets.long().contiguous()
    M, n = x.shape
    m = lut.shape[0]
    max_rows = ((1 << 31) - 1) // (2 * max(n, 1)) - 256  # see lut_linear
    if M > max_rows:
        step = max(256, max_rows // 256 * 256)
        parts = [lut_head_nll(x[r:r + step], qweight, lut, bias, bits, targets[r:r + step]) for r in range(0, M, step)]
        return tuple(torch.cat([p[i] for p in parts]) for i in range(3))
    out = torch.empty((3, M), dtype=torch.float32, device=x.device)
    if M == 0:
        return out[0], out[1], out[2]
    ws = _workspace(lib().ganq_lut_head_nll_workspace_bytes(M, m, n, bits), x.device)
    _call("ganq_lut_head_nll", (x, qweight, lut, bias, targets, out, ws), x.data_ptr(), qweight.data_ptr(), lut.data_ptr(), _ptr(bias),
          targets.data_ptr(), code, M, m, n, bits, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), ws.data_ptr(), ws.numel(), _ST)
    return out[0], out[1], out[2]


def lut_head_pick(x, qweight, lut, bias, bits: int, noise=None, inv_t: float = 1.0):
    """next token straight from a packed head, the logits never written (csrc/lut_head_pick.hip):
    x [M,n] fp16/bf16, qweight int32 [n*bits/32, m], lut [m,V], bias [m] or None, noise fp32 [M,m] or None, inv_t > 0
    -> (token int64, score, lse, logprob fp32), [M] each: token = the smallest argmax of s + noise with s = logits * inv_t,
    score = s[token], lse = logsumexp(s), logprob = score - lse.  noise=None, inv_t=1 is greedy; noise = -log(Exp(1)) samples."""
    code = _act_dtype(x, "x")
    if lut.dtype != x.dtype or (bias is not None and bias.dtype != x.dtype):
        raise GanqHipError("x, lut and bias must share one dtype")
    M, n = x.shape
    m = lut.shape[0]
    if noise is not None and (noise.dtype != torch.float32 or tuple(noise.shape) != (M, m)):
        raise GanqHipError(f"lut_head_pick: noise must be an fp32 [M, out_features] tensor, got {noise.dtype} {tuple(noise.shape)}")
    x, qweight, lut = x.contiguous(), qweight.contiguous(), lut.contiguous()
    noise = None if noise is None else noise.contiguous()
    max_rows = ((1 << 31) - 1) // (2 * max(n, 1)) - 256  # see lut_linear
    if M > max_rows:
        step = max(256, max_rows // 256 * 256)
        parts = [lut_head_pick(x[r:r + step], qweight, lut, bias, bits, None if noise is None else noise[r:r + step], inv_t)
                 for r in range(0, M, step)]
        return tuple(torch.cat([p[i] for p in parts]) for i in range(4))
    token = torch.empty(M, dtype=torch.int64, device=x.device)
    out = torch.empty((3, M), dtype=torch.float32, device=x.device)
    if M == 0:
        return token, out[0], out[1], out[2]
    ws = _workspace(lib().ganq_lut_head_pick_workspace_bytes(M, m, n, bits), x.device)
    _call("ganq_lut_head_pick", (x, qweight, lut, bias, noise, token, out, ws), x.data_ptr(), qweight.data_ptr(), lut.data_ptr(), _ptr(bias),
          _ptr(noise), float(inv_t), code, M, m, n, bits, token.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
          ws.data_ptr(), ws.numel(), _ST)
    return token, out[0], out[1], out[2]


def _rng_state(state, who: str):
    if state.dtype != torch.int64 or tuple(state.shape) != (2,) or not state.is_contiguous():
        raise GanqHipError(f"{who}: the rng state must be a contiguous int64 [2] tensor {{seed, offset}}, got {state.dtype} {tuple(state.shape)}")
    return state


def lut_head_pick_seeded(x, qweight, lut, bias, bits: int, state, inv_t: float = 1.0, advance: bool = True):
    """lut_head_pick with the Gumbel noise drawn inside the kernel from `state` (int64 [2] on x's device: seed, offset; Philox4x32-10,
    include/ganq_hip.h): no [M, out_features] noise exists.  advance: the call's merge launch stores offset + 1 into `state`.
    -> (token int64, score, lse, logprob fp32), [M] each: the bytes lut_head_pick returns on lut_head_pick_noise(state, M, m)."""
    code = _act_dtype(x, "x")
    if lut.dtype != x.dtype or (bias is not None and bias.dtype != x.dtype):
        raise GanqHipError("x, lut and bias must share one dtype")
    _rng_state(state, "lut_head_pick_seeded")
    M, n = x.shape
    m = lut.shape[0]
    x, qweight, lut = x.contiguous(), qweight.contiguous(), lut.contiguous()
    if M > ((1 << 31) - 1) // (2 * max(n, 1)) - 256:  # see lut_linear
        raise GanqHipError(f"lut_head_pick_seeded: {M} rows of {n} lie beyond the 2 GB window of the kernel's 32-bit offsets and one call "
                           f"consumes one offset: split the rows over several calls")
    token = torch.empty(M, dtype=torch.int64, device=x.device)
    out = torch.empty((3, M), dtype=torch.float32, device=x.device)
    if M == 0:
        return token, out[0], out[1], out[2]
    ws = _workspace(lib().ganq_lut_head_pick_workspace_bytes(M, m, n, bits), x.device)
    _call("ganq_lut_head_pick_seeded", (x, qweight, lut, bias, state, token, out, ws), x.data_ptr(), qweight.data_ptr(), lut.data_ptr(),
          _ptr(bias), state.data_ptr(), int(bool(advance)), float(inv_t), code, M, m, n, bits, token.data_ptr(), out[0].data_ptr(),
          out[1].data_ptr(), out[2].data_ptr(), ws.data_ptr(), ws.numel(), _ST)
    return token, out[0], out[1], out[2]


def lut_head_pick_noise(state, M: int, m: int, words: bool = False):
    """the Gumbel noise fp32 [M, m] lut_head_pick_seeded draws from `state` (and with words=True the raw Philox words, as int32 holding
    the uint32 bits); the state is only read"""
    _rng_state(state, "lut_head_pick_noise")
    noise = torch.empty((M, m), dtype=torch.float32, device=state.device)
    w = torch.empty((M, m), dtype=torch.int32, device=state.device) if words else None
    if M > 0 and m > 0:
        _call("ganq_lut_head_pick_noise", (state, noise, w), state.data_ptr(), M, m, noise.data_ptr(), _ptr(w), _ST)
    return (noise, w) if words else noise


def debug_head_pick_plan(M: int, m: int, n: int, bits: int):
    """(tile launches, feature blocks, merge workgroups, [RT of every tile launch]) of lut_head_pick; host only"""
    launches = -(-int(M) // 64)
    out = (ctypes.c_int * (3 + launches))()
    _check(lib().ganq_debug_head_pick_plan(M, m, n, bits, ctypes.cast(out, _c_vp), 3 + launches), "ganq_debug_head_pick_plan")
    return out[0], out[1], out[2], list(out[3:3 + launches])


def lut_linear_lora(x, qweight, lut, bias, bits: int, lora_A, lora_B, addend=None, outliers=None):
    """LUT forward with a low-rank adapter in one library call: y = round(x Wq^T + t lora_B^T (+ addend) (+ bias)) with
    t = round(x lora_A^T) in x's dtype (fp32 accumulation everywhere, one rounding of y).  x [M,n] fp16/bf16, lora_A [r,n],
    lora_B [m,r] in x's dtype, r a multiple of 16 in [16, 256]; addend: optional fp32 [M,m].
    outliers: (rowptr, cols, vals) of a layer with sparse outliers (CSR by output feature, vals in x's dtype) instead of an addend:
    added inside the decode launch at decode sizes, as the fp32 product of `outlier_matmul` otherwise."""
    code = _act_dtype(x, "x")
    if lut.dtype != x.dtype or (bias is not None and bias.dtype != x.dtype) or lora_A.dtype != x.dtype or lora_B.dtype != x.dtype:
        raise GanqHipError("x, lut, bias, lora_A and lora_B must share one dtype")
    x, qweight, lut, lora_A, lora_B = x.contiguous(), qweight.contiguous(), lut.contiguous(), lora_A.contiguous(), lora_B.contiguous()
    M, n = x.shape
    m = lut.shape[0]
    r = lora_A.shape[0]
    if tuple(lora_A.shape) != (r, n) or tuple(lora_B.shape) != (m, r):
        raise GanqHipError(f"lut_linear_lora: lora_A {tuple(lora_A.shape)} / lora_B {tuple(lora_B.shape)} do not fit x [M,{n}] and {m} out_features")
    if r < 16 or r > 256 or r % 16:
        raise GanqHipError(f"lut_linear_lora: rank {r} must be a multiple of 16 in [16, 256]")
    if addend is not None and (addend.dtype != torch.float32 or tuple(addend.shape) != (M, m) or not addend.is_contiguous()):
        raise GanqHipError("lut_linear_lora: addend must be a contiguous fp32 [M, out_features] tensor")
    max_rows = ((1 << 31) - 1) // (2 * max(n, 1)) - 256  # see lut_linear
    if M > max_rows:
        step = max(256, max_rows // 256 * 256)
        return torch.cat([lut_linear_lora(x[i:i + step], qweight, lut, bias, bits, lora_A, lora_B,
                                          None if addend is None else addend[i:i + step].contiguous(), outliers) for i in range(0, M, step)], dim=0)
    y = torch.empty((M, m), dtype=x.dtype, device=x.device)
    if outliers is not None:
        rowptr, cols, vals = outliers
        if addend is not None:
            raise GanqHipError("lut_linear_lora: pass outliers or an addend, not both")
        if vals.dtype != x.dtype or rowptr.dtype != torch.int32 or cols.dtype != torch.int32 or rowptr.numel() != m + 1:
            raise GanqHipError("lut_linear_lora: outlier vals in x's dtype, rowptr / cols int32, rowptr of length out_features + 1")
        ws = _lut_workspace(lib().ganq_lut_linear_lora_outliers_workspace_bytes(M, m, n, bits, r), x.device)
        _call("ganq_lut_linear_fwd_lora_outliers", (x, qweight, lut, bias, lora_A, lora_B, rowptr, cols, vals, y, ws), x.data_ptr(), qweight.data_ptr(),
              lut.data_ptr(), _ptr(bias), lora_A.data_ptr(), lora_B.data_ptr(), r, rowptr.data_ptr(), cols.data_ptr() if cols.numel() else None,
              vals.data_ptr() if vals.numel() else None, code, M, m, n, bits, y.data_ptr(), ws.data_ptr(), ws.numel(), _ST)
        return y
    ws = _lut_workspace(lib().ganq_lut_linear_lora_workspace_bytes(M, m, n, bits, r), x.device)
    _call("ganq_lut_linear_fwd_lora", (x, qweight, lut, bias, lora_A, lora_B, addend, y, ws), x.data_ptr(), qweight.data_ptr(), lut.data_ptr(),
          _ptr(bias), lora_A.data_ptr(), lora_B.data_ptr(), r, _ptr(addend), code, M, m, n, bits, y.data_ptr(), ws.data_ptr(), ws.numel(), _ST)
    return y


_BWD_CHUNK_BYTES = 1 << 31  # activations per backward call (tests lower it to exercise the chunking)


def _bwd_max_rows(width: int) -> int:
    """rows of a [rows, width] 16-bit activation per call: ~2 GB, as lut_linear splits x"""
    return max(256, ((_BWD_CHUNK_BYTES - 1) // (2 * max(width, 1)) - 256) // 256 * 256)


def lut_linear_bwd_input(dy, qweight, lut, bits: int, addend=None):
    """dx [M,n] = dy [M,m] @ dequant(qweight, lut) (+ addend fp32 [M,n]), fp32 accumulation and one rounding to dy's dtype.
    dy fp16/bf16 [M,m], qweight int32 [n*bits/32, m], lut [m,V] in dy's dtype."""
    code = _act_dtype(dy, "dy")
    if lut.dtype != dy.dtype:
        raise GanqHipError("dy and lut must share one dtype")
    dy, qweight, lut = dy.contiguous(), qweight.contiguous(), lut.contiguous()
    M, m = dy.shape
    n = qweight.shape[0] * 32 // bits
    if lut.shape[0] != m or qweight.shape[1] != m:
        raise GanqHipError("lut_linear_bwd_input: dy, qweight and lut disagree on out_features")
    if addend is not None and (addend.dtype != torch.float32 or tuple(addend.shape) != (M, n)):
        raise GanqHipError("lut_linear_bwd_input: addend must be fp32 [M, in_features]")
    step = _bwd_max_rows(max(m, n))
    if M > step:  # row chunks are independent
        return torch.cat([lut_linear_bwd_input(dy[r:r + step], qweight, lut, bits, None if addend is None else addend[r:r + step])
                          for r in range(0, M, step)], dim=0)
    if addend is not None:
        addend = addend.contiguous()
    dx = torch.empty((M, n), dtype=dy.dtype, device=dy.device)
    ws = _workspace(lib().ganq_lut_linear_bwd_input_workspace_bytes(M, m, n, bits), dy.device)
    _call("ganq_lut_linear_bwd_input", (dy, qweight, lut, addend, dx, ws), dy.data_ptr(), qweight.data_ptr(), lut.data_ptr(), _ptr(addend), code,
          M, m, n, bits, dx.data_ptr(), ws.data_ptr(), ws.numel(), _ST)
    return dx


def lut_linear_bwd_lut(dy, x, qweight, bits: int, m: int):
    """dlut fp32 [m, 2^bits]: dlut[o][v] = sum over rows b and input features j with Q[o][j] == v of dy[b][o] * x[b][j].
    dy [M,m], x [M,n] fp16/bf16 (one dtype), qweight int32 [n*bits/32, m].  Codes no index uses get exactly 0."""
    code = _act_dtype(dy, "dy")
    if x.dtype != dy.dtype:
        raise GanqHipError("dy and x must share one dtype")
    dy, x, qweight = dy.contiguous(), x.contiguous(), qweight.contiguous()
    M, n = x.shape
    if dy.shape != (M, m) or qweight.shape != (n * bits // 32, m):
        raise GanqHipError("lut_linear_bwd_lut: dy [M,m], x [M,n] and qweight [n*bits/32, m] disagree")
    step = _bwd_max_rows(max(m, n))
    if M > step:  # chunk sums are added in chunk order
        out = None
        for r in range(0, M, step):
            part = lut_linear_bwd_lut(dy[r:r + step], x[r:r + step], qweight, bits, m)
            out = part if out is None else out + part
        return out
    dlut = torch.empty((m, 1 << bits), dtype=torch.float32, device=dy.device)
    ws = _workspace(lib().ganq_lut_linear_bwd_lut_workspace_bytes(M, m, n, bits), dy.device)
    _call("ganq_lut_linear_bwd_lut", (dy, x, qweight, dlut, ws), dy.data_ptr(), x.data_ptr(), qweight.data_ptr(), code, M, m, n, bits,
          dlut.data_ptr(), ws.data_ptr(), ws.numel(), _ST)
    return dlut
