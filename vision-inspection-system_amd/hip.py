"""ctypes binding of ``csrc/libvis_hip.so`` (C ABI: ``include/vis_hip.h``).

PyTorch-ROCm is plumbing here: it owns device memory and the HIP stream; every
arithmetic op of the hot path is one of the ``vis_*`` entry points below.  There
is deliberately NO fallback: if the shared library is missing or an entry point
reports an error, the call raises.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Sequence

import torch  # imported BEFORE the library is dlopen-ed: libvis_hip.so must bind to the HIP runtime torch loaded

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB_PATH = os.environ.get("VIS_HIP_LIB") or os.path.join(_CSRC, "libvis_hip.so")     # VIS_HIP_LIB: another build of the same ABI (A/B runs)

ACT_NONE, ACT_QUICKGELU, ACT_GELU_ERF, ACT_SWIGLU = 0, 1, 2, 3
DECODE_KEYS_PER_SPLIT = 64   # DA_MAXKEYS of csrc/decode.hip: a decode-attention split owns this many cached keys

# name -> argtypes; every entry point returns int. 'p' = pointer, 'i' = int, 'f' = float
_SIGS = {
    "vis_abi_version": "",
    "vis_gemm_bf16": "ppppp" + "iiiiiiii" + "p",
    "vis_gemm_bf16_splitk": "pppppp" + "iiiiiiiii" + "p",
    "vis_gemm_bf16_splitk_part": "ppp" + "iiiiii" + "p",
    "vis_splitk_finalize_norm": "p" + "i" + "pppppp" + "iiiii" + "f" + "p",
    "vis_gemm_fp8": "pppppppp" + "iiiiiiiii" + "p",
    "vis_gemm_bf16_plan": "iiiiiiii" + "p" + "i",
    "vis_gemm_fp8_plan": "iiiiiiiii" + "p" + "i",
    "vis_quant_rows_fp8": "ppppp" + "iiii" + "f" + "p",
    "vis_rmsnorm_bf16": "ppp" + "iiii" + "f" + "p",
    "vis_rmsnorm_heads_bf16": "ppp" + "iiiii" + "f" + "p",
    "vis_layernorm_bf16": "pppp" + "iiii" + "f" + "p",
    "vis_qkv_rope_split": "ppppppp" + "iiiiiiii" + "p",
    "vis_qkv_rope_split_many": "ppppppp" + "iiiiiiii" + "i" + "lll" + "p" + "p",
    "vis_attn_prefill": "ppppp" + "iiiiiiiii" + "f" + "p",
    "vis_attn_prefill_rows": "ppppp" + "iiiiiiiii" + "f" + "i" + "p",
    "vis_attn_prefill_rows_many": "ppppp" + "iiiiiiiii" + "f" + "i" + "i" + "lll" + "p" + "p",
    "vis_attn_prefill_pairs": "ppppp" + "iiiiiiii" + "f" + "i" + "p",
    "vis_attn_prefill_pairs_many": "ppppp" + "iiiiiiii" + "f" + "i" + "i" + "lll" + "p" + "p",
    "vis_attn_split_ws_bytes": "ii",
    "vis_attn_prefill_split": "ppppp" + "iiiiiiii" + "f" + "i" + "p" + "l" + "p",
    "vis_gemv_bf16": "pppppp" + "iiiii" + "f" + "p",
    "vis_gemv_fp8w": "ppppppp" + "iiiii" + "f" + "p",
    "vis_gemv_bf16_rows": "pppppp" + "iiiiiiiii" + "f" + "p",
    "vis_gemv_fp8w_rows": "ppppppp" + "iiiiiiiii" + "f" + "p",
    "vis_gemv_mxfp4w": "ppppppp" + "iiiiii" + "f" + "p",
    "vis_gemv_mxfp4w_rows": "ppppppp" + "iiiiiiiiii" + "f" + "p",
    "vis_gemm_decode_mxfp4_ksplit": "ii",
    "vis_gemm_decode_mxfp4": "ppppp" + "iiiiiiiii" + "p",
    "vis_decode_attn": "ppppppppp" + "iiiii" + "f" + "i" + "lll" + "p",
    "vis_decode_attn_shared": "ppppppppp" + "iiiii" + "f" + "i" + "lll" + "i" + "p",
    "vis_decode_attn_parts": "p" + "ii" + "p" * 11 + "iiiii" + "f" + "i" + "ll" + "i" + "p",
    "vis_decode_attn_forked": "ppppppppp" + "iiiii" + "f" + "i" + "lll" + "pp" + "p",
    "vis_decode_attn_parts_forked": "p" + "ii" + "p" * 11 + "iiiii" + "f" + "i" + "ll" + "pp" + "p",
    "vis_decode_chain_sync_ints": "",
    "vis_decode_chain_ws_bytes": "iii",
    "vis_decode_chain_ctx_limit": "iii",
    "vis_decode_chain": "ppi" + "p" * 12 + "i" * 9 + "ff" + "p",
    "vis_gemv_bf16_argmax": "pppp" + "iii" + "f" + "ppp" + "i" + "pp" + "fu" + "p",
    "vis_argmax_f32": "p" + "i" + "ppp" + "i" + "pp" + "fu" + "ii" + "p",
    "vis_logprobs_ws_bytes": "ii",
    "vis_logprobs_f32": "p" + "ii" + "p" + "i" + "p" + "i" + "ppp" + "l" + "i" + "p",
    "vis_json_mask": "pp" + "i" + "p" * 5 + "iip" + "ii" + "p",
    "vis_schema_mask": "pp" + "i" + "p" * 5 + "iip" + "i" + "pppp" + "iii" + "p",
    "vis_argmax_masked_f32": "p" + "i" + "ppp" + "i" + "pp" + "fu" + "ii" + "p" + "i" + "p",
    "vis_gemv_bf16_argmax_masked": "pppp" + "iii" + "f" + "ppp" + "i" + "pp" + "fu" + "p" + "p",
    "vis_gemv_partition": "ii" + "pppp",
    "vis_sample_ws_bytes": "ii",
    "vis_sample_f32": "p" + "ii" + "p" + "i" + "ff" + "pp" + "i" + "pp" + "i" + "pp" + "p",
    "vis_penalty_state_bytes": "ii",
    "vis_penalty_prompt": "pi" + "pi" + "p",
    "vis_penalize_f32": "p" + "ii" + "ppp" + "i" + "pp" + "ii" + "p",
    "vis_shape_ws_bytes": "ii",
    "vis_shape_f32": "p" + "ii" + "p" + "i" + "ppppp" + "p" + "i" + "pp" + "i" + "p",
    "vis_ban_f32": "p" + "ii" + "p" + "i" + "pp" + "i" + "pppppp" + "i" + "p" + "i" + "p" + "ii" + "p",
    "vis_decode_attn_draft": "ppppppppp" + "iiiii" + "f" + "i" + "l" + "p",
    "vis_decode_cross_attn_draft": "pppppppp" + "iiiii" + "ff" + "il" + "p",
    "vis_decode_cross_attn_fp8_draft": "pppppppppp" + "iiiii" + "ff" + "il" + "p",
    "vis_spec_accept": "p" + "iii" + "pppppp" + "i" + "ppp" + "p",
    "vis_spec_accept_sampled": "p" + "iii" + "pppppp" + "i" + "ppp" + "p" + "p",
    "vis_spec_accept_masked": "p" + "iii" + "pppppp" + "i" + "ppp" + "p" + "pi" + "p",
    "vis_schema_mask_rows": "pp" + "i" + "ppp" + "i" + "pppp" + "ii" + "p" + "i" + "pppp" + "ii" + "p",
    "vis_spec_draft_schema": "pp" + "i" + "pppp" + "i" + "pppp" + "ii" + "pp" + "i" + "pp" + "p",
    "vis_spec_draft": "pi" + "pp" + "i" + "pp" + "iiii" + "pp" + "p",
    "vis_spec_draft_pred": "pi" + "pp" + "i" + "pp" + "iiii" + "pi" + "pp" + "pp" + "p",
    "vis_decode_attn_streams": "ii",
    "vis_decode_attn_draft_batch": "ppppppppp" + "iiiii" + "f" + "ii" + "lll" + "p",
    "vis_spec_gather_batch": "pppp" + "iiii" + "p",
    "vis_spec_accept_batch": "p" + "iiii" + "pppppp" + "i" + "ppp" + "p" + "p",
    "vis_spec_draft_batch": "pi" + "pp" + "i" + "pp" + "iiiii" + "pp" + "p",
    "vis_stop_scan": "pp" + "i" + "pppp" + "i" + "pppp" + "iiii" + "p",
    "vis_stream_publish": "pp" + "i" + "pp" + "i" + "pp" + "i" + "pp" + "i" + "p",
    "vis_host_coherent_alloc": "ppl",
    "vis_host_free": "p",
    "vis_gemm_decode_ksplit": "ii",
    "vis_gemm_decode_bf16": "pppp" + "iiiiiiii" + "p",
    "vis_gemm_decode_fp8_ksplit": "ii",
    "vis_gemm_decode_fp8": "pppppp" + "iiiiiiii" + "p",
    "vis_skinny_finalize_fp8": "p" + "i" + "ppppp" + "pppp" + "iiiiiii" + "f" + "p",
    "vis_skinny_finalize": "p" + "i" + "ppppp" + "iiiiii" + "f" + "p",
    "vis_decode_proj_ws_bytes": "iiii",
    "vis_decode_proj_bf16": "p" * 12 + "i" * 13 + "f" + "p",
    "vis_decode_proj_fp8": "p" * 14 + "i" * 14 + "f" + "p",
    "vis_decode_prep_rows": "p" * 8 + "i" * 6 + "p",
    "vis_decode_proj_colpar_covers": "iii",
    "vis_decode_proj_colpar_bf16": "p" * 11 + "i" * 13 + "f" + "p",
    "vis_decode_proj_colpar_fp8": "p" * 13 + "i" * 14 + "f" + "p",
    "vis_patchify_u8": "pp" + "iiii" + "pp" + "p",
    "vis_resize_rgb_u8": "ppp" + "iiii" + "ppi" + "ppi" + "p",
    "vis_jpeg_to_rgb": "pppp" + "i" * 11 + "p",
    "vis_patchify_tiles_u8": "pp" + "iiiiii" + "pp" + "p",
    "vis_add_rows_bf16": "ppp" + "iiii" + "p",
    "vis_decode_cross_attn": "pppppppp" + "iiiii" + "ff" + "p",
    "vis_decode_cross_attn_batch": "pppppppp" + "iiiii" + "ff" + "ill" + "p",
    "vis_decode_cross_attn_fp8": "pppppppppp" + "iiiii" + "ff" + "p",
    "vis_decode_cross_attn_fp8_batch": "pppppppppp" + "iiiii" + "ff" + "illl" + "p",
    "vis_image_stats_u8": "p" + "ii" + "p" + "p",
    "vis_gather_rows": "ppp" + "iii" + "p",
    "vis_scatter_rows": "ppp" + "iii" + "p",
}
_CT = {"p": ctypes.c_void_p, "i": ctypes.c_int, "f": ctypes.c_float, "u": ctypes.c_uint, "l": ctypes.c_longlong}


_UPLOAD_STREAMS: dict = {}


def upload(arr, device) -> "torch.Tensor":
    """Host array -> device tensor WITHOUT blocking the launching thread.

    ``torch.from_numpy(a).to(device)`` copies from pageable memory: the call is synchronous AND stream-ordered, i.e. the
    host sleeps until everything already queued on the current stream has run (cProfile of run_batch_inspection, r03: 192
    such calls = 0.98 s of a 2.8 s batch - the launch thread could not run ahead of the GPU).  Here the array goes through
    a pinned staging copy on a dedicated upload stream; the current stream is made to wait for it with an event, the host
    is not.  PyTorch's pinned-memory allocator keeps the staging block alive until the copy has completed."""
    import numpy as _np
    dev = torch.device(device)
    st = _UPLOAD_STREAMS.get(dev)
    if st is None:
        st = _UPLOAD_STREAMS[dev] = torch.cuda.Stream(device=dev)
    if isinstance(arr, torch.Tensor) and arr.device.type == "cpu" and arr.is_pinned():
        src = arr                                        # already page-locked (jpeg.parse on a pool thread): no staging copy
    else:
        src = torch.from_numpy(_np.ascontiguousarray(arr)).pin_memory()
    with torch.cuda.stream(st):
        out = src.to(dev, non_blocking=True)
    cur = torch.cuda.current_stream(dev)
    cur.wait_stream(st)
    out.record_stream(cur)
    return out


class HipLibraryError(RuntimeError):
    """The gfx950 extension is missing or an entry point rejected its arguments."""


class ChainRefused(HipLibraryError):
    """vis_decode_chain returned VIS_ERR_UNSUPPORTED: the head shape is outside the chained form or its grid is larger than the
    device holds resident.  Nothing was launched; the caller issues the four launches (same results bit for bit)."""


class ChainStalled(HipLibraryError):
    """A bounded wait inside a chained layer-head launch (vis_decode_chain) gave up: its workgroups could not all be resident
    - another process or stream was running a chained launch on the same device at the same time."""


_lib: Optional[ctypes.CDLL] = None

# Optional host-side accounting of the time a thread spends INSIDE the library's entry points (launch + argument marshalling;
# the GIL is released during the C call): hip.call_trace_start() / call_trace_stop() -> {thread id: [calls, seconds]}.  Used
# by the seam blocks of bench.py to tell "the launch thread is busy launching" from "the launch thread is waiting" (VERDICT r4
# item 6b); off by default (one global read per call).
_CALL_TRACE: Optional[dict] = None


class _Entry:
    """ctypes function + the optional per-thread call accounting."""
    __slots__ = ("fn",)

    def __init__(self, fn):
        self.fn = fn

    def __call__(self, *args):
        tr = _CALL_TRACE
        if tr is None:
            return self.fn(*args)
        import threading
        import time
        t0 = time.perf_counter()
        rc = self.fn(*args)
        e = tr.setdefault(threading.get_ident(), [0, 0.0])
        e[0] += 1
        e[1] += time.perf_counter() - t0
        return rc


class _Lib:
    """Attribute access to the wrapped entry points (same spelling as the ctypes.CDLL it replaces)."""

    def __init__(self, cdll):
        self._cdll = cdll

    def __getattr__(self, name):
        e = _Entry(getattr(self._cdll, name))
        object.__setattr__(self, name, e)
        return e


def call_trace_start() -> None:
    global _CALL_TRACE
    _CALL_TRACE = {}


def call_trace_stop() -> dict:
    global _CALL_TRACE
    tr, _CALL_TRACE = _CALL_TRACE, None
    return tr or {}


def exported_symbols() -> list:
    return list(_SIGS)


def load() -> ctypes.CDLL:
    """Load libvis_hip.so (once).  Raises HipLibraryError when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryError(
            f"{LIB_PATH} not found: build it with `make -C {_CSRC}` (or __graft_entry__.build()); "
            "this package has no CPU fallback")
    lib = ctypes.CDLL(LIB_PATH)
    for name, sig in _SIGS.items():
        fn = getattr(lib, name)  # AttributeError here means header and library disagree
        fn.restype = ctypes.c_int
        fn.argtypes = [_CT[c] for c in sig]
    lib.vis_decode_chain_ws_bytes.restype = ctypes.c_longlong
    lib.vis_decode_proj_ws_bytes.restype = ctypes.c_longlong
    lib.vis_logprobs_ws_bytes.restype = ctypes.c_longlong
    lib.vis_sample_ws_bytes.restype = ctypes.c_longlong
    lib.vis_penalty_state_bytes.restype = ctypes.c_longlong
    lib.vis_shape_ws_bytes.restype = ctypes.c_longlong
    _lib = _Lib(lib)
    return _lib


def _check(rc: int, name: str) -> None:
    if rc != 0:
        why = {1: "argument/shape/alignment precondition violated", 2: "HIP launch error",
               3: "shape not covered by this kernel form on this device"}.get(rc, "unknown")
        raise HipLibraryError(f"{name} failed with status {rc} ({why})")


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise HipLibraryError("device tensor required (no CPU path exists)")
    return t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _bf16(t: torch.Tensor, name: str) -> None:
    if t.dtype != torch.bfloat16:
        raise HipLibraryError(f"{name}: bf16 tensor required, got {t.dtype}")


# --------------------------------------------------------------------------- K2
def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None,
         residual: Optional[torch.Tensor] = None, act: int = ACT_NONE,
         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[M,N(/2)] = act(a[M,K] @ w[N,K].T + bias) + residual."""
    _bf16(a, "gemm a"); _bf16(w, "gemm w")
    M, K = a.shape
    N, K2 = w.shape
    if K != K2 or a.stride(1) != 1 or w.stride(1) != 1:
        raise HipLibraryError(f"gemm: bad operand shapes/strides {tuple(a.shape)} x {tuple(w.shape)}")
    n_out = N // 2 if act == ACT_SWIGLU else N
    if out is None:
        out = torch.empty((M, n_out), dtype=torch.bfloat16, device=a.device)
    if out.shape != (M, n_out) or out.stride(1) != 1:
        raise HipLibraryError("gemm: bad output shape")
    if residual is not None and (residual.shape != (M, N) or residual.stride(1) != 1):
        raise HipLibraryError("gemm: bad residual shape")
    if bias is not None and bias.numel() != N:
        raise HipLibraryError("gemm: bad bias shape")
    rc = load().vis_gemm_bf16(_ptr(a), _ptr(w), _ptr(bias), _ptr(residual), _ptr(out), M, N, K,
                              a.stride(0), w.stride(0), out.stride(0),
                              residual.stride(0) if residual is not None else 0, act, _stream())
    _check(rc, "vis_gemm_bf16")
    return out


def gemm_splitk(a: torch.Tensor, w: torch.Tensor, work: torch.Tensor, ksplit: int = 2,
                bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None, act: int = ACT_NONE,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Split-K GEMM (256x256 tiles, f32 partials in ``work``, fixed-order finalisation)."""
    _bf16(a, "gemm a"); _bf16(w, "gemm w")
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K or a.stride(1) != 1 or w.stride(1) != 1 or act == ACT_SWIGLU:
        raise HipLibraryError("gemm_splitk: bad operands")
    if work.dtype != torch.float32 or work.numel() < ksplit * M * N:
        raise HipLibraryError("gemm_splitk: workspace too small")
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=a.device)
    rc = load().vis_gemm_bf16_splitk(_ptr(a), _ptr(w), _ptr(bias), _ptr(residual), _ptr(out), _ptr(work), M, N, K,
                                     a.stride(0), w.stride(0), out.stride(0),
                                     residual.stride(0) if residual is not None else 0, act, ksplit, _stream())
    _check(rc, "vis_gemm_bf16_splitk")
    return out


def gemm_splitk_part(a: torch.Tensor, w: torch.Tensor, work: torch.Tensor, ksplit: int = 2) -> torch.Tensor:
    """The K-sliced tiles of gemm_splitk alone: work[:ksplit*M*N] (f32) = partial sums of a @ w.T per K slice."""
    _bf16(a, "gemm a"); _bf16(w, "gemm w")
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K or a.stride(1) != 1 or w.stride(1) != 1:
        raise HipLibraryError("gemm_splitk_part: bad operands")
    if work.dtype != torch.float32 or work.numel() < ksplit * M * N:
        raise HipLibraryError("gemm_splitk_part: workspace too small")
    rc = load().vis_gemm_bf16_splitk_part(_ptr(a), _ptr(w), _ptr(work), M, N, K, a.stride(0), w.stride(0), ksplit, _stream())
    _check(rc, "vis_gemm_bf16_splitk_part")
    return work


def splitk_finalize_norm(work: torch.Tensor, ksplit: int, x_out: torch.Tensor, bias: Optional[torch.Tensor] = None,
                         residual: Optional[torch.Tensor] = None, norm_w: Optional[torch.Tensor] = None,
                         norm_b: Optional[torch.Tensor] = None, y_out: Optional[torch.Tensor] = None,
                         eps: float = 1e-6) -> None:
    """x_out = bf16(sum of the K-slice partials + bias + residual); y_out (optional) = RMSNorm (norm_b None) or LayerNorm
    of x_out - one row pass instead of finalise + norm.  residual may alias x_out."""
    M, N = x_out.shape
    if work.dtype != torch.float32 or work.numel() < ksplit * M * N or x_out.stride(1) != 1:
        raise HipLibraryError("splitk_finalize_norm: bad operands")
    if y_out is not None and (norm_w is None or y_out.shape != x_out.shape or y_out.stride(1) != 1):
        raise HipLibraryError("splitk_finalize_norm: bad norm operands")
    rc = load().vis_splitk_finalize_norm(_ptr(work), ksplit, _ptr(bias), _ptr(residual), _ptr(x_out), _ptr(norm_w),
                                         _ptr(norm_b), _ptr(y_out), M, N,
                                         residual.stride(0) if residual is not None else 0, x_out.stride(0),
                                         y_out.stride(0) if y_out is not None else 0, float(eps), _stream())
    _check(rc, "vis_splitk_finalize_norm")


def quant_rows_fp8(x: torch.Tensor, q: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None,
                   norm_w: Optional[torch.Tensor] = None, eps: float = 1e-6, norm_b: Optional[torch.Tensor] = None):
    """bf16 [M, K] -> (e4m3 bytes [M, >= K] uint8, f32 row scales [M]) on the GPU; optional fused RMSNorm (norm_w) or
    LayerNorm (norm_w + norm_b) in front."""
    _bf16(x, "quant_rows_fp8 x")
    M, K = x.shape
    if q is None:
        q = torch.empty((M, K), dtype=torch.uint8, device=x.device)
    if scale is None:
        scale = torch.empty(M, dtype=torch.float32, device=x.device)
    if q.dtype != torch.uint8 or q.shape[0] != M or q.shape[1] < K or q.stride(1) != 1 or scale.numel() != M \
            or x.stride(1) != 1:
        raise HipLibraryError("quant_rows_fp8: bad shapes")
    rc = load().vis_quant_rows_fp8(_ptr(x), _ptr(norm_w), _ptr(norm_b), _ptr(q), _ptr(scale), M, K, x.stride(0), q.stride(0), eps,
                                   _stream())
    _check(rc, "vis_quant_rows_fp8")
    return q, scale


def gemm_fp8(aq: torch.Tensor, sa: torch.Tensor, wq: torch.Tensor, sw: torch.Tensor,
             bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None, act: int = ACT_NONE,
             out: Optional[torch.Tensor] = None, work: Optional[torch.Tensor] = None, ksplit: int = 0) -> torch.Tensor:
    """out[M, N(/2)] = act((aq @ wq.T) * sa[:, None] * sw[None, :] + bias) + residual on the fp8 MFMA.
    ``work`` (f32, >= ksplit*M*N) + ``ksplit`` select the split-K form."""
    M, K = aq.shape
    N = wq.shape[0]
    if aq.dtype != torch.uint8 or wq.dtype != torch.uint8 or wq.shape[1] != K or aq.stride(1) != 1 or wq.stride(1) != 1:
        raise HipLibraryError("gemm_fp8: uint8 (e4m3) operands [M,K] / [N,K] required")
    if sa.dtype != torch.float32 or sw.dtype != torch.float32 or sa.numel() != M or sw.numel() != N:
        raise HipLibraryError("gemm_fp8: bad scales")
    n_out = N // 2 if act == ACT_SWIGLU else N
    if out is None:
        out = torch.empty((M, n_out), dtype=torch.bfloat16, device=aq.device)
    if out.shape != (M, n_out) or out.stride(1) != 1:
        raise HipLibraryError("gemm_fp8: bad output shape")
    if work is not None and (work.dtype != torch.float32 or work.numel() < ksplit * M * N):
        raise HipLibraryError("gemm_fp8: split-K workspace too small")
    rc = load().vis_gemm_fp8(_ptr(aq), _ptr(sa), _ptr(wq), _ptr(sw), _ptr(bias), _ptr(residual), _ptr(out),
                             _ptr(work), ksplit if work is not None else 0, M, N, K,
                             aq.stride(0), wq.stride(0), out.stride(0),
                             residual.stride(0) if residual is not None else 0, act, _stream())
    _check(rc, "vis_gemm_fp8")
    return out


# kernel ids of the plan queries (csrc/gemm_bf16.hip, csrc/gemm_fp8.hip); an id names the same tile shape in both
GEMM_KERNEL_NAMES = {1: "128x128", 7: "256x256_pp", 8: "128x256_pp"}
GEMM_FP8_KERNEL_NAMES = {1: "128x128", 7: "256x256_pp"}


def _gemm_plan(fn, args, names) -> dict:
    import ctypes
    buf = (ctypes.c_int * 23)()
    n = fn(*args, ctypes.cast(buf, ctypes.c_void_p), 23)
    if n <= 0:
        raise HipLibraryError(f"gemm plan: arguments rejected {args}")
    launches = [dict(kernel=names[buf[3 + 5 * i]], n0=buf[4 + 5 * i], ncols=buf[5 + 5 * i],
                     tiles_m=buf[6 + 5 * i], tiles_n=buf[7 + 5 * i]) for i in range(n)]
    return dict(wide=bool(buf[1]), nt=bool(buf[2]), launches=launches, kernels=tuple(l["kernel"] for l in launches))


def gemm_plan(M: int, N: int, K: int, act: int = ACT_NONE, ldc: Optional[int] = None, ldr: Optional[int] = None,
              residual: bool = False, aligned16: bool = True) -> dict:
    """Host-only: the launches vis_gemm_bf16 makes for this problem (kernel per column range), its epilogue form and
    store policy.  Needs no GPU."""
    n_out = N // 2 if act == ACT_SWIGLU else N
    ldc = n_out if ldc is None else ldc
    ldr = (ldc if ldr is None else ldr) if residual else 0
    return _gemm_plan(load().vis_gemm_bf16_plan, (M, N, K, ldc, ldr, act, int(residual), int(aligned16)),
                      GEMM_KERNEL_NAMES)


def gemm_fp8_plan(M: int, N: int, K: int, act: int = ACT_NONE, ldc: Optional[int] = None, ldr: Optional[int] = None,
                  residual: bool = False, aligned16: bool = True, split: bool = False) -> dict:
    """Host-only: the launches vis_gemm_fp8 makes for this problem.  Needs no GPU."""
    n_out = N // 2 if act == ACT_SWIGLU else N
    ldc = n_out if ldc is None else ldc
    ldr = (ldc if ldr is None else ldr) if residual else 0
    return _gemm_plan(load().vis_gemm_fp8_plan, (M, N, K, ldc, ldr, act, int(residual), int(aligned16), int(split)),
                      GEMM_FP8_KERNEL_NAMES)


# --------------------------------------------------------------------------- K3 / K5
def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _bf16(x, "rmsnorm x")
    rows, N = x.shape
    if out is None:
        out = torch.empty_like(x)
    rc = load().vis_rmsnorm_bf16(_ptr(x), _ptr(w), _ptr(out), rows, N, x.stride(0), out.stride(0), eps, _stream())
    _check(rc, "vis_rmsnorm_bf16")
    return out


def rmsnorm_heads(x: torch.Tensor, w: torch.Tensor, heads: int, eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """RMSNorm of every 128-wide head slice x[:, 128 h : 128 (h + 1)], h < heads, with the one weight w [128] - ``rmsnorm`` on each
    slice (bit-identical), one launch.  x [tokens, >= heads * 128] (columns beyond are left alone); in place unless ``out``."""
    _bf16(x, "rmsnorm_heads x"); _bf16(w, "rmsnorm_heads w")
    if out is None:
        out = x
    if x.dim() != 2 or x.stride(1) != 1 or out.shape != x.shape or out.stride(1) != 1 or w.numel() != 128 or x.shape[1] < heads * 128:
        raise HipLibraryError("rmsnorm_heads: bad shapes")
    rc = load().vis_rmsnorm_heads_bf16(_ptr(x), _ptr(w), _ptr(out), x.shape[0], heads, 128, x.stride(0), out.stride(0), eps, _stream())
    _check(rc, "vis_rmsnorm_heads_bf16")
    return out


def layernorm(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _bf16(x, "layernorm x")
    rows, N = x.shape
    if out is None:
        out = torch.empty_like(x)
    rc = load().vis_layernorm_bf16(_ptr(x), _ptr(w), _ptr(b), _ptr(out), rows, N, x.stride(0), out.stride(0),
                                   eps, _stream())
    _check(rc, "vis_layernorm_bf16")
    return out


# --------------------------------------------------------------------------- K4
def qkv_rope_split(qkv: torch.Tensor, cos: Optional[torch.Tensor], sin: Optional[torch.Tensor],
                   q: Optional[torch.Tensor], k: Optional[torch.Tensor], v: Optional[torch.Tensor],
                   vt: Optional[torch.Tensor], n_q: int, n_kv: int, head_dim: int, k_pos0: int = 0,
                   vt_col0: int = 0) -> None:
    """qkv [S, (Hq+2Hkv)*HD] -> q [Hq,S,HD], k/v [Hkv,T,HD] rows k_pos0.., vt [Hkv,HD,ld] columns vt_col0.. (a
    multiple of 64: a row-range of a longer sequence writes its own 64-key column blocks).
    n_q == 0 (k/v only) or n_kv == 0 (q only) give a partial split; cos = sin = None means no rotation."""
    _bf16(qkv, "qkv")
    S = qkv.shape[0]
    if (cos is None) != (sin is None):
        raise HipLibraryError("qkv_rope_split: give both cos and sin or neither")
    if cos is not None:
        if cos.dtype != torch.float32 or cos.shape != (S, head_dim) or sin.shape != (S, head_dim):
            raise HipLibraryError("qkv_rope_split: cos/sin must be f32 [S, head_dim]")
        if not (cos.is_contiguous() and sin.is_contiguous()):
            raise HipLibraryError("qkv_rope_split: contiguous tensors required")
    if n_q > 0 and (q is None or q.shape != (n_q, S, head_dim) or not q.is_contiguous()):
        raise HipLibraryError("qkv_rope_split: bad q shape")
    if n_kv > 0 and (k is None or k.shape[0] != n_kv or k.shape[2] != head_dim or not k.is_contiguous()):
        raise HipLibraryError("qkv_rope_split: bad k shape")
    if v is not None and (k is None or v.shape != k.shape or not v.is_contiguous()):
        raise HipLibraryError("qkv_rope_split: bad v shape")
    vt_ld = 0
    if vt is not None:
        if vt.shape[0] != n_kv or vt.shape[1] != head_dim or not vt.is_contiguous():
            raise HipLibraryError("qkv_rope_split: bad vt shape")
        vt_ld = vt.shape[2]
        if vt_col0 % 64 or vt_col0 + (S + 63) // 64 * 64 > vt_ld:
            raise HipLibraryError("qkv_rope_split: bad vt column offset")
    vt_ptr = (_ptr(vt) + 2 * vt_col0) if vt is not None else None
    rc = load().vis_qkv_rope_split(_ptr(qkv), _ptr(cos), _ptr(sin), _ptr(q), _ptr(k), _ptr(v), vt_ptr,
                                   S, qkv.stride(0), n_q, n_kv, head_dim, k.shape[1] if k is not None else 0,
                                   k_pos0, vt_ld, _stream())
    _check(rc, "vis_qkv_rope_split")


MAX_GROUP_REQUESTS = 8      # VIS_MAX_REQ of csrc/common.hip.h


def _kv_offsets(name: str, base: torch.Tensor, kv_off: Sequence[int], need: int):
    import ctypes
    n = len(kv_off)
    if not 1 <= n <= MAX_GROUP_REQUESTS:
        raise HipLibraryError(f"{name}: 1..{MAX_GROUP_REQUESTS} requests per launch")
    if not base.is_contiguous() or any(o < 0 or o % 8 or o + need > base.numel() for o in kv_off):
        raise HipLibraryError(f"{name}: cache offsets must be multiples of 8 inside the (contiguous) cache tensor")
    return (ctypes.c_longlong * n)(*[int(o) for o in kv_off])


def qkv_rope_split_many(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, q: torch.Tensor, k_base: torch.Tensor,
                        v_base: torch.Tensor, vt: torch.Tensor, n_q: int, n_kv: int, head_dim: int, kv_off: Sequence[int],
                        k_tokens: int, k_pos0: int = 0, vt_col0: int = 0) -> None:
    """``qkv_rope_split`` for the k requests of a prompt-pass group in ONE launch: qkv [k * S, nq] (request r = rows r S ..), one
    cos / sin [S, D] for all, q [k, Hq, S, D], the caches as whole tensors with ``kv_off[r]`` = element offset of request r's
    [Hkv, k_tokens, D] block (same for k and v), vt [k, Hkv, D, ld] (any stride between requests)."""
    import ctypes
    _bf16(qkv, "qkv"); _bf16(q, "q"); _bf16(k_base, "k"); _bf16(v_base, "v"); _bf16(vt, "vt")
    k = len(kv_off)
    S = cos.shape[0]
    if cos.dtype != torch.float32 or cos.shape != (S, head_dim) or sin.shape != cos.shape or not (cos.is_contiguous() and sin.is_contiguous()):
        raise HipLibraryError("qkv_rope_split_many: cos/sin must be contiguous f32 [S, head_dim]")
    if qkv.shape[0] != k * S or qkv.stride(1) != 1 or q.shape != (k, n_q, S, head_dim) or not q.is_contiguous():
        raise HipLibraryError("qkv_rope_split_many: bad qkv / q shape")
    if vt.dim() != 4 or vt.shape[:3] != (k, n_kv, head_dim) or not vt[0].is_contiguous() or v_base.shape != k_base.shape:
        raise HipLibraryError("qkv_rope_split_many: bad vt / cache shape")
    vt_ld = vt.shape[3]
    if vt_col0 % 64 or vt_col0 + (S + 63) // 64 * 64 > vt_ld or k_pos0 + S > k_tokens:
        raise HipLibraryError("qkv_rope_split_many: bad offsets")
    offs = _kv_offsets("qkv_rope_split_many", k_base, kv_off, n_kv * k_tokens * head_dim)
    rc = load().vis_qkv_rope_split_many(_ptr(qkv), _ptr(cos), _ptr(sin), _ptr(q), _ptr(k_base), _ptr(v_base),
                                        _ptr(vt) + 2 * vt_col0, S, qkv.stride(0), n_q, n_kv, head_dim, k_tokens, k_pos0, vt_ld,
                                        k, S * qkv.stride(0), q.stride(0), vt.stride(0) if k > 1 else 0,
                                        ctypes.cast(offs, ctypes.c_void_p), _stream())
    _check(rc, "vis_qkv_rope_split_many")


def attn_prefill_pairs_many(q: torch.Tensor, k_base: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, work: torch.Tensor,
                            scale: float, kv_off: Sequence[int], k_tokens: int, q_row0: int = 0) -> torch.Tensor:
    """``attn_prefill_pairs`` for the k requests of a prompt-pass group in ONE launch (same work list): q [k, Hq, S, D], the K cache
    as a whole tensor + ``kv_off`` (as qkv_rope_split_many), vt [k, Hkv, D, ld], out [k * S, >= Hq * D] (request r = rows r S ..)."""
    import ctypes
    _bf16(q, "q"); _bf16(k_base, "k"); _bf16(vt, "vt"); _bf16(out, "out")
    k, Hq, S, HD = q.shape
    if len(kv_off) != k or not q.is_contiguous() or HD != 128:
        raise HipLibraryError("attn_prefill_pairs_many: bad q shape")
    Hkv = vt.shape[1]
    if vt.dim() != 4 or vt.shape[0] != k or vt.shape[2] != HD or not vt[0].is_contiguous() or out.shape[0] != k * S or out.stride(1) != 1:
        raise HipLibraryError("attn_prefill_pairs_many: bad vt / out shape")
    if work.dtype != torch.int32 or work.dim() != 2 or work.shape[1] != 4 or not work.is_contiguous():
        raise HipLibraryError("attn_prefill_pairs_many: work must be int32 [n,4]")
    offs = _kv_offsets("attn_prefill_pairs_many", k_base, kv_off, Hkv * k_tokens * HD)
    rc = load().vis_attn_prefill_pairs_many(_ptr(q), _ptr(k_base), _ptr(vt), _ptr(out), _ptr(work), work.shape[0], Hq, Hkv, HD,
                                            S, k_tokens, vt.shape[3], out.stride(0), scale, int(q_row0), k, q.stride(0),
                                            vt.stride(0) if k > 1 else 0, S * out.stride(0),
                                            ctypes.cast(offs, ctypes.c_void_p), _stream())
    _check(rc, "vis_attn_prefill_pairs_many")
    return out


# --------------------------------------------------------------------------- K6 / K7
ATTN_SLOTS = 768          # resident head_dim-80 attention workgroups on MI355X: 256 CUs x 3 (head_dim 128: x 2)
ATTN_HALF_COST = 0.6      # a 64-row item relative to a 128-row item (same K/V staging, half the MFMAs)


def _attn_makespan(n_full: int, n_half: int, slots: int = ATTN_SLOTS) -> float:
    """Greedy list schedule of n_full unit items followed by n_half cheaper ones on `slots` workgroup slots."""
    import heapq
    free = [0.0] * slots
    for cost, n in ((1.0, n_full), (ATTN_HALF_COST, n_half)):
        for _ in range(n):
            heapq.heappush(free, heapq.heappop(free) + cost)
    return max(free)


def plan_attn_items(segments, heads: int, block_q: int = 128, slots: int = ATTN_SLOTS):
    """Non-causal work items [(q0, qn, k0, k1)], full (<= block_q rows) items first, then 64-row halves.
    Measured rule (MI355X, ViT 4900 x 16 heads): as long as everything stays ONE round of the resident slots, finer
    items balance the CUs better (30 full + 17 half items per head: 0.214 ms; 39 full: 0.226 ms); one workgroup past
    the round costs 20 % (28 + 21: 0.260 ms).  So trailing full items are cut in two while items x heads <= slots;
    grids that need several rounds anyway use the modelled list schedule to fill the last round with halves."""
    full, half = [], []
    for (s, e) in segments:
        for q0 in range(s, e, block_q):
            qn = min(block_q, e - q0)
            (half if qn <= block_q // 2 else full).append((q0, qn, s, e))
    if heads <= 0 or not full:
        return full + half
    k = len(full)
    if (len(full) + len(half)) * heads <= slots:
        while k > 0 and (k - 1 + len(half) + 2 * (len(full) - k + 1)) * heads <= slots - heads:   # one item of slack
            k -= 1
    elif len(full) * heads > slots:
        keep = (len(full) * heads // slots) * slots // heads       # fulls that fill whole rounds
        best = (_attn_makespan(len(full) * heads, len(half) * heads, slots), len(full))
        for c in (keep, keep - 1):
            if 0 < c < len(full):
                t = _attn_makespan(c * heads, (len(half) + 2 * (len(full) - c)) * heads, slots)
                if t < best[0] - 1e-9:
                    best = (t, c)
        k = best[1]
    for (q0, qn, s, e) in full[k:]:
        h1 = min(block_q // 2, ((qn + 1) // 2 + 15) // 16 * 16)
        half.append((q0, h1, s, e))
        half.append((q0 + h1, qn - h1, s, e))
    return full[:k] + half


ATTN_SPLIT_MIN_BLOCKS = 24      # segments shorter than this many 128-row blocks are never key-split


def plan_attn_items_split(segments, heads: int, block_q: int = 128, slots: int = ATTN_SLOTS):
    """Non-causal head_dim-80 work items with KEY-SPLIT blocks (vis_attn_prefill_split) -> (items, n_pairs).

    A segment of nb >= ATTN_SPLIT_MIN_BLOCKS row blocks gets its last min(whole blocks, slots // heads - nb) whole
    blocks cut in two along the keys (at the multiple of 64 nearest the middle of the segment): one 1024 x 1024 image at
    16 heads becomes 30 whole + 2 x 9 half workgroups per head = exactly the 768 resident slots, two whole and one half
    per CU, instead of 2450 wave tasks of which some SIMDs get three and others two (measured 171 -> 154 us).
    The rule looks at ONE segment and the head count only - never at what else shares the launch - so an image's
    features stay bit-identical whether it runs alone or stacked with others.  Whole items first, split ones last."""
    whole, split, n_pairs = [], [], 0
    budget = slots // max(heads, 1)
    for seg in segments:
        # (start, end): queries and keys are the same range; (start, end, k0, k1): queries [start, end) over keys [k0, k1)
        # (the mllama tower: a present tile's rows see every canvas row, the pad rows only the present ones)
        s, e = seg[0], seg[1]
        ks, ke = (seg[2], seg[3]) if len(seg) == 4 else (s, e)
        blocks = [(q0, min(block_q, e - q0)) for q0 in range(s, e, block_q)]
        nb = len(blocks)
        n_whole = sum(1 for b in blocks if b[1] == block_q)
        # fill whole rounds: a segment of nb <= budget blocks is topped up to one round (budget - nb splits), a longer one -
        # 51 blocks per head on 48 slots for a 2 x 2-tile mllama canvas: two rounds with the second 6 % full - to the next
        # whole number of rounds
        rounds = -(-nb // budget) if budget > 0 else 1
        ns = min(n_whole, max(0, rounds * budget - nb)) if (heads > 0 and nb >= ATTN_SPLIT_MIN_BLOCKS) else 0
        mid = ((ks + ke) // 2 + 32) // 64 * 64
        if not (ks < mid < ke):
            ns = 0
        first_split = n_whole - ns
        for i, (q0, qn) in enumerate(blocks):
            if qn == block_q and i >= first_split and ns > 0:
                for part, (k0, k1) in enumerate(((ks, mid), (mid, ke))):
                    split.append((q0, qn | ((1 | part << 1 | n_pairs << 2) << 8), k0, k1))
                n_pairs += 1
            else:
                whole.append((q0, qn, ks, ke))
    return whole + split, n_pairs


class AttnPlan:
    """Work list of one ViT attention layout (+ the key-split workspaces when the plan has split items: one per stream
    that launches it - launches of one stream are ordered, two streams must not share counters and partial slots)."""
    __slots__ = ("work", "n_pairs", "ws_bytes", "heads", "_ws")

    def __init__(self, work, n_pairs, ws_bytes, heads):
        self.work, self.n_pairs, self.ws_bytes, self.heads = work, n_pairs, ws_bytes, heads
        self._ws = {}

    @property
    def ws(self) -> "torch.Tensor":
        """The workspace of the CURRENT stream (zeroed on that stream when first used)."""
        key = torch.cuda.current_stream(self.work.device).cuda_stream
        w = self._ws.get(key)
        if w is None:
            w = self._ws[key] = torch.zeros(self.ws_bytes, dtype=torch.uint8, device=self.work.device)
        return w


def make_vit_attn_plan(segments, device, heads: int, split: bool = True) -> AttnPlan:
    """Plan for attn_prefill_plan over independent token ranges [(start, end)] - or [(start, end, k0, k1)]: queries over a
    key range of their own - (non-causal, head_dim 80)."""
    n_pairs = 0
    if split:
        items, n_pairs = plan_attn_items_split(segments, heads)
    if n_pairs == 0:
        if any(len(sg) == 4 for sg in segments):
            items = [(q0, min(128, sg[1] - q0), sg[2] if len(sg) == 4 else sg[0], sg[3] if len(sg) == 4 else sg[1])
                     for sg in segments for q0 in range(sg[0], sg[1], 128)]
            work = torch.tensor(items, dtype=torch.int32, device=device).reshape(-1, 4).contiguous()
            return AttnPlan(work, 0, 0, heads)
        return AttnPlan(make_attn_work(segments, False, device, heads=heads), 0, 0, heads)
    work = torch.tensor(items, dtype=torch.int32, device=device).reshape(-1, 4).contiguous()
    nbytes = int(load().vis_attn_split_ws_bytes(n_pairs, heads))
    if nbytes <= 0:
        raise HipLibraryError("vis_attn_split_ws_bytes refused the plan")
    return AttnPlan(work, n_pairs, nbytes, heads)


def attn_prefill_plan(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, plan: AttnPlan,
                      scale: float) -> torch.Tensor:
    """Non-causal attention over plan's items; q [Hq,S,80], k [Hkv,T,80], vt [Hkv,80,ld] -> out [S, Hq*80].  Launches of
    one stream are ordered on that stream's workspace; different streams get their own."""
    if plan.n_pairs == 0:
        return attn_prefill(q, k, vt, out, plan.work, False, scale)
    _bf16(q, "q"); _bf16(k, "k"); _bf16(vt, "vt"); _bf16(out, "out")
    Hq, S, HD = q.shape
    Hkv, T, _ = k.shape
    if not (q.is_contiguous() and k.is_contiguous() and vt.is_contiguous()):
        raise HipLibraryError("attn_prefill_plan: contiguous tensors required")
    if vt.shape[0] != Hkv or vt.shape[1] != HD or out.shape[0] != S or out.stride(1) != 1 or Hq != plan.heads:
        raise HipLibraryError("attn_prefill_plan: bad shapes")
    ws = plan.ws
    rc = load().vis_attn_prefill_split(_ptr(q), _ptr(k), _ptr(vt), _ptr(out), _ptr(plan.work), plan.work.shape[0], Hq, Hkv,
                                       HD, S, T, vt.shape[2], out.stride(0), scale, plan.n_pairs, _ptr(ws), ws.numel(),
                                       _stream())
    _check(rc, "vis_attn_prefill_split")
    return out


def make_attn_work(segments, causal: bool, device, block_q: int = 128, heads: int = 0) -> torch.Tensor:
    """Work list for attn_prefill: segments = [(start, end)] of independent token ranges.

    Each item {q0, qn, k0, k1}: queries [q0, q0+qn) attend keys [k0, k1) (and key <= query
    when causal).  Workgroups are dispatched in list order (heads fastest).  Causal: heavy (late) tiles
    first.  Non-causal with ``heads`` given: see plan_attn_items.
    """
    if causal:
        items = []
        for (s, e) in segments:
            for q0 in range(s, e, block_q):
                items.append((q0, min(block_q, e - q0), s, e))
        items.sort(key=lambda it: -(it[0] + it[1]))
    else:
        items = plan_attn_items(segments, heads, block_q)
    return torch.tensor(items, dtype=torch.int32, device=device).reshape(-1, 4).contiguous()


def vt_key_order(n_cols: int, device=None) -> torch.Tensor:
    """key_of_col [n_cols] (n_cols % 32 == 0): the key stored at every V^T column (ABI version 2: inside each aligned
    group of 32 keys, key 16a + 4h + r sits at column 8h + 4a + r).  ``vt = v_transposed[..., vt_key_order(ld)]`` turns
    a plainly transposed V into the layout vis_attn_prefill reads (vis_qkv_rope_split writes it directly)."""
    if n_cols % 32:
        raise HipLibraryError("vt_key_order: column count must be a multiple of 32")
    c = torch.arange(n_cols, device=device)
    return (c & ~31) | (((c >> 2) & 1) << 4) | (((c >> 3) & 3) << 2) | (c & 3)


def attn_prefill(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, work: torch.Tensor,
                 causal: bool, scale: float, q_row0: int = 0) -> torch.Tensor:
    """q [Hq,S,HD], k [Hkv,T,HD], vt [Hkv,HD,ld] -> out [S, Hq*HD].  q_row0 > 0: q / out hold rows q_row0.. of a longer
    sequence whose positions the work items (and the causal rule) refer to."""
    _bf16(q, "q"); _bf16(k, "k"); _bf16(vt, "vt"); _bf16(out, "out")
    Hq, S, HD = q.shape
    Hkv, T, _ = k.shape
    if not (q.is_contiguous() and k.is_contiguous() and vt.is_contiguous()):
        raise HipLibraryError("attn_prefill: contiguous tensors required")
    if vt.shape[0] != Hkv or vt.shape[1] != HD or out.shape[0] != S or out.stride(1) != 1:
        raise HipLibraryError("attn_prefill: bad shapes")
    if work.dtype != torch.int32 or work.dim() != 2 or work.shape[1] != 4 or not work.is_contiguous():
        raise HipLibraryError("attn_prefill: work must be int32 [n,4]")
    rc = load().vis_attn_prefill_rows(_ptr(q), _ptr(k), _ptr(vt), _ptr(out), _ptr(work), work.shape[0], Hq, Hkv, HD,
                                      S, T, vt.shape[2], out.stride(0), 1 if causal else 0, scale, int(q_row0), _stream())
    _check(rc, "vis_attn_prefill_rows")
    return out


def attn_prefill_many(q: torch.Tensor, k_base: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, work: torch.Tensor,
                      causal: bool, scale: float, kv_off: Sequence[int], k_tokens: int, q_row0: int = 0) -> torch.Tensor:
    """``attn_prefill`` (head_dim 128) for the k requests of a prompt-pass group in ONE launch: q [k, Hq, S, D], the K tensor as a
    whole + ``kv_off[r]`` = element offset of request r's [Hkv, k_tokens, D] block, vt [k, Hkv, D, ld], work int32 [k, n, 4] (one
    list per request), out [k * S, >= Hq * D] (request r = rows r S ..)."""
    import ctypes
    _bf16(q, "q"); _bf16(k_base, "k"); _bf16(vt, "vt"); _bf16(out, "out")
    k, Hq, S, HD = q.shape
    if len(kv_off) != k or not q.is_contiguous() or HD != 128:
        raise HipLibraryError("attn_prefill_many: bad q shape")
    Hkv = vt.shape[1]
    if vt.dim() != 4 or vt.shape[0] != k or vt.shape[2] != HD or not vt[0].is_contiguous() or out.shape[0] != k * S or out.stride(1) != 1:
        raise HipLibraryError("attn_prefill_many: bad vt / out shape")
    if work.dtype != torch.int32 or work.dim() != 3 or work.shape[0] != k or work.shape[2] != 4 or not work.is_contiguous():
        raise HipLibraryError("attn_prefill_many: work must be int32 [k, n, 4]")
    offs = _kv_offsets("attn_prefill_many", k_base, kv_off, Hkv * k_tokens * HD)
    rc = load().vis_attn_prefill_rows_many(_ptr(q), _ptr(k_base), _ptr(vt), _ptr(out), _ptr(work), work.shape[1], Hq, Hkv, HD,
                                           S, k_tokens, vt.shape[3], out.stride(0), 1 if causal else 0, scale, int(q_row0), k,
                                           q.stride(0), vt.stride(0) if k > 1 else 0, S * out.stride(0),
                                           ctypes.cast(offs, ctypes.c_void_p), _stream())
    _check(rc, "vis_attn_prefill_rows_many")
    return out


def make_attn_pairs(q_start: int, q_end: int, device, block_q: int = 128) -> torch.Tensor:
    """Work list of attn_prefill_pairs for the causal pass over query rows [q_start, q_end) of one sequence (keys from
    0): the 128-row blocks are paired latest-with-earliest, so every workgroup - and every wave in it - covers the
    same number of (16-row block x 64-key tile) units.  Items {qB0, qBn, qA0, qAn}; an odd middle block has qAn = 0."""
    blocks = [(q0, min(block_q, q_end - q0)) for q0 in range(q_start, q_end, block_q)]
    items = []
    i, j = 0, len(blocks) - 1
    while i < j:
        items.append((blocks[j][0], blocks[j][1], blocks[i][0], blocks[i][1]))
        i += 1
        j -= 1
    if i == j:
        items.append((blocks[i][0], blocks[i][1], 0, 0))
    return torch.tensor(items, dtype=torch.int32, device=device).reshape(-1, 4).contiguous()


def attn_prefill_pairs(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, work: torch.Tensor,
                       scale: float, q_row0: int = 0) -> torch.Tensor:
    """Causal head_dim-128 prefill attention with paired query blocks (work from make_attn_pairs); same tensors and
    results as attn_prefill(..., causal=True)."""
    _bf16(q, "q"); _bf16(k, "k"); _bf16(vt, "vt"); _bf16(out, "out")
    Hq, S, HD = q.shape
    Hkv, T, _ = k.shape
    if not (q.is_contiguous() and k.is_contiguous() and vt.is_contiguous()):
        raise HipLibraryError("attn_prefill_pairs: contiguous tensors required")
    if HD != 128 or vt.shape[0] != Hkv or vt.shape[1] != HD or out.shape[0] != S or out.stride(1) != 1:
        raise HipLibraryError("attn_prefill_pairs: bad shapes")
    if work.dtype != torch.int32 or work.dim() != 2 or work.shape[1] != 4 or not work.is_contiguous():
        raise HipLibraryError("attn_prefill_pairs: work must be int32 [n,4]")
    rc = load().vis_attn_prefill_pairs(_ptr(q), _ptr(k), _ptr(vt), _ptr(out), _ptr(work), work.shape[0], Hq, Hkv, HD,
                                       S, T, vt.shape[2], out.stride(0), scale, int(q_row0), _stream())
    _check(rc, "vis_attn_prefill_pairs")
    return out


# --------------------------------------------------------------------------- K10 / K11 / K12
def gemv(x: torch.Tensor, w: torch.Tensor, out: torch.Tensor, bias: Optional[torch.Tensor] = None,
         residual: Optional[torch.Tensor] = None, norm_w: Optional[torch.Tensor] = None,
         act: int = ACT_NONE, eps: float = 1e-6) -> torch.Tensor:
    _bf16(x, "gemv x"); _bf16(w, "gemv w")
    N, K = w.shape
    if x.numel() != K or w.stride(1) != 1:
        raise HipLibraryError("gemv: bad shapes")
    n_out = N // 2 if act == ACT_SWIGLU else N
    if out.numel() != n_out or out.dtype not in (torch.bfloat16, torch.float32):
        raise HipLibraryError("gemv: bad output")
    rc = load().vis_gemv_bf16(_ptr(x), _ptr(w), _ptr(bias), _ptr(residual), _ptr(norm_w), _ptr(out), N, K,
                              w.stride(0), act, 1 if out.dtype == torch.float32 else 0, eps, _stream())
    _check(rc, "vis_gemv_bf16")
    return out


def gemv_grid(N: int, act: int = ACT_NONE):
    """(row pairs, workgroups) of a single-row bf16 gemv launch over N weight rows: the grid rule of csrc/decode.hip."""
    n_pairs = N // 2 if act == ACT_SWIGLU else (N + 1) // 2
    blocks = (n_pairs + 3) // 4
    if blocks > 1024:
        blocks = 1024 + (blocks - 1024) // 8
    return n_pairs, min(blocks, 2048)


def gemv_partition(n_pairs: int, n_waves: int):
    """(q, r, m, s) with which the shape-specialised gemv instances split n_pairs row pairs over n_waves waves: wave w owns
    [b(w), b(w + 1)), b(w) = q * w + ((r * w * m) >> s).  Host arithmetic only (vis_gemv_partition); no GPU needed."""
    q, r, s, m = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_uint()
    rc = load().vis_gemv_partition(n_pairs, n_waves, ctypes.addressof(q), ctypes.addressof(r), ctypes.addressof(m),
                                   ctypes.addressof(s))
    _check(rc, "vis_gemv_partition")
    return q.value, r.value, m.value, s.value


def quantize_fp8_rows(w: torch.Tensor):
    """bf16/f32 [N, K] -> (OCP e4m3 bytes [N, K] as uint8, f32 per-row scale [N]); scale = amax / 448, RNE cast.
    Load-time plumbing (torch), not part of the per-token path."""
    wf = w.float()
    scale = (wf.abs().amax(dim=1) / 448.0).clamp_min(1e-12)
    q = (wf / scale[:, None]).to(torch.float8_e4m3fn)
    return q.view(torch.uint8).contiguous(), scale.contiguous()


def gemv_fp8(x: torch.Tensor, wq: torch.Tensor, scale: torch.Tensor, out: torch.Tensor,
             bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
             norm_w: Optional[torch.Tensor] = None, act: int = ACT_NONE, eps: float = 1e-6) -> torch.Tensor:
    """gemv with fp8 (e4m3) weights + per-row scales; same options as gemv."""
    _bf16(x, "gemv_fp8 x")
    N, K = wq.shape
    if wq.dtype != torch.uint8 or scale.dtype != torch.float32 or scale.numel() != N or x.numel() != K or wq.stride(1) != 1:
        raise HipLibraryError("gemv_fp8: bad shapes / dtypes")
    n_out = N // 2 if act == ACT_SWIGLU else N
    if out.numel() != n_out or out.dtype not in (torch.bfloat16, torch.float32):
        raise HipLibraryError("gemv_fp8: bad output")
    rc = load().vis_gemv_fp8w(_ptr(x), _ptr(wq), _ptr(scale), _ptr(bias), _ptr(residual), _ptr(norm_w), _ptr(out), N, K,
                              wq.stride(0), act, 1 if out.dtype == torch.float32 else 0, eps, _stream())
    _check(rc, "vis_gemv_fp8w")
    return out


def _rows_check(name, x, K, out, n_out, residual):
    if x.dim() != 2 or not (1 <= x.shape[0] <= 4) or x.shape[1] != K or x.stride(1) != 1:
        raise HipLibraryError(f"{name}: x must be [1..4, K] with unit column stride")
    B = x.shape[0]
    if out.dim() != 2 or out.shape != (B, n_out) or out.stride(1) != 1 or out.dtype not in (torch.bfloat16, torch.float32):
        raise HipLibraryError(f"{name}: bad output")
    if residual is not None and (residual.shape != (B, n_out) or residual.stride(1) != 1):
        raise HipLibraryError(f"{name}: bad residual")
    return B


def gemv_rows(x: torch.Tensor, w: torch.Tensor, out: torch.Tensor, bias: Optional[torch.Tensor] = None,
              residual: Optional[torch.Tensor] = None, norm_w: Optional[torch.Tensor] = None,
              act: int = ACT_NONE, eps: float = 1e-6) -> torch.Tensor:
    """gemv for 1..4 input rows x [B, K] -> out [B, n_out]: one pass over the weights for all rows, every row bit-identical
    to ``gemv`` on it (no partial buffer, no finalisation launch)."""
    _bf16(x, "gemv_rows x"); _bf16(w, "gemv_rows w")
    N, K = w.shape
    if w.stride(1) != 1:
        raise HipLibraryError("gemv_rows: bad weight")
    B = _rows_check("gemv_rows", x, K, out, N // 2 if act == ACT_SWIGLU else N, residual)
    rc = load().vis_gemv_bf16_rows(_ptr(x), _ptr(w), _ptr(bias), _ptr(residual), _ptr(norm_w), _ptr(out), B, N, K,
                                   w.stride(0), x.stride(0), out.stride(0), residual.stride(0) if residual is not None else 0,
                                   act, 1 if out.dtype == torch.float32 else 0, eps, _stream())
    _check(rc, "vis_gemv_bf16_rows")
    return out


def gemv_fp8_rows(x: torch.Tensor, wq: torch.Tensor, scale: torch.Tensor, out: torch.Tensor,
                  bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
                  norm_w: Optional[torch.Tensor] = None, act: int = ACT_NONE, eps: float = 1e-6) -> torch.Tensor:
    """gemv_fp8 for 1..4 input rows (W8A16), every row bit-identical to ``gemv_fp8`` on it."""
    _bf16(x, "gemv_fp8_rows x")
    N, K = wq.shape
    if wq.dtype != torch.uint8 or scale.dtype != torch.float32 or scale.numel() != N or wq.stride(1) != 1:
        raise HipLibraryError("gemv_fp8_rows: bad shapes / dtypes")
    B = _rows_check("gemv_fp8_rows", x, K, out, N // 2 if act == ACT_SWIGLU else N, residual)
    rc = load().vis_gemv_fp8w_rows(_ptr(x), _ptr(wq), _ptr(scale), _ptr(bias), _ptr(residual), _ptr(norm_w), _ptr(out), B,
                                   N, K, wq.stride(0), x.stride(0), out.stride(0),
                                   residual.stride(0) if residual is not None else 0, act,
                                   1 if out.dtype == torch.float32 else 0, eps, _stream())
    _check(rc, "vis_gemv_fp8w_rows")
    return out


# --------------------------------------------------------------------------- K10 on MXFP4 weights (W4A16)
# OCP Microscaling FP4: E2M1 codes (sign << 3 | exp << 1 | man), one E8M0 scale byte per 32 consecutive K-elements of a row
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def quantize_mxfp4_rows(w: torch.Tensor):
    """bf16/f32 [N, K] (K % 32 == 0) -> (Wq uint8 [N, K/2], Ws uint8 [N, K/32]): byte j of a row holds element 2j in its low
    and 2j+1 in its high nibble; Ws is the E8M0 byte b of each block of 32, X = 2^(b-127) the SMALLEST power of two with
    block_amax / X <= 6 (amax = m 2^E, m in [1, 2): b = E + 125 when m <= 1.5, else E + 126), clamped to 3..250; an all-zero
    block gets b = 127.  Elements round to the nearest E2M1 value, ties to the even mantissa bit.  Every step is exact
    integer / power-of-two arithmetic, so CPU and GPU tensors give identical bytes.  Load-time plumbing (torch)."""
    if w.dim() != 2 or w.shape[1] % 32 != 0:
        raise HipLibraryError("quantize_mxfp4_rows: [N, K] with K % 32 == 0 required")
    N, K = w.shape
    blk = w.float().reshape(N, K // 32, 32)
    amax = blk.abs().amax(-1)
    bits = amax.contiguous().view(torch.int32)
    e, man = (bits >> 23) & 0xFF, bits & 0x7FFFFF
    b = (e - torch.where(man <= 0x400000, 2, 1)).clamp(3, 250)
    b = torch.where(amax == 0, torch.full_like(b, 127), b)
    a = torch.ldexp(blk.abs(), (127 - b)[..., None]).clamp_max(6.0)     # |w| / X, exact
    # grid steps 0.5 below 2, 1 below 4, 2 up to 6; torch.round is half-to-even, and an even multiple of the step is the
    # code with mantissa bit 0
    code = torch.where(a < 2, torch.round(a * 2), torch.where(a < 4, torch.round(a) + 2, torch.round(a * 0.5) + 4))
    code = code.to(torch.uint8) | (torch.signbit(blk).to(torch.uint8) << 3)
    code = code.reshape(N, K // 2, 2)
    return (code[..., 0] | (code[..., 1] << 4)).contiguous(), b.to(torch.uint8).contiguous()


def dequantize_mxfp4(wq: torch.Tensor, ws: torch.Tensor) -> torch.Tensor:
    """(Wq uint8 [N, K/2], Ws uint8 [N, >= K/32]) -> f32 [N, K], exactly what vis_gemv_mxfp4w multiplies with."""
    if wq.dtype != torch.uint8 or ws.dtype != torch.uint8 or wq.dim() != 2 or ws.dim() != 2 or wq.shape[1] % 16 != 0 \
            or ws.shape[0] != wq.shape[0] or ws.shape[1] < wq.shape[1] // 16:
        raise HipLibraryError("dequantize_mxfp4: bad shapes / dtypes")
    N, K = wq.shape[0], wq.shape[1] * 2
    code = torch.stack((wq & 15, wq >> 4), dim=-1).reshape(N, K).long()
    table = torch.tensor(E2M1_VALUES + tuple(-v for v in E2M1_VALUES), dtype=torch.float32, device=wq.device)
    v = table[code].reshape(N, K // 32, 32)
    return torch.ldexp(v, (ws[:, :K // 32].to(torch.int32) - 127)[..., None]).reshape(N, K)


def _mxfp4_check(name, wq, ws):
    if wq.dtype != torch.uint8 or ws.dtype != torch.uint8 or wq.dim() != 2 or ws.dim() != 2 or wq.stride(1) != 1 \
            or ws.stride(1) != 1 or ws.shape[0] != wq.shape[0]:
        raise HipLibraryError(f"{name}: bad shapes / dtypes")
    return wq.shape[0], wq.shape[1] * 2


def gemv_mxfp4(x: torch.Tensor, wq: torch.Tensor, ws: torch.Tensor, out: torch.Tensor,
               bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
               norm_w: Optional[torch.Tensor] = None, act: int = ACT_NONE, eps: float = 1e-6) -> torch.Tensor:
    """gemv with MXFP4 weights (quantize_mxfp4_rows); same options as gemv."""
    _bf16(x, "gemv_mxfp4 x")
    N, K = _mxfp4_check("gemv_mxfp4", wq, ws)
    if x.numel() != K:
        raise HipLibraryError("gemv_mxfp4: bad shapes / dtypes")
    n_out = N // 2 if act == ACT_SWIGLU else N
    if out.numel() != n_out or out.dtype not in (torch.bfloat16, torch.float32):
        raise HipLibraryError("gemv_mxfp4: bad output")
    rc = load().vis_gemv_mxfp4w(_ptr(x), _ptr(wq), _ptr(ws), _ptr(bias), _ptr(residual), _ptr(norm_w), _ptr(out), N, K,
                                wq.stride(0), ws.stride(0), act, 1 if out.dtype == torch.float32 else 0, eps, _stream())
    _check(rc, "vis_gemv_mxfp4w")
    return out


def gemv_mxfp4_rows(x: torch.Tensor, wq: torch.Tensor, ws: torch.Tensor, out: torch.Tensor,
                    bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
                    norm_w: Optional[torch.Tensor] = None, act: int = ACT_NONE, eps: float = 1e-6) -> torch.Tensor:
    """gemv_mxfp4 for 1..4 input rows (W4A16), every row bit-identical to ``gemv_mxfp4`` on it."""
    _bf16(x, "gemv_mxfp4_rows x")
    N, K = _mxfp4_check("gemv_mxfp4_rows", wq, ws)
    B = _rows_check("gemv_mxfp4_rows", x, K, out, N // 2 if act == ACT_SWIGLU else N, residual)
    rc = load().vis_gemv_mxfp4w_rows(_ptr(x), _ptr(wq), _ptr(ws), _ptr(bias), _ptr(residual), _ptr(norm_w), _ptr(out), B,
                                     N, K, wq.stride(0), ws.stride(0), x.stride(0), out.stride(0),
                                     residual.stride(0) if residual is not None else 0, act,
                                     1 if out.dtype == torch.float32 else 0, eps, _stream())
    _check(rc, "vis_gemv_mxfp4w_rows")
    return out


def decode_gemm_mxfp4_ksplit(N: int, K: int) -> int:
    """Partial slots ``decode_gemm_mxfp4`` writes for (N, K): 1..16, fixed by the shape alone (0: shape not covered)."""
    return load().vis_gemm_decode_mxfp4_ksplit(int(N), int(K))


def decode_gemm_mxfp4(x: torch.Tensor, wq: torch.Tensor, ws: torch.Tensor, part: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None, ksplit: int = 0) -> int:
    """``decode_gemm`` on MXFP4 weights (quantize_mxfp4_rows) for 5..64 rows: f32 partials part[slot][part_rows(B)][N] whose
    sum over the returned number of slots is x[B,K] @ dequantize_mxfp4(wq, ws).T (every slot is written), or - with ``out``
    instead of ``part`` - a direct bf16 / f32 result.  The codes and scales are streamed once for all rows."""
    _bf16(x, "decode_gemm_mxfp4 x")
    N, K = _mxfp4_check("decode_gemm_mxfp4", wq, ws)
    if x.dim() != 2 or x.shape[1] != K or x.stride(1) != 1 or ws.shape[1] * 32 < K or (part is None) == (out is None):
        raise HipLibraryError("decode_gemm_mxfp4: bad shapes (give exactly one of part / out)")
    B = x.shape[0]
    lib = load()
    if part is not None:
        ks = ksplit or lib.vis_gemm_decode_mxfp4_ksplit(N, K)
        if part.dtype != torch.float32 or part.numel() < ks * part_rows(B) * N:
            raise HipLibraryError("decode_gemm_mxfp4: partial workspace too small")
        rc = lib.vis_gemm_decode_mxfp4(_ptr(x), _ptr(wq), _ptr(ws), _ptr(part), None, B, N, K, x.stride(0), wq.stride(0),
                                       ws.stride(0), 0, ks, 0, _stream())
    else:
        ks = 1
        if out.shape != (B, N) or out.stride(1) != 1 or out.dtype not in (torch.bfloat16, torch.float32):
            raise HipLibraryError("decode_gemm_mxfp4: bad output")
        rc = lib.vis_gemm_decode_mxfp4(_ptr(x), _ptr(wq), _ptr(ws), None, _ptr(out), B, N, K, x.stride(0), wq.stride(0),
                                       ws.stride(0), out.stride(0), 1, 1 if out.dtype == torch.float32 else 0, _stream())
    _check(rc, "vis_gemm_decode_mxfp4")
    return ks


def _fork_tables(who: str, fork, B: int, device, shared_len: int):
    """(parent, fork_len) of a forked attention call: int32 device tensors with one entry per sequence."""
    par, fl = fork
    if shared_len:
        raise HipLibraryError(f"{who}: give the fork tables or shared_len, not both")
    for t in (par, fl):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.numel() != B or not t.is_contiguous() \
                or t.device != device:
            raise HipLibraryError(f"{who}: fork tables must be contiguous int32 device tensors of {B} entries")
    return par, fl


def decode_attn_parts(part: torch.Tensor, ksplit: int, cos_t: torch.Tensor, sin_t: torch.Tensor, k_cache: torch.Tensor,
                      v_cache: torch.Tensor, step: torch.Tensor, part_o: torch.Tensor, part_ml: torch.Tensor,
                      out: torch.Tensor, n_q: int, n_kv: int, head_dim: int, nsplit: int, scale: float,
                      bias: Optional[torch.Tensor] = None, sx: Optional[torch.Tensor] = None,
                      sw: Optional[torch.Tensor] = None, shared_len: int = 0,
                      fork: Optional[tuple] = None) -> torch.Tensor:
    """``skinny_finalize[_fp8](part, ksplit, qkv, ..)`` + ``decode_attn(qkv, ..)`` of a batch as ONE launch: the attention
    workgroups finalise the qkv columns they need from the projection's partial slabs (same bits as the pair).
    Batch of B: caches [B,Hkv,T,D], tables [B,T,D], step [B], out [B, Hq*D]; ``part`` as decode_gemm[_fp8] left it.
    ``fork`` = (parent, fork_len), two int32 device tensors [B], in place of ``shared_len``: vis_decode_attn_parts_forked."""
    _bf16(k_cache, "k_cache")
    if step.dtype != torch.int32 or cos_t.dtype != torch.float32 or sin_t.dtype != torch.float32 or part.dtype != torch.float32:
        raise HipLibraryError("decode_attn_parts: step int32 / cos,sin,part f32 required")
    if k_cache.dim() != 4:
        raise HipLibraryError("decode_attn_parts: batched caches [B, Hkv, T, D] required")
    B = k_cache.shape[0]
    kc = k_cache[0]
    if kc.shape[0] != n_kv or kc.shape[2] != head_dim or v_cache.shape != k_cache.shape \
            or kc.stride(2) != 1 or kc.stride(1) != head_dim or kc.stride(0) != kc.shape[1] * head_dim:
        raise HipLibraryError("decode_attn_parts: bad cache shape")
    T = kc.shape[1]
    if cos_t[0].shape != (T, head_dim) or sin_t.shape != cos_t.shape or not cos_t[0].is_contiguous():
        raise HipLibraryError("decode_attn_parts: cos/sin tables must be [B, cache_tokens, head_dim]")
    nq = (n_q + 2 * n_kv) * head_dim
    rows = part_rows(B)
    if part.numel() < ksplit * rows * nq or step.numel() != B:
        raise HipLibraryError("decode_attn_parts: partial buffer too small / bad step shape")
    if part_o.dtype != torch.float32 or part_o.numel() < B * n_q * nsplit * head_dim \
            or part_ml.numel() < B * n_q * nsplit * 2 or out.numel() != B * n_q * head_dim:
        raise HipLibraryError("decode_attn_parts: workspace/output too small")
    if bias is not None and (bias.dtype != torch.bfloat16 or bias.numel() != nq):
        raise HipLibraryError("decode_attn_parts: bad bias")
    if (sx is None) != (sw is None) or (sx is not None and (sx.dtype != torch.float32 or sw.dtype != torch.float32
                                                          or sx.numel() < B or sw.numel() != nq)):
        raise HipLibraryError("decode_attn_parts: bad scales")
    if v_cache.stride(0) != k_cache.stride(0) or cos_t.stride(0) != sin_t.stride(0):
        raise HipLibraryError("decode_attn_parts: k/v caches (cos/sin tables) must share their batch stride")
    if fork is not None:
        par, fl = _fork_tables("decode_attn_parts", fork, B, k_cache.device, shared_len)
        rc = load().vis_decode_attn_parts_forked(_ptr(part), int(ksplit), rows, _ptr(bias), _ptr(sx), _ptr(sw), _ptr(cos_t),
                                                 _ptr(sin_t), _ptr(k_cache), _ptr(v_cache), _ptr(step), _ptr(part_o),
                                                 _ptr(part_ml), _ptr(out), n_q, n_kv, head_dim, T, nsplit, scale, B,
                                                 k_cache.stride(0), cos_t.stride(0), _ptr(par), _ptr(fl), _stream())
        _check(rc, "vis_decode_attn_parts_forked")
        return out
    rc = load().vis_decode_attn_parts(_ptr(part), int(ksplit), rows, _ptr(bias), _ptr(sx), _ptr(sw), _ptr(cos_t), _ptr(sin_t),
                                      _ptr(k_cache), _ptr(v_cache), _ptr(step), _ptr(part_o), _ptr(part_ml), _ptr(out),
                                      n_q, n_kv, head_dim, T, nsplit, scale, B, k_cache.stride(0), cos_t.stride(0),
                                      int(shared_len), _stream())
    _check(rc, "vis_decode_attn_parts")
    return out


def decode_attn(qkv: torch.Tensor, cos_t: torch.Tensor, sin_t: torch.Tensor, k_cache: torch.Tensor,
                v_cache: torch.Tensor, step: torch.Tensor, part_o: torch.Tensor, part_ml: torch.Tensor,
                out: torch.Tensor, n_q: int, n_kv: int, head_dim: int, nsplit: int, scale: float,
                shared_len: int = 0, fork: Optional[tuple] = None) -> torch.Tensor:
    """Fused decode step attention: rope(q,k) + KV append at slot step[b] + attention over step[b]+1 keys.

    Single sequence: qkv [nq*D], caches [Hkv,T,D], tables [T,D], step [1].
    Batch of B: qkv [B, nq*D], caches [B,Hkv,T,D], tables [B,T,D], step [B], out [B, Hq*D].
    ``shared_len`` (batch only, a multiple of 64): the first shared_len cached keys are identical in every sequence and are
    read from sequence 0's copy (vis_decode_attn_shared; same result bit for bit).
    ``fork`` (batch only) = (parent, fork_len), two int32 device tensors [B]: sequence b reads keys [0, fork_len[b]) from
    sequence parent[b]'s cache (vis_decode_attn_forked; same result bit for bit)."""
    _bf16(qkv, "qkv"); _bf16(k_cache, "k_cache")
    if step.dtype != torch.int32 or cos_t.dtype != torch.float32 or sin_t.dtype != torch.float32:
        raise HipLibraryError("decode_attn: step int32 / cos,sin f32 required")
    batched = k_cache.dim() == 4
    B = k_cache.shape[0] if batched else 1
    kc = k_cache[0] if batched else k_cache
    if kc.shape[0] != n_kv or kc.shape[2] != head_dim or v_cache.shape != k_cache.shape \
            or kc.stride(2) != 1 or kc.stride(1) != head_dim or kc.stride(0) != kc.shape[1] * head_dim:
        raise HipLibraryError("decode_attn: bad cache shape")
    T = kc.shape[1]
    tab = cos_t[0] if batched else cos_t
    if tab.shape != (T, head_dim) or sin_t.shape != cos_t.shape or not tab.is_contiguous():
        raise HipLibraryError("decode_attn: cos/sin tables must be [cache_tokens, head_dim]")
    nq = (n_q + 2 * n_kv) * head_dim
    if qkv.numel() != B * nq or step.numel() != B:
        raise HipLibraryError("decode_attn: bad qkv / step shape")
    if part_o.dtype != torch.float32 or part_o.numel() < B * n_q * nsplit * head_dim \
            or part_ml.numel() < B * n_q * nsplit * 2 or out.numel() != B * n_q * head_dim:
        raise HipLibraryError("decode_attn: workspace/output too small")
    qkv_bs = qkv.stride(0) if (batched and qkv.dim() == 2) else nq
    cache_bs = k_cache.stride(0) if batched else 0
    if batched and (v_cache.stride(0) != cache_bs or cos_t.stride(0) != sin_t.stride(0)):
        raise HipLibraryError("decode_attn: k/v caches (cos/sin tables) must share their batch stride")
    tab_bs = cos_t.stride(0) if batched else 0
    if fork is not None:
        if not batched:
            raise HipLibraryError("decode_attn: fork tables need batched caches [B, Hkv, T, D]")
        par, fl = _fork_tables("decode_attn", fork, B, k_cache.device, shared_len)
        rc = load().vis_decode_attn_forked(_ptr(qkv), _ptr(cos_t), _ptr(sin_t), _ptr(k_cache), _ptr(v_cache), _ptr(step),
                                           _ptr(part_o), _ptr(part_ml), _ptr(out), n_q, n_kv, head_dim, T, nsplit, scale,
                                           B, qkv_bs, cache_bs, tab_bs, _ptr(par), _ptr(fl), _stream())
        _check(rc, "vis_decode_attn_forked")
        return out
    if shared_len and batched:
        rc = load().vis_decode_attn_shared(_ptr(qkv), _ptr(cos_t), _ptr(sin_t), _ptr(k_cache), _ptr(v_cache), _ptr(step),
                                           _ptr(part_o), _ptr(part_ml), _ptr(out), n_q, n_kv, head_dim, T, nsplit, scale,
                                           B, qkv_bs, cache_bs, tab_bs, int(shared_len), _stream())
        _check(rc, "vis_decode_attn_shared")
        return out
    rc = load().vis_decode_attn(_ptr(qkv), _ptr(cos_t), _ptr(sin_t), _ptr(k_cache), _ptr(v_cache), _ptr(step),
                                _ptr(part_o), _ptr(part_ml), _ptr(out), n_q, n_kv, head_dim, T, nsplit, scale,
                                B, qkv_bs, cache_bs, tab_bs, _stream())
    _check(rc, "vis_decode_attn")
    return out


CHAIN_STATUS_WORD = 32     # int index of the status word inside a decode-chain sync block (csrc/decode_chain.hip: CH_STATUS)


def decode_chain_state(device, n_q: int, n_kv: int, nsplit: int):
    """(granule workspace, sync block) of vis_decode_chain, zeroed - one pair per engine / stream."""
    lib = load()
    nbytes = int(lib.vis_decode_chain_ws_bytes(n_q, n_kv, nsplit))
    return (torch.zeros(nbytes // 8, dtype=torch.int64, device=device),
            torch.zeros(lib.vis_decode_chain_sync_ints(), dtype=torch.int32, device=device))


def decode_chain_supported(n_q: int, n_kv: int, head_dim: int, hidden: int) -> bool:
    """Shapes the chained layer head covers (the launcher additionally checks that its grid is resident)."""
    return head_dim == 128 and n_q <= 64 and n_q % n_kv == 0 and (n_q // n_kv) in (1, 2, 4, 7, 8) \
        and hidden % 8 == 0 and hidden <= 4096 and n_q * head_dim <= 4096 and hidden // 2 <= (n_q + 2 * n_kv) * head_dim // 2


def decode_chain_ctx_limit(n_q: int, n_kv: int, hidden: int) -> int:
    """Largest context (cached keys incl. the new one) for which the chained layer head is resident on the current device
    (0: shape not covered).  Only the workgroups that wait count: projection and merge roles + the attention items of splits
    the context reaches - so the limit does not depend on the cache size."""
    return int(load().vis_decode_chain_ctx_limit(n_q, n_kv, hidden))


def decode_chain(x: torch.Tensor, qkv_w: torch.Tensor, qkv_b: Optional[torch.Tensor], norm_w: torch.Tensor,
                 o_w: torch.Tensor, y: torch.Tensor, cos_t: torch.Tensor, sin_t: torch.Tensor, k_cache: torch.Tensor,
                 v_cache: torch.Tensor, step: torch.Tensor, ws: torch.Tensor, sync: torch.Tensor, n_q: int, n_kv: int,
                 head_dim: int, nsplit: int, scale: float, eps: float, x_index: Optional[torch.Tensor] = None,
                 ctx_bound: int = 0) -> None:
    """qkv projection (+ RMSNorm, bias) -> rope / KV append / split attention + merge -> o projection (+ residual x) in ONE
    launch, bit-identical to gemv + decode_attn + gemv.  Single sequence: x [K], caches [Hkv, T, D], tables [T, D], step [1];
    ws / sync from decode_chain_state.  With ``x_index`` (device int32 [1]) ``x`` is an [rows, K] table and the layer input is
    its row x_index[0] (the new token's embedding: no separate gather launch).  ``ctx_bound``: the caller's promise that no
    launch with these arguments (a captured launch is replayed at growing positions) sees more cached keys than that; 0 =
    the whole cache.  The launcher refuses (ChainRefused) when the bound exceeds decode_chain_ctx_limit."""
    for t, n in ((x, "x"), (qkv_w, "qkv_w"), (norm_w, "norm_w"), (o_w, "o_w"), (y, "y"), (k_cache, "k_cache"),
                 (v_cache, "v_cache")):
        _bf16(t, "decode_chain " + n)
    if x_index is not None:
        if x.dim() != 2 or not x.is_contiguous() or x_index.dtype != torch.int32 or x_index.numel() != 1:
            raise HipLibraryError("decode_chain: x_index needs a contiguous [rows, K] table and one int32")
        K, x_rows = x.shape[1], x.shape[0]
    else:
        K, x_rows = x.numel(), 0
    nq = (n_q + 2 * n_kv) * head_dim
    if qkv_w.shape != (nq, K) or qkv_w.stride(1) != 1 or o_w.shape != (K, n_q * head_dim) or o_w.stride(1) != 1 \
            or norm_w.numel() != K or y.numel() != K or (qkv_b is not None and qkv_b.numel() != nq):
        raise HipLibraryError("decode_chain: bad projection shapes")
    if k_cache.dim() != 3 or k_cache.shape[0] != n_kv or k_cache.shape[2] != head_dim or v_cache.shape != k_cache.shape \
            or not k_cache.is_contiguous() or not v_cache.is_contiguous():
        raise HipLibraryError("decode_chain: bad cache shape")
    T = k_cache.shape[1]
    if cos_t.shape != (T, head_dim) or sin_t.shape != cos_t.shape or cos_t.dtype != torch.float32 or not cos_t.is_contiguous() \
            or not sin_t.is_contiguous() or step.dtype != torch.int32 or step.numel() != 1:
        raise HipLibraryError("decode_chain: bad tables / step")
    lib = load()
    if ws.dtype != torch.int64 or ws.numel() * 8 < lib.vis_decode_chain_ws_bytes(n_q, n_kv, nsplit) \
            or sync.dtype != torch.int32 or sync.numel() < lib.vis_decode_chain_sync_ints():
        raise HipLibraryError("decode_chain: workspace too small")
    rc = lib.vis_decode_chain(_ptr(x), _ptr(x_index), x_rows, _ptr(qkv_w), _ptr(qkv_b), _ptr(norm_w), _ptr(o_w), _ptr(y), _ptr(cos_t), _ptr(sin_t),
                              _ptr(k_cache), _ptr(v_cache), _ptr(step), _ptr(ws), _ptr(sync), n_q, n_kv, head_dim, K,
                              qkv_w.stride(0), o_w.stride(0), T, nsplit, ctx_bound, scale, eps, _stream())
    if rc == 3:
        raise ChainRefused(f"vis_decode_chain: {n_q}/{n_kv} heads, hidden {K}, {nsplit} context splits are outside the chained "
                           "form on this device (shape, or grid larger than the device holds resident); nothing was launched")
    _check(rc, "vis_decode_chain")


def decode_chain_rows(ws: torch.Tensor, n_q: int, n_kv: int):
    """(packed projection row [(n_q + 2 n_kv) * 128], merged attention row [n_q * 128]) bf16 of the last chained launch, read
    back from the granule workspace (tests / taps)."""
    nq = (n_q + 2 * n_kv) * 64
    g = ws[:nq + n_q * 64] & 0xFFFFFFFF
    rows = g.to(torch.int32).view(torch.bfloat16)
    return rows[:2 * nq], rows[2 * nq:]


def gemv_argmax(x: torch.Tensor, w: torch.Tensor, logits: torch.Tensor, ws_val: torch.Tensor, ws_idx: torch.Tensor,
                tokens: torch.Tensor, cur_token: torch.Tensor, step: torch.Tensor, norm_w: Optional[torch.Tensor] = None,
                eps: float = 1e-6, temperature: float = 0.0, seed: int = 0) -> None:
    """lm_head GEMV (f32 logits, optional fused RMSNorm) + next-token pick in two launches: gemv(out f32) + argmax with the
    pick's first stage in the GEMV epilogue.  Single sequence."""
    _bf16(x, "gemv_argmax x"); _bf16(w, "gemv_argmax w")
    N, K = w.shape
    if x.numel() != K or w.stride(1) != 1 or logits.dtype != torch.float32 or logits.numel() != N:
        raise HipLibraryError("gemv_argmax: bad shapes")
    if ws_val.dtype != torch.float32 or ws_idx.dtype != torch.int32 or ws_val.numel() < 2048 or ws_idx.numel() < 2048 \
            or tokens.dtype != torch.int32 or cur_token.numel() != 1 or step.numel() != 1 or not tokens.is_contiguous():
        raise HipLibraryError("gemv_argmax: workspace too small / bad state shapes")
    rc = load().vis_gemv_bf16_argmax(_ptr(x), _ptr(w), _ptr(norm_w), _ptr(logits), N, K, w.stride(0), eps, _ptr(ws_val),
                                     _ptr(ws_idx), _ptr(tokens), tokens.numel(), _ptr(cur_token), _ptr(step),
                                     (1.0 / temperature) if temperature > 0 else 0.0, seed & 0xFFFFFFFF, _stream())
    _check(rc, "vis_gemv_bf16_argmax")


def argmax(logits: torch.Tensor, ws_val: torch.Tensor, ws_idx: torch.Tensor, tokens: torch.Tensor,
           cur_token: torch.Tensor, step: torch.Tensor, temperature: float = 0.0, seed: int = 0) -> None:
    """Greedy (temperature 0) or Gumbel-max sampled next token; advances the device-side step.
    logits [V] (tokens [T], cur/step [1]) or logits [B,V] (tokens [B,T], cur/step [B])."""
    if logits.dtype != torch.float32 or tokens.dtype != torch.int32 or cur_token.dtype != torch.int32:
        raise HipLibraryError("argmax: f32 logits / int32 tokens required")
    B = logits.shape[0] if logits.dim() == 2 else 1
    V = logits.shape[-1]
    if ws_val.numel() < 256 * B or ws_idx.numel() < 256 * B or cur_token.numel() != B or step.numel() != B:
        raise HipLibraryError("argmax: workspace too small / bad state shapes")
    if logits.stride(-1) != 1 or not tokens.is_contiguous() or tokens.numel() % B:
        raise HipLibraryError("argmax: bad strides")
    rc = load().vis_argmax_f32(_ptr(logits), V, _ptr(ws_val), _ptr(ws_idx), _ptr(tokens), tokens.numel() // B,
                               _ptr(cur_token), _ptr(step), (1.0 / temperature) if temperature > 0 else 0.0,
                               seed & 0xFFFFFFFF, B, logits.stride(0) if logits.dim() == 2 else V, _stream())
    _check(rc, "vis_argmax_f32")


LOGPROBS_MAX_K = 20     # top_ids / lp row widths of vis_logprobs_f32 (OpenAI's top_logprobs limit)


def logprobs_ws(V: int, batch: int, device) -> torch.Tensor:
    """Workspace of vis_logprobs_f32 for up to ``batch`` rows of V logits, [batch, n] f32 (row b's slice serves one row)."""
    n = int(load().vis_logprobs_ws_bytes(V, batch))
    if n <= 0:
        raise HipLibraryError(f"logprobs_ws: unsupported V={V} batch={batch}")
    return torch.empty((batch, n // 4 // batch), dtype=torch.float32, device=device)


def logprobs(logits: torch.Tensor, tokens: torch.Tensor, step: torch.Tensor, top_k: int, lp: torch.Tensor,
             top_ids: torch.Tensor, ws: torch.Tensor) -> None:
    """Log-probabilities of the token the pick just stored at tokens[b][step[b] - 1] and of the top_k largest logits.
    logits [V] (tokens [T], step [1], lp [T, 21], top_ids [T, 20]) or [B, V] (tokens [B, T], step [B], lp [B, T, 21],
    top_ids [B, T, 20]); ws from logprobs_ws (rows >= B).  Raw logits: the values do not depend on the temperature."""
    if logits.dtype != torch.float32 or tokens.dtype != torch.int32 or step.dtype != torch.int32:
        raise HipLibraryError("logprobs: f32 logits / int32 tokens and step required")
    if lp.dtype != torch.float32 or top_ids.dtype != torch.int32 or ws.dtype != torch.float32:
        raise HipLibraryError("logprobs: f32 lp / ws and int32 top_ids required")
    B = logits.shape[0] if logits.dim() == 2 else 1
    V = logits.shape[-1]
    if step.numel() != B or tokens.numel() % B or not 0 <= top_k <= LOGPROBS_MAX_K:
        raise HipLibraryError("logprobs: bad state shapes / top_k")
    T = tokens.numel() // B
    if lp.numel() != B * T * (LOGPROBS_MAX_K + 1) or top_ids.numel() != B * T * LOGPROBS_MAX_K:
        raise HipLibraryError("logprobs: lp / top_ids must be [B, T, 21] / [B, T, 20]")
    if logits.stride(-1) != 1 or not (tokens.is_contiguous() and step.is_contiguous() and lp.is_contiguous()
                                      and top_ids.is_contiguous() and ws.is_contiguous()):
        raise HipLibraryError("logprobs: bad strides")
    rc = load().vis_logprobs_f32(_ptr(logits), V, logits.stride(0) if logits.dim() == 2 else V, _ptr(tokens), T, _ptr(step),
                                 top_k, _ptr(lp), _ptr(top_ids), _ptr(ws), ws.numel() * 4, B, _stream())
    _check(rc, "vis_logprobs_f32")


JSON_STATE_INTS = 32    # int32 words of one sequence's vis_json_mask state (json_grammar.STATE_INTS)


def json_mask(state: torch.Tensor, tokens: torch.Tensor, step: torch.Tensor, tok_off: torch.Tensor, tok_bytes: torch.Tensor,
              tok_flags: torch.Tensor, eos_ids: torch.Tensor, allow: torch.Tensor) -> None:
    """Fold the tokens picked since the last call into the grammar state and write the allowed-token bitmask of the next pick.
    state [B, 32] int32 (zeroed = fresh), tokens [B, T] int32, step [B] int32, allow [B, ceil(V / 64)] int64; the token table
    (json_grammar.TokenTable) as device tensors: tok_off [V + 1] int32, tok_bytes uint8, tok_flags [V] uint8, eos_ids int32."""
    if state.dim() != 2 or tokens.dim() != 2 or allow.dim() != 2:
        raise HipLibraryError("json_mask: state / tokens / allow must be 2-D")
    B = state.shape[0]
    V = tok_flags.numel()
    if state.dtype != torch.int32 or state.shape[1] != JSON_STATE_INTS or tokens.dtype != torch.int32 or step.dtype != torch.int32:
        raise HipLibraryError("json_mask: int32 state [B, 32] / tokens / step required")
    if tokens.shape[0] != B or step.numel() != B or allow.shape[0] != B or allow.dtype != torch.int64:
        raise HipLibraryError("json_mask: bad batch shapes / int64 allow required")
    if tok_off.dtype != torch.int32 or tok_off.numel() != V + 1 or tok_bytes.dtype != torch.uint8 \
            or tok_flags.dtype != torch.uint8 or eos_ids.dtype != torch.int32:
        raise HipLibraryError("json_mask: bad token table")
    if allow.shape[1] < (V + 63) // 64 or allow.stride(1) != 1 or tokens.stride(1) != 1 or not (
            state.is_contiguous() and step.is_contiguous() and tok_off.is_contiguous() and tok_bytes.is_contiguous()
            and tok_flags.is_contiguous() and eos_ids.is_contiguous()):
        raise HipLibraryError("json_mask: bad strides")
    if B > 1 and (tokens.stride(0) != tokens.shape[1] or state.stride(0) != JSON_STATE_INTS):
        raise HipLibraryError("json_mask: rows must be contiguous")
    rc = load().vis_json_mask(_ptr(state), _ptr(tokens), tokens.shape[1], _ptr(step), _ptr(tok_off), _ptr(tok_bytes),
                              _ptr(tok_flags), _ptr(eos_ids), eos_ids.numel(), V, _ptr(allow), allow.stride(0), B, _stream())
    _check(rc, "vis_json_mask")


def schema_mask(state: torch.Tensor, tokens: torch.Tensor, step: torch.Tensor, tok_off: torch.Tensor, tok_bytes: torch.Tensor,
                tok_flags: torch.Tensor, eos_ids: torch.Tensor, allow: torch.Tensor, header: torch.Tensor, trans: torch.Tensor,
                byte_class: torch.Tensor, state_flags: torch.Tensor) -> None:
    """json_mask with a compiled schema (json_schema.SchemaDFA) in place of the JSON grammar: fold the tokens picked since
    the last call into the DFA state, write the allowed-token bitmask of the next pick.  state / tokens / step / allow and the
    token table as in json_mask.  The DFA in fixed-capacity device tensors the kernel sizes from ``header`` (int32 [4]:
    n_states, n_classes, start, 0): trans [cap_states, cap_classes] int16 (the u16 bits) holding the live [n_states, n_classes] table
    packed at its front, byte_class [256] uint8, state_flags [cap_states] uint8."""
    if state.dim() != 2 or tokens.dim() != 2 or allow.dim() != 2:
        raise HipLibraryError("schema_mask: state / tokens / allow must be 2-D")
    B = state.shape[0]
    V = tok_flags.numel()
    if state.dtype != torch.int32 or state.shape[1] != JSON_STATE_INTS or tokens.dtype != torch.int32 or step.dtype != torch.int32:
        raise HipLibraryError("schema_mask: int32 state [B, 32] / tokens / step required")
    if tokens.shape[0] != B or step.numel() != B or allow.shape[0] != B or allow.dtype != torch.int64:
        raise HipLibraryError("schema_mask: bad batch shapes / int64 allow required")
    if tok_off.dtype != torch.int32 or tok_off.numel() != V + 1 or tok_bytes.dtype != torch.uint8 \
            or tok_flags.dtype != torch.uint8 or eos_ids.dtype != torch.int32:
        raise HipLibraryError("schema_mask: bad token table")
    if header.dtype != torch.int32 or header.numel() != 4 or trans.dtype != torch.int16 or trans.dim() != 2 \
            or byte_class.dtype != torch.uint8 or byte_class.numel() != 256 or state_flags.dtype != torch.uint8 \
            or state_flags.numel() != trans.shape[0]:
        raise HipLibraryError("schema_mask: bad DFA tables")
    if allow.shape[1] < (V + 63) // 64 or allow.stride(1) != 1 or tokens.stride(1) != 1 or not (
            state.is_contiguous() and step.is_contiguous() and tok_off.is_contiguous() and tok_bytes.is_contiguous()
            and tok_flags.is_contiguous() and eos_ids.is_contiguous() and header.is_contiguous() and trans.is_contiguous()
            and byte_class.is_contiguous() and state_flags.is_contiguous()):
        raise HipLibraryError("schema_mask: bad strides")
    if B > 1 and (tokens.stride(0) != tokens.shape[1] or state.stride(0) != JSON_STATE_INTS):
        raise HipLibraryError("schema_mask: rows must be contiguous")
    rc = load().vis_schema_mask(_ptr(state), _ptr(tokens), tokens.shape[1], _ptr(step), _ptr(tok_off), _ptr(tok_bytes),
                                _ptr(tok_flags), _ptr(eos_ids), eos_ids.numel(), V, _ptr(allow), allow.stride(0), _ptr(header),
                                _ptr(trans), _ptr(byte_class), _ptr(state_flags), trans.shape[0], trans.shape[1], B, _stream())
    _check(rc, "vis_schema_mask")


def argmax_masked(logits: torch.Tensor, ws_val: torch.Tensor, ws_idx: torch.Tensor, tokens: torch.Tensor,
                  cur_token: torch.Tensor, step: torch.Tensor, allow: torch.Tensor, temperature: float = 0.0,
                  seed: int = 0) -> None:
    """argmax over the ids allowed by ``allow`` (int64 [ceil(V / 64)] or [B, ceil(V / 64)], json_mask's rows); the same
    comparison and noise as argmax, so an all-ones mask gives its pick bit for bit."""
    if logits.dtype != torch.float32 or tokens.dtype != torch.int32 or cur_token.dtype != torch.int32:
        raise HipLibraryError("argmax_masked: f32 logits / int32 tokens required")
    B = logits.shape[0] if logits.dim() == 2 else 1
    V = logits.shape[-1]
    if ws_val.numel() < 256 * B or ws_idx.numel() < 256 * B or cur_token.numel() != B or step.numel() != B:
        raise HipLibraryError("argmax_masked: workspace too small / bad state shapes")
    if logits.stride(-1) != 1 or not tokens.is_contiguous() or tokens.numel() % B:
        raise HipLibraryError("argmax_masked: bad strides")
    a2 = allow if allow.dim() == 2 else allow.view(1, -1)
    if allow.dtype != torch.int64 or a2.shape[0] != B or a2.shape[1] < (V + 63) // 64 or a2.stride(-1) != 1:
        raise HipLibraryError("argmax_masked: allow must be int64 [B, ceil(V / 64)]")
    rc = load().vis_argmax_masked_f32(_ptr(logits), V, _ptr(ws_val), _ptr(ws_idx), _ptr(tokens), tokens.numel() // B,
                                      _ptr(cur_token), _ptr(step), (1.0 / temperature) if temperature > 0 else 0.0,
                                      seed & 0xFFFFFFFF, B, logits.stride(0) if logits.dim() == 2 else V, _ptr(a2),
                                      a2.stride(0) if B > 1 else a2.shape[1], _stream())
    _check(rc, "vis_argmax_masked_f32")


def gemv_argmax_masked(x: torch.Tensor, w: torch.Tensor, logits: torch.Tensor, ws_val: torch.Tensor, ws_idx: torch.Tensor,
                       tokens: torch.Tensor, cur_token: torch.Tensor, step: torch.Tensor, allow: torch.Tensor,
                       norm_w: Optional[torch.Tensor] = None, eps: float = 1e-6, temperature: float = 0.0,
                       seed: int = 0) -> None:
    """gemv_argmax with the pick restricted to the ids allowed by ``allow`` (int64 [ceil(N / 64)]).  Single sequence."""
    _bf16(x, "gemv_argmax_masked x"); _bf16(w, "gemv_argmax_masked w")
    N, K = w.shape
    if x.numel() != K or w.stride(1) != 1 or logits.dtype != torch.float32 or logits.numel() != N:
        raise HipLibraryError("gemv_argmax_masked: bad shapes")
    if ws_val.dtype != torch.float32 or ws_idx.dtype != torch.int32 or ws_val.numel() < 2048 or ws_idx.numel() < 2048 \
            or tokens.dtype != torch.int32 or cur_token.numel() != 1 or step.numel() != 1 or not tokens.is_contiguous():
        raise HipLibraryError("gemv_argmax_masked: workspace too small / bad state shapes")
    if allow.dtype != torch.int64 or allow.numel() < (N + 63) // 64 or not allow.is_contiguous():
        raise HipLibraryError("gemv_argmax_masked: allow must be int64 [ceil(N / 64)]")
    rc = load().vis_gemv_bf16_argmax_masked(_ptr(x), _ptr(w), _ptr(norm_w), _ptr(logits), N, K, w.stride(0), eps, _ptr(ws_val),
                                            _ptr(ws_idx), _ptr(tokens), tokens.numel(), _ptr(cur_token), _ptr(step),
                                            (1.0 / temperature) if temperature > 0 else 0.0, seed & 0xFFFFFFFF, _ptr(allow),
                                            _stream())
    _check(rc, "vis_gemv_bf16_argmax_masked")


def sample_ws(V: int, batch: int, device) -> torch.Tensor:
    """Workspace of vis_sample_f32 for up to ``batch`` rows of V logits, [batch, n] uint8 (row b's slice serves one row)."""
    n = int(load().vis_sample_ws_bytes(V, batch))
    if n <= 0:
        raise HipLibraryError(f"sample_ws: unsupported V={V} batch={batch}")
    return torch.empty((batch, n // batch), dtype=torch.uint8, device=device)


def sample(logits: torch.Tensor, tokens: torch.Tensor, cur_token: torch.Tensor, step: torch.Tensor, seeds: torch.Tensor,
           ws: torch.Tensor, temperature: float = 0.0, top_p: float = 1.0, allow: Optional[torch.Tensor] = None,
           nkeep: Optional[torch.Tensor] = None) -> None:
    """Nucleus pick (vis_sample_f32): the Gumbel-max over the shortest (logit desc, id asc) prefix holding top_p of the
    temperature-scaled mass, with row b's seed read from seeds[b] (int32 / uint32 bits) at launch time, so a captured
    launch serves any seeds.  logits [V] or [B, V]; tokens [T] / [B, T]; cur_token, step, seeds [B]; ws from sample_ws
    (rows >= B); allow: vis_json_mask's int64 rows [B, ceil(V / 64)] or None; nkeep: int32 [B] receives |K| or None.
    top_p = 1 picks what argmax(..., seed) does for the same row seed."""
    if logits.dtype != torch.float32 or tokens.dtype != torch.int32 or cur_token.dtype != torch.int32 \
            or step.dtype != torch.int32 or seeds.dtype not in (torch.int32, torch.uint32) or ws.dtype != torch.uint8:
        raise HipLibraryError("sample: f32 logits / int32 tokens, step, seeds / uint8 workspace required")
    B = logits.shape[0] if logits.dim() == 2 else 1
    V = logits.shape[-1]
    if cur_token.numel() != B or step.numel() != B or seeds.numel() < B or not seeds.is_contiguous():
        raise HipLibraryError("sample: bad state shapes")
    if logits.stride(-1) != 1 or not tokens.is_contiguous() or tokens.numel() % B or not ws.is_contiguous() \
            or ws.numel() < int(load().vis_sample_ws_bytes(V, B)):
        raise HipLibraryError("sample: bad strides / workspace too small")
    if nkeep is not None and (nkeep.dtype != torch.int32 or nkeep.numel() < B or not nkeep.is_contiguous()):
        raise HipLibraryError("sample: nkeep must be int32 [B]")
    a2 = None
    if allow is not None:
        a2 = allow if allow.dim() == 2 else allow.view(1, -1)
        if allow.dtype != torch.int64 or a2.shape[0] != B or a2.shape[1] < (V + 63) // 64 or a2.stride(-1) != 1:
            raise HipLibraryError("sample: allow must be int64 [B, ceil(V / 64)]")
    rc = load().vis_sample_f32(_ptr(logits), V, logits.stride(0) if logits.dim() == 2 else V, _ptr(a2),
                               (a2.stride(0) if B > 1 else a2.shape[1]) if a2 is not None else 0,
                               (1.0 / temperature) if temperature > 0 else 0.0, float(top_p), _ptr(seeds), _ptr(tokens),
                               tokens.numel() // B, _ptr(cur_token), _ptr(step), B, _ptr(ws), _ptr(nkeep), _stream())
    _check(rc, "vis_sample_f32")


def penalty_state(V: int, batch: int, device) -> torch.Tensor:
    """Zeroed token statistics of vis_penalize_f32 for ``batch`` rows of V ids, [batch, n] uint8 (a zeroed row = a fresh
    sequence; row b's slice serves one row)."""
    n = int(load().vis_penalty_state_bytes(V, batch))
    if n <= 0:
        raise HipLibraryError(f"penalty_state: unsupported V={V} batch={batch}")
    return torch.zeros((batch, n // batch), dtype=torch.uint8, device=device)


def penalty_prompt(state_row: torch.Tensor, V: int, ids: torch.Tensor) -> None:
    """Mark the prompt ids (int32, device) of ONE row of penalty_state; ids outside [0, V) are skipped."""
    if state_row.dtype != torch.uint8 or not state_row.is_contiguous() or ids.dtype != torch.int32 or not ids.is_contiguous() \
            or state_row.numel() != int(load().vis_penalty_state_bytes(V, 1)):
        raise HipLibraryError("penalty_prompt: one uint8 row of penalty_state / contiguous int32 ids required")
    rc = load().vis_penalty_prompt(_ptr(state_row), V, _ptr(ids), ids.numel(), _stream())
    _check(rc, "vis_penalty_prompt")


def penalize(logits: torch.Tensor, state: torch.Tensor, params: torch.Tensor, tokens: torch.Tensor, step: torch.Tensor,
             out: torch.Tensor) -> None:
    """Penalised copy of the raw logits (vis_penalize_f32): folds the tokens picked since the last call into the rows' counts,
    then out = repetition / frequency / presence penalties applied to logits, which stay intact.  logits, out [V] or [B, V]
    f32; state: B rows of penalty_state; params [B, 3] f32 = (r, f, q) in device memory; tokens [T] / [B, T], step [B]."""
    if logits.dtype != torch.float32 or out.dtype != torch.float32 or params.dtype != torch.float32 \
            or tokens.dtype != torch.int32 or step.dtype != torch.int32 or state.dtype != torch.uint8:
        raise HipLibraryError("penalize: f32 logits, out, params / int32 tokens, step / uint8 state required")
    B = logits.shape[0] if logits.dim() == 2 else 1
    V = logits.shape[-1]
    if out.shape != logits.shape or step.numel() != B or params.numel() != 3 * B or tokens.numel() % B:
        raise HipLibraryError("penalize: bad state shapes")
    if logits.stride(-1) != 1 or out.stride(-1) != 1 or not (tokens.is_contiguous() and step.is_contiguous()
                                                             and params.is_contiguous() and state.is_contiguous()) \
            or state.numel() != int(load().vis_penalty_state_bytes(V, B)):
        raise HipLibraryError("penalize: bad strides / state is not B rows of penalty_state")
    rc = load().vis_penalize_f32(_ptr(logits), V, logits.stride(0) if logits.dim() == 2 else V, _ptr(state), _ptr(params),
                                 _ptr(tokens), tokens.numel() // B, _ptr(step), _ptr(out),
                                 out.stride(0) if out.dim() == 2 else V, B, _stream())
    _check(rc, "vis_penalize_f32")


SHAPE_MAX_BIAS = 300    # entries of one row's bias list (shaping.MAX_BIAS; OpenAI's limit for logit_bias)


def shape_ws(V: int, batch: int, device) -> torch.Tensor:
    """Workspace of vis_shape_f32 for up to ``batch`` rows of V logits, [batch, n] uint8 (row b's slice serves one row and
    receives its record {f32 t, f32 m, int32 |A|, int32 path})."""
    n = int(load().vis_shape_ws_bytes(V, batch))
    if n <= 0:
        raise HipLibraryError(f"shape_ws: unsupported V={V} batch={batch}")
    return torch.zeros((batch, n // batch), dtype=torch.uint8, device=device)


def shape_logits(logits: torch.Tensor, k: torch.Tensor, delta: torch.Tensor, nbias: torch.Tensor, bias_ids: torch.Tensor,
                 bias_vals: torch.Tensor, out: torch.Tensor, nkept: torch.Tensor, ws: torch.Tensor,
                 allow: Optional[torch.Tensor] = None) -> None:
    """Shaped copy of the logits (vis_shape_f32): out = logits + the rows' bias lists, then -inf for every id outside the
    allow rows, below the rows' k-th largest value, or more than -delta below the row maximum; logits stay intact.  logits,
    out [V] or [B, V] f32; k, nbias, nkept int32 [B]; delta f32 [B]; bias_ids int32 / bias_vals f32 [B, 300], all in device
    memory and read at run time; ws from shape_ws (rows >= B); allow: vis_json_mask's int64 rows [B, ceil(V / 64)] or None."""
    if logits.dtype != torch.float32 or out.dtype != torch.float32 or delta.dtype != torch.float32 \
            or bias_vals.dtype != torch.float32 or k.dtype != torch.int32 or nbias.dtype != torch.int32 \
            or bias_ids.dtype != torch.int32 or nkept.dtype != torch.int32 or ws.dtype != torch.uint8:
        raise HipLibraryError("shape_logits: f32 logits, out, delta, bias_vals / int32 k, nbias, bias_ids, nkept / uint8 "
                              "workspace required")
    B = logits.shape[0] if logits.dim() == 2 else 1
    V = logits.shape[-1]
    if out.shape != logits.shape or k.numel() != B or delta.numel() != B or nbias.numel() != B or nkept.numel() != B \
            or bias_ids.numel() != B * SHAPE_MAX_BIAS or bias_vals.numel() != B * SHAPE_MAX_BIAS:
        raise HipLibraryError("shape_logits: bad parameter shapes")
    if logits.stride(-1) != 1 or out.stride(-1) != 1 or not (k.is_contiguous() and delta.is_contiguous() and nbias.is_contiguous()
                                                             and bias_ids.is_contiguous() and bias_vals.is_contiguous()
                                                             and nkept.is_contiguous() and ws.is_contiguous()) \
            or ws.numel() < int(load().vis_shape_ws_bytes(V, B)):
        raise HipLibraryError("shape_logits: bad strides / workspace too small")
    a2 = None
    if allow is not None:
        a2 = allow if allow.dim() == 2 else allow.view(1, -1)
        if allow.dtype != torch.int64 or a2.shape[0] != B or a2.shape[1] < (V + 63) // 64 or a2.stride(-1) != 1:
            raise HipLibraryError("shape_logits: allow must be int64 [B, ceil(V / 64)]")
    rc = load().vis_shape_f32(_ptr(logits), V, logits.stride(0) if logits.dim() == 2 else V, _ptr(a2),
                              (a2.stride(0) if B > 1 else a2.shape[1]) if a2 is not None else 0, _ptr(k), _ptr(delta),
                              _ptr(nbias), _ptr(bias_ids), _ptr(bias_vals), _ptr(out),
                              out.stride(0) if out.dim() == 2 else V, _ptr(nkept), _ptr(ws), B, _stream())
    _check(rc, "vis_shape_f32")


BAN_MAX_WORDS, BAN_MAX_WORD_LEN, BAN_MAX_EOS = 16, 8, 8     # the tables of vis_ban_f32 (ban.py)


def ban(logits: torch.Tensor, prompt_ids: torch.Tensor, prompt_len: torch.Tensor, tokens: torch.Tensor, gen_start: torch.Tensor,
        step: torch.Tensor, ngram: torch.Tensor, min_tokens: torch.Tensor, words: torch.Tensor, word_len: Sequence[int],
        eos_ids: torch.Tensor, n_eos: int, out: torch.Tensor) -> None:
    """Copy of the logits with the banned ids at -inf (vis_ban_f32): no_repeat_ngram_size, bad_words and min_tokens over the
    rows' history = prompt_ids[b][:prompt_len[b]] followed by tokens[b][gen_start[b]:step[b]]; logits stay intact.  logits,
    out [V] or [B, V] f32; prompt_ids int32 [B, P]; tokens int32 [T] / [B, T]; prompt_len, gen_start, step, ngram, min_tokens
    int32 [B]; words int32 [16, 8] (row w = word w, its length word_len[w], a host sequence); eos_ids int32 [8], the first
    n_eos in use - all tensors in device memory, read at run time."""
    ints = (prompt_ids, prompt_len, tokens, gen_start, step, ngram, min_tokens, words, eos_ids)
    if logits.dtype != torch.float32 or out.dtype != torch.float32 or any(t.dtype != torch.int32 for t in ints):
        raise HipLibraryError("ban: f32 logits, out / int32 ids, tokens and per-row parameters required")
    B = logits.shape[0] if logits.dim() == 2 else 1
    V = logits.shape[-1]
    if out.shape != logits.shape or any(t.numel() != B for t in (prompt_len, gen_start, step, ngram, min_tokens)) \
            or tokens.numel() % B or prompt_ids.numel() % B or prompt_ids.numel() == 0 \
            or words.numel() != BAN_MAX_WORDS * BAN_MAX_WORD_LEN or eos_ids.numel() != BAN_MAX_EOS:
        raise HipLibraryError("ban: bad parameter shapes")
    if logits.stride(-1) != 1 or out.stride(-1) != 1 or not all(t.is_contiguous() for t in ints):
        raise HipLibraryError("ban: bad strides")
    lens = [int(m) for m in word_len]
    arr = (ctypes.c_int * max(1, len(lens)))(*lens)
    rc = load().vis_ban_f32(_ptr(logits), V, logits.stride(0) if logits.dim() == 2 else V, _ptr(prompt_ids),
                            prompt_ids.numel() // B, _ptr(prompt_len), _ptr(tokens), tokens.numel() // B, _ptr(gen_start),
                            _ptr(step), _ptr(ngram), _ptr(min_tokens), _ptr(words), arr, len(lens), _ptr(eos_ids), int(n_eos),
                            _ptr(out), out.stride(0) if out.dim() == 2 else V, B, _stream())
    _check(rc, "vis_ban_f32")


SPEC_MAX_ROWS, SPEC_MAX_LOOKUP = 4, 8     # SP_MAXROWS / SP_MAXLOOKUP of csrc/spec.hip (spec.py)


def decode_attn_draft(qkv: torch.Tensor, cos_t: torch.Tensor, sin_t: torch.Tensor, k_cache: torch.Tensor,
                      v_cache: torch.Tensor, step: torch.Tensor, part_o: torch.Tensor, part_ml: torch.Tensor,
                      out: torch.Tensor, n_q: int, n_kv: int, head_dim: int, nsplit: int, scale: float) -> torch.Tensor:
    """decode_attn for the R = 1..4 rows of ONE sequence's speculative step (vis_decode_attn_draft): row r of qkv [R, nq*D]
    sits at position step[0] + r - its rope row, its cache row, keys [0, step[0] + r].  Caches [Hkv, T, D], tables [T, D],
    step int32 [1] (left as it is), workspaces for R rows, out [R, Hq*D].  Row r and the cache are bit-identical to R
    successive decode_attn calls at advancing steps; a row at a position >= T reads and writes nothing."""
    _bf16(qkv, "qkv"); _bf16(k_cache, "k_cache"); _bf16(v_cache, "v_cache"); _bf16(out, "out")
    if step.dtype != torch.int32 or step.numel() != 1 or cos_t.dtype != torch.float32 or sin_t.dtype != torch.float32:
        raise HipLibraryError("decode_attn_draft: step int32 [1] / cos,sin f32 required")
    if k_cache.dim() != 3 or k_cache.shape[0] != n_kv or k_cache.shape[2] != head_dim or v_cache.shape != k_cache.shape \
            or not k_cache.is_contiguous() or not v_cache.is_contiguous():
        raise HipLibraryError("decode_attn_draft: caches must be contiguous [Hkv, cache_tokens, head_dim]")
    T = k_cache.shape[1]
    if cos_t.shape != (T, head_dim) or sin_t.shape != cos_t.shape or not cos_t.is_contiguous() or not sin_t.is_contiguous():
        raise HipLibraryError("decode_attn_draft: cos/sin tables must be [cache_tokens, head_dim]")
    nq = (n_q + 2 * n_kv) * head_dim
    if qkv.dim() != 2 or not 1 <= qkv.shape[0] <= SPEC_MAX_ROWS or qkv.shape[1] != nq or qkv.stride(1) != 1:
        raise HipLibraryError("decode_attn_draft: qkv must be [1..4, (Hq + 2 Hkv) * D]")
    R = qkv.shape[0]
    if part_o.dtype != torch.float32 or part_ml.dtype != torch.float32 or part_o.numel() < R * n_q * nsplit * head_dim \
            or part_ml.numel() < R * n_q * nsplit * 2 or out.shape != (R, n_q * head_dim) or not out.is_contiguous():
        raise HipLibraryError("decode_attn_draft: workspace/output too small")
    rc = load().vis_decode_attn_draft(_ptr(qkv), _ptr(cos_t), _ptr(sin_t), _ptr(k_cache), _ptr(v_cache), _ptr(step),
                                      _ptr(part_o), _ptr(part_ml), _ptr(out), n_q, n_kv, head_dim, T, nsplit, scale, R,
                                      qkv.stride(0), _stream())
    _check(rc, "vis_decode_attn_draft")
    return out


def spec_accept(logits: torch.Tensor, draft: torch.Tensor, n_draft: torch.Tensor, limit: torch.Tensor, ws_val: torch.Tensor,
                ws_idx: torch.Tensor, tokens: torch.Tensor, cur_token: torch.Tensor, step: torch.Tensor,
                counters: torch.Tensor) -> None:
    """The accept step of a speculative step (vis_spec_accept): logits f32 [R, V] (R = 1..4), draft int32 [>= R - 1], n_draft
    / limit / cur_token / step int32 [1], tokens int32 [T], counters int32 [3] (steps, proposed, accepted), ws_val f32 /
    ws_idx int32 of >= 256 * R entries - all device memory.  spec.accept_ref() is the numpy restatement."""
    ints = (draft, n_draft, limit, ws_idx, tokens, cur_token, step, counters)
    if logits.dtype != torch.float32 or ws_val.dtype != torch.float32 or any(t.dtype != torch.int32 for t in ints):
        raise HipLibraryError("spec_accept: f32 logits, ws_val / int32 everything else required")
    if logits.dim() != 2 or not 1 <= logits.shape[0] <= SPEC_MAX_ROWS or logits.stride(1) != 1:
        raise HipLibraryError("spec_accept: logits must be [1..4, V] with unit column stride")
    R, V = logits.shape
    if draft.numel() < max(1, R - 1) or any(t.numel() != 1 for t in (n_draft, limit, cur_token, step)) or counters.numel() != 3 \
            or ws_val.numel() < 256 * R or ws_idx.numel() < 256 * R or not all(t.is_contiguous() for t in ints):
        raise HipLibraryError("spec_accept: bad parameter shapes")
    rc = load().vis_spec_accept(_ptr(logits), V, logits.stride(0), R, _ptr(draft), _ptr(n_draft), _ptr(limit), _ptr(ws_val),
                                _ptr(ws_idx), _ptr(tokens), tokens.numel(), _ptr(cur_token), _ptr(step), _ptr(counters),
                                _stream())
    _check(rc, "vis_spec_accept")


def spec_accept_sampled(logits: torch.Tensor, draft: torch.Tensor, n_draft: torch.Tensor, limit: torch.Tensor,
                        ws_val: torch.Tensor, ws_idx: torch.Tensor, tokens: torch.Tensor, cur_token: torch.Tensor,
                        step: torch.Tensor, counters: torch.Tensor, params: torch.Tensor) -> None:
    """spec_accept with the sampled pick (vis_spec_accept_sampled): row r's pick is argmax's token for that row at step[0] + r.
    params int32 [2] in device memory: the bits of the f32 inv_temp (1 / temperature; 0 = greedy) and the uint32 seed,
    read when the launch runs.  Everything else as spec_accept."""
    ints = (draft, n_draft, limit, ws_idx, tokens, cur_token, step, counters, params)
    if logits.dtype != torch.float32 or ws_val.dtype != torch.float32 or any(t.dtype != torch.int32 for t in ints):
        raise HipLibraryError("spec_accept_sampled: f32 logits, ws_val / int32 everything else required")
    if logits.dim() != 2 or not 1 <= logits.shape[0] <= SPEC_MAX_ROWS or logits.stride(1) != 1:
        raise HipLibraryError("spec_accept_sampled: logits must be [1..4, V] with unit column stride")
    R, V = logits.shape
    if draft.numel() < max(1, R - 1) or any(t.numel() != 1 for t in (n_draft, limit, cur_token, step)) or counters.numel() != 3 \
            or params.numel() != 2 or ws_val.numel() < 256 * R or ws_idx.numel() < 256 * R \
            or not all(t.is_contiguous() for t in ints):
        raise HipLibraryError("spec_accept_sampled: bad parameter shapes")
    rc = load().vis_spec_accept_sampled(_ptr(logits), V, logits.stride(0), R, _ptr(draft), _ptr(n_draft), _ptr(limit),
                                        _ptr(ws_val), _ptr(ws_idx), _ptr(tokens), tokens.numel(), _ptr(cur_token), _ptr(step),
                                        _ptr(counters), _ptr(params), _stream())
    _check(rc, "vis_spec_accept_sampled")


def spec_draft(prompt_ids: torch.Tensor, prompt_len: torch.Tensor, tokens: torch.Tensor, gen_start: torch.Tensor,
               step: torch.Tensor, k: int, lookup_max: int, lookup_min: int, vocab: int, draft: torch.Tensor,
               n_draft: torch.Tensor) -> None:
    """The prompt-lookup drafter (vis_spec_draft) over the history prompt_ids[:prompt_len[0]] followed by
    tokens[gen_start[0]:step[0]]: up to k ids into draft int32 [>= k], their count into n_draft int32 [1] - all device
    memory, read at run time.  Equals spec.propose() exactly."""
    ints = (prompt_ids, prompt_len, tokens, gen_start, step, draft, n_draft)
    if any(t.dtype != torch.int32 for t in ints) or not all(t.is_contiguous() for t in ints):
        raise HipLibraryError("spec_draft: contiguous int32 tensors required")
    if any(t.numel() != 1 for t in (prompt_len, gen_start, step, n_draft)) or prompt_ids.numel() == 0 or draft.numel() < k:
        raise HipLibraryError("spec_draft: bad parameter shapes")
    rc = load().vis_spec_draft(_ptr(prompt_ids), prompt_ids.numel(), _ptr(prompt_len), _ptr(tokens), tokens.numel(),
                               _ptr(gen_start), _ptr(step), int(k), int(lookup_max), int(lookup_min), int(vocab), _ptr(draft),
                               _ptr(n_draft), _stream())
    _check(rc, "vis_spec_draft")


class AttnStreams(HipLibraryError):
    """vis_decode_attn_draft_batch returned VIS_ERR_UNSUPPORTED: the plain step of that many sequences takes the streaming
    attention form, which has no draft form.  Nothing was launched."""


def decode_attn_streams(n_kv: int, batch: int) -> bool:
    """Whether decode_attn takes the streaming form for ``batch`` sequences of ``n_kv`` kv heads (host only, no launch)."""
    return bool(load().vis_decode_attn_streams(int(n_kv), int(batch)))


def decode_attn_draft_batch(qkv: torch.Tensor, cos_t: torch.Tensor, sin_t: torch.Tensor, k_cache: torch.Tensor,
                            v_cache: torch.Tensor, step: torch.Tensor, part_o: torch.Tensor, part_ml: torch.Tensor,
                            out: torch.Tensor, n_q: int, n_kv: int, head_dim: int, nsplit: int, scale: float) -> torch.Tensor:
    """decode_attn_draft for B sequences of R rows each (vis_decode_attn_draft_batch): qkv [B * R, nq*D], row b * R + r at
    position step[b] + r of sequence b; caches [B, Hkv, T, D], tables [B, T, D], step int32 [B] (left as it is), workspaces
    for B * R rows, out [B * R, Hq*D].  Row (b, r) and the caches are bit-identical to R successive decode_attn calls on the
    batch at advancing steps.  AttnStreams where decode_attn_streams(n_kv, B) holds."""
    _bf16(qkv, "qkv"); _bf16(k_cache, "k_cache"); _bf16(v_cache, "v_cache"); _bf16(out, "out")
    if step.dtype != torch.int32 or not step.is_contiguous() or cos_t.dtype != torch.float32 or sin_t.dtype != torch.float32:
        raise HipLibraryError("decode_attn_draft_batch: step int32 / cos,sin f32 required")
    if k_cache.dim() != 4 or v_cache.shape != k_cache.shape or v_cache.stride() != k_cache.stride():
        raise HipLibraryError("decode_attn_draft_batch: batched caches [B, Hkv, T, D] with one stride required")
    B, kc = k_cache.shape[0], k_cache[0]
    if kc.shape[0] != n_kv or kc.shape[2] != head_dim or kc.stride(2) != 1 or kc.stride(1) != head_dim \
            or kc.stride(0) != kc.shape[1] * head_dim:
        raise HipLibraryError("decode_attn_draft_batch: bad cache shape")
    T = kc.shape[1]
    if cos_t.dim() != 3 or cos_t.shape != (B, T, head_dim) or sin_t.shape != cos_t.shape or not cos_t[0].is_contiguous() \
            or not sin_t[0].is_contiguous() or cos_t.stride(0) != sin_t.stride(0):
        raise HipLibraryError("decode_attn_draft_batch: cos/sin tables must be [B, cache_tokens, head_dim] with one batch stride")
    nq = (n_q + 2 * n_kv) * head_dim
    if qkv.dim() != 2 or qkv.shape[0] % B or not 1 <= qkv.shape[0] // B <= SPEC_MAX_ROWS or qkv.shape[1] != nq \
            or qkv.stride(1) != 1 or step.numel() != B:
        raise HipLibraryError("decode_attn_draft_batch: qkv must be [B * (1..4), (Hq + 2 Hkv) * D], step [B]")
    n = qkv.shape[0]
    if part_o.dtype != torch.float32 or part_ml.dtype != torch.float32 or part_o.numel() < n * n_q * nsplit * head_dim \
            or part_ml.numel() < n * n_q * nsplit * 2 or out.shape != (n, n_q * head_dim) or not out.is_contiguous():
        raise HipLibraryError("decode_attn_draft_batch: workspace/output too small")
    rc = load().vis_decode_attn_draft_batch(_ptr(qkv), _ptr(cos_t), _ptr(sin_t), _ptr(k_cache), _ptr(v_cache), _ptr(step),
                                            _ptr(part_o), _ptr(part_ml), _ptr(out), n_q, n_kv, head_dim, T, nsplit, scale,
                                            n // B, B, qkv.stride(0), k_cache.stride(0), cos_t.stride(0), _stream())
    if rc == 3:
        raise AttnStreams(f"vis_decode_attn_draft_batch: {B} sequences of {n_kv} kv heads take the streaming attention form")
    _check(rc, "vis_decode_attn_draft_batch")
    return out


def spec_gather_batch(table: torch.Tensor, cur_token: torch.Tensor, draft: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """The input rows of a batched speculative step (vis_spec_gather_batch): out [B * R, D] row b * R + r = table[cur_token[b]]
    for r = 0, table[draft[b, r - 1]] behind it; cur_token int32 [B], draft int32 [B, 3]."""
    _bf16(table, "spec_gather_batch table"); _bf16(out, "spec_gather_batch out")
    B = cur_token.numel()
    if cur_token.dtype != torch.int32 or draft.dtype != torch.int32 or draft.shape != (B, SPEC_MAX_ROWS - 1) \
            or not (table.is_contiguous() and out.is_contiguous() and cur_token.is_contiguous() and draft.is_contiguous()):
        raise HipLibraryError("spec_gather_batch: contiguous int32 cur_token [B] / draft [B, 3] and bf16 rows required")
    if out.dim() != 2 or out.shape[0] % B or not 1 <= out.shape[0] // B <= SPEC_MAX_ROWS or out.shape[1] != table.shape[1]:
        raise HipLibraryError("spec_gather_batch: out must be [B * (1..4), D]")
    rc = load().vis_spec_gather_batch(_ptr(table), _ptr(cur_token), _ptr(draft), _ptr(out), out.shape[0] // B, B,
                                      table.shape[1], table.shape[0], _stream())
    _check(rc, "vis_spec_gather_batch")
    return out


def spec_accept_batch(logits: torch.Tensor, draft: torch.Tensor, n_draft: torch.Tensor, limit: torch.Tensor,
                      ws_val: torch.Tensor, ws_idx: torch.Tensor, tokens: torch.Tensor, cur_token: torch.Tensor,
                      step: torch.Tensor, counters: torch.Tensor, params: Optional[torch.Tensor] = None) -> None:
    """spec_accept (``params`` None) / spec_accept_sampled per sequence (vis_spec_accept_batch): logits f32 [B * R, V], draft
    int32 [B, 3], n_draft / limit / cur_token / step int32 [B], tokens int32 [B, T], counters int32 [B, 3], params int32
    [B, 2] (the bits of sequence b's f32 inv_temp, its uint32 seed), ws_val f32 / ws_idx int32 of >= 256 * B * R entries."""
    ints = (draft, n_draft, limit, ws_idx, tokens, cur_token, step, counters) + (() if params is None else (params,))
    if logits.dtype != torch.float32 or ws_val.dtype != torch.float32 or any(t.dtype != torch.int32 for t in ints):
        raise HipLibraryError("spec_accept_batch: f32 logits, ws_val / int32 everything else required")
    B = step.numel()
    if logits.dim() != 2 or logits.stride(1) != 1 or logits.shape[0] % B or not 1 <= logits.shape[0] // B <= SPEC_MAX_ROWS:
        raise HipLibraryError("spec_accept_batch: logits must be [B * (1..4), V] with unit column stride")
    n, V = logits.shape
    if draft.shape != (B, SPEC_MAX_ROWS - 1) or any(t.numel() != B for t in (n_draft, limit, cur_token)) \
            or tokens.dim() != 2 or tokens.shape[0] != B or counters.shape != (B, 3) \
            or (params is not None and params.shape != (B, 2)) or ws_val.numel() < 256 * n or ws_idx.numel() < 256 * n \
            or not all(t.is_contiguous() for t in ints):
        raise HipLibraryError("spec_accept_batch: bad parameter shapes")
    rc = load().vis_spec_accept_batch(_ptr(logits), V, logits.stride(0), n // B, B, _ptr(draft), _ptr(n_draft), _ptr(limit),
                                      _ptr(ws_val), _ptr(ws_idx), _ptr(tokens), tokens.shape[1], _ptr(cur_token), _ptr(step),
                                      _ptr(counters), _ptr(params), _stream())
    _check(rc, "vis_spec_accept_batch")


def spec_draft_batch(prompt_ids: torch.Tensor, prompt_len: torch.Tensor, tokens: torch.Tensor, gen_start: torch.Tensor,
                     step: torch.Tensor, k: int, lookup_max: int, lookup_min: int, vocab: int, draft: torch.Tensor,
                     n_draft: torch.Tensor) -> None:
    """spec_draft per sequence (vis_spec_draft_batch): prompt_ids int32 [B, P], tokens int32 [B, T], prompt_len / gen_start /
    step / n_draft int32 [B], draft int32 [B, 3].  Sequence b's draft equals spec.propose() on its own history."""
    ints = (prompt_ids, prompt_len, tokens, gen_start, step, draft, n_draft)
    if any(t.dtype != torch.int32 for t in ints) or not all(t.is_contiguous() for t in ints):
        raise HipLibraryError("spec_draft_batch: contiguous int32 tensors required")
    B = step.numel()
    if any(t.numel() != B for t in (prompt_len, gen_start, n_draft)) or prompt_ids.dim() != 2 or prompt_ids.shape[0] != B \
            or prompt_ids.shape[1] == 0 or tokens.dim() != 2 or tokens.shape[0] != B or draft.shape != (B, SPEC_MAX_ROWS - 1):
        raise HipLibraryError("spec_draft_batch: bad parameter shapes")
    rc = load().vis_spec_draft_batch(_ptr(prompt_ids), prompt_ids.shape[1], _ptr(prompt_len), _ptr(tokens), tokens.shape[1],
                                     _ptr(gen_start), _ptr(step), int(k), int(lookup_max), int(lookup_min), int(vocab), B,
                                     _ptr(draft), _ptr(n_draft), _stream())
    _check(rc, "vis_spec_draft_batch")


def spec_accept_masked(logits: torch.Tensor, draft: torch.Tensor, n_draft: torch.Tensor, limit: torch.Tensor,
                       ws_val: torch.Tensor, ws_idx: torch.Tensor, tokens: torch.Tensor, cur_token: torch.Tensor,
                       step: torch.Tensor, counters: torch.Tensor, allow: torch.Tensor,
                       params: Optional[torch.Tensor] = None) -> None:
    """spec_accept (``params`` None) or spec_accept_sampled with row r's pick restricted to allow[r] (vis_spec_accept_masked):
    allow int64 [R, >= ceil(V / 64)], schema_mask_rows' rows.  Row r's pick is argmax_masked's token for that row at
    step[0] + r, bit for bit.  Everything else as spec_accept / spec_accept_sampled."""
    ints = (draft, n_draft, limit, ws_idx, tokens, cur_token, step, counters) + (() if params is None else (params,))
    if logits.dtype != torch.float32 or ws_val.dtype != torch.float32 or any(t.dtype != torch.int32 for t in ints):
        raise HipLibraryError("spec_accept_masked: f32 logits, ws_val / int32 everything else required")
    if logits.dim() != 2 or not 1 <= logits.shape[0] <= SPEC_MAX_ROWS or logits.stride(1) != 1:
        raise HipLibraryError("spec_accept_masked: logits must be [1..4, V] with unit column stride")
    R, V = logits.shape
    if draft.numel() < max(1, R - 1) or any(t.numel() != 1 for t in (n_draft, limit, cur_token, step)) or counters.numel() != 3 \
            or (params is not None and params.numel() != 2) or ws_val.numel() < 256 * R or ws_idx.numel() < 256 * R \
            or not all(t.is_contiguous() for t in ints):
        raise HipLibraryError("spec_accept_masked: bad parameter shapes")
    if allow.dtype != torch.int64 or allow.dim() != 2 or allow.shape[0] != R or allow.shape[1] < (V + 63) // 64 \
            or allow.stride(1) != 1:
        raise HipLibraryError("spec_accept_masked: allow must be int64 [R, ceil(V / 64)]")
    rc = load().vis_spec_accept_masked(_ptr(logits), V, logits.stride(0), R, _ptr(draft), _ptr(n_draft), _ptr(limit),
                                       _ptr(ws_val), _ptr(ws_idx), _ptr(tokens), tokens.numel(), _ptr(cur_token), _ptr(step),
                                       _ptr(counters), _ptr(params), _ptr(allow), allow.stride(0), _stream())
    _check(rc, "vis_spec_accept_masked")


SCHEMA_ROWS_RECORD_INTS = 32     # int32 words of vis_schema_mask_rows' record (SR_INTS of csrc/spec_schema.hip)


def _schema_tables(name, tok_off, tok_bytes, tok_flags, header, trans, byte_class, state_flags) -> int:
    V = tok_flags.numel()
    if tok_off.dtype != torch.int32 or tok_off.numel() != V + 1 or tok_bytes.dtype != torch.uint8 or tok_flags.dtype != torch.uint8:
        raise HipLibraryError(f"{name}: bad token table")
    if header.dtype != torch.int32 or header.numel() != 4 or trans.dtype != torch.int16 or trans.dim() != 2 \
            or byte_class.dtype != torch.uint8 or byte_class.numel() != 256 or state_flags.dtype != torch.uint8 \
            or state_flags.numel() != trans.shape[0]:
        raise HipLibraryError(f"{name}: bad DFA tables")
    if not all(t.is_contiguous() for t in (tok_off, tok_bytes, tok_flags, header, trans, byte_class, state_flags)):
        raise HipLibraryError(f"{name}: bad strides")
    return V


def schema_mask_rows(record: torch.Tensor, tokens: torch.Tensor, step: torch.Tensor, draft: torch.Tensor,
                     n_draft: torch.Tensor, tok_off: torch.Tensor, tok_bytes: torch.Tensor, tok_flags: torch.Tensor,
                     eos_ids: torch.Tensor, allow: torch.Tensor, header: torch.Tensor, trans: torch.Tensor,
                     byte_class: torch.Tensor, state_flags: torch.Tensor) -> None:
    """The allow rows of ONE sequence's speculative step under a schema (vis_schema_mask_rows): allow int64 [R, >= ceil(V /
    64)], R = 1..4; row 0 = schema_mask's row at step[0], row r the row behind draft[:r]; rows behind a missing, EOS, out-of-
    range or rejected draft are zero.  record int32 [32] (zeroed = a reply that starts at tokens[0] in the start state),
    tokens int32 [T], step / n_draft int32 [1], draft int32 [>= R - 1]; the token table and the DFA as in schema_mask."""
    V = _schema_tables("schema_mask_rows", tok_off, tok_bytes, tok_flags, header, trans, byte_class, state_flags)
    ints = (record, tokens, step, draft, n_draft, eos_ids)
    if any(t.dtype != torch.int32 for t in ints) or not all(t.is_contiguous() for t in ints):
        raise HipLibraryError("schema_mask_rows: contiguous int32 record / tokens / step / draft / n_draft / eos_ids required")
    if allow.dtype != torch.int64 or allow.dim() != 2 or not 1 <= allow.shape[0] <= SPEC_MAX_ROWS \
            or allow.shape[1] < (V + 63) // 64 or allow.stride(1) != 1:
        raise HipLibraryError("schema_mask_rows: allow must be int64 [1..4, ceil(V / 64)]")
    R = allow.shape[0]
    if record.numel() != SCHEMA_ROWS_RECORD_INTS or tokens.dim() != 1 or step.numel() != 1 or n_draft.numel() != 1 \
            or draft.numel() < max(1, R - 1):
        raise HipLibraryError("schema_mask_rows: bad parameter shapes")
    rc = load().vis_schema_mask_rows(_ptr(record), _ptr(tokens), tokens.numel(), _ptr(step), _ptr(draft), _ptr(n_draft), R,
                                     _ptr(tok_off), _ptr(tok_bytes), _ptr(tok_flags), _ptr(eos_ids), eos_ids.numel(), V,
                                     _ptr(allow), allow.stride(0), _ptr(header), _ptr(trans), _ptr(byte_class),
                                     _ptr(state_flags), trans.shape[0], trans.shape[1], _stream())
    _check(rc, "vis_schema_mask_rows")


def spec_draft_schema(record: torch.Tensor, tokens: torch.Tensor, step: torch.Tensor, tok_off: torch.Tensor,
                      tok_bytes: torch.Tensor, tok_flags: torch.Tensor, header: torch.Tensor, trans: torch.Tensor,
                      byte_class: torch.Tensor, state_flags: torch.Tensor, jump_tok: torch.Tensor, jump_next: torch.Tensor,
                      k: int, draft: torch.Tensor, n_draft: torch.Tensor) -> None:
    """The drafter that reads the schema (vis_spec_draft_schema; schema_draft.propose is its definition): the state of
    schema_mask_rows' record advanced over tokens[position:step[0]], then up to k jumps through jump_tok / jump_next (int32
    [cap_states]) into draft / n_draft; with no draft both are left alone."""
    V = _schema_tables("spec_draft_schema", tok_off, tok_bytes, tok_flags, header, trans, byte_class, state_flags)
    ints = (record, tokens, step, jump_tok, jump_next, draft, n_draft)
    if any(t.dtype != torch.int32 for t in ints) or not all(t.is_contiguous() for t in ints):
        raise HipLibraryError("spec_draft_schema: contiguous int32 tensors required")
    if record.numel() != SCHEMA_ROWS_RECORD_INTS or step.numel() != 1 or n_draft.numel() != 1 or draft.numel() < k \
            or jump_tok.numel() < trans.shape[0] or jump_next.numel() < trans.shape[0]:
        raise HipLibraryError("spec_draft_schema: bad parameter shapes")
    rc = load().vis_spec_draft_schema(_ptr(record), _ptr(tokens), tokens.numel(), _ptr(step), _ptr(tok_off), _ptr(tok_bytes),
                                      _ptr(tok_flags), V, _ptr(header), _ptr(trans), _ptr(byte_class), _ptr(state_flags),
                                      trans.shape[0], trans.shape[1], _ptr(jump_tok), _ptr(jump_next), int(k), _ptr(draft),
                                      _ptr(n_draft), _stream())
    _check(rc, "vis_spec_draft_schema")


SPEC_PRED_STATE_INTS = 7     # cursor, last, seen, src, n_out, accepted, rejected (spec.PredState; SP_ST_INTS of csrc/spec.hip)


def spec_draft_pred(prompt_ids: torch.Tensor, prompt_len: torch.Tensor, tokens: torch.Tensor, gen_start: torch.Tensor,
                    step: torch.Tensor, k: int, lookup_max: int, lookup_min: int, vocab: int, pred_ids: torch.Tensor,
                    pred_len: torch.Tensor, state: torch.Tensor, draft: torch.Tensor, n_draft: torch.Tensor) -> None:
    """The drafter of a request with a prediction (vis_spec_draft_pred): one spec.propose_pred() call over the reply
    tokens[gen_start[0]:step[0]], the prediction pred_ids[:pred_len[0]] and the 7 state ints - all device memory, read and
    written at run time.  Up to k ids into draft int32 [>= k], their count into n_draft.  Equals spec.propose_pred() exactly."""
    ints = (prompt_ids, prompt_len, tokens, gen_start, step, pred_ids, pred_len, state, draft, n_draft)
    if any(t.dtype != torch.int32 for t in ints) or not all(t.is_contiguous() for t in ints):
        raise HipLibraryError("spec_draft_pred: contiguous int32 tensors required")
    if any(t.numel() != 1 for t in (prompt_len, gen_start, step, pred_len, n_draft)) or prompt_ids.numel() == 0 \
            or pred_ids.numel() == 0 or state.numel() != SPEC_PRED_STATE_INTS or draft.numel() < k:
        raise HipLibraryError("spec_draft_pred: bad parameter shapes")
    rc = load().vis_spec_draft_pred(_ptr(prompt_ids), prompt_ids.numel(), _ptr(prompt_len), _ptr(tokens), tokens.numel(),
                                    _ptr(gen_start), _ptr(step), int(k), int(lookup_max), int(lookup_min), int(vocab),
                                    _ptr(pred_ids), pred_ids.numel(), _ptr(pred_len), _ptr(state), _ptr(draft), _ptr(n_draft),
                                    _stream())
    _check(rc, "vis_spec_draft_pred")


STOP_STATE_INTS = 8     # int32 words of one sequence's vis_stop_scan record (stop.STATE_INTS)


def stop_scan(state: torch.Tensor, tokens: torch.Tensor, step: torch.Tensor, tok_off: torch.Tensor, tok_bytes: torch.Tensor,
              tok_flags: torch.Tensor, header: torch.Tensor, trans: torch.Tensor, byte_class: torch.Tensor,
              hits: torch.Tensor, eos_on: bool = True) -> None:
    """Fold the tokens picked since the last call through the stop strings' automaton (stop.StopDFA) and keep each row's
    sticky finish record.  Runs AFTER the pick.  state [B, 8] int32 (zeroed = fresh), tokens [B, T] int32, step [B] int32; the
    token table as in json_mask; header int32 [4] = (n_states, n_classes, 0, 0), trans [cap_states, cap_classes] int16 (the
    u16 bits, bit 15 = the target state ends a stop string) holding the live table packed at its front, byte_class [256]
    uint8, hits [cap_states, 2] uint8 = (hit_len, hit_id)."""
    if state.dim() != 2 or tokens.dim() != 2:
        raise HipLibraryError("stop_scan: state / tokens must be 2-D")
    B = state.shape[0]
    V = tok_flags.numel()
    if state.dtype != torch.int32 or state.shape[1] != STOP_STATE_INTS or tokens.dtype != torch.int32 or step.dtype != torch.int32:
        raise HipLibraryError("stop_scan: int32 state [B, 8] / tokens / step required")
    if tokens.shape[0] != B or step.numel() != B:
        raise HipLibraryError("stop_scan: bad batch shapes")
    if tok_off.dtype != torch.int32 or tok_off.numel() != V + 1 or tok_bytes.dtype != torch.uint8 or tok_flags.dtype != torch.uint8:
        raise HipLibraryError("stop_scan: bad token table")
    if header.dtype != torch.int32 or header.numel() != 4 or trans.dtype != torch.int16 or trans.dim() != 2 \
            or byte_class.dtype != torch.uint8 or byte_class.numel() != 256 or hits.dtype != torch.uint8 \
            or hits.shape != (trans.shape[0], 2):
        raise HipLibraryError("stop_scan: bad automaton tables")
    if tokens.stride(1) != 1 or not (state.is_contiguous() and step.is_contiguous() and tok_off.is_contiguous()
                                     and tok_bytes.is_contiguous() and tok_flags.is_contiguous() and header.is_contiguous()
                                     and trans.is_contiguous() and byte_class.is_contiguous() and hits.is_contiguous()):
        raise HipLibraryError("stop_scan: bad strides")
    if B > 1 and tokens.stride(0) != tokens.shape[1]:
        raise HipLibraryError("stop_scan: rows must be contiguous")
    rc = load().vis_stop_scan(_ptr(state), _ptr(tokens), tokens.shape[1], _ptr(step), _ptr(tok_off), _ptr(tok_bytes),
                              _ptr(tok_flags), V, _ptr(header), _ptr(trans), _ptr(byte_class), _ptr(hits), trans.shape[0],
                              trans.shape[1], int(bool(eos_on)), B, _stream())
    _check(rc, "vis_stop_scan")


STREAM_RECORD_INTS = 4      # int32 words of one vis_stream_publish record: token id, safe_bytes, status, cut


class HostCoherent:
    """``nbytes`` of host memory a running kernel stores to coherently (vis_host_coherent_alloc: hipHostMalloc, coherent +
    mapped, zero-filled), owned by this object.  ``array`` gives numpy views of it for the host side; ``dev_ptr + offset``
    is what a kernel is given.  Not a torch tensor on purpose: whether torch's pinned memory is fine-grained is not something
    to rest on."""

    def __init__(self, nbytes: int):
        host, dev = ctypes.c_void_p(), ctypes.c_void_p()
        _check(load().vis_host_coherent_alloc(ctypes.addressof(host), ctypes.addressof(dev), int(nbytes)),
               "vis_host_coherent_alloc")
        self.host_ptr, self.dev_ptr, self.nbytes = int(host.value), int(dev.value), int(nbytes)

    def array(self, offset: int, shape, dtype="int32"):
        import numpy as _np
        n = int(_np.prod(shape)) * _np.dtype(dtype).itemsize
        if offset < 0 or offset + n > self.nbytes or self.host_ptr is None:
            raise HipLibraryError("HostCoherent.array: outside the allocation")
        buf = (ctypes.c_char * n).from_address(self.host_ptr + offset)
        return _np.frombuffer(buf, dtype=dtype).reshape(shape)

    def free(self) -> None:
        if self.host_ptr is not None:
            _check(load().vis_host_free(self.host_ptr), "vis_host_free")
            self.host_ptr = self.dev_ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:      # noqa: BLE001 - interpreter shutdown
            pass


def stream_publish(stop_state: torch.Tensor, tokens: torch.Tensor, step: torch.Tensor, depth: torch.Tensor,
                   pub: torch.Tensor, records_ptr: int, capacity: int, count_ptr: int, start_ptr: int) -> None:
    """Append one record per row to the host arrays the reader polls (csrc/stream_publish.hip).  Runs AFTER stop_scan.
    stop_state [B, 8] int32 (the rows' stop-scan records), tokens [B, T] int32, step [B] int32, depth uint8 [n_states],
    pub [B] int32 (device mirror of count, zero = fresh); records_ptr / count_ptr / start_ptr: device addresses inside a
    HostCoherent allocation of the first row's records [capacity][4] int32 (rows ``capacity`` records apart), count and
    start (int32 [B])."""
    if stop_state.dim() != 2 or tokens.dim() != 2:
        raise HipLibraryError("stream_publish: stop_state / tokens must be 2-D")
    B = stop_state.shape[0]
    if stop_state.dtype != torch.int32 or stop_state.shape[1] != STOP_STATE_INTS or tokens.dtype != torch.int32 \
            or step.dtype != torch.int32 or pub.dtype != torch.int32 or depth.dtype != torch.uint8:
        raise HipLibraryError("stream_publish: int32 stop_state [B, 8] / tokens / step / pub and uint8 depth required")
    if tokens.shape[0] != B or step.numel() != B or pub.numel() != B:
        raise HipLibraryError("stream_publish: bad batch shapes")
    if tokens.stride(1) != 1 or (B > 1 and tokens.stride(0) != tokens.shape[1]) or not (
            stop_state.is_contiguous() and step.is_contiguous() and pub.is_contiguous() and depth.is_contiguous()):
        raise HipLibraryError("stream_publish: bad strides")
    rc = load().vis_stream_publish(_ptr(stop_state), _ptr(tokens), tokens.shape[1], _ptr(step), _ptr(depth), depth.numel(),
                                   _ptr(pub), records_ptr, int(capacity), count_ptr, start_ptr, B, _stream())
    _check(rc, "vis_stream_publish")


DP_PLAIN, DP_SWIGLU, DP_RESID_NORMW = 0, 1, 2
SSQ_LD = 64      # row stride of the [units][64] f32 sum-of-squares partials, one per 32 columns (csrc/decode_proj_common.hip.h)
SSQ_UNIT = 32


def decode_proj_ws(device, B: int, N: int, K: int, fp8: bool = False) -> torch.Tensor:
    """Zeroed workspace of decode_proj / decode_proj_fp8 for (B, N, K): arrival counters + the segment blocks of split tiles.
    Allocate for the largest (B, N, K) it will serve; one launch at a time per workspace."""
    n = int(load().vis_decode_proj_ws_bytes(B, N, K, 1 if fp8 else 0))
    if n <= 0:
        raise HipLibraryError(f"decode_proj_ws: unsupported shape B={B} N={N} K={K} fp8={fp8}")
    return torch.zeros(n, dtype=torch.uint8, device=device)


def decode_proj_form(B: int, N: int, K: int, mode: int, mx_out: bool, fp8: bool) -> str:
    """'colpar' or 'streamk' for one batched-decode projection.  The column-parallel form (no cross-workgroup reduction) needs
    every workgroup to stream all of x: taken when it covers the shape and a workgroup's x traffic (K-steps x the x tile) stays
    under 1.5 MB - i.e. everything but long-K projections at many sequences (7B down: K = 18944, 2.4 MB at 64 sequences)."""
    forced = os.environ.get("VIS_DECODE_PROJ_FORM", "")
    if forced in ("colpar", "streamk") and (forced == "streamk" or load().vis_decode_proj_colpar_covers(N, mode, 1 if mx_out else 0)):
        return forced
    if not load().vis_decode_proj_colpar_covers(N, mode, 1 if mx_out else 0):
        return "streamk"
    steps = K // (128 if fp8 else 64)
    x_tile = 8192 if B > 32 else 4096
    return "colpar" if steps * x_tile <= 1536 * 1024 else "streamk"


def _dp_common(name, B, N, mode, out, out_w, out_q, out_qs, bias, residual, norm_w, ssq_in, ssq_out, ws, need):
    n_out = N // 2 if mode == DP_SWIGLU else N
    for t, what in ((out, "out"), (out_w, "out_w")):
        if t is not None and (t.dim() != 2 or t.shape[0] != B or t.shape[1] != n_out or t.stride(1) != 1):
            raise HipLibraryError(f"{name}: bad {what} shape")
    if out is not None and out.dtype not in (torch.bfloat16, torch.float32):
        raise HipLibraryError(f"{name}: out must be bf16 or f32")
    if out_w is not None and (out is None or out_w.dtype != torch.bfloat16 or out_w.stride(0) != out.stride(0)):
        raise HipLibraryError(f"{name}: out_w needs out and its row stride")
    if (out_q is None) != (out_qs is None) or (out_q is not None and (
            out_q.dtype != torch.uint8 or out_qs.dtype != torch.uint8 or out_q.shape[0] != B or out_q.shape[1] < n_out
            or out_qs.shape[0] != B or out_qs.shape[1] * 32 < n_out or out_q.stride(1) != 1 or out_qs.stride(1) != 1)):
        raise HipLibraryError(f"{name}: bad MX outputs")
    if residual is not None and (residual.dtype != torch.bfloat16 or residual.shape != (B, N) or residual.stride(1) != 1):
        raise HipLibraryError(f"{name}: bad residual")
    if bias is not None and (bias.dtype != torch.bfloat16 or bias.numel() != N):
        raise HipLibraryError(f"{name}: bad bias")
    if norm_w is not None and (norm_w.dtype != torch.bfloat16 or norm_w.numel() != N):
        raise HipLibraryError(f"{name}: bad norm_w")
    for t, tiles in ((ssq_in, None), (ssq_out, (N + SSQ_UNIT - 1) // SSQ_UNIT)):
        if t is not None and (t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != SSQ_LD or not t.is_contiguous()
                              or (tiles is not None and t.shape[0] < tiles)):
            raise HipLibraryError(f"{name}: ssq buffers are f32 [columns / 32, {SSQ_LD}]")
    if need and (ws is None or ws.dtype != torch.uint8 or ws.numel() < need):
        raise HipLibraryError(f"{name}: workspace too small ({0 if ws is None else ws.numel()} < {need})")


def decode_proj(x: torch.Tensor, w: torch.Tensor, ws: torch.Tensor, mode: int = DP_PLAIN,
                out: Optional[torch.Tensor] = None, out_w: Optional[torch.Tensor] = None,
                out_q: Optional[torch.Tensor] = None, out_qs: Optional[torch.Tensor] = None,
                bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
                norm_w: Optional[torch.Tensor] = None, ssq_in: Optional[torch.Tensor] = None,
                ssq_out: Optional[torch.Tensor] = None, norm_dim: int = 0, eps: float = 1e-6, form: str = "auto") -> None:
    """Batched-decode projection with its epilogue in the same launch (vis_decode_proj_bf16 / vis_decode_proj_colpar_bf16;
    include/vis_hip.h): x [B, K] bf16, w [N, K] bf16.  DP_PLAIN: out = x w^T * rs + bias (bf16 / f32).  DP_SWIGLU: out [B, N/2].
    DP_RESID_NORMW: out = y = x w^T + residual, out_w = y * norm_w, ssq_out = per-unit (32 columns) sums of y^2.  rs from
    ssq_in (norm_dim columns) or 1.  form: "colpar" (whole-K column slabs, no workspace), "streamk" (needs ws) or "auto"."""
    _bf16(x, "decode_proj x"); _bf16(w, "decode_proj w")
    B, K = x.shape
    N = w.shape[0]
    if w.shape[1] != K or x.stride(1) != 1 or w.stride(1) != 1:
        raise HipLibraryError("decode_proj: bad operand shapes")
    lib = load()
    if form == "auto":
        form = decode_proj_form(B, N, K, mode, out_q is not None, False)
    colpar = form == "colpar"
    _dp_common("decode_proj", B, N, mode, out, out_w, out_q, out_qs, bias, residual, norm_w, ssq_in, ssq_out, ws,
               0 if colpar else int(lib.vis_decode_proj_ws_bytes(B, N, K, 0)))
    ldc = out.stride(0) if out is not None else 0
    tail = (B, N, K, x.stride(0), w.stride(0), ldc, residual.stride(0) if residual is not None else 0,
            out_q.stride(0) if out_q is not None else 0, out_qs.stride(0) if out_qs is not None else 0,
            mode, 1 if (out is not None and out.dtype == torch.float32) else 0,
            ssq_in.shape[0] if ssq_in is not None else 0, norm_dim, eps, _stream())
    if colpar:
        rc = lib.vis_decode_proj_colpar_bf16(_ptr(x), _ptr(w), _ptr(out), _ptr(out_w), _ptr(out_q), _ptr(out_qs), _ptr(bias),
                                             _ptr(residual), _ptr(norm_w), _ptr(ssq_in), _ptr(ssq_out), *tail)
        _check(rc, "vis_decode_proj_colpar_bf16")
        return
    rc = lib.vis_decode_proj_bf16(_ptr(x), _ptr(w), _ptr(ws), _ptr(out), _ptr(out_w), _ptr(out_q), _ptr(out_qs), _ptr(bias),
                                  _ptr(residual), _ptr(norm_w), _ptr(ssq_in), _ptr(ssq_out), *tail)
    _check(rc, "vis_decode_proj_bf16")


def decode_proj_fp8(xq: torch.Tensor, xs: torch.Tensor, wq: torch.Tensor, sw: torch.Tensor, ws: torch.Tensor,
                    mode: int = DP_PLAIN, out: Optional[torch.Tensor] = None, out_w: Optional[torch.Tensor] = None,
                    out_q: Optional[torch.Tensor] = None, out_qs: Optional[torch.Tensor] = None,
                    bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
                    norm_w: Optional[torch.Tensor] = None, ssq_in: Optional[torch.Tensor] = None,
                    ssq_out: Optional[torch.Tensor] = None, norm_dim: int = 0, eps: float = 1e-6, form: str = "auto") -> None:
    """fp8 form: xq [B, K] e4m3 bytes + xs [B, >= K/32] E8M0 block scales (MX blocks of 32 columns), wq [N, K] e4m3 + sw [N] f32."""
    B, K = xq.shape
    N = wq.shape[0]
    if xq.dtype != torch.uint8 or wq.dtype != torch.uint8 or xs.dtype != torch.uint8 or wq.shape[1] != K \
            or xq.stride(1) != 1 or wq.stride(1) != 1 or xs.stride(1) != 1 or xs.shape[0] != B or xs.shape[1] * 32 < K \
            or sw.dtype != torch.float32 or sw.numel() != N:
        raise HipLibraryError("decode_proj_fp8: bad operands")
    lib = load()
    if form == "auto":
        form = decode_proj_form(B, N, K, mode, out_q is not None, True)
    colpar = form == "colpar"
    _dp_common("decode_proj_fp8", B, N, mode, out, out_w, out_q, out_qs, bias, residual, norm_w, ssq_in, ssq_out, ws,
               0 if colpar else int(lib.vis_decode_proj_ws_bytes(B, N, K, 1)))
    ldc = out.stride(0) if out is not None else 0
    tail = (B, N, K, xq.stride(0), xs.stride(0), wq.stride(0), ldc, residual.stride(0) if residual is not None else 0,
            out_q.stride(0) if out_q is not None else 0, out_qs.stride(0) if out_qs is not None else 0,
            mode, 1 if (out is not None and out.dtype == torch.float32) else 0,
            ssq_in.shape[0] if ssq_in is not None else 0, norm_dim, eps, _stream())
    if colpar:
        rc = lib.vis_decode_proj_colpar_fp8(_ptr(xq), _ptr(xs), _ptr(wq), _ptr(sw), _ptr(out), _ptr(out_w), _ptr(out_q),
                                            _ptr(out_qs), _ptr(bias), _ptr(residual), _ptr(norm_w), _ptr(ssq_in), _ptr(ssq_out), *tail)
        _check(rc, "vis_decode_proj_colpar_fp8")
        return
    rc = lib.vis_decode_proj_fp8(_ptr(xq), _ptr(xs), _ptr(wq), _ptr(sw), _ptr(ws), _ptr(out), _ptr(out_w), _ptr(out_q),
                                 _ptr(out_qs), _ptr(bias), _ptr(residual), _ptr(norm_w), _ptr(ssq_in), _ptr(ssq_out), *tail)
    _check(rc, "vis_decode_proj_fp8")


def decode_prep_rows(table: torch.Tensor, ids: torch.Tensor, norm_w: torch.Tensor, x: torch.Tensor,
                     xw: Optional[torch.Tensor], ssq: torch.Tensor, xq: Optional[torch.Tensor] = None,
                     xqs: Optional[torch.Tensor] = None) -> None:
    """Head of a batched decode step: x[b] = table[ids[b]], xw = x * norm_w (bf16), ssq = per-tile sums of x^2, optionally
    the MX copy of xw - what the first decode_proj of the step consumes."""
    _bf16(table, "decode_prep_rows table"); _bf16(x, "decode_prep_rows x"); _bf16(norm_w, "decode_prep_rows norm_w")
    B, H = x.shape
    if table.dim() != 2 or table.shape[1] != H or not table.is_contiguous() or ids.dtype != torch.int32 or ids.numel() != B \
            or x.stride(1) != 1 or norm_w.numel() != H or (xw is not None and (xw.shape != x.shape or xw.stride() != x.stride()
                                                                                 or xw.dtype != torch.bfloat16)) \
            or ssq.dtype != torch.float32 or ssq.dim() != 2 or ssq.shape[1] != SSQ_LD or ssq.shape[0] * SSQ_UNIT < H \
            or not ssq.is_contiguous():
        raise HipLibraryError("decode_prep_rows: bad shapes")
    if (xq is None) != (xqs is None) or (xq is not None and (xq.dtype != torch.uint8 or xqs.dtype != torch.uint8
                                                             or xq.shape[0] != B or xq.shape[1] < H or xqs.shape[0] != B
                                                             or xqs.shape[1] * 32 < H)):
        raise HipLibraryError("decode_prep_rows: bad MX outputs")
    rc = load().vis_decode_prep_rows(_ptr(table), _ptr(ids), _ptr(norm_w), _ptr(x), _ptr(xw), _ptr(xq), _ptr(xqs), _ptr(ssq),
                                     B, table.shape[0], H, x.stride(0), xq.stride(0) if xq is not None else 0,
                                     xqs.stride(0) if xqs is not None else 0, _stream())
    _check(rc, "vis_decode_prep_rows")


def part_rows(B: int) -> int:
    """Rows of one partial slab of the batched-decode projection: 16 / 32 / 64 for up to 16 / 32 / 64 sequences."""
    return 16 if B <= 16 else 32 if B <= 32 else 64


def decode_gemm(x: torch.Tensor, w: torch.Tensor, part: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None, ksplit: int = 0) -> int:
    """Batched-decode projection, first half: f32 partials part[slot][part_rows(B)][N] whose sum over the returned number
    of slots is x[B,K] @ w[N,K].T (every slot is written), or - with ``out`` instead of ``part`` - a direct
    bf16 / f32 result."""
    _bf16(x, "decode_gemm x"); _bf16(w, "decode_gemm w")
    B, K = x.shape
    N = w.shape[0]
    if w.shape[1] != K or x.stride(1) != 1 or w.stride(1) != 1 or (part is None) == (out is None):
        raise HipLibraryError("decode_gemm: bad shapes (give exactly one of part / out)")
    lib = load()
    if part is not None:
        ks = ksplit or lib.vis_gemm_decode_ksplit(N, K)
        if part.dtype != torch.float32 or part.numel() < ks * part_rows(B) * N:
            raise HipLibraryError("decode_gemm: partial workspace too small")
        rc = lib.vis_gemm_decode_bf16(_ptr(x), _ptr(w), _ptr(part), None, B, N, K, x.stride(0), w.stride(0), 0, ks, 0,
                                      _stream())
    else:
        ks = 1
        if out.shape != (B, N) or out.stride(1) != 1 or out.dtype not in (torch.bfloat16, torch.float32):
            raise HipLibraryError("decode_gemm: bad output")
        rc = lib.vis_gemm_decode_bf16(_ptr(x), _ptr(w), None, _ptr(out), B, N, K, x.stride(0), w.stride(0),
                                      out.stride(0), 1, 1 if out.dtype == torch.float32 else 0, _stream())
    _check(rc, "vis_gemm_decode_bf16")
    return ks


def decode_gemm_fp8(xq: torch.Tensor, sx: torch.Tensor, wq: torch.Tensor, sw: torch.Tensor,
                    part: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, ksplit: int = 0) -> int:
    """fp8 batched-decode projection: raw f32 partials (returns the slot count) or a direct scaled bf16 / f32 result."""
    B, K = xq.shape
    N = wq.shape[0]
    if xq.dtype != torch.uint8 or wq.dtype != torch.uint8 or wq.shape[1] != K or xq.stride(1) != 1 or wq.stride(1) != 1 \
            or (part is None) == (out is None):
        raise HipLibraryError("decode_gemm_fp8: bad operands (give exactly one of part / out)")
    lib = load()
    if part is not None:
        ks = ksplit or lib.vis_gemm_decode_fp8_ksplit(N, K)
        if part.dtype != torch.float32 or part.numel() < ks * part_rows(B) * N:
            raise HipLibraryError("decode_gemm_fp8: partial workspace too small")
        rc = lib.vis_gemm_decode_fp8(_ptr(xq), _ptr(sx), _ptr(wq), _ptr(sw), _ptr(part), None, B, N, K, xq.stride(0),
                                     wq.stride(0), 0, ks, 0, _stream())
    else:
        ks = 1
        if out.shape != (B, N) or out.stride(1) != 1 or out.dtype not in (torch.bfloat16, torch.float32):
            raise HipLibraryError("decode_gemm_fp8: bad output")
        rc = lib.vis_gemm_decode_fp8(_ptr(xq), _ptr(sx), _ptr(wq), _ptr(sw), None, _ptr(out), B, N, K, xq.stride(0),
                                     wq.stride(0), out.stride(0), 1, 1 if out.dtype == torch.float32 else 0, _stream())
    _check(rc, "vis_gemm_decode_fp8")
    return ks


def skinny_finalize_fp8(part: torch.Tensor, ksplit: int, y: torch.Tensor, N: int, sx: Optional[torch.Tensor] = None,
                        sw: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
                        residual: Optional[torch.Tensor] = None, norm_w: Optional[torch.Tensor] = None,
                        yn: Optional[torch.Tensor] = None, yq: Optional[torch.Tensor] = None,
                        yq_scale: Optional[torch.Tensor] = None, swiglu: bool = False, eps: float = 1e-6) -> None:
    """Finalisation with fp8 partial scaling (sx, sw) and/or an e4m3 copy (yq, yq_scale) of the next projection's input."""
    B = y.shape[0]
    n_out = N // 2 if swiglu else N
    if y.shape[1] != n_out or (yn is not None and yn.shape != y.shape):
        raise HipLibraryError("skinny_finalize_fp8: bad output shapes")
    if yq is not None and (yq.dtype != torch.uint8 or yq.shape[0] != B or yq.shape[1] < n_out or yq_scale is None):
        raise HipLibraryError("skinny_finalize_fp8: bad yq")
    rc = load().vis_skinny_finalize_fp8(_ptr(part), ksplit, _ptr(sx), _ptr(sw), _ptr(bias), _ptr(residual),
                                        _ptr(norm_w), _ptr(y), _ptr(yn), _ptr(yq), _ptr(yq_scale), B, N,
                                        residual.stride(0) if residual is not None else 0, y.stride(0),
                                        yn.stride(0) if yn is not None else 0, yq.stride(0) if yq is not None else 0,
                                        1 if swiglu else 0, eps, _stream())
    _check(rc, "vis_skinny_finalize_fp8")


def skinny_finalize(part: torch.Tensor, ksplit: int, y: torch.Tensor, N: int, bias: Optional[torch.Tensor] = None,
                    residual: Optional[torch.Tensor] = None, norm_w: Optional[torch.Tensor] = None,
                    yn: Optional[torch.Tensor] = None, swiglu: bool = False, eps: float = 1e-6) -> None:
    """Batched-decode projection, second half (see include/vis_hip.h): y [B, N or N/2], optional normalised yn."""
    _bf16(y, "finalize y")
    B = y.shape[0]
    n_out = N // 2 if swiglu else N
    if y.shape[1] != n_out or y.stride(1) != 1 or (yn is not None and (yn.shape != y.shape or yn.stride(1) != 1)):
        raise HipLibraryError("skinny_finalize: bad output shapes")
    if residual is not None and (residual.shape != y.shape or residual.stride(1) != 1):
        raise HipLibraryError("skinny_finalize: bad residual")
    rc = load().vis_skinny_finalize(_ptr(part), ksplit, _ptr(bias), _ptr(residual), _ptr(norm_w), _ptr(y), _ptr(yn),
                                    B, N, residual.stride(0) if residual is not None else 0, y.stride(0),
                                    yn.stride(0) if yn is not None else 0, 1 if swiglu else 0, eps, _stream())
    _check(rc, "vis_skinny_finalize")


_MEAN = (ctypes.c_float * 3)()
_STD = (ctypes.c_float * 3)()


_RESIZE_TABLES: dict = {}


def resize_rgb(frame: torch.Tensor, out_h: int, out_w: int, kind: str = "bicubic") -> torch.Tensor:
    """uint8 [H, W, 3] device frame -> uint8 [out_h, out_w, 3], bit-exact with PIL's BICUBIC / BILINEAR resize."""
    from .image_processing import resample_coeffs
    if frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[2] != 3 or not frame.is_contiguous():
        raise HipLibraryError("resize_rgb: contiguous uint8 [H, W, 3] frame required")
    in_h, in_w = int(frame.shape[0]), int(frame.shape[1])
    if (in_h, in_w) == (out_h, out_w):
        return frame
    key = (in_h, in_w, out_h, out_w, kind, str(frame.device))
    tabs = _RESIZE_TABLES.get(key)
    if tabs is None:
        bx, kx = resample_coeffs(in_w, out_w, kind)
        by, ky = resample_coeffs(in_h, out_h, kind)
        tabs = tuple(torch.from_numpy(a).to(frame.device) for a in (kx, bx, ky, by))
        if len(_RESIZE_TABLES) > 32:
            _RESIZE_TABLES.pop(next(iter(_RESIZE_TABLES)))
        _RESIZE_TABLES[key] = tabs
    kx, bx, ky, by = tabs
    tmp = torch.empty((in_h, out_w, 3), dtype=torch.uint8, device=frame.device)
    dst = torch.empty((out_h, out_w, 3), dtype=torch.uint8, device=frame.device)
    rc = load().vis_resize_rgb_u8(_ptr(frame), _ptr(tmp), _ptr(dst), in_h, in_w, out_h, out_w, _ptr(kx), _ptr(bx),
                                  kx.shape[1], _ptr(ky), _ptr(by), ky.shape[1], _stream())
    _check(rc, "vis_resize_rgb_u8")
    return dst


def jpeg_to_rgb(coeffs: torch.Tensor, qt: torch.Tensor, jc) -> torch.Tensor:
    """Entropy-decoded JPEG (jpeg.JpegCoeffs geometry; ``coeffs`` int16 [total_blocks, 64] and ``qt`` int32 [3, 64] on the
    device) -> uint8 [H, W, 3]: dequantise + integer IDCT per block, triangle chroma upsampling, fixed-point YCbCr -> RGB,
    bit-exact with libjpeg-turbo / PIL."""
    if coeffs.dtype != torch.int16 or coeffs.dim() != 2 or coeffs.shape[1] != 64 or not coeffs.is_contiguous():
        raise HipLibraryError("jpeg_to_rgb: contiguous int16 [blocks, 64] coefficients required")
    if qt.dtype != torch.int32 or qt.numel() != 192 or not qt.is_contiguous():
        raise HipLibraryError("jpeg_to_rgb: int32 [3, 64] quantisation tables required")
    n = jc.ncomp
    bw_c, bh_c, dw_c, dh_c = (jc.bw[1], jc.bh[1], jc.dw[1], jc.dh[1]) if n == 3 else (0, 0, 0, 0)
    total = jc.bw[0] * jc.bh[0] + 2 * bw_c * bh_c
    if coeffs.shape[0] != total:
        raise HipLibraryError(f"jpeg_to_rgb: {coeffs.shape[0]} coefficient blocks, geometry says {total}")
    planes = torch.empty(total * 64, dtype=torch.uint8, device=coeffs.device)
    rgb = torch.empty((jc.height, jc.width, 3), dtype=torch.uint8, device=coeffs.device)
    rc = load().vis_jpeg_to_rgb(_ptr(coeffs), _ptr(qt), _ptr(planes), _ptr(rgb), jc.width, jc.height, n, jc.hs[0], jc.vs[0],
                                jc.bw[0], jc.bh[0], bw_c, bh_c, dw_c, dh_c, _stream())
    _check(rc, "vis_jpeg_to_rgb")
    return rgb


def image_stats(frame: torch.Tensor):
    """uint8 device frame [H, W, 3] -> (sum gray, sum laplacian, sum laplacian^2) as Python ints (exact)."""
    if frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[2] != 3 or not frame.is_contiguous():
        raise HipLibraryError("image_stats: contiguous uint8 [H, W, 3] frame required")
    stats = torch.empty(3, dtype=torch.int64, device=frame.device)
    rc = load().vis_image_stats_u8(_ptr(frame), frame.shape[0], frame.shape[1], _ptr(stats), _stream())
    _check(rc, "vis_image_stats_u8")
    return tuple(int(v) for v in stats.cpu().tolist())


def patchify_tiles(frame: torch.Tensor, out: torch.Tensor, tiles_h: int, tiles_w: int, tile: int, mean, std) -> None:
    """mllama: resized uint8 [H, W, 3] frame -> patch rows of the (zero-padded) tiles_h x tiles_w canvas."""
    if frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[2] != 3 or not frame.is_contiguous():
        raise HipLibraryError("patchify_tiles: contiguous uint8 [H, W, 3] frame required")
    _bf16(out, "patchify_tiles out")
    per = (tile // 14) ** 2 + 1
    if out.dim() != 2 or out.shape[0] < tiles_h * tiles_w * per or out.stride(1) != 1:
        raise HipLibraryError("patchify_tiles: output too small")
    m = (ctypes.c_float * 3)(*mean)
    sd = (ctypes.c_float * 3)(*std)
    rc = load().vis_patchify_tiles_u8(_ptr(frame), _ptr(out), frame.shape[0], frame.shape[1], tiles_h, tiles_w, tile,
                                      out.stride(0), ctypes.cast(m, ctypes.c_void_p), ctypes.cast(sd, ctypes.c_void_p),
                                      _stream())
    _check(rc, "vis_patchify_tiles_u8")


def add_rows(x: torch.Tensor, table: torch.Tensor, idx: torch.Tensor) -> None:
    """x[i] += table[idx[i]] (bf16 rows, int32 device indices)."""
    _bf16(x, "add_rows x"); _bf16(table, "add_rows table")
    if idx.dtype != torch.int32 or idx.numel() != x.shape[0] or table.shape[1] != x.shape[1] or x.stride(1) != 1 \
            or not table.is_contiguous():
        raise HipLibraryError("add_rows: bad shapes")
    rc = load().vis_add_rows_bf16(_ptr(x), _ptr(table), _ptr(idx), x.shape[0], x.shape[1], x.stride(0),
                                  table.shape[0], _stream())
    _check(rc, "vis_add_rows_bf16")


def _cross_q_out(name, q, out, nkeys_m1, part_o, part_ml, n_q, head_dim, nsplit, B) -> None:
    """The q / out / count / workspace checks of the single (B None) and batch forms of either key format."""
    _bf16(q, "q")
    if B is None:
        bad = q.numel() != n_q * head_dim or out.numel() != n_q * head_dim or nkeys_m1.dtype != torch.int32
    else:
        bad = q.shape[1] != n_q * head_dim or q.stride(1) != 1 or out.shape != (B, n_q * head_dim) or not out.is_contiguous() \
            or nkeys_m1.dtype != torch.int32 or nkeys_m1.numel() != B
    if bad:
        raise HipLibraryError(f"{name}: bad q/out/nkeys")
    if part_o.numel() < (B or 1) * n_q * nsplit * head_dim or part_ml.numel() < (B or 1) * n_q * nsplit * 2:
        raise HipLibraryError(f"{name}: workspace too small")


def _cross_bf16_kv(name, k, v, lead, n_kv, head_dim) -> None:
    """bf16 keys / values [Hkv, T, D] behind ``lead`` batch dims (0 or 1; a batch may have any stride, the same for k and v)."""
    _bf16(k, "k"); _bf16(v, "v")
    if k.dim() != lead + 3 or k.shape != v.shape or k.shape[lead] != n_kv or k.shape[lead + 2] != head_dim \
            or not all((t[0] if lead else t).is_contiguous() for t in (k, v)) or (lead and k.stride(0) != v.stride(0)):
        raise HipLibraryError(f"{name}: bad k/v")


def decode_cross_attn(q: torch.Tensor, q_norm_w: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                      nkeys_m1: torch.Tensor, part_o: torch.Tensor, part_ml: torch.Tensor, out: torch.Tensor,
                      n_q: int, n_kv: int, head_dim: int, nsplit: int, scale: float, eps: float) -> None:
    """One new token's cross-attention over static keys/values k, v [Hkv, T, 128] (q_norm applied inside)."""
    _cross_bf16_kv("decode_cross_attn", k, v, 0, n_kv, head_dim)
    _cross_q_out("decode_cross_attn", q, out, nkeys_m1, part_o, part_ml, n_q, head_dim, nsplit, None)
    rc = load().vis_decode_cross_attn(_ptr(q), _ptr(q_norm_w), _ptr(k), _ptr(v), _ptr(nkeys_m1), _ptr(part_o),
                                      _ptr(part_ml), _ptr(out), n_q, n_kv, head_dim, k.shape[1], nsplit, scale, eps,
                                      _stream())
    _check(rc, "vis_decode_cross_attn")


def decode_cross_attn_batch(q: torch.Tensor, q_norm_w: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                            nkeys_m1: torch.Tensor, part_o: torch.Tensor, part_ml: torch.Tensor, out: torch.Tensor,
                            n_q: int, n_kv: int, head_dim: int, nsplit: int, scale: float, eps: float) -> None:
    """Batch of B new tokens, each over ITS OWN static keys/values: q [B, Hq*128], k / v [B, Hkv, T, 128] (any batch
    stride), nkeys_m1 [B] int32, out [B, Hq*128]."""
    B = q.shape[0]
    _cross_bf16_kv("decode_cross_attn_batch", k, v, 1, n_kv, head_dim)
    if k.shape[0] != B:
        raise HipLibraryError("decode_cross_attn_batch: bad k/v")
    _cross_q_out("decode_cross_attn_batch", q, out, nkeys_m1, part_o, part_ml, n_q, head_dim, nsplit, B)
    rc = load().vis_decode_cross_attn_batch(_ptr(q), _ptr(q_norm_w), _ptr(k), _ptr(v), _ptr(nkeys_m1), _ptr(part_o),
                                            _ptr(part_ml), _ptr(out), n_q, n_kv, head_dim, k.shape[2], nsplit, scale, eps,
                                            B, q.stride(0), k.stride(0), _stream())
    _check(rc, "vis_decode_cross_attn_batch")


def quantize_cross_kv(x: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor) -> None:
    """The fp8 copy of static cross-attention keys or values: bf16 [..., 128] contiguous -> e4m3 codes (uint8, same shape) and
    one f32 scale per row (shape without the last dim), by vis_quant_rows_fp8 without a norm: scale = max(amax / 448, 1e-12),
    an all-zero row gets scale 1e-12 and codes 0."""
    _bf16(x, "quantize_cross_kv x")
    if x.shape[-1] != 128 or codes.dtype != torch.uint8 or codes.shape != x.shape or scales.dtype != torch.float32 \
            or scales.shape != x.shape[:-1] or not (x.is_contiguous() and codes.is_contiguous() and scales.is_contiguous()):
        raise HipLibraryError("quantize_cross_kv: bad shapes")
    quant_rows_fp8(x.view(-1, 128), codes.view(-1, 128), scales.view(-1))


def _cross_fp8_kv(name, kq, ksc, vq, vsc, lead, n_kv, head_dim) -> None:
    """fp8 keys / values behind ``lead`` batch dims (0 or 1): uint8 codes [Hkv, T, D], f32 row scales [Hkv, T], T a multiple of
    64, each sequence's arrays contiguous (a batch may have any stride, one for the codes and one for the scales)."""
    if kq.dtype != torch.uint8 or vq.dtype != torch.uint8 or ksc.dtype != torch.float32 or vsc.dtype != torch.float32:
        raise HipLibraryError(f"{name}: uint8 codes and f32 scales required")
    if kq.dim() != lead + 3 or kq.shape != vq.shape or kq.shape[lead] != n_kv or kq.shape[lead + 2] != head_dim \
            or ksc.shape != kq.shape[:-1] or vsc.shape != kq.shape[:-1] or kq.shape[lead + 1] % DECODE_KEYS_PER_SPLIT \
            or not all((t[0] if lead else t).is_contiguous() for t in (kq, vq, ksc, vsc)) \
            or (lead and (kq.stride(0) != vq.stride(0) or ksc.stride(0) != vsc.stride(0))):
        raise HipLibraryError(f"{name}: bad codes/scales")


def decode_cross_attn_fp8(q: torch.Tensor, q_norm_w: torch.Tensor, kq: torch.Tensor, ksc: torch.Tensor, vq: torch.Tensor,
                          vsc: torch.Tensor, nkeys_m1: torch.Tensor, part_o: torch.Tensor, part_ml: torch.Tensor,
                          out: torch.Tensor, n_q: int, n_kv: int, head_dim: int, nsplit: int, scale: float,
                          eps: float) -> None:
    """decode_cross_attn over fp8 keys / values: codes kq, vq [Hkv, T, 128] uint8 with row scales ksc, vsc [Hkv, T] f32
    (T a multiple of 64)."""
    _cross_fp8_kv("decode_cross_attn_fp8", kq, ksc, vq, vsc, 0, n_kv, head_dim)
    _cross_q_out("decode_cross_attn_fp8", q, out, nkeys_m1, part_o, part_ml, n_q, head_dim, nsplit, None)
    rc = load().vis_decode_cross_attn_fp8(_ptr(q), _ptr(q_norm_w), _ptr(kq), _ptr(ksc), _ptr(vq), _ptr(vsc), _ptr(nkeys_m1),
                                          _ptr(part_o), _ptr(part_ml), _ptr(out), n_q, n_kv, head_dim, kq.shape[1], nsplit,
                                          scale, eps, _stream())
    _check(rc, "vis_decode_cross_attn_fp8")


def decode_cross_attn_fp8_batch(q: torch.Tensor, q_norm_w: torch.Tensor, kq: torch.Tensor, ksc: torch.Tensor,
                                vq: torch.Tensor, vsc: torch.Tensor, nkeys_m1: torch.Tensor, part_o: torch.Tensor,
                                part_ml: torch.Tensor, out: torch.Tensor, n_q: int, n_kv: int, head_dim: int, nsplit: int,
                                scale: float, eps: float) -> None:
    """Batch of B new tokens, each over ITS OWN fp8 keys / values: q [B, Hq*128], codes [B, Hkv, T, 128], scales [B, Hkv, T]
    (any batch stride, the same for K and V), nkeys_m1 [B] int32, out [B, Hq*128]."""
    B = q.shape[0]
    _cross_fp8_kv("decode_cross_attn_fp8_batch", kq, ksc, vq, vsc, 1, n_kv, head_dim)
    if kq.shape[0] != B:
        raise HipLibraryError("decode_cross_attn_fp8_batch: bad codes/scales")
    _cross_q_out("decode_cross_attn_fp8_batch", q, out, nkeys_m1, part_o, part_ml, n_q, head_dim, nsplit, B)
    rc = load().vis_decode_cross_attn_fp8_batch(_ptr(q), _ptr(q_norm_w), _ptr(kq), _ptr(ksc), _ptr(vq), _ptr(vsc),
                                                _ptr(nkeys_m1), _ptr(part_o), _ptr(part_ml), _ptr(out), n_q, n_kv, head_dim,
                                                kq.shape[2], nsplit, scale, eps, B, q.stride(0), kq.stride(0), ksc.stride(0),
                                                _stream())
    _check(rc, "vis_decode_cross_attn_fp8_batch")


def _cross_draft_rows(name, q, out, nkeys_m1, part_o, part_ml, n_q, head_dim, nsplit) -> int:
    """The checks the two draft forms share -> the number of rows R."""
    _bf16(q, "q"); _bf16(out, "out")
    if q.dim() != 2 or not 1 <= q.shape[0] <= SPEC_MAX_ROWS or q.shape[1] != n_q * head_dim or q.stride(1) != 1 \
            or (q.shape[0] > 1 and q.stride(0) < n_q * head_dim):
        raise HipLibraryError(f"{name}: q must be [1..4, Hq * D] (rows of a wider buffer allowed)")
    R = q.shape[0]
    if out.shape != (R, n_q * head_dim) or not out.is_contiguous() or nkeys_m1.dtype != torch.int32 or nkeys_m1.numel() != 1:
        raise HipLibraryError(f"{name}: bad out/nkeys")
    if part_o.numel() < R * n_q * nsplit * head_dim or part_ml.numel() < R * n_q * nsplit * 2:
        raise HipLibraryError(f"{name}: workspace too small")
    return R


def decode_cross_attn_draft(q: torch.Tensor, q_norm_w: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                            nkeys_m1: torch.Tensor, part_o: torch.Tensor, part_ml: torch.Tensor, out: torch.Tensor,
                            n_q: int, n_kv: int, head_dim: int, nsplit: int, scale: float, eps: float) -> None:
    """decode_cross_attn for the R = 1..4 rows of ONE sequence's speculative step (vis_decode_cross_attn_draft): q [R, Hq*128]
    (a column slice of wider rows is fine), all rows over the same keys / values k, v [Hkv, T, 128] and the one count
    nkeys_m1 [1]; out [R, Hq*128]; workspaces R x the single-row ones.  R * (Hq / Hkv) <= 16, or the library refuses.  Row r
    is bit-identical to decode_cross_attn on q[r] alone."""
    _cross_bf16_kv("decode_cross_attn_draft", k, v, 0, n_kv, head_dim)
    R = _cross_draft_rows("decode_cross_attn_draft", q, out, nkeys_m1, part_o, part_ml, n_q, head_dim, nsplit)
    rc = load().vis_decode_cross_attn_draft(_ptr(q), _ptr(q_norm_w), _ptr(k), _ptr(v), _ptr(nkeys_m1), _ptr(part_o),
                                            _ptr(part_ml), _ptr(out), n_q, n_kv, head_dim, k.shape[1], nsplit, scale, eps,
                                            R, q.stride(0), _stream())
    _check(rc, "vis_decode_cross_attn_draft")


def decode_cross_attn_fp8_draft(q: torch.Tensor, q_norm_w: torch.Tensor, kq: torch.Tensor, ksc: torch.Tensor,
                                vq: torch.Tensor, vsc: torch.Tensor, nkeys_m1: torch.Tensor, part_o: torch.Tensor,
                                part_ml: torch.Tensor, out: torch.Tensor, n_q: int, n_kv: int, head_dim: int, nsplit: int,
                                scale: float, eps: float) -> None:
    """decode_cross_attn_draft over fp8 keys / values (decode_cross_attn_fp8's operands): row r is bit-identical to
    decode_cross_attn_fp8 on q[r] alone."""
    _cross_fp8_kv("decode_cross_attn_fp8_draft", kq, ksc, vq, vsc, 0, n_kv, head_dim)
    R = _cross_draft_rows("decode_cross_attn_fp8_draft", q, out, nkeys_m1, part_o, part_ml, n_q, head_dim, nsplit)
    rc = load().vis_decode_cross_attn_fp8_draft(_ptr(q), _ptr(q_norm_w), _ptr(kq), _ptr(ksc), _ptr(vq), _ptr(vsc),
                                                _ptr(nkeys_m1), _ptr(part_o), _ptr(part_ml), _ptr(out), n_q, n_kv, head_dim,
                                                kq.shape[1], nsplit, scale, eps, R, q.stride(0), _stream())
    _check(rc, "vis_decode_cross_attn_fp8_draft")


def patchify(img_u8: torch.Tensor, out: torch.Tensor, row0: int, mean, std) -> None:
    """img_u8 [H,W,3] uint8 (device) -> out[row0 + p, :] normalised bf16 patch rows."""
    if img_u8.dtype != torch.uint8 or img_u8.dim() != 3 or img_u8.shape[2] != 3 or not img_u8.is_contiguous():
        raise HipLibraryError("patchify: uint8 [H,W,3] contiguous required")
    H, W, _ = img_u8.shape
    n = (H // 14) * (W // 14)
    if row0 + n > out.shape[0]:
        raise HipLibraryError("patchify: output too small")
    for i in range(3):
        _MEAN[i] = mean[i]
        _STD[i] = std[i]
    rc = load().vis_patchify_u8(_ptr(img_u8), _ptr(out), H, W, out.stride(0), row0,
                                ctypes.cast(_MEAN, ctypes.c_void_p), ctypes.cast(_STD, ctypes.c_void_p), _stream())
    _check(rc, "vis_patchify_u8")


def gather_rows(table: torch.Tensor, ids: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    if ids.dtype != torch.int32 or not table.is_contiguous() or not out.is_contiguous():
        raise HipLibraryError("gather_rows: int32 ids and contiguous tensors required")
    rc = load().vis_gather_rows(_ptr(table), _ptr(ids), _ptr(out), ids.numel(), table.shape[1], table.shape[0],
                                _stream())
    _check(rc, "vis_gather_rows")
    return out


def scatter_rows(src: torch.Tensor, idx: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    if idx.dtype != torch.int32 or not src.is_contiguous() or not dst.is_contiguous():
        raise HipLibraryError("scatter_rows: int32 idx and contiguous tensors required")
    rc = load().vis_scatter_rows(_ptr(src), _ptr(idx), _ptr(dst), idx.numel(), src.shape[1], dst.shape[0],
                                 _stream())
    _check(rc, "vis_scatter_rows")
    return dst
