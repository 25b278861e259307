"""SwiGLU feed-forward: gate and up projection as ONE GEMM, the gate kernel, the down projection - one autograd node.

Part of apertis_llm_amd.ops (`from apertis_llm_amd import ops` exposes every name as for the other modules).
torch is used for device memory, streams and autograd bookkeeping only; every computation is a HIP kernel launch through
apertis_llm_amd._lib.  Tensors must live on a ROCm device.
"""
import os as _os

import torch

from .. import _lib
from .._lib import dtype_code, ptr, stream_ptr
from ._base import _apply, _grad_wanted, _launch, _require_gpu
from .prep import cast_transpose
from . import gemm as _gemm
from .gemm import _RowsWork, _dense_tag, _launch_nt, _tn_workspace, dense_offsets
from .moe import grad_destination


# APERTIS_SWIGLU_FUSED=0: model.SwiGLUFFN keeps its stock-torch line (three nn.Linear calls, F.silu, a multiply)
SWIGLU_FUSED = _os.environ.get("APERTIS_SWIGLU_FUSED", "1") == "1"


def _autocast_or(dtype):
    if torch.is_autocast_enabled():
        dt = torch.get_autocast_dtype("cuda")
        return torch.bfloat16 if dt in (torch.bfloat16, torch.float16) else dt
    return dtype


def swiglu_supported(x, F):
    """What swiglu_mlp takes: a ROCm tensor [..., H] with at least one row, computed in fp32 or bf16 (the autocast dtype, else
    x's own), H and F multiples of 8 (16-byte bf16 rows for the GEMMs and the gate kernel) - and the switch on."""
    H = x.shape[-1] if x.dim() else 0
    return bool(SWIGLU_FUSED and x.is_cuda and _autocast_or(x.dtype) in (torch.float32, torch.bfloat16)
                and H > 0 and H % 8 == 0 and F > 0 and F % 8 == 0 and x.numel() >= H)


def _weight_copies(w, cd, need):
    """(plain, transposed) compute copies of a 2-D master weight as one group, the way _GroupedLinear takes them."""
    w3 = w.unsqueeze(0)
    if cd == torch.float32 and w.dtype == torch.float32 and w.is_contiguous():
        return w3.detach(), (cast_transpose(w3, cd, want_plain=False)[1] if need else None)
    return cast_transpose(w3, cd, want_transposed=need, cache=not need)


def _dense_nt(lib, a, w, out, rows, N, K, code):
    """out[rows, N] = a[rows, K] @ w[0, N, :K].T: one group, no bias, no activation - which kernel is launch_nt's decision."""
    offsets = dense_offsets(rows, a.device)
    _launch_nt("apertis_grouped_gemm_nt[dense]", lib,
               (ptr(a), ptr(w), None, ptr(offsets), ptr(out), None, None, rows, N, K, w.shape[-1], 1, _lib.ACT_NONE, 0.0, 0,
                code, code, stream_ptr()), _RowsWork(offsets, 1, 2.0 * N * K), a.device,
               *_dense_tag(1, rows, N, K, a.element_size()))


class _SwiGLUMLP(torch.autograd.Function):
    """y = (silu(g) * u) @ w_down.T with [g | u] = x @ w_gu.T, as ONE autograd node: the forward keeps x and gu only, the
    backward's gate kernel re-forms h next to dgu and both weight gradients leave in one launch."""

    @staticmethod
    def forward(ctx, x, w_gu, w_down, cd):
        _require_gpu(x, w_gu, w_down)
        lib = _lib.load()
        x = x.to(cd).contiguous()
        T, H = x.shape
        F = w_down.shape[1]
        if tuple(w_gu.shape) != (2 * F, H) or tuple(w_down.shape) != (H, F):
            raise _lib.ApertisHipError(f"swiglu_mlp: x {tuple(x.shape)}, w_gu {tuple(w_gu.shape)}, w_down {tuple(w_down.shape)}")
        need = _grad_wanted(ctx, 3)
        wgu_c, wgu_t = _weight_copies(w_gu, cd, need)
        wd_c, wd_t = _weight_copies(w_down, cd, need)
        code, dev = dtype_code(x), x.device
        gu = torch.empty(T, 2 * F, device=dev, dtype=cd)
        _dense_nt(lib, x, wgu_c, gu, T, 2 * F, H, code)
        h = torch.empty(T, F, device=dev, dtype=cd)
        _launch("apertis_swiglu_fwd", lib.apertis_swiglu_fwd, (ptr(gu), ptr(h), T, F, code, stream_ptr()),
                3.0 * T * F * x.element_size())
        y = torch.empty(T, H, device=dev, dtype=cd)
        _dense_nt(lib, h, wd_c, y, T, H, F, code)
        if need:
            ctx.save_for_backward(x, gu, wgu_t, wd_t)
            ctx.cfg = (T, H, F, w_gu.dtype, w_down.dtype)
            ctx.w_down = w_down     # for grad_destination() in the backward
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, gu, wgu_t, wd_t = ctx.saved_tensors
        T, H, F, gu_dt, down_dt = ctx.cfg
        code, dev = dtype_code(x), x.device
        dy = dy.to(x.dtype).contiguous()
        want_w = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        dh = torch.empty(T, F, device=dev, dtype=x.dtype)
        _dense_nt(lib, dy, wd_t, dh, T, F, H, code)
        dgu = torch.empty_like(gu)
        h = torch.empty_like(dh) if want_w else None
        _launch("apertis_swiglu_bwd", lib.apertis_swiglu_bwd, (ptr(dh), ptr(gu), ptr(dgu), ptr(h), T, F, code, stream_ptr()),
                (6.0 if want_w else 5.0) * T * F * x.element_size())
        dx = dw_gu = dw_down = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _dense_nt(lib, dgu, wgu_t, dx, T, H, 2 * F, code)
        if want_w:
            # both weight gradients in ONE launch: dW_down = dy^T h, dW_gu = dgu^T x
            offsets = dense_offsets(T, dev)
            dw_down = grad_destination(ctx.w_down, (H, F), dev)
            dw_gu = torch.empty(2 * F, H, device=dev, dtype=torch.float32)
            ws, ws_bytes = _tn_workspace(1, 2, dev, T)
            _launch("apertis_grouped_gemm_tn", lib.apertis_grouped_gemm_tn_pair_q,
                    (ptr(dy), ptr(h), ptr(dw_down), None, H, F, ptr(dgu), ptr(x), ptr(dw_gu), None, 2 * F, H, ptr(offsets), T, 1,
                     ptr(ws), ws_bytes, code, int(_gemm.GEMM_DYNAMIC_QUEUE and _gemm.TN_DYNAMIC_QUEUE), stream_ptr()),
                    _RowsWork(offsets, 1, 6.0 * F * H))
            dw_gu, dw_down = dw_gu.to(gu_dt), dw_down.to(down_dt)
        return dx, dw_gu, dw_down, None


def swiglu_mlp(x, w_gu, w_down, compute_dtype=None):
    """SwiGLU feed-forward (reference core.py:925-993): w_down(silu(w_gate x) * w_up x) for rows x [T, H]; w_gu [2F, H] is
    the row-stacked [w_gate; w_up] (fp32 master, or the TrainPrep placeholder of that stack), w_down [H, F].  Splitting w_gu's
    gradient back into the two parameters is the job of whatever built it (torch.cat's backward, the placeholder's)."""
    return _apply(_SwiGLUMLP, x, w_gu, w_down, compute_dtype or x.dtype)
