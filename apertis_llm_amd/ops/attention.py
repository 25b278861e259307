"""standard_mha: interleaved-pair RoPE over the full width and causal softmax attention (flash style).

Part of apertis_llm_amd.ops.  torch is used for device memory, streams and autograd bookkeeping only; every computation is a
HIP kernel launch through apertis_llm_amd._lib (csrc/attention.hip).  Tensors must live on a ROCm device.
"""
import torch

from .. import _lib
from .._lib import ApertisHipError, dtype_code, ptr, stream_ptr
from ._base import _launch, _require_gpu, _rows

# the model's standard_mha layers take the fused path below (RoPE + attention kernels) when this is on and the call qualifies
# (ApertisAttention._fused_ok); off: the stock torch attention everywhere (A/B and tests)
ATTN_FUSED = True


def _positions(position_ids, B, L, max_pos):
    """(int64 tensor or None, batch stride).  Explicit positions are range-checked here, on the host: the stock module's
    cos_cached[position_ids] raises IndexError for them, so this does too (one sync; the model passes None for its own
    arange positions)."""
    if position_ids is None:
        if L > max_pos:
            raise IndexError(f"sequence length {L} exceeds the rotary table ({max_pos} positions)")
        return None, 0
    pos = position_ids
    if pos.dim() == 1:
        pos = pos.unsqueeze(0)
    if pos.dim() != 2 or pos.shape[-1] != L or pos.shape[0] not in (1, B):
        raise ApertisHipError(f"position_ids of shape {tuple(position_ids.shape)} for q of [{B}, {L}, ...]")
    if pos.dtype != torch.int64 or pos.stride(-1) != 1:
        pos = pos.to(torch.int64).contiguous()
    if pos.numel():
        lo, hi = torch.aminmax(pos)
        lo, hi = int(lo), int(hi)
        if lo < -max_pos or hi >= max_pos:            # (negative positions wrap, as torch indexing wraps them)
            raise IndexError(f"position_ids in [{lo}, {hi}] outside the rotary table of {max_pos} positions")
    return pos, (pos.stride(0) if pos.shape[0] > 1 else 0)


class _RopeQK(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, pos, pos_bs, cos, sin):
        lib = _lib.load()
        B, L, W = q.shape
        q, q_rs = _rows(q, W)
        k, k_rs = _rows(k, W)
        qo = torch.empty(B, L, W, device=q.device, dtype=q.dtype)
        ko = torch.empty(B, L, W, device=q.device, dtype=q.dtype)
        _launch("apertis_rope_qk_fwd", lib.apertis_rope_qk_fwd,
                (ptr(q), q_rs, ptr(k), k_rs, ptr(pos), pos_bs, ptr(cos), ptr(sin), cos.shape[0], ptr(qo), ptr(ko), B, L, W,
                 dtype_code(q), stream_ptr()), work=4.0 * B * L * W * q.element_size())
        ctx.save_for_backward(pos, cos, sin)
        ctx.pos_bs = pos_bs
        return qo, ko

    @staticmethod
    def backward(ctx, gq, gk):
        lib = _lib.load()
        pos, cos, sin = ctx.saved_tensors
        B, L, W = gq.shape
        gq, gq_rs = _rows(gq, W)
        gk, gk_rs = _rows(gk, W)
        dq = torch.empty(B, L, W, device=gq.device, dtype=gq.dtype)
        dk = torch.empty(B, L, W, device=gq.device, dtype=gq.dtype)
        _launch("apertis_rope_qk_bwd", lib.apertis_rope_qk_bwd,
                (ptr(gq), gq_rs, ptr(gk), gk_rs, ptr(pos), ctx.pos_bs, ptr(cos), ptr(sin), cos.shape[0], ptr(dq), ptr(dk), B, L,
                 W, dtype_code(gq), stream_ptr()), work=4.0 * B * L * W * gq.element_size())
        return dq, dk, None, None, None, None


def rope_qk(q, k, position_ids, cos, sin):
    """RotaryEmbedding.forward applied to q and k [B, L, W] in one launch (reference core.py:258-293: interleaved pairs over the
    FULL width).  cos / sin: the module's fp32 cos_cached / sin_cached [max_pos, W/2]; position_ids int64 [1 or B, L] or None
    (positions 0..L-1).  Bit-identical to the stock module for fp32 and bf16; q and k share a shape and a dtype."""
    _require_gpu(q, k, position_ids, cos, sin)
    if q.shape != k.shape or q.dtype != k.dtype or q.dim() != 3:
        raise ApertisHipError(f"rope_qk: q {tuple(q.shape)} {q.dtype} and k {tuple(k.shape)} {k.dtype} must match, [B, L, W]")
    B, L, W = q.shape
    if cos.dtype != torch.float32 or sin.dtype != torch.float32 or cos.shape != sin.shape or 2 * cos.shape[-1] != W:
        raise ApertisHipError(f"rope_qk: cos/sin must be fp32 [max_pos, {W // 2}]")
    pos, pos_bs = _positions(position_ids, B, L, cos.shape[0])
    return _RopeQK.apply(q, k, pos, pos_bs, cos.contiguous(), sin.contiguous())


def _attn_flops(B, L, H, D):
    """Causal forward: 4*B*H*D*L(L+1)/2 (two products over the lower triangle)."""
    return 4.0 * B * H * D * L * (L + 1) / 2


class _CausalAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, heads, key_valid, p, seed):
        lib = _lib.load()
        B, L, W = q.shape
        D = W // heads
        q, q_rs = _rows(q, W)
        k, k_rs = _rows(k, W)
        v, v_rs = _rows(v, W)
        out = torch.empty(B, L, W, device=q.device, dtype=q.dtype)
        lse = torch.empty(B, heads, L, device=q.device, dtype=torch.float32)
        _launch("apertis_attention_fwd", lib.apertis_attention_fwd,
                (ptr(q), q_rs, ptr(k), k_rs, ptr(v), v_rs, ptr(key_valid), ptr(out), W, ptr(lse), B, L, heads, D, p, seed,
                 dtype_code(q), stream_ptr()), work=_attn_flops(B, L, heads, D))
        ctx.save_for_backward(q, k, v, out, lse, key_valid)
        ctx.cfg = (heads, p, seed)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        q, k, v, out, lse, key_valid = ctx.saved_tensors
        heads, p, seed = ctx.cfg
        B, L, W = q.shape
        D = W // heads
        dout = dout.to(q.dtype)
        dout, do_rs = _rows(dout, W)
        if dout.data_ptr() % 16:
            dout = dout.clone()
        ws = torch.empty(lib.apertis_attention_bwd_workspace_bytes(B, L, heads) // 4, device=q.device, dtype=torch.float32)
        dq = torch.empty(B, L, W, device=q.device, dtype=q.dtype)
        dk = torch.empty_like(dq)
        dv = torch.empty_like(dq)
        _launch("apertis_attention_bwd", lib.apertis_attention_bwd,
                (ptr(q), q.stride(-2), ptr(k), k.stride(-2), ptr(v), v.stride(-2), ptr(out), W, ptr(dout), do_rs, ptr(lse),
                 ptr(key_valid), ptr(ws), ptr(dq), ptr(dk), ptr(dv), W, B, L, heads, D, p, seed, dtype_code(q), stream_ptr()),
                work=2.5 * _attn_flops(B, L, heads, D))
        return dq, dk, dv, None, None, None, None


def attention_supported(q, heads):
    """Whether causal_attention takes q [B, L, heads*D] of this dtype and head dim (D 64 or 128, fp32 or bf16)."""
    return (q.dim() == 3 and q.shape[-1] % heads == 0 and q.shape[-1] // heads in (64, 128)
            and q.dtype in (torch.float32, torch.bfloat16))


def causal_attention(q, k, v, heads, key_valid=None, dropout_p=0.0, training=False):
    """softmax(Q K^T / sqrt(D) + causal and key-padding mask) V per head, with attention dropout in training.
    q, k, v: [B, L, heads*D] (head h in columns [h*D, (h+1)*D)), one dtype, fp32 or bf16, D in {64, 128}; returns O in the same
    layout (out_proj reads it directly).  key_valid: [B, L] (the raw attention_mask, nonzero = attend) or None.  Dropout keeps
    element (i, j) of head (b, h) by the library's counter hash with a seed drawn from torch's RNG here (a checkpointed
    recompute draws the same one); the backward regenerates the mask.  Saved for the backward: q, k, v, O and LSE [B, heads, L]
    fp32, never an L x L tensor."""
    _require_gpu(q, k, v, key_valid)
    if not (q.shape == k.shape == v.shape and q.dtype == k.dtype == v.dtype) or not attention_supported(q, heads):
        raise ApertisHipError(f"causal_attention: q/k/v {tuple(q.shape)} {q.dtype} with {heads} heads (D 64 or 128, fp32 or bf16, "
                              "one shape and dtype)")
    B, L, _ = q.shape
    if key_valid is not None:
        if tuple(key_valid.shape) != (B, L):
            raise ApertisHipError(f"causal_attention: key_valid {tuple(key_valid.shape)}, expected ({B}, {L})")
        if key_valid.dtype != torch.int64 or not key_valid.is_contiguous():
            key_valid = key_valid.to(torch.int64).contiguous()
    p = float(dropout_p) if training else 0.0
    if not 0.0 <= p < 1.0:
        raise ApertisHipError(f"causal_attention: dropout_p {dropout_p} outside [0, 1)")
    seed = int(torch.empty((), dtype=torch.int64).random_().item()) if p > 0 else 0
    return _CausalAttention.apply(q, k, v, int(heads), key_valid, p, seed)
