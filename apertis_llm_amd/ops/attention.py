"""standard_mha: interleaved-pair RoPE over the full width, causal softmax attention (flash style), and decode against a
preallocated KV cache (KVCache): single-token steps (kv_append_rope, attention_decode) and multi-token steps
(kv_append_rope_chunk, attention_chunk); the dead query rows of a left-padded batch (attention_dead_rows).  The vision tower's
bidirectional attention (full_attention, full_attention_qkv: the same kernels with the diagonal compiled out).  Packed rows
(document_layout, document_attention: the causal kernels under a document mask, with the tiles of other documents skipped).
Sliding windows, opt-in (ATTN_WINDOW; window_attention, window_layout, attention_decode(window=): the causal kernels with
bounds computed from the query index, packed rows on a clipped layout, a decode step that reads the last W cache rows; and,
under ATTN_WINDOW_CACHE on top, the device-length step and the chunk step past the window: KVCache.step_state_begin(window=),
attention_chunk(window=)).  KV-cache slots with a length per row, opt-in (ATTN_SLOTS; KVCache.slots_begin,
kv_append_rope_slots, attention_decode_slots: generate_many() of a standard_mha model).

Part of apertis_llm_amd.ops.  torch is used for device memory, streams and autograd bookkeeping only; every computation is a
HIP kernel launch through apertis_llm_amd._lib (csrc/attention.hip, csrc/attention_decode.hip, csrc/attention_deadrows.hip).
Tensors must live on a ROCm device.
"""
import os

import torch

from .. import _lib
from .._lib import ApertisHipError, dtype_code, ptr, stream_ptr
from ._base import _launch, _require_gpu, _rows

# the model's standard_mha layers take the fused path below (RoPE + attention kernels) when this is on and the call qualifies
# (ApertisAttention._fused_ok); off: the stock torch attention everywhere (A/B and tests)
ATTN_FUSED = True
# a batch whose key 0 is masked in some sequence (left padding) takes the fused / chunk / decode kernels too, inference only:
# its dead query rows - no valid key at or before their own position - are filled in by attention_dead_rows below.  OFF by
# default (APERTIS_MHA_LEFT_PAD=1 turns it on): tests pin that such a batch runs the stock path under the default switches
ATTN_LEFT_PAD = os.environ.get("APERTIS_MHA_LEFT_PAD", "0") == "1"
# a standard_mha model honours `config.sliding_window` (query i attends the last W keys, its own included) on every path:
# window_attention, document_attention on a clipped layout, attention_decode(window=), a band on the stock branch.  OFF by
# default (APERTIS_MHA_WINDOW=1 turns it on): the reference never reads the field, and neither does the default path
ATTN_WINDOW = os.environ.get("APERTIS_MHA_WINDOW", "0") == "1"
# under ATTN_WINDOW, for a model with an active window: generate()'s graph replay and its multi-token cache steps stay on the
# KV-cache kernels past the window (attention_decode_at with the cache's step_window, attention_chunk(window=)) instead of
# declining.  OFF by default; without ATTN_WINDOW it does nothing.
ATTN_WINDOW_CACHE = os.environ.get("APERTIS_MHA_WINDOW_CACHE", "0") == "1"


# ------------------------------------------------------------------------------------------------------ operand checks
# (host arithmetic on shapes, strides and pointers; none of them reads a device value)
def _aligned_rows(t, rs, W, bs=0):
    """(t, row stride) as the kernels' 16-byte loads take them: a packed copy (row stride W) when the pointer, the row
    stride or - where the caller passes one - the batch stride `bs` is off a 16-byte boundary."""
    es = t.element_size()
    if t.data_ptr() % 16 or (rs * es) % 16 or (bs * es) % 16:
        return t.clone(memory_format=torch.contiguous_format), W
    return t, rs


def _row2d(t, W, what):
    """[B, W] or [B, 1, W] -> ([B, W] view with unit inner stride, row stride)."""
    if t.dim() == 3 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 2 or t.shape[-1] != W:
        raise ApertisHipError(f"{what}: expected [B, {W}] or [B, 1, {W}], got {tuple(t.shape)}")
    if t.stride(-1) != 1 or (t.shape[0] > 1 and t.stride(0) < W):
        t = t.contiguous()
    return t, (t.stride(0) if t.shape[0] > 1 else W)


def _chunk3d(t, B, W, what):
    """[B, Lq, W] -> (tensor with unit inner stride, row stride, batch stride)."""
    if t.dim() != 3 or t.shape[0] != B or t.shape[-1] != W:
        raise ApertisHipError(f"{what}: expected [{B}, Lq, {W}], got {tuple(t.shape)}")
    Lq = t.shape[1]
    if t.stride(-1) != 1 or (Lq > 1 and t.stride(1) < W) or (B > 1 and t.stride(0) < Lq * t.stride(1)):
        t = t.contiguous()
    rs = t.stride(1) if Lq > 1 else W
    return t, rs, (t.stride(0) if B > 1 else Lq * rs)


def _key_valid_exact(what, key_valid, B, L):
    """key_valid of exactly [B, L] (or None) as the training / prefill kernels read it: int64, contiguous."""
    if key_valid is None:
        return None
    if tuple(key_valid.shape) != (B, L):
        raise ApertisHipError(f"{what}: key_valid {tuple(key_valid.shape)}, expected ({B}, {L})")
    if key_valid.dtype != torch.int64 or not key_valid.is_contiguous():
        key_valid = key_valid.to(torch.int64).contiguous()
    return key_valid


def _mask_rows(what, key_valid, B, Lk):
    """key_valid [B, >= Lk] as the cache kernels read it: (int64 tensor with unit inner stride, row stride); None: (None, 0)."""
    if key_valid is None:
        return None, 0
    if key_valid.dim() != 2 or key_valid.shape[0] != B or key_valid.shape[1] < Lk:
        raise ApertisHipError(f"{what}: key_valid {tuple(key_valid.shape)}, expected ({B}, >= {Lk})")
    if key_valid.dtype != torch.int64 or key_valid.stride(1) != 1:
        key_valid = key_valid.to(torch.int64).contiguous()
    return key_valid, (key_valid.stride(0) if B > 1 else key_valid.shape[1])


def _dropout(what, dropout_p, training):
    """(p, seed) of an attention call: p is 0 outside training, and the seed of the library's counter hash is ONE draw from
    torch's CPU generator, made only when p > 0 (a checkpointed recompute restores that generator and draws the same one)."""
    p = float(dropout_p) if training else 0.0
    if not 0.0 <= p < 1.0:
        raise ApertisHipError(f"{what}: dropout_p {dropout_p} outside [0, 1)")
    return p, (int(torch.empty((), dtype=torch.int64).random_().item()) if p > 0 else 0)


def _rope_table(what, cos, sin, W, required=False):
    """(cos, sin, max_pos): the module's fp32 cos_cached / sin_cached [max_pos, W/2], contiguous.  They come together; without
    a table (the appends: no rotation) max_pos is 0."""
    if (cos is None) != (sin is None):
        raise ApertisHipError(f"{what}: cos and sin come together")
    if cos is None and not required:
        return None, None, 0
    if (cos is None or cos.dtype != torch.float32 or sin.dtype != torch.float32 or cos.shape != sin.shape
            or 2 * cos.shape[-1] != W):
        raise ApertisHipError(f"{what}: cos/sin must be fp32 [max_pos, {W // 2}]")
    return cos.contiguous(), sin.contiguous(), cos.shape[0]


def _positions(position_ids, B, L, max_pos, in_range=False):
    """(int64 tensor or None, batch stride).  Explicit positions are range-checked here, on the host: the stock module's
    cos_cached[position_ids] raises IndexError for them, so this does too (one sync; the model passes None for its own
    arange positions).  in_range: the caller vouches that every position lies in [0, L) (a document layout's positions:
    ops.document_layout built them), so L against the table is the whole check and nothing is read back.  in_range = an
    integer n (not True): the caller knows more - every position lies in [0, n), n the longest document of a packed row -
    and n against the table is the check, so a row longer than the table passes when none of its documents is."""
    if position_ids is None or in_range:
        n = L if position_ids is None or in_range is True else int(in_range)
        if n > max_pos:
            raise IndexError(f"sequence length {n} exceeds the rotary table ({max_pos} positions)")
    if position_ids is None:
        return None, 0
    pos = position_ids
    if pos.dim() == 1:
        pos = pos.unsqueeze(0)
    if pos.dim() != 2 or pos.shape[-1] != L or pos.shape[0] not in (1, B):
        raise ApertisHipError(f"position_ids of shape {tuple(position_ids.shape)} for q of [{B}, {L}, ...]")
    if pos.dtype != torch.int64 or pos.stride(-1) != 1:
        pos = pos.to(torch.int64).contiguous()
    if pos.numel() and not in_range:
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


def rope_qk(q, k, position_ids, cos, sin, in_range=False):
    """RotaryEmbedding.forward applied to q and k [B, L, W] in one launch (reference core.py:258-293: interleaved pairs over the
    FULL width).  cos / sin: the module's fp32 cos_cached / sin_cached [max_pos, W/2]; position_ids int64 [1 or B, L] or None
    (positions 0..L-1).  Bit-identical to the stock module for fp32 and bf16; q and k share a shape and a dtype.
    in_range=True: the positions are known to lie in [0, L) (_positions), no host range check; an integer n: in [0, n)."""
    _require_gpu(q, k, position_ids, cos, sin)
    if q.shape != k.shape or q.dtype != k.dtype or q.dim() != 3:
        raise ApertisHipError(f"rope_qk: q {tuple(q.shape)} {q.dtype} and k {tuple(k.shape)} {k.dtype} must match, [B, L, W]")
    B, L, W = q.shape
    cos, sin, max_pos = _rope_table("rope_qk", cos, sin, W, required=True)
    pos, pos_bs = _positions(position_ids, B, L, max_pos, in_range)
    return _RopeQK.apply(q, k, pos, pos_bs, cos, sin)


# ------------------------------------------------------------------------------- training / prefill attention: one node
class DocumentLayout:
    """What document_layout returns: `start` / `end` int32 [B, L] (first token / one past the last token of each token's
    document, as the kernels read them), `positions` int64 [B, L] (index - start: the position within the document) and
    `pairs`, a host integer: the number of (query, key) pairs the mask keeps in the whole batch, sum of len*(len+1)/2."""
    __slots__ = ("start", "end", "positions", "pairs")

    def __init__(self, start, end, positions, pairs):
        self.start, self.end, self.positions, self.pairs = start, end, positions, pairs


def window_pairs(L, window):
    """The (query, key) pairs a sliding window of `window` keys keeps in one causal row of L tokens: sum_i min(i + 1, window)."""
    w = min(int(window), L)
    return w * (w + 1) // 2 + (L - w) * w


# csrc/attention.hip has ONE kernel set templated on <CAUSAL, mask mode> behind four pairs of entry points, and this is all
# that differs between them on the host: form -> (forward launch, backward launch, forward work(B, L, H, D, layout) in flops -
# two products over the pairs the mask keeps; the backward's is 2.5 times it - and what follows key_valid in both argument
# lists: layout.start / layout.end of "doc", the window of "window" - `layout` is then that integer - else nothing)
_FORMS = {
    "causal": ("apertis_attention_fwd", "apertis_attention_bwd", lambda B, L, H, D, layout: 4.0 * B * H * D * L * (L + 1) / 2,
               lambda layout: ()),
    "full": ("apertis_attention_full_fwd", "apertis_attention_full_bwd", lambda B, L, H, D, layout: 4.0 * B * H * D * L * L,
             lambda layout: ()),
    "doc": ("apertis_attention_doc_fwd", "apertis_attention_doc_bwd", lambda B, L, H, D, layout: 4.0 * H * D * layout.pairs,
            lambda layout: (ptr(layout.start), ptr(layout.end))),
    "window": ("apertis_attention_window_fwd", "apertis_attention_window_bwd",
               lambda B, L, H, D, layout: 4.0 * B * H * D * window_pairs(L, layout), lambda layout: (int(layout),)),
}


def _attn_fwd(form, q, q_rs, k, k_rs, v, v_rs, key_valid, layout, B, L, W, heads, p, seed):
    """One forward launch of `form`: (O [B, L, W] packed, LSE [B, heads, L] fp32)."""
    name, _, work, bounds = _FORMS[form]
    bounds = bounds(layout)
    out = torch.empty(B, L, W, device=q.device, dtype=q.dtype)
    lse = torch.empty(B, heads, L, device=q.device, dtype=torch.float32)
    _launch(name, getattr(_lib.load(), name),
            (ptr(q), q_rs, ptr(k), k_rs, ptr(v), v_rs, ptr(key_valid), *bounds, ptr(out), W, ptr(lse), B, L, heads, W // heads,
             p, seed, dtype_code(q), stream_ptr()), work=work(B, L, heads, W // heads, layout))
    return out, lse


def _attn_bwd(form, q, q_rs, k, k_rs, v, v_rs, out, dout, lse, key_valid, layout, dq, dk, dv, d_rs, B, L, W, heads, p, seed):
    """One backward launch of `form` into dq, dk, dv (one row stride d_rs).  The incoming gradient is whatever autograd hands
    over: another dtype is cast, and rows the kernels cannot take as they are (_rows, _aligned_rows) are copied."""
    _, name, work, bounds = _FORMS[form]
    bounds = bounds(layout)
    lib = _lib.load()
    dout = dout.to(q.dtype)
    dout, do_rs = _aligned_rows(*_rows(dout, W), W)
    ws = torch.empty(lib.apertis_attention_bwd_workspace_bytes(B, L, heads) // 4, device=q.device, dtype=torch.float32)
    _launch(name, getattr(lib, name),
            (ptr(q), q_rs, ptr(k), k_rs, ptr(v), v_rs, ptr(out), W, ptr(dout), do_rs, ptr(lse), ptr(key_valid), *bounds, ptr(ws),
             ptr(dq), ptr(dk), ptr(dv), d_rs, B, L, heads, W // heads, p, seed, dtype_code(q), stream_ptr()),
            work=2.5 * work(B, L, heads, W // heads, layout))


class _Attention(torch.autograd.Function):
    """causal_attention, full_attention, document_attention and window_attention (`form`, a key of _FORMS; `layout`: the
    DocumentLayout of "doc", the window - a host integer - of "window", else None)."""

    @staticmethod
    def forward(ctx, form, q, k, v, heads, key_valid, p, seed, layout=None):
        B, L, W = q.shape
        q, q_rs = _rows(q, W)
        k, k_rs = _rows(k, W)
        v, v_rs = _rows(v, W)
        out, lse = _attn_fwd(form, q, q_rs, k, k_rs, v, v_rs, key_valid, layout, B, L, W, heads, p, seed)
        doc = (layout.start, layout.end) if form == "doc" else ()
        ctx.save_for_backward(q, k, v, out, lse, key_valid, *doc)
        ctx.cfg = (form, heads, p, seed, layout.pairs if doc else layout)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse, key_valid, *doc = ctx.saved_tensors
        form, heads, p, seed, pairs = ctx.cfg
        layout = DocumentLayout(*doc, None, pairs) if doc else pairs         # (the window of "window"; None otherwise)
        B, L, W = q.shape
        dq = torch.empty(B, L, W, device=q.device, dtype=q.dtype)
        dk = torch.empty_like(dq)
        dv = torch.empty_like(dq)
        _attn_bwd(form, q, q.stride(-2), k, k.stride(-2), v, v.stride(-2), out, dout, lse, key_valid, layout, dq, dk, dv, W,
                  B, L, W, heads, p, seed)
        return None, dq, dk, dv, None, None, None, None, None


class _FullAttentionQKV(torch.autograd.Function):
    """The "full" form on the column slices of ONE [B, L, 3W] tensor: nothing is copied on the way in (row stride 3W), and the
    backward writes dq | dk | dv into the column slices of ONE [B, L, 3W] gradient - three slice backwards would each
    materialise a zero-filled [B, L, 3W] and autograd would add them."""

    @staticmethod
    def forward(ctx, qkv, heads, p, seed):
        B, L, W3 = qkv.shape
        W = W3 // 3
        qkv, rs = _aligned_rows(*_rows(qkv, W3), W3)
        out, lse = _attn_fwd("full", qkv[..., :W], rs, qkv[..., W:2 * W], rs, qkv[..., 2 * W:], rs, None, None, B, L, W, heads,
                             p, seed)
        ctx.save_for_backward(qkv, out, lse)
        ctx.cfg = (heads, p, seed)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        heads, p, seed = ctx.cfg
        B, L, W3 = qkv.shape
        W, rs = W3 // 3, qkv.stride(-2)
        d = torch.empty(B, L, W3, device=qkv.device, dtype=qkv.dtype)
        _attn_bwd("full", qkv[..., :W], rs, qkv[..., W:2 * W], rs, qkv[..., 2 * W:], rs, out, dout, lse, None, None,
                  d[..., :W], d[..., W:2 * W], d[..., 2 * W:], W3, B, L, W, heads, p, seed)
        return d, None, None, None


def attention_supported(q, heads):
    """Whether causal_attention takes q [B, L, heads*D] of this dtype and head dim (D 64 or 128, fp32 or bf16)."""
    return (q.dim() == 3 and q.shape[-1] % heads == 0 and q.shape[-1] // heads in (64, 128)
            and q.dtype in (torch.float32, torch.bfloat16))


def attention_dead_rows(out, v, key_valid, n=0):
    """The dead rows of a causal attention output, IN PLACE on `out` [B, Lq, W]: row i sits at key position n + i and is dead
    iff key_valid[b, :n + i + 1] is all zero (left padding; any mask).  The reference's finfo.min masks saturate on such a row
    and its softmax is uniform over all Lk = n + Lq keys, so the row becomes the column mean of v[b, :Lk] (fp32 accumulation,
    one rounding), the same for every head; causal_attention and attention_chunk leave zeros there.  Every other row keeps its
    bits.  v: [B, >= Lk, W] in out's dtype (fp32 or bf16; a KV-cache buffer's strides are taken as they are); key_valid:
    [B, >= Lk], nonzero = attend.  Returns `out`.  Inference only: nothing is saved for a backward."""
    _require_gpu(out, v, key_valid)
    if (out.dim() != 3 or v.dim() != 3 or out.shape[1] < 1 or out.dtype != v.dtype
            or out.dtype not in (torch.float32, torch.bfloat16) or v.shape[0] != out.shape[0] or v.shape[2] != out.shape[2]
            or n < 0 or v.shape[1] < n + out.shape[1] or key_valid is None):
        raise ApertisHipError(f"attention_dead_rows: out {tuple(out.shape)} {out.dtype}, v {tuple(v.shape)} {v.dtype}, n {n} "
                              "(out [B, Lq, W] and v [B, >= n + Lq, W], one dtype, fp32 or bf16, with a key_valid)")
    B, Lq, W = out.shape
    Lk, es = n + Lq, out.element_size()
    if W % (16 // es):
        raise ApertisHipError(f"attention_dead_rows: width {W} is not a multiple of {16 // es}")
    o, o_rs, o_bs = _chunk3d(out, B, W, "attention_dead_rows out")
    if o is not out or out.data_ptr() % 16 or (o_rs * es) % 16 or (B > 1 and (o_bs * es) % 16):
        raise ApertisHipError("attention_dead_rows: out is written in place: unit inner stride, rows and batches on 16-byte "
                              "boundaries")
    v, v_rs, v_bs = _chunk3d(v[:, :Lk], B, W, "attention_dead_rows v")
    v, v_rs = _aligned_rows(v, v_rs, W, v_bs if B > 1 else 0)
    v_bs = v.stride(0) if B > 1 else Lk * v_rs                      # (as _chunk3d gave it, or the packed copy's)
    key_valid, kv_rs = _mask_rows("attention_dead_rows", key_valid, B, Lk)
    _launch("apertis_attention_dead_rows", _lib.load().apertis_attention_dead_rows,
            (ptr(v), v_rs, v_bs, ptr(key_valid), kv_rs, ptr(out), o_rs, o_bs, B, Lq, int(n), W, dtype_code(out), stream_ptr()),
            work=float(B) * Lk * W, detail=f"{B}x{Lk}x{W}", nbytes=float(B) * Lk * W * es)
    return out


def _dead_rows_inference(what, training, dropout_p, *ts):
    """dead_rows=True is inference only: the reference's backward of a dead row is a dense uniform row that reaches every
    key, and the backward kernels do not compute it."""
    if (torch.is_grad_enabled() and any(t.requires_grad for t in ts)) or (training and dropout_p > 0):
        raise ApertisHipError(f"{what}: dead_rows=True is inference only (no input that requires grad under autograd, no "
                              "attention dropout in training)")


def causal_attention(q, k, v, heads, key_valid=None, dropout_p=0.0, training=False, dead_rows=False):
    """softmax(Q K^T / sqrt(D) + causal and key-padding mask) V per head, with attention dropout in training.
    q, k, v: [B, L, heads*D] (head h in columns [h*D, (h+1)*D)), one dtype, fp32 or bf16, D in {64, 128}; returns O in the same
    layout (out_proj reads it directly).  key_valid: [B, L] (the raw attention_mask, nonzero = attend) or None.  Dropout keeps
    element (i, j) of head (b, h) by the library's counter hash with a seed drawn from torch's RNG here (a checkpointed
    recompute draws the same one); the backward regenerates the mask.  Saved for the backward: q, k, v, O and LSE [B, heads, L]
    fp32, never an L x L tensor.
    A query row with no valid key at or before it (left padding) comes out as zeros; dead_rows=True (inference only: it raises
    when an input requires grad under autograd, or with dropout in training) fills such rows with the reference's value
    instead, the column mean of v over all L keys (attention_dead_rows)."""
    _require_gpu(q, k, v, key_valid)
    if dead_rows:
        _dead_rows_inference("causal_attention", training, dropout_p, q, k, v)
    if not (q.shape == k.shape == v.shape and q.dtype == k.dtype == v.dtype) or not attention_supported(q, heads):
        raise ApertisHipError(f"causal_attention: q/k/v {tuple(q.shape)} {q.dtype} with {heads} heads (D 64 or 128, fp32 or bf16, "
                              "one shape and dtype)")
    B, L, _ = q.shape
    key_valid = _key_valid_exact("causal_attention", key_valid, B, L)
    p, seed = _dropout("causal_attention", dropout_p, training)
    out = _Attention.apply("causal", q, k, v, int(heads), key_valid, p, seed, None)
    if dead_rows and key_valid is not None and B:
        attention_dead_rows(out, v, key_valid)
    return out


# --------------------------------------------------------------------------------- packed rows: document-masked attention
def document_layout(document_ids):
    """The layout of packed rows from `document_ids` [B, L] (integers, non-decreasing along L in every row: a document is a
    run of equal ids).  Built with torch ops on the ids' device (a running maximum over the run starts and its mirror over
    the run ends), once per forward; ONE host read brings back the check - ids that decrease raise ValueError - together
    with the pair count of the launches' work accounting."""
    ids = document_ids
    if ids.dim() != 2 or ids.dtype.is_floating_point or ids.dtype == torch.bool:
        raise ValueError(f"document_ids must be integers [B, L], got {tuple(ids.shape)} {ids.dtype}")
    B, L = ids.shape
    if L >= 2 ** 31:
        raise ValueError(f"document_ids: rows of {L} tokens do not fit the int32 layout")
    idx = torch.arange(L, device=ids.device)
    step = ids[:, 1:] - ids[:, :-1]
    first = torch.ones(B, L, dtype=torch.bool, device=ids.device)
    last = torch.ones(B, L, dtype=torch.bool, device=ids.device)
    first[:, 1:] = step != 0
    last[:, :-1] = step != 0
    if L:
        start = torch.cummax(torch.where(first, idx, 0), dim=1).values
        end = torch.cummin(torch.where(last, idx + 1, L).flip(1), dim=1).values.flip(1)
    else:
        start = end = torch.zeros(B, 0, dtype=torch.int64, device=ids.device)
    positions = idx - start
    decreasing, pairs = torch.stack(((step < 0).sum(), (positions + 1).sum())).tolist()
    if decreasing:
        raise ValueError("document_ids must not decrease along a row (documents are contiguous runs of equal ids)")
    return DocumentLayout(start.to(torch.int32).contiguous(), end.to(torch.int32).contiguous(), positions, int(pairs))


def document_attention(q, k, v, heads, layout, key_valid=None, dropout_p=0.0, training=False):
    """causal_attention on PACKED rows: query i of row b attends key j iff layout.start[b, i] <= j <= i (and key_valid),
    so the documents of a row - contiguous runs, document_layout - do not see each other.  The layout contract, the dropout
    hash and seed, the saved tensors and the determinism of the backward are causal_attention's; with one document per row
    every output and gradient has causal_attention's bits.  The kernels skip the key tiles in front of a wave's earliest
    document and the query tiles past a wave's latest document end: the work is the documents' triangles
    (4*heads*D*layout.pairs flops forward), not the row's."""
    _require_gpu(q, k, v, key_valid)
    if not (q.shape == k.shape == v.shape and q.dtype == k.dtype == v.dtype) or not attention_supported(q, heads):
        raise ApertisHipError(f"document_attention: q/k/v {tuple(q.shape)} {q.dtype} with {heads} heads (D 64 or 128, fp32 or "
                              "bf16, one shape and dtype)")
    B, L, _ = q.shape
    if not isinstance(layout, DocumentLayout):
        raise ApertisHipError("document_attention: layout is what ops.document_layout returns")
    for t in (layout.start, layout.end):
        if tuple(t.shape) != (B, L) or t.dtype != torch.int32 or not t.is_contiguous() or t.device != q.device:
            raise ApertisHipError(f"document_attention: layout of {tuple(t.shape)} {t.dtype} on {t.device} for q of [{B}, {L}, ...] "
                                  f"on {q.device}")
    key_valid = _key_valid_exact("document_attention", key_valid, B, L)
    p, seed = _dropout("document_attention", dropout_p, training)
    return _Attention.apply("doc", q, k, v, int(heads), key_valid, p, seed, layout)


# ------------------------------------------------------------------------------------------------- sliding-window attention
def _window(what, window):
    """The window as the host integer the launches take: >= 1, else ValueError (bool and float are not integers here)."""
    if isinstance(window, bool) or not isinstance(window, int) or window < 1:
        raise ValueError(f"{what}: window must be an integer >= 1, got {window!r}")
    return min(window, 2 ** 63 - 1)


def window_attention(q, k, v, heads, window, key_valid=None, dropout_p=0.0, training=False, dead_rows=False):
    """causal_attention under a SLIDING WINDOW: query i attends key j iff max(0, i - window + 1) <= j <= i (and key_valid) -
    `window` keys, its own included; a host integer >= 1 (ValueError otherwise), any value >= L is the plain causal mask with
    causal_attention's bits.  The layout contract, the dropout hash and seed, the saved tensors, the determinism of the
    backward and the inference-only dead_rows fill are causal_attention's (a dead row of a windowed forward is still one with
    no valid key at or before it, and gets the column mean over all L keys: the reference's value under its full mask).  The
    kernels are the causal ones with bounds computed from the index (csrc/attention.hip, MASK_WINDOW): nothing is loaded for
    them, key tiles in front of a wave's window and query tiles past it are never touched, and every output and gradient has
    the bits of document_attention on window_layout((B, L), window, device).  Work: 4*B*heads*D*sum_i min(i + 1, window)
    flops forward."""
    window = _window("window_attention", window)
    _require_gpu(q, k, v, key_valid)
    if dead_rows:
        _dead_rows_inference("window_attention", training, dropout_p, q, k, v)
    if not (q.shape == k.shape == v.shape and q.dtype == k.dtype == v.dtype) or not attention_supported(q, heads):
        raise ApertisHipError(f"window_attention: q/k/v {tuple(q.shape)} {q.dtype} with {heads} heads (D 64 or 128, fp32 or bf16, "
                              "one shape and dtype)")
    B, L, _ = q.shape
    key_valid = _key_valid_exact("window_attention", key_valid, B, L)
    p, seed = _dropout("window_attention", dropout_p, training)
    out = _Attention.apply("window", q, k, v, int(heads), key_valid, p, seed, window)
    if dead_rows and key_valid is not None and B:
        attention_dead_rows(out, v, key_valid)
    return out


_WINDOW_ARRAYS = {}          # (L, window, device) -> (start, end) int32 [L] of a row that is one document: window_layout


def window_layout(layout_or_shape, window, device=None):
    """The DocumentLayout of a sliding window of `window` keys (an integer >= 1): for a shape (B, L), start[b, i] =
    max(0, i - window + 1) and end[b, j] = min(L, j + window) on `device`; for a packed DocumentLayout, its bounds clipped to
    the window, start = max(doc_start, i - window + 1), end = min(doc_end, j + window) (on the layout's device) - a document
    shorter than the window keeps its triangle.  `positions` are the layout's own (0..L-1 for a shape), `pairs` is recomputed
    on the host for a shape and with ONE host read for a layout.  document_attention on the result is the windowed attention,
    on the document kernels as they are.  The unclipped arrays are built once per (L, window, device)."""
    window = _window("window_layout", window)
    lay = layout_or_shape if isinstance(layout_or_shape, DocumentLayout) else None
    B, L = (tuple(lay.start.shape) if lay is not None else tuple(int(n) for n in layout_or_shape))
    if L >= 2 ** 31:
        raise ValueError(f"window_layout: rows of {L} tokens do not fit the int32 layout")
    device = torch.device(lay.start.device if lay is not None else (device if device is not None else "cpu"))
    key = (L, min(window, L), str(device))
    if key not in _WINDOW_ARRAYS:
        idx = torch.arange(L, device=device, dtype=torch.int64)
        _WINDOW_ARRAYS[key] = ((idx - (key[1] - 1)).clamp_(min=0).to(torch.int32), (idx + key[1]).clamp_(max=L).to(torch.int32))
    ws, we = _WINDOW_ARRAYS[key]
    if lay is None:
        positions = torch.arange(L, device=device, dtype=torch.int64).unsqueeze(0).expand(B, L)
        return DocumentLayout(ws.unsqueeze(0).expand(B, L).contiguous(), we.unsqueeze(0).expand(B, L).contiguous(), positions,
                              B * window_pairs(L, window))
    start, end = torch.maximum(lay.start, ws), torch.minimum(lay.end, we)
    pairs = int((torch.arange(1, L + 1, device=device) - start).sum()) if B and L else 0
    return DocumentLayout(start.contiguous(), end.contiguous(), lay.positions, pairs)


# ------------------------------------------------------------------------------------------- bidirectional attention
# the vision tower (multimodal.py) runs its encoder layers on the project's kernels - LayerNorm boundaries, MFMA GEMMs, the
# attention below, the expert-MLP pair - when this is on and the tower qualifies (UnifiedMultimodalEncoder.fused_supported).
# OFF by default (APERTIS_VIT_FUSED=1 turns it on): it changes the default path's bits and the tower's train-mode dropout
# stream (counter hash instead of Philox); flipping the default is a change of its own
VIT_FUSED = os.environ.get("APERTIS_VIT_FUSED", "0") == "1"


def full_attention_supported(q, heads, packed=False):
    """Whether full_attention takes q [B, L, heads*D] - or, packed=True, full_attention_qkv takes qkv [B, L, 3*heads*D] - of
    this dtype, head dim and batch (D 64 or 128, fp32 or bf16, B*heads <= 65535: the grid's y dimension)."""
    if q.dim() != 3 or heads < 1 or (packed and q.shape[-1] % 3):
        return False
    W = q.shape[-1] // 3 if packed else q.shape[-1]
    return (W % heads == 0 and W // heads in (64, 128) and q.dtype in (torch.float32, torch.bfloat16)
            and q.shape[0] * heads <= 65535)


def full_attention(q, k, v, heads, key_valid=None, dropout_p=0.0, training=False):
    """softmax(Q K^T / sqrt(D) + key-padding mask) V per head WITHOUT a causal mask (bidirectional: the vision tower), with
    attention dropout in training.  The layout contract of causal_attention: q, k, v [B, L, heads*D] (head h in columns
    [h*D, (h+1)*D)), one dtype, fp32 or bf16, D in {64, 128}, B*heads <= 65535, row-strided views taken as they are; returns
    O in the same layout.  key_valid: [B, L] (nonzero = attend), ANY pattern, holes included, or None.  Dropout: the counter
    hash of causal_attention with a seed drawn from torch's RNG here; the backward regenerates the mask and is deterministic
    (no atomics).  Saved for the backward: q, k, v, O and LSE [B, heads, L] fp32, never an L x L tensor.
    There is no dead-row notion here - every query sees the same keys.  A SEQUENCE WITH NO VALID KEY AT ALL comes out as
    zeros (LSE +inf) and all three of its gradients are zero."""
    _require_gpu(q, k, v, key_valid)
    if not (q.shape == k.shape == v.shape and q.dtype == k.dtype == v.dtype) or not full_attention_supported(q, heads):
        raise ApertisHipError(f"full_attention: q/k/v {tuple(q.shape)} {q.dtype} with {heads} heads (D 64 or 128, fp32 or bf16, "
                              "one shape and dtype, B*heads <= 65535)")
    B, L, _ = q.shape
    key_valid = _key_valid_exact("full_attention", key_valid, B, L)
    p, seed = _dropout("full_attention", dropout_p, training)
    return _Attention.apply("full", q, k, v, int(heads), key_valid, p, seed, None)


def full_attention_qkv(qkv, heads, dropout_p=0.0, training=False):
    """full_attention (no key mask) on the stacked [B, L, 3*W] output of ONE in-projection GEMM: q, k, v are its three column
    slices, read in place with row stride 3*W, and the backward returns ONE [B, L, 3*W] gradient whose column slices the two
    backward kernels wrote (dq | dk | dv).  Bit-identical to full_attention on copies of the slices.  Raises on a width
    whose slices do not start on 16-byte boundaries."""
    _require_gpu(qkv)
    if not full_attention_supported(qkv, heads, packed=True):
        raise ApertisHipError(f"full_attention_qkv: qkv {tuple(qkv.shape)} {qkv.dtype} with {heads} heads ([B, L, 3*heads*D], "
                              "D 64 or 128, fp32 or bf16, B*heads <= 65535)")
    if (qkv.shape[-1] // 3 * qkv.element_size()) % 16:
        raise ApertisHipError(f"full_attention_qkv: the slices of width {qkv.shape[-1] // 3} are not 16-byte aligned")
    p, seed = _dropout("full_attention_qkv", dropout_p, training)
    return _FullAttentionQKV.apply(qkv, int(heads), p, seed)


# ---------------------------------------------------------------------------------------------------- KV-cache decode
# single-token steps of a standard_mha model against a KVCache take the kernels of csrc/attention_decode.hip when this AND
# ATTN_FUSED are on (ATTN_FUSED = False keeps meaning "stock torch attention everywhere"); off: torch.cat + stock SDPA
ATTN_DECODE_FUSED = True
# generate() replays the KV-cache token step of a standard_mha model as one captured HIP graph (model.py:
# _generate_graph_tail; kv_append_rope_at / attention_decode_at below).  OFF by default (APERTIS_MHA_DECODE_GRAPH=1 turns it
# on): the eager loop's launch counts are pinned by tests, and flipping the default is a change of its own
ATTN_DECODE_GRAPH = os.environ.get("APERTIS_MHA_DECODE_GRAPH", "0") == "1"
# generate_many() serves a standard_mha model on KV-cache SLOTS - one row of the decode batch per prompt, every row with a
# length of its own (KVCache.slots_begin; kv_append_rope_slots / attention_decode_slots below).  OFF by default
# (APERTIS_MHA_SLOTS=1 turns it on): without it generate_many() refuses such a model as it always did
ATTN_SLOTS = os.environ.get("APERTIS_MHA_SLOTS", "0") == "1"

ATTN_DECODE_MAX_SPLITS = _lib.CONSTANTS["APERTIS_ATTN_DECODE_MAX_SPLITS"]


class KVLayer:
    """`cache[i]`: layer i of a KVCache, indexable like the (k, v) pair it replaces - [0] and [1] are VIEWS of the layer's
    first `length` rows ([B, length, W]), built when asked for."""
    __slots__ = ("cache", "layer")

    def __init__(self, cache, layer):
        self.cache, self.layer = cache, layer

    def __len__(self):
        return 2

    def __getitem__(self, j):
        if j not in (0, 1, -1, -2):
            raise IndexError(j)
        c = self.cache
        return (c.k if j in (0, -2) else c.v)[self.layer][:, :c.lengths[self.layer]]

    def __iter__(self):
        return iter((self[0], self[1]))


class KVCache:
    """Preallocated KV cache of a standard_mha model: per layer one `k` and one `v` buffer [B, capacity, W] (W = heads * D,
    token-major, the layout of a prefill's `past_key_values`) and one length per layer.  `cache[i]` is (k[:, :len], v[:, :len])
    as views, `len(cache)` the number of layers, so it reads like the tuple of pairs it replaces.

    It is an explicit, MUTABLE object: a decode step (kv_append_rope) writes row `len` of every layer IN PLACE and the layer's
    length grows by one - there is no copy of the cache per token, and therefore ONE continuation per cache: a caller that wants
    to branch a generation builds a second cache (from_prefill) for the second branch.  All layers of one step append at the
    same row: each layer keeps its own length, so layer i's append does not move what layer i + 1 sees.  A step that raised
    half-way leaves the layers at different lengths; such a cache is not used again.

    DEVICE STEP STATE (opt-in, for a captured graph of the step: a graph freezes host values).  step_state_begin() copies the
    host state to the device: `dev_len` int64[1] (the rows held; ONE for all layers), `dev_valid` int64 [B, capacity] (the key
    validity, nonzero = attend; columns the caller's mask does not reach are 1) and `dev_err` int32[1] (set by a step that
    would have left the cache or the rotary table; such a step writes nothing).  kv_append_rope_at / attention_decode_at
    read the step from there and never touch `lengths`; whoever drives the steps adds one to `dev_len` after the last layer
    and writes the validity column of the new token.  WHILE THE DEVICE STATE DRIVES THE STEPS THE HOST `lengths` ARE STALE
    (and with them the views `cache[i]` hands out); step_state_end() makes them current again - from `dev_len` with one
    host read, or from the length its caller knows - and the by-value steps may go on.  Still one continuation per cache.
    step_state_begin(window=W) also keeps `step_window`: while it is set, attention_decode_at attends the newest W rows only.

    SLOTS (opt-in, generate_many() of a standard_mha model: every row of the batch is a sequence of its own, installed and
    freed while the others go on).  slots_begin() allocates `dev_lens` int64 [B] (the rows each slot holds), `dev_len`
    int64[1] (their maximum: the one length the attention launch reads), `dev_valid` int64 [B, capacity], ZEROS - column j
    of row b is nonzero iff j <= dev_lens[b] once the step's helper has run; the rows of a slot beyond its length hold the
    previous occupant's keys and must stay masked - and `dev_err`.  slot_install / slot_free move a sequence in and out,
    kv_append_rope_slots / attention_decode_slots are the step, slots_step_begin / slots_step_end bracket it once per token
    step.  The host `lengths` are stale throughout, and the device step state and the slots exclude each other.

    `multi_token` (a flag, default False): a forward of several tokens extends this cache in place on the chunk kernels
    (kv_append_rope_chunk, attention_chunk) and hands the same object back, as a single-token step does; without the flag such
    a forward runs the stock branch on the cache's views, returns plain tensors and leaves the cache as it was."""

    def __init__(self, k, v, length=0, multi_token=False):
        if len(k) != len(v) or not k:
            raise ApertisHipError("KVCache: one k and one v buffer per layer")
        for a, b in zip(k, v):
            if (a.dim() != 3 or a.shape != b.shape or a.dtype != b.dtype or a.shape != k[0].shape or a.dtype != k[0].dtype
                    or a.stride(2) != 1 or b.stride(2) != 1):
                raise ApertisHipError("KVCache: buffers are [B, capacity, W] with unit inner stride, one shape and dtype")
        self.k, self.v = list(k), list(v)
        if not 0 <= length <= self.capacity:
            raise ApertisHipError(f"KVCache: length {length} outside [0, {self.capacity}]")
        self.lengths = [int(length)] * len(self.k)
        self.multi_token = bool(multi_token)
        self._ws = None
        self.dev_len = self.dev_valid = self.dev_err = self.dev_lens = None
        self.step_active, self.step_splits, self.step_window = False, 1, None
        self.slot_active = False

    @classmethod
    def empty(cls, layers, B, capacity, W, dtype=torch.float32, device=None, multi_token=False):
        if layers < 1 or B < 0 or capacity < 1 or W < 1:
            raise ApertisHipError(f"KVCache.empty: layers {layers}, B {B}, capacity {capacity}, W {W}")
        mk = lambda: [torch.empty(B, capacity, W, dtype=dtype, device=device) for _ in range(layers)]     # noqa: E731
        return cls(mk(), mk(), 0, multi_token)

    @classmethod
    def from_prefill(cls, past, capacity, multi_token=False):
        """From a prefill's `past_key_values` (per layer (k, v), [B, L, W]): one copy per layer into buffers of `capacity`
        rows, in the prefill's dtype, once per generation."""
        L = past[0][0].shape[1]
        if capacity < L:
            raise ApertisHipError(f"KVCache.from_prefill: capacity {capacity} below the prefill's {L} positions")
        B, _, W = past[0][0].shape
        c = cls.empty(len(past), B, capacity, W, past[0][0].dtype, past[0][0].device, multi_token)
        for i, (k, v) in enumerate(past):
            c.k[i][:, :L].copy_(k)
            c.v[i][:, :L].copy_(v)
        c.lengths = [L] * len(past)
        return c

    capacity = property(lambda self: self.k[0].shape[1])
    dtype = property(lambda self: self.k[0].dtype)
    length = property(lambda self: self.lengths[0], doc="positions held (layer 0's: all layers agree between steps)")

    def __len__(self):
        return len(self.k)

    def __getitem__(self, i):
        if not -len(self.k) <= i < len(self.k):
            raise IndexError(i)
        return KVLayer(self, i % len(self.k))

    def __iter__(self):
        return (KVLayer(self, i) for i in range(len(self.k)))

    def step_state_begin(self, heads, key_valid=None, L_end=None, splits=None, window=None):
        """Device step state from the host state (class docstring).  key_valid: the mask so far, [B, <= capacity], or None
        (every key valid).  The split count of attention_decode_at is fixed here, once - apertis_attention_decode_splits at
        `L_end` keys (the length the steps can reach; default: the capacity) unless `splits` gives it - and the workspace is
        sized for it, so nothing is allocated by a step.
        window (an integer >= 1, or None): the steps attend the newest `window` rows only - it is kept as `step_window`,
        attention_decode_at launches the window form while it is set, and the split count is sized at min(L_end, window)
        keys, the most a step reads.  step_state_end() clears it."""
        if window is not None:
            window = _window("KVCache.step_state_begin", window)
        if self.slot_active:
            raise ApertisHipError("KVCache.step_state_begin: the cache is in slot mode (KVCache.slots_end() first)")
        if len(set(self.lengths)) != 1:
            raise ApertisHipError(f"KVCache.step_state_begin: the layers disagree on the length ({self.lengths})")
        B, cap, W = self.k[0].shape
        dev = self.k[0].device
        if W % heads:
            raise ApertisHipError(f"KVCache.step_state_begin: width {W} with {heads} heads")
        keys = min(max(int(L_end if L_end is not None else cap), 1), cap)
        if window is not None:
            keys = min(keys, window)
        n = self._fixed_splits("KVCache.step_state_begin", heads, keys, splits)
        valid = torch.ones(B, cap, dtype=torch.int64, device=dev)
        if key_valid is not None:
            if key_valid.dim() != 2 or key_valid.shape[0] != B or key_valid.shape[1] > cap:
                raise ApertisHipError(f"KVCache.step_state_begin: key_valid {tuple(key_valid.shape)}, expected ({B}, <= {cap})")
            valid[:, :key_valid.shape[1]] = key_valid.to(torch.int64)
        self.dev_valid = valid
        self.dev_len = torch.full((1,), self.lengths[0], dtype=torch.int64, device=dev)
        self.dev_err = torch.zeros(1, dtype=torch.int32, device=dev)
        self.step_active, self.step_splits, self.step_window = True, n, window

    def step_state_end(self, length=None):
        """The host lengths (every layer) from the device state: `length` if the caller knows it (no host read; `dev_len` is
        set to it too), else one read of `dev_len`.  The by-value steps go on from there; the device buffers stay readable."""
        if self.dev_len is None:
            raise ApertisHipError("KVCache.step_state_end: no device step state")
        if length is None:
            length = int(self.dev_len.item())
        else:
            self.dev_len.fill_(int(length))
        if not 0 <= length <= self.capacity:
            raise ApertisHipError(f"KVCache.step_state_end: length {length} outside [0, {self.capacity}]")
        self.lengths = [int(length)] * len(self.k)
        self.step_active, self.step_window = False, None

    def _fixed_splits(self, what, heads, keys, splits):
        """The split count of a run of device-length steps, fixed once (`splits`, or the library's choice at `keys` keys),
        with the workspace sized for it."""
        B, _, W = self.k[0].shape
        lib = _lib.load()
        n = int(splits) if splits is not None else int(lib.apertis_attention_decode_splits(max(B, 1), heads, keys, W // heads))
        nbytes = int(lib.apertis_attention_decode_workspace_bytes(B, heads, W // heads, n))
        if nbytes < 0:
            raise ApertisHipError(f"{what}: {n} splits outside [1, {ATTN_DECODE_MAX_SPLITS}]")
        self._workspace(nbytes)
        return n

    # ---- slots (class docstring) ----------------------------------------------------------------------------------------
    def slots_begin(self, heads, L_end=None, splits=None):
        """Slot mode: every row of the batch empty (`dev_lens` zeros, `dev_valid` ZEROS - the step state's default is ones;
        here a column beyond a row's length must be 0).  The split count of attention_decode_slots is fixed here, once, at
        `L_end` keys (default: the capacity) and B = the number of slots, unless `splits` gives it, and the workspace is
        sized for it.  Refuses a cache whose device step state is active."""
        if self.step_active:
            raise ApertisHipError("KVCache.slots_begin: the device step state is active (KVCache.step_state_end() first)")
        S, cap, W = self.k[0].shape
        dev = self.k[0].device
        if S < 1 or W % heads:
            raise ApertisHipError(f"KVCache.slots_begin: {S} slots of width {W} with {heads} heads")
        keys = min(max(int(L_end if L_end is not None else cap), 1), cap)
        self.step_splits = self._fixed_splits("KVCache.slots_begin", heads, keys, splits)
        self.dev_lens = torch.zeros(S, dtype=torch.int64, device=dev)
        self.dev_len = torch.zeros(1, dtype=torch.int64, device=dev)
        self.dev_valid = torch.zeros(S, cap, dtype=torch.int64, device=dev)
        self.dev_err = torch.zeros(1, dtype=torch.int32, device=dev)
        self._cols = torch.arange(cap, dtype=torch.int64, device=dev)
        self.step_window, self.slot_active = None, True

    def slots_end(self):
        """Leaves slot mode; the device buffers stay readable.  The host `lengths` are what they were before slots_begin."""
        if not self.slot_active:
            raise ApertisHipError("KVCache.slots_end: the cache is not in slot mode")
        self.slot_active = False

    def _slot(self, what, b):
        if not self.slot_active:
            raise ApertisHipError(f"{what}: the cache is not in slot mode (KVCache.slots_begin)")
        if isinstance(b, bool) or not isinstance(b, int) or not 0 <= b < self.k[0].shape[0]:
            raise ApertisHipError(f"{what}: slot {b!r} outside [0, {self.k[0].shape[0]})")

    def slot_install(self, b, past):
        """A batch-1 prefill's `past_key_values` (per layer (k, v), [1, L, W]) into slot b: rows [0, L) of every layer are
        copied, `dev_lens[b]` = L, `dev_valid[b]` = (column < L).  The slot's next step appends row L at rotary position L."""
        self._slot("KVCache.slot_install", b)
        _, cap, W = self.k[0].shape
        if len(past) != len(self.k):
            raise ApertisHipError(f"KVCache.slot_install: a prefill of {len(past)} layers for a cache of {len(self.k)}")
        L = past[0][0].shape[1] if past[0][0].dim() == 3 else -1
        for k, v in past:
            if tuple(k.shape) != (1, L, W) or tuple(v.shape) != (1, L, W) or k.dtype != self.dtype or v.dtype != self.dtype:
                raise ApertisHipError(f"KVCache.slot_install: k {tuple(k.shape)} {k.dtype}, v {tuple(v.shape)} {v.dtype} for a "
                                      f"slot of [{cap}, {W}] {self.dtype} (one [1, L, {W}] pair per layer)")
        if L > cap:
            raise ApertisHipError(f"KVCache.slot_install: {L} rows do not fit a slot of {cap}")
        for i, (k, v) in enumerate(past):
            self.k[i][b, :L].copy_(k[0])
            self.v[i][b, :L].copy_(v[0])
        self.dev_lens[b] = L
        self.dev_valid[b].copy_(self._cols < L)

    def slot_free(self, b):
        """Slot b empty: `dev_lens[b]` = 0 and `dev_valid[b]` = 0, so that a free row does not hold `dev_len` (the maximum,
        the keys every row's work-groups walk) up.  Its K and V rows stay as they are: nothing reads them."""
        self._slot("KVCache.slot_free", b)
        self.dev_lens[b] = 0
        self.dev_valid[b].zero_()

    def slots_step_begin(self):
        """Once per token step, BEFORE the forward: the validity column of the row each slot is about to append
        (`dev_valid[b, dev_lens[b]]` = 1 - attention_decode_slots counts the new token's own key) and `dev_len` = the largest
        `dev_lens`.  Device work only (a captured graph replays it).  A FULL slot (slot_install of `capacity` rows) has no
        row to append: its step writes nothing and sets `dev_err` (kv_append_rope_slots); the index is clamped here so that
        the scatter stays inside the buffer for it too."""
        self.dev_valid.scatter_(1, self.dev_lens.clamp(max=self.capacity - 1).unsqueeze(1), 1)
        torch.amax(self.dev_lens, 0, keepdim=True, out=self.dev_len)

    def slots_step_end(self, alive):
        """Once per token step, AFTER the selection: `dev_lens` = min(dev_lens + alive, capacity - 1), `alive` int64 [B] of
        0 / 1.  THE CLAMP IS REQUIRED: inside a burst a row that has used up its budget is still alive on the device until
        the host reads the burst; such a row must neither trip `dev_err` nor write outside its slot, so it rewrites its own
        last row, and the host discards its tokens.  A row that is not alive (free, or past its eos) stays where it is and
        rewrites that row."""
        self.dev_lens.add_(alive).clamp_(max=self.capacity - 1)

    def _workspace(self, nbytes):
        if nbytes and (self._ws is None or self._ws.numel() * 4 < nbytes):
            self._ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=self.k[0].device)
        return self._ws if nbytes else None


def _append_operands(what, q, k, v, cache, layer, cos, sin):
    """What both appends hand to the library: q, k, v as rows with their strides, the rotary table and its length (0: no
    rotation) and the output for the rotated q."""
    B, cap, W = cache.k[layer].shape
    q, q_rs = _row2d(q, W, f"{what} q")
    k, k_rs = _row2d(k, W, f"{what} k")
    v, v_rs = _row2d(v, W, f"{what} v")
    if not (q.shape[0] == k.shape[0] == v.shape[0] == B and q.dtype == k.dtype == v.dtype == cache.dtype):
        raise ApertisHipError(f"{what}: q/k/v {tuple(q.shape)} {q.dtype} against a cache of [{B}, {cap}, {W}] {cache.dtype}")
    cos, sin, max_pos = _rope_table(what, cos, sin, W)
    qo = torch.empty(B, W, device=q.device, dtype=q.dtype)
    return (q, q_rs), (k, k_rs), (v, v_rs), cos, sin, max_pos, qo


def _decode_operands(what, lib, q, cache, layer, heads, splits):
    """What both attentions hand to the library: the query rows, 16-byte aligned, with their stride, D, the cache's
    workspace for `splits` pieces (a count, or a function of D asked once q has passed its check; None where the library
    refuses the count) and the output."""
    B, cap, W = cache.k[layer].shape
    q, q_rs = _row2d(q, W, f"{what} q")
    if not attention_decode_supported(q, heads) or q.shape[0] != B or q.dtype != cache.dtype:
        raise ApertisHipError(f"{what}: q {tuple(q.shape)} {q.dtype} with {heads} heads against a cache of "
                              f"[{B}, {cap}, {W}] {cache.dtype} (D 64 or 128, fp32 or bf16, one dtype)")
    q, q_rs = _aligned_rows(q, q_rs, W)
    D, ws = W // heads, None
    n = splits(D) if callable(splits) else splits
    if 1 <= n <= ATTN_DECODE_MAX_SPLITS:
        ws = cache._workspace(max(int(lib.apertis_attention_decode_workspace_bytes(B, heads, D, n)), 0))
    return q, q_rs, D, ws, torch.empty(B, W, device=q.device, dtype=q.dtype)


def kv_append_rope(q, k, v, cache, layer, t=None, cos=None, sin=None):
    """One token of every sequence into layer `layer` of `cache`, in ONE launch: q and k ([B, W] or [B, 1, W]) are rotated at
    rotary position `t` (a host integer; default: the row appended to) with the module's fp32 cos_cached / sin_cached - the
    same bits as rope_qk - rotated k and v go into cache row `lengths[layer]`, IN PLACE, and that length grows by one.
    cos = sin = None: no rotation, a plain append.  Returns the rotated q [B, W].  `t` outside [-max_pos, max_pos) raises
    IndexError as the stock module's table lookup does; a full cache raises before anything is written."""
    _require_gpu(q, k, v, cache.k[layer], cos, sin)
    lib = _lib.load()
    B, cap, W = cache.k[layer].shape
    row = cache.lengths[layer]
    if row >= cap:
        raise ApertisHipError(f"kv_append_rope: the cache is full ({cap} rows)")
    (q, q_rs), (k, k_rs), (v, v_rs), cos, sin, max_pos, qo = _append_operands("kv_append_rope", q, k, v, cache, layer, cos, sin)
    t = row if t is None else int(t)
    if cos is not None and not -max_pos <= t < max_pos:
        raise IndexError(f"position {t} outside the rotary table of {max_pos} positions")
    kc, vc = cache.k[layer], cache.v[layer]
    _launch("apertis_rope_kv_append", lib.apertis_rope_kv_append,
            (ptr(q), q_rs, ptr(k), k_rs, ptr(v), v_rs, ptr(cos), ptr(sin), max_pos, t, ptr(qo), W, ptr(kc), kc.stride(1),
             kc.stride(0), ptr(vc), vc.stride(1), vc.stride(0), cap, row, B, W, dtype_code(q), stream_ptr()),
            work=5.0 * B * W * q.element_size())
    cache.lengths[layer] = row + 1
    return qo


def attention_decode_supported(q, heads):
    """Whether attention_decode takes one query row per sequence of this width and dtype (D 64 or 128, fp32 or bf16);
    q: [B, W] or [B, L, W]."""
    return (q.dim() in (2, 3) and q.shape[-1] % heads == 0 and q.shape[-1] // heads in (64, 128)
            and q.dtype in (torch.float32, torch.bfloat16))


def attention_decode_splits(B, heads, Lk, D):
    """The number of pieces attention_decode cuts Lk keys into when splits = 0 (a pure function of the shape)."""
    return int(_lib.load().apertis_attention_decode_splits(B, heads, Lk, D))


def attention_decode(q, cache, layer, heads, key_valid=None, splits=0, window=None):
    """softmax(q K^T / sqrt(D)) V for ONE query row per sequence and head over the rows layer `layer` of `cache` holds
    (Lk = lengths[layer]: after kv_append_rope, the new token's own key included).  q: [B, W] or [B, 1, W] in the cache's dtype
    (fp32 or bf16, D = W / heads in {64, 128}); returns O [B, W] where out_proj reads it.  key_valid: [B, >= Lk] (the raw
    attention_mask, nonzero = attend; columns >= Lk are never read) or None.  splits: 0 = apertis_attention_decode_splits'
    choice, else 1..min(Lk, ATTN_DECODE_MAX_SPLITS) pieces of the key range (tests reach every value); the same inputs and split count give
    the same bits.
    window (an integer >= 1, or None): only the last `window` rows count (a sliding window: the query is the newest row).
    With Lk > window the SAME launch runs on k, v and key_valid offset by begin = Lk - window rows / columns, with Lk' =
    window and capacity' = capacity - begin: nothing is copied, the split count is chosen for Lk', and rows before `begin`
    are never read.  With Lk <= window the call is the one without a window."""
    _require_gpu(q, cache.k[layer], key_valid)
    lib = _lib.load()
    kc, vc = cache.k[layer], cache.v[layer]
    B, cap, W = kc.shape
    Lk = cache.lengths[layer]
    begin = max(Lk - _window("attention_decode", window), 0) if window is not None else 0
    n = int(splits) if splits else lambda D: int(lib.apertis_attention_decode_splits(B, heads, max(Lk - begin, 1), D)) if B else 1
    q, q_rs, D, ws, out = _decode_operands("attention_decode", lib, q, cache, layer, heads, n)
    key_valid, kv_rs = _mask_rows("attention_decode", key_valid, B, Lk)
    # (pointer arithmetic on the host, no views: the launch reads the same buffers from row / column `begin` on)
    es, cap, Lk = q.element_size(), cap - begin, Lk - begin
    kp, vp = ptr(kc) + begin * kc.stride(1) * es, ptr(vc) + begin * vc.stride(1) * es
    kvp = ptr(key_valid) + begin * 8 if key_valid is not None else None
    nbytes = 2.0 * B * Lk * W * es
    _launch("apertis_attention_decode", lib.apertis_attention_decode,
            (ptr(q), q_rs, kp, kc.stride(1), kc.stride(0), vp, vc.stride(1), vc.stride(0), cap, kvp, kv_rs,
             ptr(out), W, ptr(ws), B, Lk, heads, D, int(splits), dtype_code(q), stream_ptr()),
            work=4.0 * B * Lk * W, detail=f"{B}x{heads}x{D}", nbytes=nbytes)
    return out


# ------------------------------------------------------------------------------------------------- multi-token steps
def kv_append_rope_chunk(q, k, v, cache, layer, t0=None, cos=None, sin=None):
    """A chunk of Lq tokens of every sequence into layer `layer` of `cache`, in ONE launch: rows l of q and k ([B, Lq, W]) are
    rotated at rotary position `t0 + l` (a host integer; default: the first row appended to) with the module's fp32
    cos_cached / sin_cached - the same bits as rope_qk at those positions - rotated k and v go into cache rows
    `lengths[layer] + l`, IN PLACE, and that length grows by Lq.  cos = sin = None: no rotation, a plain append.  Returns
    the rotated q [B, Lq, W].  A position outside [-max_pos, max_pos) raises IndexError as the stock module's table lookup
    does; a chunk that does not fit raises before anything is written."""
    _require_gpu(q, k, v, cache.k[layer], cos, sin)
    lib = _lib.load()
    kc, vc = cache.k[layer], cache.v[layer]
    B, cap, W = kc.shape
    row = cache.lengths[layer]
    (q, q_rs, q_bs), (k, k_rs, k_bs), (v, v_rs, v_bs) = (_chunk3d(t, B, W, f"kv_append_rope_chunk {n}")
                                                          for t, n in ((q, "q"), (k, "k"), (v, "v")))
    Lq = q.shape[1]
    if not (k.shape[1] == v.shape[1] == Lq and q.dtype == k.dtype == v.dtype == cache.dtype):
        raise ApertisHipError(f"kv_append_rope_chunk: q/k/v {tuple(q.shape)} {tuple(k.shape)} {tuple(v.shape)} {q.dtype} against "
                              f"a cache of [{B}, {cap}, {W}] {cache.dtype}")
    if row + Lq > cap:
        raise ApertisHipError(f"kv_append_rope_chunk: {Lq} rows do not fit ({row} of {cap} rows held)")
    cos, sin, max_pos = _rope_table("kv_append_rope_chunk", cos, sin, W)
    t0 = row if t0 is None else int(t0)
    if cos is not None and Lq and not (-max_pos <= t0 and t0 + Lq <= max_pos):
        raise IndexError(f"positions {t0}..{t0 + Lq - 1} outside the rotary table of {max_pos} positions")
    qo = torch.empty(B, Lq, W, device=q.device, dtype=q.dtype)
    _launch("apertis_rope_kv_append_chunk", lib.apertis_rope_kv_append_chunk,
            (ptr(q), q_rs, q_bs, ptr(k), k_rs, k_bs, ptr(v), v_rs, v_bs, ptr(cos), ptr(sin), max_pos, t0, ptr(qo), ptr(kc),
             kc.stride(1), kc.stride(0), ptr(vc), vc.stride(1), vc.stride(0), cap, row, B, Lq, W, dtype_code(q), stream_ptr()),
            work=5.0 * B * Lq * W * q.element_size())
    cache.lengths[layer] = row + Lq
    return qo


def attention_chunk_splits(B, heads, Lq, Lk, D):
    """The number of runs attention_chunk cuts every wave's key tiles into when splits = 0 (a pure function of the shape)."""
    return int(_lib.load().apertis_attention_chunk_splits(B, heads, Lq, Lk, D))


def attention_chunk_workspace_bytes(B, heads, Lq, D, splits):
    """Bytes of fp32 workspace attention_chunk takes from the cache for `splits` runs (0 for one)."""
    return int(_lib.load().apertis_attention_chunk_workspace_bytes(B, heads, Lq, D, splits))


def attention_chunk(q, cache, layer, heads, key_valid=None, splits=0, dead_rows=False, window=None):
    """Causal softmax attention of the Lq rows kv_append_rope_chunk has JUST appended to layer `layer` of `cache` over
    everything the layer holds: row i of q ([B, Lq, W], the cache's dtype, D = W / heads in {64, 128}) sits at key position
    n + i, n = lengths[layer] - Lq, and attends keys j <= n + i.  Returns O [B, Lq, W] where out_proj reads it.  key_valid:
    [B, >= n + Lq] (the raw attention_mask, nonzero = attend; later columns are never read) or None.  splits: 0 =
    apertis_attention_chunk_splits' choice, else 1..ATTN_DECODE_MAX_SPLITS runs of every wave's key tiles; the same inputs and
    split count give the same bits, and at one split row i has the bits causal_attention gives row n + i of the whole
    sequence.  Inference only (no dropout, nothing saved for a backward).  A row with no valid key at or before it comes out
    as zeros; dead_rows=True fills such rows (after the merge of the runs) with the reference's value, the column mean of the
    layer's v rows [0, n + Lq) (attention_dead_rows; it raises when q requires grad under autograd).
    window (an integer >= 1, or None): a sliding window - row i attends keys j with n + i - window < j <= n + i.  With
    n + Lq > window the launch is apertis_attention_chunk_window (key tiles in front of a wave's window are never touched; at
    one split row i has the bits window_attention gives row n + i of the whole sequence; splits = 0 asks the same rule at
    min(n + Lq, window + Lq) keys, the most a wave walks - no sizing point has been measured for the windowed walk);
    otherwise it is the call without a window.  dead_rows keeps its meaning (a row with no valid key at or before it, over
    [0, n + Lq), as window_attention(dead_rows=True) fills them)."""
    _require_gpu(q, cache.k[layer], key_valid)
    if dead_rows:
        _dead_rows_inference("attention_chunk", False, 0.0, q)
    lib = _lib.load()
    kc, vc = cache.k[layer], cache.v[layer]
    B, cap, W = kc.shape
    if q.dim() != 3 or q.shape[0] != B or q.shape[1] < 1 or not attention_decode_supported(q, heads) or q.dtype != cache.dtype:
        raise ApertisHipError(f"attention_chunk: q {tuple(q.shape)} {q.dtype} with {heads} heads against a cache of "
                              f"[{B}, {cap}, {W}] {cache.dtype} (D 64 or 128, fp32 or bf16, one dtype)")
    Lq, Lk = q.shape[1], cache.lengths[layer]
    if window is not None and _window("attention_chunk", window) >= Lk:
        window = None                                      # (every row sees all of its keys: the call without a window)
    if Lq > Lk:
        raise ApertisHipError(f"attention_chunk: {Lq} query rows but the layer holds {Lk} (kv_append_rope_chunk first)")
    q, q_rs = _aligned_rows(*_rows(q, W), W)
    D, ns, ws = W // heads, int(splits), None              # ns: the split count the workspace is sized for AND the launch takes
    walk = Lk if window is None else min(Lk, window + Lq)  # the keys a wave walks at most
    if ns == 0:
        ns = int(lib.apertis_attention_chunk_splits(B, heads, Lq, walk, D)) if B else 1
    if 1 <= ns <= ATTN_DECODE_MAX_SPLITS:
        ws = cache._workspace(max(int(lib.apertis_attention_chunk_workspace_bytes(B, heads, Lq, D, ns)), 0))
    key_valid, kv_rs = _mask_rows("attention_chunk", key_valid, B, Lk)
    out = torch.empty(B, Lq, W, device=q.device, dtype=q.dtype)
    if window is None:
        _launch("apertis_attention_chunk", lib.apertis_attention_chunk,
                (ptr(q), q_rs, ptr(kc), kc.stride(1), kc.stride(0), ptr(vc), vc.stride(1), vc.stride(0), cap, ptr(key_valid), kv_rs,
                 ptr(out), W, ptr(ws), B, Lq, Lk - Lq, heads, D, ns, dtype_code(q), stream_ptr()),
                work=4.0 * B * W * Lq * (Lk - Lq + (Lq + 1) / 2), detail=f"{B}x{heads}x{D}x{Lq}",
                nbytes=(2.0 * B * Lk + 2.0 * B * Lq) * W * q.element_size())
    else:
        pairs = window_pairs(Lk, window) - window_pairs(Lk - Lq, window)           # (query, key) pairs of the chunk's rows
        _launch("apertis_attention_chunk_window", lib.apertis_attention_chunk_window,
                (ptr(q), q_rs, ptr(kc), kc.stride(1), kc.stride(0), ptr(vc), vc.stride(1), vc.stride(0), cap, ptr(key_valid), kv_rs,
                 ptr(out), W, ptr(ws), B, Lq, Lk - Lq, window, heads, D, ns, dtype_code(q), stream_ptr()),
                work=4.0 * B * W * pairs, detail=f"{B}x{heads}x{D}x{Lq}",
                nbytes=(2.0 * B * walk + 2.0 * B * Lq) * W * q.element_size())
    if dead_rows and key_valid is not None and B:
        attention_dead_rows(out, vc, key_valid, Lk - Lq)
    return out


def _step_state(cache, what):
    if cache.dev_len is None:
        raise ApertisHipError(f"{what}: the cache has no device step state (KVCache.step_state_begin)")


def kv_append_rope_at(q, k, v, cache, layer, cos=None, sin=None, pos_offset=0):
    """kv_append_rope at the cache's DEVICE length: row `dev_len[0]` of layer `layer`, rotary position `dev_len[0] +
    pos_offset`, both read by the kernel - no host length, nothing a captured graph would freeze.  The same bits as
    kv_append_rope for the same row and position.  It moves neither `dev_len` (one step of all layers shares it; the caller
    adds one after the last) nor the host `lengths`.  A row outside the cache or a position outside the rotary table writes
    NOTHING and sets `cache.dev_err` - the host cannot check a replayed step, so the kernel does.  Returns the rotated q."""
    _step_state(cache, "kv_append_rope_at")
    _require_gpu(q, k, v, cache.k[layer], cos, sin)
    lib = _lib.load()
    B, cap, W = cache.k[layer].shape
    (q, q_rs), (k, k_rs), (v, v_rs), cos, sin, max_pos, qo = _append_operands("kv_append_rope_at", q, k, v, cache, layer, cos, sin)
    kc, vc = cache.k[layer], cache.v[layer]
    _launch("apertis_rope_kv_append_at", lib.apertis_rope_kv_append_at,
            (ptr(q), q_rs, ptr(k), k_rs, ptr(v), v_rs, ptr(cos), ptr(sin), max_pos, ptr(cache.dev_len), int(pos_offset),
             ptr(cache.dev_err), ptr(qo), W, ptr(kc), kc.stride(1), kc.stride(0), ptr(vc), vc.stride(1), vc.stride(0), cap, B, W,
             dtype_code(q), stream_ptr()), work=5.0 * B * W * q.element_size())
    return qo


def _decode_dev(what, q, cache, layer, heads, splits, win):
    """The launch attention_decode_at and attention_decode_slots share: `dev_len`, `dev_valid` and the fixed split count of
    `cache`, under a window `win` or None."""
    _require_gpu(q, cache.k[layer])
    lib = _lib.load()
    kc, vc = cache.k[layer], cache.v[layer]
    B, cap, W = kc.shape
    n = cache.step_splits if splits is None else int(splits)
    q, q_rs, D, ws, out = _decode_operands(what, lib, q, cache, layer, heads, n)
    kv = cache.dev_valid
    if win is None:
        _launch("apertis_attention_decode_at", lib.apertis_attention_decode_at,
                (ptr(q), q_rs, ptr(kc), kc.stride(1), kc.stride(0), ptr(vc), vc.stride(1), vc.stride(0), cap, ptr(cache.dev_len),
                 ptr(kv), kv.stride(0), ptr(out), W, ptr(ws), B, heads, D, n, dtype_code(q), stream_ptr()),
                work=4.0 * B * cap * W, detail=f"{B}x{heads}x{D}", nbytes=2.0 * B * cap * W * q.element_size())
    else:
        keys = min(cap, win)                               # (the most a step reads: the device length is not known here)
        _launch("apertis_attention_decode_window_at", lib.apertis_attention_decode_window_at,
                (ptr(q), q_rs, ptr(kc), kc.stride(1), kc.stride(0), ptr(vc), vc.stride(1), vc.stride(0), cap, ptr(cache.dev_len),
                 win, ptr(kv), kv.stride(0), ptr(out), W, ptr(ws), B, heads, D, n, dtype_code(q), stream_ptr()),
                work=4.0 * B * keys * W, detail=f"{B}x{heads}x{D}", nbytes=2.0 * B * keys * W * q.element_size())
    return out


def attention_decode_at(q, cache, layer, heads, splits=None):
    """attention_decode over Lk = min(dev_len[0] + 1, capacity) keys, read by the kernel (after kv_append_rope_at and BEFORE
    `dev_len` moves: the new token's own key included), under the cache's `dev_valid`.  splits: the FIXED number of pieces,
    1..ATTN_DECODE_MAX_SPLITS, not bounded by Lk (default: what step_state_begin chose) - grid and workspace depend on it
    alone, an empty piece contributes nothing.  The same bits as attention_decode(..., splits=n) for the same Lk.
    With `cache.step_window` set (step_state_begin(window=)) the launch is apertis_attention_decode_window_at: only keys
    [max(Lk - window, 0), Lk) are cut into the pieces and read - the bits of attention_decode(..., window=, splits=n)."""
    _step_state(cache, "attention_decode_at")
    return _decode_dev("attention_decode_at", q, cache, layer, heads, splits, cache.step_window)


# ------------------------------------------------------------------------------------------------- slots: per-row lengths
# The library's appends take ONE row and ONE position for all sequences, and its attentions read ONE length.  A slot has a
# length of its own.  These two ops are the only places that know how that is driven through the entry points as they are;
# a per-row kernel, once the C ABI has one, replaces their bodies and nothing above them.
def _slot_state(cache, what):
    if not cache.slot_active:
        raise ApertisHipError(f"{what}: the cache is not in slot mode (KVCache.slots_begin)")


def kv_append_rope_slots(q, k, v, cache, layer, cos=None, sin=None):
    """kv_append_rope_at for a cache in slot mode: row b of q, k, v ([S, W] or [S, 1, W]) goes into row `dev_lens[b]` of slot
    b at rotary position `dev_lens[b]`.  S launches of apertis_rope_kv_append_at with B = 1, each on pointers offset to its
    row (host arithmetic, no views) and on `&dev_lens[b]` as its length: the same kernel, position and per-thread arithmetic
    as kv_append_rope on that row alone, so the same bits.  It moves no length (slots_step_end does, once per step).  A row
    outside the slot or a position outside the rotary table writes nothing and sets `cache.dev_err`.  Returns the rotated
    q [S, W], one buffer."""
    _slot_state(cache, "kv_append_rope_slots")
    _require_gpu(q, k, v, cache.k[layer], cos, sin)
    lib = _lib.load()
    S, cap, W = cache.k[layer].shape
    (q, q_rs), (k, k_rs), (v, v_rs), cos, sin, max_pos, qo = _append_operands("kv_append_rope_slots", q, k, v, cache, layer, cos,
                                                                              sin)
    kc, vc = cache.k[layer], cache.v[layer]
    es, fn, code, st = q.element_size(), lib.apertis_rope_kv_append_at, dtype_code(q), stream_ptr()
    qp, kp, vp, qop, kcp, vcp = ptr(q), ptr(k), ptr(v), ptr(qo), ptr(kc), ptr(vc)
    lens, err, cs, sn = ptr(cache.dev_lens), ptr(cache.dev_err), ptr(cos), ptr(sin)
    kc_rs, kc_bs, vc_rs, vc_bs = kc.stride(1), kc.stride(0), vc.stride(1), vc.stride(0)
    for b in range(S):
        _launch("apertis_rope_kv_append_at", fn,
                (qp + b * q_rs * es, q_rs, kp + b * k_rs * es, k_rs, vp + b * v_rs * es, v_rs, cs, sn, max_pos, lens + 8 * b, 0,
                 err, qop + b * W * es, W, kcp + b * kc_bs * es, kc_rs, kc_bs, vcp + b * vc_bs * es, vc_rs, vc_bs, cap, 1, W,
                 code, st), work=5.0 * W * es)
    return qo


def attention_decode_slots(q, cache, layer, heads, splits=None):
    """attention_decode for a cache in slot mode, after kv_append_rope_slots: row b attends keys [0, dev_lens[b]] of slot b.
    ONE apertis_attention_decode_at launch over all slots on `dev_len` (the largest slot length, slots_step_begin) under
    `dev_valid`: a key past a slot's own length is masked, a masked key is never read and scores -inf exactly like a key out
    of range - no bit of (m, l, o) moves - and a wave's walk starts at j0 + w * KPW whatever the key count is; so at
    splits = 1 row b has the bits of attention_decode(..., splits=1) on that row alone with Lk = dev_lens[b] + 1.  splits:
    the fixed number of pieces (default: what slots_begin chose); the pieces cut the LONGEST row's range."""
    _slot_state(cache, "attention_decode_slots")
    return _decode_dev("attention_decode_slots", q, cache, layer, heads, splits, None)
