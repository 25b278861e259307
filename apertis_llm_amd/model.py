"""Host-side mirror of the reference's model API for the hot path (Python, as the reference is).

Same importable names, constructor keywords, config fields, state-dict keys and forward
contracts as /root/reference/src/model/core.py, so a checkpoint or a `config.json` written by
either side loads in the other and `apertis train` / `apertis chat` callers need no change.
What differs is underneath: the selective scan, the depthwise conv, the gate, the SSM block's
dense projections, LayerNorm and the sub-block boundaries, the whole MoE dispatch, the expert
GEMMs, the dense FFN, the cross-entropy and the optimizer step run as HIP kernels through
libapertis_hip.so (apertis_llm_amd.ops); stock torch (hipBLASLt) keeps the embedding, the LM head's
GEMMs, the ViT body and the `standard_mha` paths the attention kernels do not take (decode with a KV cache,
output_attentions, head dims other than 64 / 128, left padding).  There is no eager fallback for the kernel
paths: off-GPU they raise ApertisHipError.
"""
import functools
import inspect
import itertools
import json
import logging
import math
import os
from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple, Union

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .multimodal import UnifiedMultimodalEncoder
from .ops._base import _compute_dtype          # (shared with the vision tower)

logger = logging.getLogger(__name__)


def _on_input_device(fn):
    """Run a module's forward with its first tensor argument's device current.  Stock torch ops guard themselves; the
    C-ABI kernels launch on the CURRENT HIP device and stream, so a model placed on cuda:1 without
    torch.cuda.set_device(1) (the reference's trainer never calls it, pipeline.py:447-460) would otherwise launch its
    kernels on GPU 0's stream.  No-op when the device is already current or the input is not on a GPU."""
    @functools.wraps(fn)
    def wrapper(self, *args, **kwargs):
        t = next((a for a in (*args, *kwargs.values()) if isinstance(a, torch.Tensor)), None)
        if t is None or not t.is_cuda or t.device.index == torch.cuda.current_device():
            return fn(self, *args, **kwargs)
        with ops.device_guard(t):
            return fn(self, *args, **kwargs)
    return wrapper


# ----------------------------------------------------------------------------------------------
# ApertisConfig  (reference core.py:67-256)
# ----------------------------------------------------------------------------------------------
class ApertisConfig:
    """Flat config object; `to_dict()` is the full attribute dict and round-trips through
    `config.json` exactly like the reference's (core.py:212-256)."""

    def __init__(self, vocab_size: int = 32000, hidden_size: int = 768, num_hidden_layers: int = 12,
                 num_attention_heads: int = 12, intermediate_size: int = 3072, hidden_act: str = "gelu",
                 hidden_dropout_prob: float = 0.1, attention_probs_dropout_prob: float = 0.1,
                 max_position_embeddings: int = 2048, type_vocab_size: int = 2, initializer_range: float = 0.02,
                 layer_norm_eps: float = 1e-12, pad_token_id: int = 0, bos_token_id: int = 1, eos_token_id: int = 2,
                 unk_token_id: int = 3, position_embedding_type: str = "rotary", use_cache: bool = True,
                 classifier_dropout: float = None, model_type: str = "apertis", tie_word_embeddings: bool = True,
                 rope_theta: float = 10000.0, sliding_window: Optional[int] = None,
                 attention_type: str = "standard_mha", ssm_d_inner: Optional[int] = None, ssm_d_state: int = 16,
                 ssm_dt_rank: Union[int, str] = "auto", ssm_conv_kernel: int = 4, use_flash_attention: bool = False,
                 use_expert_system: bool = False, num_experts: int = 8, experts_per_token: int = 2,
                 multimodal: bool = False, image_size: int = 224, vision_embed_dim: int = 768,
                 vision_patch_size: int = 16, vision_layers: int = 12, vision_heads: int = 12,
                 output_attentions: bool = False, output_hidden_states: bool = False,
                 load_balancing_loss_coef: float = 0.01, expert_capacity_factor: float = 1.25,
                 noisy_routing_alpha: float = 0.1, expert_dropout_prob: float = 0.1,
                 router_z_loss_coef: float = 0.001, expert_output_gating: bool = False,
                 use_noisy_top_k_routing: bool = True, use_expert_capacity_limit: bool = True,
                 use_expert_dropout: bool = True, use_router_z_loss: bool = True,
                 use_load_balancing_loss: bool = True, use_rmsnorm: bool = False, use_swiglu: bool = False,
                 **kwargs):
        given = dict(locals())
        # attribute order follows the reference so a dumped config.json lists keys identically
        for name in ("vocab_size", "hidden_size", "num_hidden_layers", "num_attention_heads", "hidden_act",
                     "intermediate_size", "hidden_dropout_prob", "attention_probs_dropout_prob",
                     "max_position_embeddings", "type_vocab_size", "initializer_range", "layer_norm_eps",
                     "pad_token_id", "bos_token_id", "eos_token_id", "unk_token_id", "position_embedding_type",
                     "use_cache", "classifier_dropout", "model_type", "tie_word_embeddings", "rope_theta",
                     "sliding_window", "attention_type", "ssm_d_state"):
            setattr(self, name, given[name])
        derived = num_attention_heads * ssm_d_state
        if attention_type == "selective_ssm":                         # core.py:153-157
            if ssm_d_inner is not None and ssm_d_inner != derived:
                logger.warning("ssm_d_inner=%s overridden by num_attention_heads*ssm_d_state=%s", ssm_d_inner, derived)
            self.ssm_d_inner = derived
        else:
            self.ssm_d_inner = 2 * hidden_size if ssm_d_inner is None else ssm_d_inner
        self.ssm_dt_rank = math.ceil(hidden_size / 16) if ssm_dt_rank == "auto" else int(ssm_dt_rank)
        for name in ("ssm_conv_kernel", "use_flash_attention", "use_expert_system", "num_experts",
                     "experts_per_token", "multimodal", "image_size", "vision_embed_dim", "vision_patch_size",
                     "vision_layers", "vision_heads", "output_attentions", "output_hidden_states",
                     "load_balancing_loss_coef", "expert_capacity_factor", "noisy_routing_alpha",
                     "expert_dropout_prob", "router_z_loss_coef", "expert_output_gating", "use_noisy_top_k_routing",
                     "use_expert_capacity_limit", "use_expert_dropout", "use_router_z_loss",
                     "use_load_balancing_loss", "use_rmsnorm", "use_swiglu"):
            setattr(self, name, given[name])
        if not use_expert_system:                                     # core.py:200-204
            self.num_experts = 0
            self.experts_per_token = 0
        else:
            self.experts_per_token = min(num_experts, experts_per_token) if num_experts > 0 else 0
        for key, value in kwargs.items():
            if not hasattr(self, key):
                logger.warning("Ignoring unknown config parameter: %s=%s", key, value)

    @classmethod
    def from_dict(cls, config_dict: Dict[str, Any]):
        params = inspect.signature(cls.__init__).parameters
        keep = {k: v for k, v in config_dict.items() if (k in params and k != "self") or k == "kwargs"}
        if keep.get("ssm_dt_rank") == "auto":
            keep["ssm_dt_rank"] = math.ceil(keep.get("hidden_size", 768) / 16)
        return cls(**keep)

    def to_dict(self) -> Dict[str, Any]:
        return self.__dict__

    @classmethod
    def from_pretrained(cls, model_name_or_path: str):
        if os.path.isfile(model_name_or_path) and model_name_or_path.endswith(".json"):
            path = model_name_or_path
        else:
            path = os.path.join(model_name_or_path, "config.json")
            if not os.path.exists(path) and os.path.isdir(model_name_or_path):
                parent = os.path.join(Path(model_name_or_path).parent, "config.json")
                if os.path.exists(parent):
                    path = parent
        if not os.path.exists(path):
            raise FileNotFoundError(f"Config file not found. Looked for: '{path}' based on input '{model_name_or_path}'")
        with open(path, "r", encoding="utf-8") as f:
            return cls.from_dict(json.load(f))

    def save_pretrained(self, save_directory: str):
        os.makedirs(save_directory, exist_ok=True)
        with open(os.path.join(save_directory, "config.json"), "w", encoding="utf-8") as f:
            json.dump(self.to_dict(), f, indent=2)


def _activation_module(name: str) -> nn.Module:
    if name == "relu":
        return nn.ReLU()
    if name in ("silu", "swish"):
        return nn.SiLU()
    if name != "gelu":
        logger.warning("Unsupported activation %s; using GELU", name)
    return nn.GELU()


def _activation_name(name: str) -> str:
    return name if name in ("gelu", "relu", "silu", "swish") else "gelu"


class HipLayerNorm(nn.LayerNorm):
    """nn.LayerNorm (same parameters / checkpoint keys) whose GPU forward+backward are the HIP row
    kernels; under autocast it emits the compute dtype directly instead of fp32 + a cast kernel.
    Off-GPU (only the stock-torch standard_mha fallback gets there) it is plain F.layer_norm."""

    def forward(self, x):
        H = x.shape[-1]
        if x.is_cuda and H % 4 == 0 and H <= 4096 and x.dtype in (torch.float32, torch.bfloat16):
            return ops.layer_norm(x, self.weight, self.bias, self.eps, out_dtype=_compute_dtype(x))
        return super().forward(x)

    def forward_pass(self, x):
        """(LayerNorm(x), x) for a pre-norm residual block: adding the residual through the returned x lets
        the backward kernel fold the residual gradient into dx (ops.layer_norm_pass)."""
        H = x.shape[-1]
        if x.is_cuda and H % 4 == 0 and H <= 4096 and x.dtype in (torch.float32, torch.bfloat16):
            return ops.layer_norm_pass(x, self.weight, self.bias, self.eps, out_dtype=_compute_dtype(x))
        return self.forward(x), x


def _norm_pass(norm, x):
    return norm.forward_pass(x) if isinstance(norm, (HipLayerNorm, RMSNorm)) else (norm(x), x)


class _LazyCombine:
    """The MoE block's output before its combine (reference core.py:594,605): expert rows yr [rows,H], gate
    weights w [S,K] and the dispatch plan.  `_enter_block` forms the combine inside the boundary kernel;
    `materialise()` is the stand-alone combine."""
    __slots__ = ("yr", "w", "plan", "shape", "dtype")

    def __init__(self, yr, w, plan, shape, dtype):
        self.yr, self.w, self.plan, self.shape, self.dtype = yr, w, plan, shape, dtype

    def materialise(self):
        return ops.moe_combine(self.yr, self.w, self.plan, out_dtype=self.dtype).reshape(self.shape)


class _SsmLayerPast:
    """One SSM layer's cache as the layer receives it: it reads like the (conv window, SSM state) pair and carries the step's
    state.  `pre`: the layer's row of ApertisModel._decode_prepass (C s + D xc of this token step, the state already advanced)
    or None; `inplace`: the single-token step may update the buffers it is handed (generate()'s graph tail)."""
    __slots__ = ("conv", "state", "pre", "inplace")

    def __init__(self, conv, state, pre=None, inplace=False):
        self.conv, self.state, self.pre, self.inplace = conv, state, pre, inplace

    def __len__(self):
        return 2

    def __getitem__(self, j):
        return (self.conv, self.state)[j]

    def __iter__(self):
        return iter((self.conv, self.state))


class _StackedPast(list):
    """generate()'s static cache of an all-SSM model as ONE tensor per kind - conv windows [NL,B,Dn,k-1], states [NL,B,Dn] fp32 -
    with the usual per-layer (conv_state, ssm_state) pairs as views into them (_SsmLayerPast): the model then runs the
    cache-only half of a token step for every layer at once (ApertisModel._decode_prepass)."""

    def __init__(self, conv_all, state_all, heads, d_state, inplace=False):
        NL, B = conv_all.shape[0], conv_all.shape[1]
        super().__init__(_SsmLayerPast(conv_all[l], state_all[l].view(B, heads, d_state), inplace=inplace) for l in range(NL))
        self.conv_all, self.state_all = conv_all, state_all
        self._offs = None

    def offsets(self, NL, B):
        if self._offs is None:
            self._offs = (torch.arange(NL + 1, device=self.conv_all.device, dtype=torch.int32) * B).contiguous()
        return self._offs


class _Pending:
    """A sub-block's output that has not been added to the residual stream yet: the consumer either resolves
    it (`residual + dropout(out)`) or folds the add into its own pre-norm (`_enter_block`)."""
    __slots__ = ("out", "res", "drop")

    def __init__(self, out, res, drop):
        self.out, self.res, self.drop = out, res, drop

    def resolve(self):
        out = self.out.materialise() if isinstance(self.out, _LazyCombine) else self.out
        return _dropout_add(self.drop, out, self.res)


def _enter_block(norm, h, router=None):
    """(normalised input, residual) of a pre-norm sub-block.  When `h` is a _Pending boundary and the norm is a
    HipLayerNorm on the GPU, the residual add, its dropout and the norm run as ONE kernel in each direction.
    `router` = (router_norm, router Linear) of the MoE feed-forward this block is: its logits are then formed in the same
    forward pass and ride on the returned activation (`_apertis_router_logits`; AdaptiveExpertSystem.forward picks them up)."""
    if isinstance(h, _Pending):
        out, res = h.out, h.res
        H = res.shape[-1]
        cd = _compute_dtype(res)
        lazy = out if isinstance(out, _LazyCombine) else None
        if (isinstance(norm, RMSNorm) and ops.rms_norm_supported(res) and tuple(out.shape) == tuple(res.shape) and
                (res.dtype == torch.float32 or cd == res.dtype) and (lazy is None or lazy.dtype == lazy.yr.dtype == cd)):
            # the same boundary with an RMSNorm behind it; an MoE router in front keeps ops.router_ln_linear on xn
            blk, comb = (out, None) if lazy is None else (lazy.yr, (lazy.w, lazy.plan))
            y, xn = ops.dropout_add_rms_norm(blk, res, norm.scale, norm.eps, h.drop.p, h.drop.training, out_dtype=cd,
                                             combine=comb)
            return xn, y
        if (isinstance(norm, HipLayerNorm) and res.is_cuda and tuple(out.shape) == tuple(res.shape) and H % 4 == 0 and
                H <= 4096 and res.dtype in (torch.float32, torch.bfloat16) and
                (res.dtype == torch.float32 or cd == res.dtype) and (lazy is None or lazy.dtype == lazy.yr.dtype == cd)):
            if (router is not None and lazy is None and isinstance(router[0], nn.LayerNorm) and H <= 1024 and
                    router[1].weight.shape[0] in (2, 4, 8) and cd in (torch.float32, torch.bfloat16)):
                rn, rl = router
                y, xn, logits = ops.dropout_add_layer_norm_router(out, res, norm.weight, norm.bias, norm.eps, h.drop.p,
                                                                  h.drop.training, rn.weight, rn.bias, rn.eps, rl.weight,
                                                                  rl.bias, out_dtype=cd)
                xn._apertis_router_logits = logits
                return xn, y
            if lazy is not None:
                y, xn = ops.dropout_add_layer_norm(lazy.yr, res, norm.weight, norm.bias, norm.eps, h.drop.p,
                                                   h.drop.training, out_dtype=cd, combine=(lazy.w, lazy.plan))
            else:
                y, xn = ops.dropout_add_layer_norm(out, res, norm.weight, norm.bias, norm.eps, h.drop.p,
                                                   h.drop.training, out_dtype=cd)
            return xn, y
        h = h.resolve()
    return _norm_pass(norm, h)


def _dropout_add(drop: nn.Dropout, out, residual):
    """residual + dropout(out): one HIP kernel on the GPU, stock torch elsewhere."""
    if out.is_cuda and out.numel() % 4 == 0 and out.shape == residual.shape and \
            out.dtype in (torch.float32, torch.bfloat16) and residual.dtype in (torch.float32, torch.bfloat16) and \
            (residual.dtype == torch.float32 or out.dtype == residual.dtype):
        return ops.dropout_add(out, residual, drop.p, drop.training)
    return drop(out) + residual


# generate(): from this many remaining greedy tokens on, the single-token steps of an SSM model are replayed from a captured HIP
# graph (APERTIS_DECODE_GRAPH=0: always eager).  Capture costs about three eager steps.
DECODE_GRAPH = os.environ.get("APERTIS_DECODE_GRAPH", "1") == "1"
DECODE_GRAPH_MIN_STEPS = 24
# APERTIS_DECODE_PREPASS=0: every layer runs its whole single-token SSM step itself (conv, x_param_proj, state update inside the layer loop)
DECODE_PREPASS = os.environ.get("APERTIS_DECODE_PREPASS", "1") == "1"
# generate_many(): rows of the decode batch at most (the bound of ops.decode_dense_gemv and ops.moe_enter_small), and replayed
# token steps between two host reads at most (the cadence of generate()'s graph tail)
GENERATE_MANY_MAX_SLOTS = 16
GENERATE_MANY_BURST = 16


def _mfma_linear(x, weight, bias=None):
    """x @ W.T (+b) on the MFMA GEMM tile when the shapes allow 16-byte rows, else stock F.linear
    (both run on the GPU; this is a provider choice, not a fallback to the host)."""
    K = weight.shape[1]
    if x.is_cuda and K % 8 == 0 and weight.shape[0] % 8 == 0:
        return ops.linear_mfma(x, weight, bias, compute_dtype=_compute_dtype(x))
    if getattr(weight, "_apertis_prep", None) is not None:
        # (a TrainPrep placeholder carries shape and gradient route only: its values are uninitialised memory)
        raise ops.ApertisHipError(f"prepared-weight placeholder {tuple(weight.shape)} on the stock linear path")
    return F.linear(x, weight, bias)


class RMSNorm(nn.Module):
    """x / (||x||_2 / sqrt(D) + eps) * scale  (reference core.py:30-59).  On the GPU (fp32 / bf16, H % 4 == 0, H <= 4096,
    ops.RMSNORM_FUSED) forward and backward are the HIP row kernels, emitting the compute dtype under autocast as
    HipLayerNorm does; elsewhere the reference's stock-torch arithmetic."""

    def __init__(self, hidden_size: int, eps: float = 1e-6):
        super().__init__()
        self.hidden_size, self.eps = hidden_size, eps
        self.scale = nn.Parameter(torch.ones(hidden_size))

    def forward(self, x):
        if ops.rms_norm_supported(x):
            return ops.rms_norm(x, self.scale, self.eps, out_dtype=_compute_dtype(x))
        rms = x.norm(p=2, dim=-1, keepdim=True) * (self.hidden_size ** -0.5)
        return self.scale * (x / (rms + self.eps))

    def forward_pass(self, x):
        """(RMSNorm(x), x) for a pre-norm residual block: adding the residual through the returned x lets the backward
        kernel fold the residual gradient into dx (ops.rms_norm_pass)."""
        if ops.rms_norm_supported(x):
            return ops.rms_norm_pass(x, self.scale, self.eps, out_dtype=_compute_dtype(x))
        return self.forward(x), x


class RotaryEmbedding(nn.Module):
    """Interleaved-pair rotary embedding over the full projection width (reference core.py:258-293)."""

    def __init__(self, dim: int, max_position_embeddings: int = 2048, base: float = 10000):
        super().__init__()
        if dim % 2:
            raise ValueError(f"RoPE dimension must be even, got {dim}")
        self.dim, self.max_position_embeddings, self.base = dim, max_position_embeddings, base
        inv = 1.0 / (base ** (torch.arange(0, dim, 2, dtype=torch.float32) / dim))
        ang = torch.outer(torch.arange(max_position_embeddings, dtype=torch.float32), inv)
        self.register_buffer("inv_freq", inv, persistent=False)
        self.register_buffer("cos_cached", ang.cos(), persistent=False)
        self.register_buffer("sin_cached", ang.sin(), persistent=False)

    def forward(self, x, position_ids=None):
        B, L, _ = x.shape
        if position_ids is None:
            position_ids = torch.arange(L, device=x.device).unsqueeze(0)
        cos, sin = self.cos_cached[position_ids], self.sin_cached[position_ids]
        pairs = x.float().reshape(B, L, -1, 2)
        a, b = pairs[..., 0], pairs[..., 1]
        return torch.stack((a * cos - b * sin, a * sin + b * cos), dim=-1).reshape(B, L, self.dim).type_as(x)


# ----------------------------------------------------------------------------------------------
# SelectiveLinearAttention  (reference core.py:295-401) on HIP kernels
# ----------------------------------------------------------------------------------------------
class _SsmStarts:
    """What ApertisModel.forward hands the SSM layers in the mask slot (None otherwise) for a left-padded prefill under
    ops.SSM_LEFT_PAD: `start` int32 [B], the first valid token of every row (ops.left_pad_starts)."""
    __slots__ = ("start",)

    def __init__(self, start):
        self.start = start


class _SsmDocs:
    """What ApertisModel.forward hands the SSM layers in the mask slot for PACKED rows under ops.SSM_PACKED: `layout`, the
    ops.DocumentLayout of the forward (computed once; a checkpointed layer is recomputed with the same object)."""
    __slots__ = ("layout",)

    def __init__(self, layout):
        self.layout = layout


class SelectiveLinearAttention(nn.Module):
    """in_proj_x/z -> depthwise causal conv + SiLU -> x_param_proj -> (dt feats, Bt, C) ->
    softplus(dt_proj_head) -> selective scan -> +D*x -> *SiLU(z) -> out_proj.

    One code path for training, prefill and cached decode: the chunked HIP scan reproduces the
    sequential recurrence (core.py:337-353), which is what the reference's trainer actually
    executes (use_cache defaults to True).  The overflow-prone cumsum form (core.py:324-335) is
    not emulated."""

    def __init__(self, config: ApertisConfig):
        super().__init__()
        self.hidden_size = config.hidden_size
        self.num_heads = config.num_attention_heads
        self.d_state = config.ssm_d_state
        self.d_inner = self.num_heads * self.d_state
        self.dt_rank = config.ssm_dt_rank
        self.conv_kernel_size = config.ssm_conv_kernel
        self.in_proj_x = nn.Linear(self.hidden_size, self.d_inner, bias=False)
        self.in_proj_z = nn.Linear(self.hidden_size, self.d_inner, bias=False)
        # kept as nn.Conv1d so parameter names/shapes/initialisation match the checkpoint format
        self.conv1d = nn.Conv1d(self.d_inner, self.d_inner, self.conv_kernel_size, groups=self.d_inner,
                                padding=self.conv_kernel_size - 1)
        self.x_param_proj = nn.Linear(self.d_inner, self.dt_rank + 2 * self.d_inner, bias=False)
        self.dt_proj_head = nn.Linear(self.dt_rank, self.num_heads, bias=True)
        nn.init.uniform_(self.dt_proj_head.bias, a=math.log(1e-3), b=math.log(1e-2))
        self.A_log = nn.Parameter(torch.empty(self.num_heads, self.d_state).uniform_(math.log(0.5), math.log(0.99)))
        self.D = nn.Parameter(torch.ones(self.d_inner))
        self.out_proj = nn.Linear(self.d_inner, self.hidden_size, bias=False)
        self._pad_idx = None

    def _pad_index(self, device):
        """Destination row of every row of x_param_proj.weight ([dt | Bt | C]) in the padded layout [Bt | 0 | C | 0 | dt | 0]."""
        Dn, R = self.d_inner, self.dt_rank
        Wb = -(-Dn // 64) * 64
        idx = self._pad_idx
        if idx is None or idx.device != device:
            i = torch.arange(R + 2 * Dn)
            dst = torch.where(i < R, 2 * Wb + i, torch.where(i < R + Dn, i - R, Wb + i - R - Dn))
            idx = self._pad_idx = dst.to(device)
        return idx

    def register_train_prep(self, prep):
        """This block's GEMM weights into a TrainPrep (ops/prep.py): stacked in_proj, padded x_param_proj, out_proj."""
        Dn, R = self.d_inner, self.dt_rank
        Wb, Wr = -(-Dn // 64) * 64, -(-R // 64) * 64
        prep.add_stack(("in_proj_xz", id(self)), (self.in_proj_x.weight, self.in_proj_z.weight))
        prep.add_rowmap(("x_param_padded", id(self)), self.x_param_proj.weight, self._pad_index(self.x_param_proj.weight.device),
                        2 * Wb + Wr)
        prep.add_plain(self.out_proj.weight)

    def _padded_param_weight(self):
        """x_param_proj.weight with its output columns re-ordered and zero-padded so that, in the GEMM output p, the Bt
        and C column blocks each start on a 128-byte boundary and every row does too (core.py:376-381 reads them as
        [dt | Bt | C]; the scan reads whole 128-byte row segments): rows [Bt | 0 | C | 0 | dt | 0], block widths
        (Wb, Wb, Wr) multiples of 64 columns.  The GEMM tiles are 128 columns wide either way, so the pad costs no MFMA
        work.  Returns (weight [2*Wb + Wr, Dn], Wb, Wr)."""
        w, Dn, R = self.x_param_proj.weight, self.d_inner, self.dt_rank
        Wb, Wr = -(-Dn // 64) * 64, -(-R // 64) * 64
        if w.is_cuda:
            # source row i of [dt | Bt | C] lands at: dt -> 2*Wb + i, Bt -> i - R, C -> Wb + i - R - Dn
            return ops.scatter_rows(w, self._pad_index(w.device), 2 * Wb + Wr), Wb, Wr
        zb = w.new_zeros(Wb - Dn, Dn)
        zr = w.new_zeros(Wr - R, Dn)
        return torch.cat([w[R:R + Dn], zb, w[R + Dn:], zb, w[:R], zr], dim=0), Wb, Wr

    def _stacked_in_proj(self):
        """in_proj_x | in_proj_z as one [2 Dn, H] weight (core.py:366-367 share their input: one GEMM, the outputs are column views).
        Under no_grad - generate() - it is prepared once, not per token; inside a training step it comes prepared (ops.TrainPrep:
        one launch per step for the whole model) and is a placeholder that carries shape and gradient route only."""
        w_xz = ops.prepared_weight(("in_proj_xz", id(self)), (self.in_proj_x.weight, self.in_proj_z.weight))
        if w_xz is None:
            w_xz = ops.cached_prep("in_proj_xz", (self.in_proj_x.weight, self.in_proj_z.weight),
                                   lambda: torch.cat([self.in_proj_x.weight, self.in_proj_z.weight], dim=0))
        return w_xz

    def _param_weight(self):
        """(_padded_param_weight's weight, Wb, Wr), prepared per step / per generate() like the stacked in_proj."""
        wp = ops.prepared_weight(("x_param_padded", id(self)), (self.x_param_proj.weight,))
        if wp is not None:
            return wp, -(-self.d_inner // 64) * 64, -(-self.dt_rank // 64) * 64
        return ops.cached_prep("x_param_padded", (self.x_param_proj.weight,), self._padded_param_weight)

    def _have_window(self, conv_prev, use_cache):
        return conv_prev is not None and use_cache and conv_prev.shape[1] == self.d_inner and conv_prev.shape[2] == self.conv_kernel_size - 1

    def _token_step_ok(self, h, conv_prev, ssm_prev, use_cache, output_attentions):
        """Whether this call is a single-token step on the caches (generate(), core.py:1578-1603): inference on the GPU."""
        return (h.shape[1] == 1 and self._have_window(conv_prev, use_cache) and ssm_prev is not None and not output_attentions
                and not torch.is_grad_enabled() and h.is_cuda and self.conv_kernel_size > 1)

    def decode_finish(self, gated, past_key_value):
        """out_proj of a single-token step whose gate already ran (ops.decode_inproj's epilogue)."""
        out = ops.decode_dense_gemv(gated, self.out_proj.weight, self.out_proj.bias)
        if out is None:
            out = _mfma_linear(gated.reshape(-1, 1, self.d_inner), self.out_proj.weight, self.out_proj.bias)
        return out.reshape(gated.shape[0], 1, -1), None, tuple(past_key_value)

    @_on_input_device
    def forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_value=None,
                output_attentions: bool = False, use_cache: bool = False):
        conv_prev, ssm_prev = past_key_value if past_key_value is not None else (None, None)
        pre = getattr(past_key_value, "pre", None)
        if self._token_step_ok(hidden_states, conv_prev, ssm_prev, use_cache, output_attentions):
            return (self._token_step if pre is None else self._prepass_step)(hidden_states, past_key_value)
        if pre is not None:
            raise ops.ApertisHipError("SelectiveLinearAttention: the model ran this step's cache-only half ahead (_decode_prepass: the "
                                      "SSM state is already updated) but the layer is not on its single-token path")
        return self._sequence(hidden_states, attention_mask, conv_prev, ssm_prev, output_attentions, use_cache)

    def _prepass_step(self, hidden_states, past):
        """Single-token step whose first half - conv, x_param_proj, dt, state update: functions of the caches alone - ran for every
        layer at the start of the token step (ApertisModel._decode_prepass; `past.pre`): the gate and the window push are left."""
        B, Dn = hidden_states.shape[0], self.d_inner
        if hidden_states.dtype == torch.bfloat16:
            # in_proj with the gate and the window push in its epilogue - xz is never written
            gated = ops.decode_inproj(self._stacked_in_proj(), past.pre, past.conv, xn=hidden_states)
            if gated is not None:
                return self.decode_finish(gated, past)
        xz = _mfma_linear(hidden_states, self._stacked_in_proj())
        self._param_weight()    # (not read here: prepared at the same point of the step as in _token_step, so a cold cache fills alike)
        gated = ops.decode_post(past.pre, xz.reshape(B, 2 * Dn), past.conv)
        out = _mfma_linear(gated.reshape(B, 1, Dn), self.out_proj.weight, self.out_proj.bias)
        return out, None, tuple(past)

    def _token_step(self, hidden_states, past):
        """Single-token decode step (generate(), core.py:1578-1603): two small kernels around the projections instead of the
        chunk machinery.  A _SsmLayerPast says whether the buffers it holds may be updated in place; a plain tuple's may not."""
        B, Dn, R = hidden_states.shape[0], self.d_inner, self.dt_rank
        conv_prev, ssm_prev = past
        inplace = getattr(past, "inplace", False)
        xz2 = _mfma_linear(hidden_states, self._stacked_in_proj()).reshape(B, 2 * Dn)
        wp, Wb, Wr = self._param_weight()
        xc, conv_state = ops.ssm_decode_step(xz2[:, :Dn], conv_prev, self.conv1d.weight, self.conv1d.bias, inplace=inplace)
        p = _mfma_linear(xc, wp)                                                   # [B, 2*Wb + Wr]
        dt_in = p[:, 2 * Wb:2 * Wb + R]
        state = ssm_prev.reshape(B, Dn).float()
        if not (inplace and state.data_ptr() == ssm_prev.data_ptr()):
            state = state.clone()            # (the captured decode graph owns its cache buffers and updates them in place)
        if ops.tiny_linear_supported(dt_in, R, self.num_heads):
            # dt_proj_head inside the state kernel (one launch less per layer of a token step; the same bits)
            gated = ops.ssm_decode_state_dt(dt_in, self.dt_proj_head.weight, self.dt_proj_head.bias, self.A_log, p[:, :Dn],
                                            p[:, Wb:Wb + Dn], xc, xz2[:, Dn:], self.D, state)
        else:
            gated = ops.ssm_decode_state(self.dt_proj_head(dt_in).float(), self.A_log, p[:, :Dn], p[:, Wb:Wb + Dn], xc, xz2[:, Dn:], self.D, state)
        out = _mfma_linear(gated.reshape(B, 1, Dn), self.out_proj.weight)
        return out, None, (conv_state, state.reshape(B, self.num_heads, self.d_state))

    def _sequence(self, hidden_states, attention_mask, conv_prev, ssm_prev, output_attentions, use_cache):
        """Training, prefill and multi-token steps on a cache: the conv over the whole sequence and the chunked scan."""
        B, L, _ = hidden_states.shape
        Dn, R, kw = self.d_inner, self.dt_rank, self.conv_kernel_size
        have_window = self._have_window(conv_prev, use_cache)
        xz = _mfma_linear(hidden_states, self._stacked_in_proj())
        wp, Wb, Wr = self._param_weight()
        xp, z = ops.split_cols(xz, (Dn, Dn))
        conv_in = xp
        if have_window:
            # the reference prepends the cached window and keeps the FIRST L conv outputs
            # (core.py:369-373); reproduced as is so cached decode matches `apertis chat`
            conv_in = torch.cat([conv_prev.transpose(1, 2).to(xp.dtype), xp], dim=1)
        conv_state = conv_in[:, -(kw - 1):].transpose(1, 2).detach() if use_cache else None
        layout = attention_mask.layout if isinstance(attention_mask, _SsmDocs) else None
        if layout is not None:
            # packed rows under ops.SSM_PACKED (ApertisModel._packed_layout has the conditions): conv and scan - the two
            # operations of this block that look across tokens - stop at the document boundaries; everything else is per token
            if have_window or use_cache or ssm_prev is not None or output_attentions or not hidden_states.is_cuda:
                raise ValueError("document_ids: a packed selective_ssm forward takes no cache, keeps none and returns no "
                                 "attention weights (output_attentions), on a ROCm device")
            if ops.DWCONV_PAIR:
                xc_p, xc = ops.dwconv_silu_pair(conv_in, self.conv1d.weight, self.conv1d.bias, layout=layout)
            else:
                xc_p = xc = ops.dwconv_silu(conv_in, self.conv1d.weight, self.conv1d.bias, layout=layout)
        elif isinstance(attention_mask, _SsmStarts):
            # left-padded prefill under ops.SSM_LEFT_PAD (ApertisModel._ssm_left_pad has the conditions: inference, no incoming
            # cache): a row's pads count as "before the sequence" - the conv output is exactly 0 there, x_param_proj has no
            # bias, so Bt = C = dt_in = 0 and the state every scan form carries stays at 0 up to the first real token
            xc_p = xc = ops.dwconv_silu(conv_in, self.conv1d.weight, self.conv1d.bias, start=attention_mask.start)
        elif hidden_states.is_cuda and ops.DWCONV_PAIR:
            # (two views of the one conv output, one per consumer - x_param_proj and the scan: the conv backward adds their
            #  gradients where it reads the rows)
            xc_p, xc = ops.dwconv_silu_pair(conv_in, self.conv1d.weight, self.conv1d.bias)  # core.py:373-375
        else:
            xc_p = xc = ops.dwconv_silu(conv_in, self.conv1d.weight, self.conv1d.bias)
        if have_window:
            xc_p, xc = xc_p[:, :L], xc[:, :L]
        p = _mfma_linear(xc_p, wp)                                           # x_param_proj (core.py:376), padded layout
        # Bt / C / dt are column slices of p taken in place (core.py:382-385); the Bt and C slices keep their zero pad
        Btp, Cp, dt_in = ops.split_cols(p, (Wb, Wb, R, Wr - R))[:3]
        h0 = ssm_prev.reshape(B, Dn) if (use_cache and ssm_prev is not None) else None
        two_op = output_attentions or not hidden_states.is_cuda
        tiny = ops.tiny_linear_supported(dt_in, R, self.num_heads)
        if tiny and not two_op:
            # dt_proj_head, softplus, recurrence, skip and gate as ONE op (core.py:382-396): the logits come from the
            # stand-alone kernel or - APERTIS_SCAN_DT_FUSED=1 - from inside the scan's state pass (the same bits)
            res = ops.scan_gate_dt(dt_in, self.dt_proj_head.weight, self.dt_proj_head.bias, self.A_log, Btp, Cp, xc, z, self.D,
                                   h0=h0, delta_softplus=True, return_last=use_cache, layout=layout)
            (gated, h_last), y = (res if use_cache else (res, None)), None
            out = _mfma_linear(gated, self.out_proj.weight)                 # core.py:397
            cache = (conv_state, h_last.reshape(B, self.num_heads, self.d_state)) if use_cache else None
            return out, None, cache
        if tiny:
            dt_logits = ops.tiny_linear(dt_in, self.dt_proj_head.weight, self.dt_proj_head.bias)   # [B,L,h] fp32
        else:
            dt_logits = self.dt_proj_head(dt_in).float()
        # softplus (core.py:383) is applied inside the scan kernel
        if two_op:
            # the caller wants y_ssm itself (core.py:401): scan and gate as two ops, y in fp32
            res = ops.selective_scan(dt_logits, self.A_log, Btp[..., :Dn], Cp[..., :Dn], h0=h0,
                                     delta_softplus=True, y_dtype=torch.float32, return_last=use_cache)
            y, h_last = res if use_cache else (res, None)
            gated = ops.ssm_gate(y, xc, z, self.D)                           # core.py:395-396
        else:
            # recurrence + skip + gate in one kernel per direction; y is never written (core.py:388-396)
            res = ops.scan_gate(dt_logits, self.A_log, Btp, Cp, xc, z, self.D, h0=h0, delta_softplus=True,
                                return_last=use_cache, layout=layout)
            (gated, h_last), y = (res if use_cache else (res, None)), None
        out = _mfma_linear(gated, self.out_proj.weight)                     # core.py:397
        cache = (conv_state, h_last.reshape(B, self.num_heads, self.d_state)) if use_cache else None
        return out, (y if output_attentions else None), cache


# ----------------------------------------------------------------------------------------------
# AdaptiveExpertSystem  (reference core.py:403-607) on HIP kernels
# ----------------------------------------------------------------------------------------------
_ZERO_SCALARS = {}


def _zero_scalar(device, dtype):
    """A shared 0-dim zero (never written in place): the auxiliary-loss slots of layers without an expert system."""
    key = (device, dtype)
    z = _ZERO_SCALARS.get(key)
    if z is None:
        z = _ZERO_SCALARS[key] = torch.zeros((), device=device, dtype=dtype)
    return z


class AdaptiveExpertSystem(nn.Module):
    """Top-K routed mixture of `LayerNorm -> Linear -> act -> Dropout -> Linear` experts.

    Parameters are held stacked ([E, ...]) for the grouped GEMMs; `state_dict()` /
    `load_state_dict()` expose the reference's per-expert names `experts.{e}.{0,1,4}.*`."""

    _STACKED = (("0.weight", "expert_ln_weight"), ("0.bias", "expert_ln_bias"), ("1.weight", "expert_w1"),
                ("1.bias", "expert_b1"), ("4.weight", "expert_w2"), ("4.bias", "expert_b2"))

    def register_train_prep(self, prep):
        """The stacked expert weights into a TrainPrep (ops/prep.py): bf16 and transposed bf16 copies, one launch per step."""
        prep.add_plain(self.expert_w1)
        prep.add_plain(self.expert_w2)

    def __init__(self, config: ApertisConfig, activation_function_override: Optional[str] = None):
        super().__init__()
        self.config = config
        self.hidden_size = config.hidden_size
        self.intermediate_size = config.intermediate_size
        self.num_experts = config.num_experts
        self.experts_per_token = config.experts_per_token
        self.load_balancing_loss_coef = config.load_balancing_loss_coef if self.num_experts > 0 else 0.0
        self.expert_capacity_factor = config.expert_capacity_factor
        self.router_z_loss_coef = config.router_z_loss_coef if self.num_experts > 0 else 0.0
        self.noisy_routing_alpha = config.noisy_routing_alpha if self.num_experts > 0 else 0.0
        self.expert_dropout_prob = config.expert_dropout_prob if self.num_experts > 0 else 0.0
        on = self.num_experts > 0
        self.use_noisy_top_k_routing = config.use_noisy_top_k_routing and on
        self.use_expert_capacity_limit = config.use_expert_capacity_limit and on
        self.use_expert_dropout = config.use_expert_dropout and on
        self.use_router_z_loss = config.use_router_z_loss and on
        self.use_load_balancing_loss = config.use_load_balancing_loss and on
        self.router = self.experts = self.w_noise = None
        if not on:
            return
        E, H, I = self.num_experts, self.hidden_size, self.intermediate_size
        self.activation = _activation_name(activation_function_override or config.hidden_act)
        self.hidden_dropout_prob = config.hidden_dropout_prob
        self.router_norm = HipLayerNorm(H, eps=config.layer_norm_eps)
        self.router = nn.Linear(H, E)
        self.experts = True  # marker: experts exist (the reference holds an nn.ModuleList here)
        k1, k2 = 1.0 / math.sqrt(H), 1.0 / math.sqrt(I)     # nn.Linear default init bounds
        self.expert_ln_weight = nn.Parameter(torch.ones(E, H))
        self.expert_ln_bias = nn.Parameter(torch.zeros(E, H))
        self.expert_w1 = nn.Parameter(torch.empty(E, I, H).uniform_(-k1, k1))
        self.expert_b1 = nn.Parameter(torch.empty(E, I).uniform_(-k1, k1))
        self.expert_w2 = nn.Parameter(torch.empty(E, H, I).uniform_(-k2, k2))
        self.expert_b2 = nn.Parameter(torch.empty(E, H).uniform_(-k2, k2))
        if config.use_noisy_top_k_routing:
            self.w_noise = nn.Parameter(torch.zeros(E))
        self._register_state_dict_hook(self._split_experts)
        self._register_load_state_dict_pre_hook(self._stack_experts)

    # -- checkpoint format: experts.{e}.{0,1,4}.{weight,bias} -----------------------------------
    @staticmethod
    def _split_experts(module, state_dict, prefix, local_metadata):
        for suffix, name in module._STACKED:
            stacked = state_dict.pop(prefix + name)
            for e in range(module.num_experts):
                state_dict[f"{prefix}experts.{e}.{suffix}"] = stacked[e]
        return state_dict

    def _stack_experts(self, state_dict, prefix, *args):
        for suffix, name in self._STACKED:
            keys = [f"{prefix}experts.{e}.{suffix}" for e in range(self.num_experts)]
            if all(k in state_dict for k in keys):
                state_dict[prefix + name] = torch.stack([state_dict.pop(k) for k in keys])

    def init_expert_weights(self, std: float):
        """ApertisModel._init_weights applied to the stacked experts (core.py:1045-1054)."""
        with torch.no_grad():
            self.expert_w1.normal_(0.0, std)
            self.expert_w2.normal_(0.0, std)
            self.expert_b1.zero_()
            self.expert_b2.zero_()
            self.expert_ln_weight.fill_(1.0)
            self.expert_ln_bias.zero_()

    @_on_input_device
    def forward(self, hidden_states, lazy_combine=False, aux_dtype=None):
        """`aux_dtype`: dtype of the two auxiliary losses (core.py:607 casts them to hidden_states.dtype; the layer passes
        the residual stream's dtype, which is what hidden_states has in the reference under autocast - here the
        pre-norm kernels hand over the bf16 activation, and bf16 losses would also cost two mixed-dtype adds per layer)."""
        aux_dtype = aux_dtype or hidden_states.dtype
        if self.num_experts <= 0 or self.router is None:
            zero = _zero_scalar(hidden_states.device, aux_dtype)
            return hidden_states, zero, zero
        B, L, H = hidden_states.shape
        S, E, K = B * L, self.num_experts, self.experts_per_token
        xf = hidden_states.reshape(S, H)
        pre_logits = getattr(hidden_states, "_apertis_router_logits", None)
        if pre_logits is not None:
            # the boundary kernel in front of this block already formed them (_enter_block); the gather op below hands its
            # gradient rows to that op through the link that rides on the activation
            logits = pre_logits.reshape(S, E)
            xf._apertis_rows_link = getattr(hidden_states, "_apertis_rows_link", None)
        elif ops.router_ln_linear_supported(xf, H, E):
            # core.py:481-482 in one pass over x; xf comes back as the pass-through the expert path reads
            logits, xf = ops.router_ln_linear(xf, self.router_norm.weight, self.router_norm.bias, self.router_norm.eps,
                                              self.router.weight, self.router.bias)
        else:
            xn = self.router_norm(xf)                                                     # core.py:481
            if xn.is_cuda and ops.skinny_linear_supported(H, E):
                logits = ops.skinny_linear(xn, self.router.weight, self.router.bias)      # core.py:482 (fp32 out)
            else:
                logits = self.router(xn).float()
        lb_loss = rz_loss = None
        lb_coef = self.load_balancing_loss_coef if (self.use_load_balancing_loss and self.training) else 0.0
        rz_coef = self.router_z_loss_coef if (self.use_router_z_loss and self.training) else 0.0
        noisy = self.use_noisy_top_k_routing and self.training
        cd = _compute_dtype(xf)
        if (not self.training and lb_coef == 0 and rz_coef == 0 and not noisy and logits.is_cuda
                and ops.moe_route_small_supported(logits, xf, K)):
            # a handful of rows under no_grad (the decode step, core.py:1578-1603): gate, plan and gather-LN in one launch
            _g, idx, w, plan, xg = ops.moe_route_small(logits, xf, self.expert_ln_weight, self.expert_ln_bias,
                                                       self.config.layer_norm_eps, K, out_dtype=cd)
            yr = ops.expert_mlp(xg, self.expert_w1, self.expert_b1, self.expert_w2, self.expert_b2, plan.offsets,
                                plan.max_rows, act=self.activation, drop_p=0.0, seed=0, compute_dtype=cd)
            out = _LazyCombine(yr, w, plan, (B, L, H), xf.dtype)
            if not lazy_combine:
                out = out.materialise()
            zero = _zero_scalar(hidden_states.device, aux_dtype)
            return out, zero, zero
        fused_gate = logits.is_cuda and S > 0 and (lb_coef > 0 or rz_coef > 0)
        if noisy and not fused_gate:                                                      # core.py:485-488
            logits = logits + torch.randn_like(logits) * (F.softplus(self.w_noise) * self.noisy_routing_alpha)
        if fused_gate:
            # noise + gate + both auxiliary losses in one pass (core.py:485-505, 524-529)
            nseed = int(torch.empty((), dtype=torch.int64).random_().item()) if noisy else 0
            idx, w, lb, rz = ops.moe_gate_topk_aux(logits, K, lb_coef, rz_coef, self.w_noise if noisy else None,
                                                   self.noisy_routing_alpha, nseed)
            lb_loss = lb if lb_coef > 0 else None
            rz_loss = rz if rz_coef > 0 else None
        else:
            gates, idx, w = ops.moe_gate_topk(logits, K)                                  # core.py:491-492,529
            if lb_coef > 0:                                                               # core.py:499-505
                frac = torch.zeros(E, device=xf.device).index_add_(0, idx.reshape(-1).long(),
                                                                   torch.ones(S * K, device=xf.device)) / S
                lb_loss = lb_coef * E * torch.sum(frac * gates.mean(dim=0))
            if rz_coef > 0:                                                               # core.py:524-526
                rz_loss = rz_coef * torch.mean(torch.logsumexp(logits, dim=-1) ** 2)
        capacity = None
        if self.use_expert_capacity_limit and self.training:                              # core.py:508-511
            capacity = max(1, math.floor((S / E) * self.expert_capacity_factor)) if S > 0 else 0
        active = None
        if self.use_expert_dropout and self.training and self.expert_dropout_prob > 0:    # core.py:514-521
            n_drop = min(math.floor(E * self.expert_dropout_prob), E - 1)
            if n_drop > 0:
                active = torch.ones(E, dtype=torch.bool)
                active[torch.randperm(E)[:n_drop]] = False
                active = active.to(xf.device)
        cd = _compute_dtype(xf)
        plan = ops.moe_plan(idx, w, E, capacity, active)                                  # core.py:547-591
        xg = ops.moe_gather_ln(xf, self.expert_ln_weight, self.expert_ln_bias, plan, self.config.layer_norm_eps,
                               out_dtype=cd)                                              # core.py:593 + :436
        p_drop = self.hidden_dropout_prob if self.training else 0.0
        seed = int(torch.empty((), dtype=torch.int64).random_().item()) if p_drop > 0 else 0
        yr = ops.expert_mlp(xg, self.expert_w1, self.expert_b1, self.expert_w2, self.expert_b2, plan.offsets,
                            plan.max_rows, act=self.activation, drop_p=p_drop, seed=seed,
                            compute_dtype=cd)                                             # core.py:437-440
        out = _LazyCombine(yr, w, plan, (B, L, H), xf.dtype)                              # core.py:594,605
        if not lazy_combine:
            out = out.materialise()
        if lb_loss is None or rz_loss is None:
            zero = _zero_scalar(hidden_states.device, aux_dtype)
            lb_loss = zero if lb_loss is None else lb_loss
            rz_loss = zero if rz_loss is None else rz_loss
        return out, lb_loss.to(aux_dtype), rz_loss.to(aux_dtype)


class StateTrackingRecurrentCell(nn.Module):
    """Present in the reference (core.py:609-637) but never instantiated by any model path; kept
    as an importable name only."""

    def __init__(self, hidden_size: int):
        super().__init__()
        raise NotImplementedError("StateTrackingRecurrentCell is dead code in the reference and is not part of "
                                  "the MI355X hot path")


# ----------------------------------------------------------------------------------------------
# Attention / feed-forward / layer glue  (reference core.py:639-1018)
# ----------------------------------------------------------------------------------------------
class ApertisAttention(nn.Module):
    def __init__(self, config: ApertisConfig):
        super().__init__()
        self.config = config
        self.hidden_size = config.hidden_size
        self.num_attention_heads = config.num_attention_heads
        self.attention_head_size = self.hidden_size // self.num_attention_heads
        if config.attention_type in ("selective_ssm", "selective_linear"):
            self.attention_mechanism_impl = SelectiveLinearAttention(config)
            self._ssm = True
        else:
            if config.attention_type != "standard_mha":
                logger.error("Unsupported attention_type '%s'; using 'standard_mha'", config.attention_type)
                config.attention_type = "standard_mha"
            bias = config.attention_probs_dropout_prob == 0.0            # reference quirk, core.py:652
            self.q_proj = nn.Linear(self.hidden_size, self.hidden_size, bias=bias)
            self.k_proj = nn.Linear(self.hidden_size, self.hidden_size, bias=bias)
            self.v_proj = nn.Linear(self.hidden_size, self.hidden_size, bias=bias)
            self.out_proj = nn.Linear(self.hidden_size, self.hidden_size, bias=bias)
            self.attention_mechanism_impl = None
            self._ssm = False
        norm = RMSNorm if config.use_rmsnorm else HipLayerNorm
        self.pre_norm = norm(config.hidden_size, eps=config.layer_norm_eps)
        self.output_dropout = nn.Dropout(config.hidden_dropout_prob)
        self.attention_dropout = nn.Dropout(config.attention_probs_dropout_prob)
        self.rope = None
        if config.position_embedding_type == "rotary" and not self._ssm:
            self.rope = RotaryEmbedding(config.hidden_size, config.max_position_embeddings, config.rope_theta)

    def _decode_entry(self, h, past_kv, use_c, output_att):
        """A single-token step whose cache-only half ran ahead (`past_kv.pre` of a _SsmLayerPast is set): the block boundary as the
        prologue of the in_proj product (ops.decode_inproj with `boundary`), whose epilogue gates and pushes the window.  None: the general path."""
        impl, pre = self.attention_mechanism_impl, getattr(past_kv, "pre", None)
        if (pre is None or not isinstance(h, _Pending) or not use_c or output_att
                or not isinstance(self.pre_norm, HipLayerNorm) or torch.is_grad_enabled() or self.training):
            return None
        out, res = h.out, h.res
        if res.shape[1] != 1 or not res.is_cuda or res.shape[0] > 4 or past_kv.conv.dim() != 3:
            return None
        lazy = out if isinstance(out, _LazyCombine) else None
        if lazy is not None:
            if not (lazy.yr.dtype == torch.bfloat16 == lazy.dtype):
                return None
            bnd = (lazy.yr, res, self.pre_norm.weight, self.pre_norm.bias, self.pre_norm.eps, (lazy.w, lazy.plan))
        elif isinstance(out, torch.Tensor) and tuple(out.shape) == tuple(res.shape) and out.dtype == torch.bfloat16:
            bnd = (out, res, self.pre_norm.weight, self.pre_norm.bias, self.pre_norm.eps, None)
        else:
            return None
        r = ops.decode_inproj(impl._stacked_in_proj(), pre, past_kv.conv, boundary=bnd)          # (y, gated), or None
        return None if r is None else (r[0], impl.decode_finish(r[1], past_kv))

    def _fused_ok(self, q, att_mask, past_kv, output_att):
        """Whether this call takes the HIP RoPE + causal attention kernels: on the GPU, fp32 or bf16, D 64 or 128, no KV cache
        to extend, no attention weights asked for, and every query row keeps at least one valid key (a row without one gets a
        uniform average over all keys in the reference, finfo.min saturating; the model's mask says so, _AttnMask) - or,
        with ops.ATTN_LEFT_PAD, such rows exist (`att_mask.dead_rows`) and this is inference (eval, no grad): ops.causal_attention
        then fills them with that average."""
        if not (ops.ATTN_FUSED and q.is_cuda and past_kv is None and not output_att
                and ops.attention_supported(q, self.num_attention_heads)):
            return False
        if att_mask is None:
            return True
        if not isinstance(att_mask, _AttnMask):          # an additive mask handed in directly: only the stock path reads it
            return False
        kv = att_mask.key_valid
        if att_mask.dead_rows and (self.training or torch.is_grad_enabled()):
            return False
        return att_mask.fused_ok and (kv is None or tuple(kv.shape) == tuple(q.shape[:2]))

    def _rope_tables(self):
        """(cos, sin) of this layer's rotary table; (None, None) without rope."""
        return (self.rope.cos_cached, self.rope.sin_cached) if self.rope is not None else (None, None)

    def _fused_attention(self, q, k, v, att_mask, pos_ids, use_c):
        key_valid, default_pos = (att_mask.key_valid, att_mask.default_pos) if att_mask is not None else (None, False)
        dead_rows = att_mask is not None and att_mask.dead_rows
        layout = att_mask.layout if att_mask is not None else None
        if self.rope is not None:
            # (the model's own positions 0..L-1 go in as None: explicit ones are range-checked on the host, a sync per call;
            #  a layout's positions lie in [0, L) by construction: L against the table is the whole check)
            q, k = ops.rope_qk(q, k, None if default_pos else pos_ids, *self._rope_tables(),
                               in_range=layout is not None and att_mask.layout_pos)
        heads, p = self.num_attention_heads, self.attention_dropout.p
        window = att_mask.window if att_mask is not None else None
        if layout is not None:                   # (packed rows under a window: the model clipped the layout, ops.window_layout)
            ctxv = ops.document_attention(q, k, v, heads, layout, key_valid, p, self.training)
        elif window is not None and q.shape[1] > window:
            ctxv = ops.window_attention(q, k, v, heads, window, key_valid, p, self.training, dead_rows=dead_rows)
        else:
            ctxv = ops.causal_attention(q, k, v, heads, key_valid, p, self.training, dead_rows=dead_rows)
        return self.out_proj(ctxv), ((k, v) if use_c else None)

    def _cache_step_ok(self, q, att_mask, past_kv, output_att, use_c):
        """What _decode_ok and _chunk_ok share: the past is a layer of an ops.KVCache in the projections' dtype and batch, both
        switches on, on the GPU, inference (use_cache, no attention weights, eval, no grad), the model's own mask saying that
        every row has a valid key (_AttnMask.decode_ok), fp32 or bf16 with D 64 or 128."""
        return (isinstance(past_kv, ops.KVLayer) and ops.ATTN_FUSED and ops.ATTN_DECODE_FUSED and q.is_cuda and use_c
                and not output_att and not self.training and not torch.is_grad_enabled()
                and isinstance(att_mask, _AttnMask) and att_mask.decode_ok
                and ops.attention_decode_supported(q, self.num_attention_heads)
                and q.dtype == past_kv.cache.dtype and q.shape[0] == past_kv.cache.k[0].shape[0])

    def _decode_ok(self, q, att_mask, past_kv, output_att, use_c):
        """Whether this call is a single-token step the KV-cache decode kernels take: the past is a layer of an ops.KVCache
        with room for one more row and the projections' dtype, one query position, inference (no grad, eval, use_cache, no
        attention weights), on the GPU, D 64 or 128, both switches on, the position known on the host, and key 0 of every
        sequence valid - with ops.ATTN_LEFT_PAD: any key of every sequence (the model's mask says so, _AttnMask: no row
        without a valid key).  Anything else with a KVCache in
        flight runs the stock branch on the cache's views and returns plain tensors.
        A cache whose DEVICE step state is active (att_mask.step_cache; a captured graph replays such a step) brings length,
        position and key validity in device buffers: no host position, no host length, and the room in the cache and in the
        rotary table is the kernel's check (ops.kv_append_rope_at).  Its host lengths are stale, so a call the kernels do not
        take cannot fall back on the views: it raises.  A cache in SLOT mode (KVCache.slots_begin: a length per row) is the
        same case: the state is on the device, the host lengths are stale."""
        step = isinstance(past_kv, ops.KVLayer) and (past_kv.cache.step_active or past_kv.cache.slot_active)
        ok = (self._cache_step_ok(q, att_mask, past_kv, output_att, use_c) and q.shape[1] == 1
              and (att_mask.step_cache is past_kv.cache if step else att_mask.pos_host is not None))
        if step:
            if not ok:
                raise ops.ApertisHipError("a KVCache whose device step state is active, or one in slot mode, takes single-token "
                                          "inference steps on the decode kernels only (its host lengths are stale): "
                                          "KVCache.step_state_end() / slots_end() first")
            return True
        if not ok:
            return False
        cache, kv = past_kv.cache, att_mask.key_valid
        n = cache.lengths[past_kv.layer]
        return n < cache.capacity and (kv is None or tuple(kv.shape) == (q.shape[0], n + 1))

    def _decode_attention(self, q, k, v, att_mask, past_kv):
        cache, layer = past_kv.cache, past_kv.layer
        cos, sin = self._rope_tables()
        if cache.slot_active:                    # (a row and a position per sequence: generate_many()'s slots)
            q = ops.kv_append_rope_slots(q, k, v, cache, layer, cos, sin)
            ctxv = ops.attention_decode_slots(q, cache, layer, self.num_attention_heads)
        elif cache.step_active:
            q = ops.kv_append_rope_at(q, k, v, cache, layer, cos, sin)
            ctxv = ops.attention_decode_at(q, cache, layer, self.num_attention_heads)
        else:
            q = ops.kv_append_rope(q, k, v, cache, layer, att_mask.pos_host, cos, sin)
            if att_mask.window is None:
                ctxv = ops.attention_decode(q, cache, layer, self.num_attention_heads, att_mask.key_valid)
            else:                                                      # (only the last `window` rows of the cache are read)
                ctxv = ops.attention_decode(q, cache, layer, self.num_attention_heads, att_mask.key_valid, window=att_mask.window)
        return self.out_proj(ctxv.unsqueeze(1)), cache

    def _chunk_ok(self, q, att_mask, past_kv, output_att, use_c):
        """Whether this call is a multi-token step the chunk kernels take (ops.kv_append_rope_chunk, ops.attention_chunk):
        the past is a layer of an ops.KVCache that opted in (`multi_token`) with no device step state active, in the
        projections' dtype and with room for the Lq > 1 new rows; inference (no grad, eval, use_cache, no attention weights),
        on the GPU, D 64 or 128, both switches on; the model's own positions, known on the host (n .. n + Lq - 1); key 0 of
        every sequence valid, so that every row has a valid key, or with ops.ATTN_LEFT_PAD the rows without one filled in
        afterwards (`att_mask.dead_rows`); the mask None or [B, n + Lq].  Anything else runs the stock
        branch on the cache's views, as every multi-token forward against a cache without the flag does."""
        if not (self._cache_step_ok(q, att_mask, past_kv, output_att, use_c) and past_kv.cache.multi_token
                and not past_kv.cache.step_active and q.shape[1] > 1 and att_mask.pos_host is not None):
            return False
        cache, kv = past_kv.cache, att_mask.key_valid
        n = cache.lengths[past_kv.layer]
        if att_mask.window is not None and n + q.shape[1] > att_mask.window and not ops.ATTN_WINDOW_CACHE:
            return False                         # (opt-in: ops.attention_chunk(window=); else the stock branch applies the band)
        return (n + q.shape[1] <= cache.capacity and att_mask.pos_host == n
                and (kv is None or tuple(kv.shape) == (q.shape[0], n + q.shape[1])))

    def _chunk_attention(self, q, k, v, att_mask, past_kv):
        cache, layer = past_kv.cache, past_kv.layer
        cos, sin = self._rope_tables()
        q = ops.kv_append_rope_chunk(q, k, v, cache, layer, att_mask.pos_host, cos, sin)
        if att_mask.window is None:
            ctxv = ops.attention_chunk(q, cache, layer, self.num_attention_heads, att_mask.key_valid, dead_rows=att_mask.dead_rows)
        else:                                    # (past the window only under ops.ATTN_WINDOW_CACHE: _chunk_ok)
            ctxv = ops.attention_chunk(q, cache, layer, self.num_attention_heads, att_mask.key_valid, dead_rows=att_mask.dead_rows,
                                       window=att_mask.window)
        return self.out_proj(ctxv), cache

    def _heads(self, t):
        B, L, _ = t.shape
        return t.view(B, L, self.num_attention_heads, self.attention_head_size).transpose(1, 2)

    def forward(self, hidden_s, att_mask=None, pos_ids=None, past_kv=None, output_att=False, use_c=False, defer=False):
        """hidden_s: the residual stream, or the previous sub-block's _Pending output (its residual add is then
        folded into this block's pre-norm).  defer=True returns this block's output as a _Pending too."""
        entry = self._decode_entry(hidden_s, past_kv, use_c, output_att) if self._ssm else None
        if entry is None:
            x, hidden_s = _enter_block(self.pre_norm, hidden_s)
        if entry is not None:
            hidden_s, (out, proxy, cache) = entry
        elif self._ssm:
            out, proxy, cache = self.attention_mechanism_impl(x, attention_mask=att_mask, position_ids=pos_ids,
                                                              past_key_value=past_kv, output_attentions=output_att,
                                                              use_cache=use_c)
        elif self._decode_ok(q := self.q_proj(x), att_mask, past_kv, output_att, use_c):
            out, cache = self._decode_attention(q, self.k_proj(x), self.v_proj(x), att_mask, past_kv)
            proxy = None
        elif self._chunk_ok(q, att_mask, past_kv, output_att, use_c):
            out, cache = self._chunk_attention(q, self.k_proj(x), self.v_proj(x), att_mask, past_kv)
            proxy = None
        elif self._fused_ok(q, att_mask, past_kv, output_att):
            out, cache = self._fused_attention(q, self.k_proj(x), self.v_proj(x), att_mask, pos_ids, use_c)
            proxy = None
        else:
            # decode with a plain-tensor KV cache (or what the decode kernels do not take of a KVCache: its views are the
            # past), output_attentions, other head dims, CPU, left padding without ops.ATTN_LEFT_PAD: stock torch.
            window = None
            if isinstance(att_mask, _AttnMask):
                window, att_mask = att_mask.window, att_mask.additive()
            k, v = self.k_proj(x), self.v_proj(x)
            if self.rope is not None:
                q, k = self.rope(q, pos_ids), self.rope(k, pos_ids)
            if use_c and past_kv is not None:
                k, v = torch.cat([past_kv[0], k], dim=1), torch.cat([past_kv[1], v], dim=1)
            cache = (k, v) if use_c else None
            qh, kh, vh = self._heads(q), self._heads(k), self._heads(v)
            Lq, Lk = qh.shape[2], kh.shape[2]
            if att_mask is None and Lq > 1:
                i = torch.arange(Lq, device=x.device).unsqueeze(1) + (Lk - Lq)
                att_mask = torch.zeros(Lq, Lk, device=x.device, dtype=qh.dtype).masked_fill_(
                    i < torch.arange(Lk, device=x.device).unsqueeze(0), torch.finfo(qh.dtype).min)
            if window is not None and Lk > window:                 # the same band the kernels apply (ops.ATTN_WINDOW)
                att_mask = _band_mask(att_mask, window, Lq, Lk, qh)
            if output_att:
                scores = qh @ kh.transpose(-1, -2) / math.sqrt(self.attention_head_size)
                probs = F.softmax(scores + att_mask if att_mask is not None else scores, dim=-1)
                proxy = probs
                ctxv = self.attention_dropout(probs) @ vh
            else:
                proxy = None
                ctxv = F.scaled_dot_product_attention(qh, kh, vh, attn_mask=att_mask,
                                                      dropout_p=self.attention_dropout.p if self.training else 0.0)
            out = self.out_proj(ctxv.transpose(1, 2).reshape(x.shape[0], Lq, self.hidden_size))
        if defer:
            return _Pending(out, hidden_s, self.output_dropout), proxy, cache
        return _dropout_add(self.output_dropout, out, hidden_s), proxy, cache


class SwiGLUFFN(nn.Module):
    """w_down(silu(w_gate x) * w_up x), width 2/3*I rounded up to 256 (reference core.py:925-993).  On the GPU (fp32 / bf16,
    H % 8 == 0, ops.SWIGLU_FUSED) the block is ops.swiglu_mlp: w_gate | w_up as one stacked GEMM, the gate on its HIP kernel, the
    down projection, one autograd node that keeps x and the stacked pre-activation only; elsewhere the stock-torch line."""

    def __init__(self, config: ApertisConfig, intermediate_size: Optional[int] = None):
        super().__init__()
        self.config = config
        self.hidden_size = config.hidden_size
        self.intermediate_size = intermediate_size if intermediate_size is not None else config.intermediate_size
        self.ffn_dim = max(256, -(-int(self.intermediate_size * 2 / 3) // 256) * 256)
        self.w_gate = nn.Linear(self.hidden_size, self.ffn_dim, bias=False)
        self.w_up = nn.Linear(self.hidden_size, self.ffn_dim, bias=False)
        self.w_down = nn.Linear(self.ffn_dim, self.hidden_size, bias=False)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)

    def _stacked_gate_up(self):
        """w_gate | w_up as one [2 F, H] weight (they share their input): prepared per step / per generate()."""
        srcs = (self.w_gate.weight, self.w_up.weight)
        w_gu = ops.prepared_weight(("swiglu_gu", id(self)), srcs)
        if w_gu is None:
            w_gu = ops.cached_prep("swiglu_gu", srcs, lambda: torch.cat(srcs, dim=0))
        return w_gu

    def forward(self, x):
        if ops.swiglu_supported(x, self.ffn_dim):
            y = ops.swiglu_mlp(x.reshape(-1, x.shape[-1]), self._stacked_gate_up(), self.w_down.weight,
                               compute_dtype=_compute_dtype(x))
            return self.dropout(y.reshape(*x.shape[:-1], self.hidden_size))
        return self.dropout(self.w_down(F.silu(self.w_gate(x)) * self.w_up(x)))


class ApertisFeedForward(nn.Module):
    def __init__(self, config: ApertisConfig):
        super().__init__()
        self.config = config
        norm = RMSNorm if config.use_rmsnorm else HipLayerNorm
        self.pre_norm = norm(config.hidden_size, eps=config.layer_norm_eps)
        self.is_expert_system = False
        if config.use_swiglu:                                            # SwiGLU wins over MoE, core.py:849-859
            self.ffn = SwiGLUFFN(config)
        elif config.use_expert_system and config.num_experts > 0:
            self.ffn = AdaptiveExpertSystem(config, activation_function_override=config.hidden_act)
            self.is_expert_system = True
        else:
            self.ffn = nn.Sequential(nn.Linear(config.hidden_size, config.intermediate_size),
                                     _activation_module(config.hidden_act), nn.Dropout(config.hidden_dropout_prob),
                                     nn.Linear(config.intermediate_size, config.hidden_size))
        self.output_dropout = nn.Dropout(config.hidden_dropout_prob)

    def register_train_prep(self, prep):
        """The plain dense FFN's two weights, or the SwiGLU block's stacked gate | up and its down projection, into a TrainPrep
        (the expert system registers its own)."""
        if isinstance(self.ffn, nn.Sequential):
            prep.add_plain(self.ffn[0].weight)
            prep.add_plain(self.ffn[3].weight)
        elif isinstance(self.ffn, SwiGLUFFN):
            prep.add_stack(("swiglu_gu", id(self.ffn)), (self.ffn.w_gate.weight, self.ffn.w_up.weight))
            prep.add_plain(self.ffn.w_down.weight)

    def _dense_ffn(self, x):
        """Linear -> act -> Dropout -> Linear (core.py:861-866).  On the GPU the plain (non-MoE, non-SwiGLU) FFN runs on the
        expert-MLP kernels as ONE group: activation and dropout in the first GEMM's epilogue, their backward in the second data
        gradient's (ops.expert_mlp) - as nn.Sequential it was two library GEMMs plus an activation and a dropout kernel each
        way (13 % of the 125m configuration's step in those four elementwise kernels).  The dropout mask is the counter
        hash of the other fused kernels, not torch's Philox stream (train-mode RNG cannot match the reference bit-wise either way)."""
        if isinstance(self.ffn, nn.Sequential) and x.is_cuda and x.dtype in (torch.float32, torch.bfloat16):
            lin1, _act, drop, lin2 = self.ffn
            H = x.shape[-1]
            xf = x.reshape(-1, H)
            T = xf.shape[0]
            if T >= 1 and lin1.bias is not None and lin2.bias is not None:
                cd = _compute_dtype(xf)
                p_drop = drop.p if self.training else 0.0
                seed = int(torch.empty((), dtype=torch.int64).random_().item()) if p_drop > 0 else 0
                out = ops.expert_mlp(xf.to(cd), lin1.weight.unsqueeze(0), lin1.bias.unsqueeze(0), lin2.weight.unsqueeze(0),
                                     lin2.bias.unsqueeze(0), ops.dense_offsets(T, xf.device), T,
                                     act=_activation_name(self.config.hidden_act), drop_p=p_drop, seed=seed, compute_dtype=cd)
                return out.reshape(*x.shape[:-1], lin2.weight.shape[0])
        return self.ffn(x)

    def _small_entry(self, h, defer):
        """A handful of rows under no_grad (the single-token decode step, core.py:1578-1603): the block boundary, the router, the
        gate, the dispatch plan and the per-expert LayerNorm as ONE launch (ops.moe_enter_small), then the two expert GEMMs.
        Returns (output or its _LazyCombine, residual stream); None when that kernel does not take the shapes / modes (general path)."""
        f = self.ffn
        if not (isinstance(h, _Pending) and not isinstance(h.out, _LazyCombine) and not self.training and not f.training
                and isinstance(self.pre_norm, HipLayerNorm) and isinstance(f.router_norm, nn.LayerNorm)
                and h.res.is_cuda and _compute_dtype(h.res) == h.out.dtype
                and ops.moe_enter_small_supported(h.out, h.res, f.num_experts, f.experts_per_token)):
            return None
        y, _logits, w, plan, xg = ops.moe_enter_small(h.out, h.res, self.pre_norm.weight, self.pre_norm.bias, self.pre_norm.eps,
                                                      f.router_norm.weight, f.router_norm.bias, f.router_norm.eps, f.router.weight,
                                                      f.router.bias, f.expert_ln_weight, f.expert_ln_bias, f.config.layer_norm_eps,
                                                      f.experts_per_token)
        yr = ops.expert_mlp(xg, f.expert_w1, f.expert_b1, f.expert_w2, f.expert_b2, plan.offsets, plan.max_rows, act=f.activation,
                            drop_p=0.0, seed=0, compute_dtype=h.out.dtype)
        out = _LazyCombine(yr, w, plan, tuple(h.res.shape), h.out.dtype)
        if not defer or os.environ.get("APERTIS_NO_LAZY_COMBINE"):
            out = out.materialise()
        return out, y

    def forward(self, hidden_s, defer=False):
        router = small = None
        if self.is_expert_system and self.ffn.router is not None and self.ffn.num_experts > 0:
            router = (self.ffn.router_norm, self.ffn.router)
            small = self._small_entry(hidden_s, defer)
        if small is not None:
            out, hidden_s = small
            lb = rz = _zero_scalar(hidden_s.device, hidden_s.dtype)
        else:
            x, hidden_s = _enter_block(self.pre_norm, hidden_s, router=router)
            if self.is_expert_system:
                out, lb, rz = self.ffn(x, lazy_combine=defer and not os.environ.get("APERTIS_NO_LAZY_COMBINE"),
                                       aux_dtype=hidden_s.dtype)
            else:
                out = self._dense_ffn(x)
                lb = rz = _zero_scalar(hidden_s.device, hidden_s.dtype)
        if defer:
            return _Pending(out, hidden_s, self.output_dropout), lb, rz
        return _dropout_add(self.output_dropout, out, hidden_s), lb, rz


def _active_window(cfg):
    """The sliding window a standard_mha model honours: `cfg.sliding_window` when ops.ATTN_WINDOW is on, else None (the
    reference never reads the field, and neither does the default path).  With the switch on the field is None or an
    integer >= 1: anything else raises ValueError, at the first forward."""
    w = cfg.sliding_window
    if not ops.ATTN_WINDOW or w is None or cfg.attention_type != "standard_mha":
        return None
    if isinstance(w, bool) or not isinstance(w, int) or w < 1:
        raise ValueError(f"sliding_window must be None or an integer >= 1 under ops.ATTN_WINDOW, got {w!r}")
    return w


def _band_mask(att_mask, window, Lq, Lk, like):
    """The stock branch's additive mask with the sliding-window band on top: query row i sits at key position Lk - Lq + i and
    keeps keys above that position minus `window`.  One additive term, clamped back to finfo.min so that a row the mask
    already emptied stays the uniform row it was (two finfo.min would add up to -inf).  att_mask None: the band alone (a
    single-token step without padding has no mask)."""
    like = like if att_mask is None else att_mask
    lo = torch.finfo(like.dtype).min
    i = torch.arange(Lq, device=like.device).unsqueeze(1) + (Lk - Lq)
    band = torch.zeros(Lq, Lk, device=like.device, dtype=like.dtype).masked_fill_(
        torch.arange(Lk, device=like.device).unsqueeze(0) <= i - window, lo)
    return band if att_mask is None else (att_mask + band).clamp_(min=lo)


class _AttnMask:
    """What a standard_mha layer receives as its mask from ApertisModel.forward: the raw key validity [B, L] (None: nothing
    padded) for the fused kernels, whether the fused path may run (no query row without a valid key), whether the positions
    are the model's own 0..L-1, and the additive mask of the stock path, built only if that path asks for it.  For a
    single-token step against a KVCache: whether the decode kernels may run (key 0 of every sequence valid, so every row has a
    valid key) and the step's position as a HOST integer (None when the caller gave position_ids: only a tensor knows them).
    A multi-token step against a `multi_token` KVCache reads the same two: `pos_host` is then the position of its first token.
    `step_cache`: the KVCache whose device step state carries length, position and key validity of this step instead (no
    host integer, no mask tensor here).
    `dead_rows` (only with ops.ATTN_LEFT_PAD): key 0 of some sequence is masked (left padding), so a multi-token forward may
    hold query rows without a valid key; the kernels still run, inference only, and ops.attention_dead_rows gives those rows
    the reference's value.
    `layout` (packed rows, `document_ids`): the ops.DocumentLayout of this forward, computed once; the fused path then runs
    ops.document_attention, and the additive mask is the block-diagonal causal one.  `layout_pos`: the positions the layers
    receive are the layout's own (positions within each document, all in [0, L)), so the per-layer RoPE call does not
    range-check them on the host again; an integer instead of True is their bound (the longest document, known on the host:
    prefill_packed), which then stands against the rotary table in place of L.
    `window`: the active sliding window (_active_window: None unless ops.ATTN_WINDOW is on and the configuration sets one) -
    a query attends its last `window` keys only.  Every path reads it: ops.window_attention, ops.attention_decode(window=),
    and the stock branch as a band on its additive mask; the chunk kernels and the graph replay decline once it matters.  A
    packed forward carries it in `layout` instead (ops.window_layout clipped the bounds), so `window` is None there."""
    __slots__ = ("key_valid", "fused_ok", "default_pos", "_make", "_additive", "decode_ok", "pos_host", "step_cache", "dead_rows",
                 "layout", "layout_pos", "window")

    def __init__(self, key_valid, fused_ok, default_pos, make_additive, decode_ok=False, pos_host=None, step_cache=None,
                 dead_rows=False, layout=None, layout_pos=False):
        self.layout, self.layout_pos, self.window = layout, layout_pos, None
        self.key_valid, self.fused_ok, self.default_pos = key_valid, fused_ok, default_pos
        self._make, self._additive = make_additive, None
        self.decode_ok, self.pos_host, self.step_cache = decode_ok, pos_host, step_cache
        self.dead_rows = dead_rows

    def additive(self):
        if self._make is not None:
            self._additive, self._make = self._make(), None
        return self._additive


class ApertisLayer(nn.Module):
    def __init__(self, config: ApertisConfig):
        super().__init__()
        self.config = config
        self.attention = ApertisAttention(config)
        self.feed_forward = ApertisFeedForward(config)

    def forward(self, hidden_s, att_mask=None, pos_ids=None, past_kv=None, output_att=False, use_c=False, defer=False):
        """defer=True (the model's layer loop): the layer accepts and returns a _Pending boundary, so every
        residual add of the stack is fused with the pre-norm that follows it (ops.dropout_add_layer_norm)."""
        x, att_w, cache = self.attention(hidden_s, att_mask, pos_ids, past_kv, output_att, use_c, defer=True)
        x, lb, rz = self.feed_forward(x, defer=defer)
        return x, att_w, cache, lb, rz


# ----------------------------------------------------------------------------------------------
# ApertisModel / ApertisForCausalLM  (reference core.py:1020-1648)
# ----------------------------------------------------------------------------------------------
class ApertisModel(nn.Module):
    def __init__(self, config: ApertisConfig):
        super().__init__()
        self.config = config
        self.padding_idx = config.pad_token_id
        self.vocab_size = config.vocab_size
        self.token_embeddings = nn.Embedding(config.vocab_size, config.hidden_size, self.padding_idx)
        self.abs_pos_embeddings = None
        if config.position_embedding_type == "absolute":
            self.abs_pos_embeddings = nn.Embedding(config.max_position_embeddings, config.hidden_size)
        self.multimodal_encoder = None
        self.vision_projection = nn.Identity()
        if config.multimodal:
            self.multimodal_encoder = UnifiedMultimodalEncoder(config)
            if config.vision_embed_dim != config.hidden_size:
                self.vision_projection = nn.Linear(config.vision_embed_dim, config.hidden_size)
        self.layers = nn.ModuleList([ApertisLayer(config) for _ in range(config.num_hidden_layers)])
        norm = RMSNorm if config.use_rmsnorm else HipLayerNorm
        self.final_post_norm = norm(config.hidden_size, eps=config.layer_norm_eps)
        self.embed_dropout = nn.Dropout(config.hidden_dropout_prob)
        self.apply(self._init_weights)
        self.gradient_checkpointing = False

    def _init_weights(self, module):
        """normal(0, initializer_range) for Linear/Embedding, zero biases, unit norms; dt bias
        re-drawn in [ln 1e-3, ln 1e-2] (reference core.py:1045-1062)."""
        std = self.config.initializer_range
        if isinstance(module, nn.Linear):
            module.weight.data.normal_(0.0, std)
            if module.bias is not None:
                module.bias.data.zero_()
        elif isinstance(module, nn.Embedding):
            module.weight.data.normal_(0.0, std)
            if module.padding_idx is not None:
                module.weight.data[module.padding_idx].zero_()
        elif isinstance(module, nn.LayerNorm):
            if module.bias is not None:
                module.bias.data.zero_()
            if module.weight is not None:
                module.weight.data.fill_(1.0)
        elif isinstance(module, RMSNorm):
            module.scale.data.fill_(1.0)
        elif isinstance(module, AdaptiveExpertSystem) and module.router is not None:
            module.init_expert_weights(std)
        if isinstance(module, SelectiveLinearAttention):
            nn.init.uniform_(module.dt_proj_head.bias, a=math.log(1e-3), b=math.log(1e-2))

    def gradient_checkpointing_enable(self):
        self.gradient_checkpointing = True

    def get_input_embeddings(self):
        return self.token_embeddings

    def set_input_embeddings(self, embs):
        self.token_embeddings = embs

    def resize_token_embeddings(self, new_num_tokens: int) -> nn.Embedding:
        old = self.token_embeddings
        new = nn.Embedding(new_num_tokens, self.config.hidden_size, self.padding_idx, device=old.weight.device,
                           dtype=old.weight.dtype)
        self._init_weights(new)
        n = min(old.num_embeddings, new_num_tokens)
        new.weight.data[:n] = old.weight.data[:n]
        self.token_embeddings = new
        self.config.vocab_size = self.vocab_size = new_num_tokens
        if self.padding_idx is not None and self.padding_idx >= new_num_tokens:
            self.padding_idx = 0
            self.token_embeddings.padding_idx = 0
        return self.token_embeddings

    def _prepare_decoder_attention_mask(self, attention_mask, input_shape, inputs_embeds, past_len):
        """Additive causal+padding mask for the stock-attention fallback, or None when nothing is
        padded (reference core.py:1088-1139).  Ignored by the selective-SSM path."""
        if attention_mask is None or bool(torch.all(attention_mask.bool())):
            return None
        B, Lq = input_shape
        allow = None
        if Lq > 1:
            Lk = past_len + Lq
            causal = torch.ones(Lk, Lk, dtype=torch.bool, device=inputs_embeds.device).tril()[past_len:]
            allow = causal[None, None] & attention_mask[:, None, None, :].bool()
        elif past_len > 0:
            allow = attention_mask[:, None, None, :].bool()
        if allow is None:
            return None
        return (1.0 - allow.to(inputs_embeds.dtype)) * torch.finfo(inputs_embeds.dtype).min

    def _packed_layout(self, document_ids, input_shape, attention_mask, past_key_values, use_c, pixel_values, device=None):
        """The ops.DocumentLayout of a packed forward, after the checks that keep such a forward well defined: standard_mha
        (an SSM state would run across documents) - or, with ops.SSM_PACKED, selective_ssm on a ROCm device (`device`: the
        inputs'), whose conv and scan then stop at the document boundaries - no cache in or out, no image tokens in front of
        the rows, and no key masking - the pad tail of a packed row is a document of its own, so every query keeps a key and
        attention_mask is None or all ones (one host read, and only when a mask is given).  Every violation raises ValueError."""
        kind = self.config.attention_type
        if kind != "standard_mha" and not (ops.SSM_PACKED and device is not None and device.type == "cuda"):
            why = "ops.SSM_PACKED / APERTIS_SSM_PACKED=1 is off" if not ops.SSM_PACKED else f"the inputs are on {device}, not a ROCm device"
            raise ValueError(f"document_ids: packed rows need attention_type 'standard_mha', not {kind!r} (the recurrent state "
                             f"would run across documents; the packed selective_ssm path is not taken: {why})")
        if past_key_values is not None or use_c:
            raise ValueError("document_ids: packed rows take no past_key_values and no use_cache=True")
        if pixel_values is not None:
            raise ValueError("document_ids: packed rows take no pixel_values")
        if tuple(document_ids.shape) != tuple(input_shape):
            raise ValueError(f"document_ids of shape {tuple(document_ids.shape)} for inputs of {tuple(input_shape)}")
        if attention_mask is not None and not bool(attention_mask.bool().all()):
            raise ValueError("document_ids: attention_mask must be None or all ones (give the pad tail a document id of its own)")
        return ops.document_layout(document_ids)

    @staticmethod
    def _document_additive_mask(layout, dtype):
        """The stock branch's additive mask of packed rows [B, 1, L, L]: 0 where start[b, i] <= j <= i, finfo.min elsewhere."""
        L = layout.start.shape[1]
        j = torch.arange(L, device=layout.start.device)
        allow = (j[None, None, :] <= j[None, :, None]) & (j[None, None, :] >= layout.start[:, :, None])
        return ((1.0 - allow.to(dtype)) * torch.finfo(dtype).min).unsqueeze(1)

    def _attention_mask(self, attention_mask, input_shape, inputs_embeds, past_len, default_pos, pos_host=None, step_cache=None):
        """The standard_mha layers' mask (_AttnMask).  One host sync when a mask is given, as before: whether anything is
        padded, whether key 0 of every sequence is valid (then every query row has a valid key: right padding, the
        trainer's form, stays on the fused path with no cache, and a step against a KVCache on the decode kernels - a
        finished sequence of generate() keeps key 0) and whether every sequence has a valid key at all come back together.
        With ops.ATTN_LEFT_PAD a batch whose key 0 is masked somewhere (left padding) qualifies as well, marked `dead_rows`,
        as long as every sequence has a valid key: a single-token step then has one, and the rows of a longer forward that
        have none are filled in after the attention (ops.attention_dead_rows).  A multi-token piece going into a KVCache
        (`pos_host` given) may still lie wholly inside a sequence's padding - the valid keys come with a later piece - and
        the fill covers that exactly, so the last condition is not asked of it: with the switch on, a sequence that is
        masked throughout such a piece takes the chunk kernels too.  A step on a cache's device step state (`step_cache`) has
        no mask tensor and NO host sync: the validity is the cache's buffer, and every sequence had a valid key (key 0,
        without ops.ATTN_LEFT_PAD) when the state was activated (those columns do not change afterwards)."""
        if step_cache is not None:
            return _AttnMask(None, False, False, None, True, None, step_cache)
        default_pos = default_pos and past_len == 0
        if attention_mask is None:
            return _AttnMask(None, True, default_pos, None, True, pos_host)
        valid = attention_mask.bool()
        all_valid, col0, each_any = torch.stack((valid.all(), valid[:, 0].all(), valid.any(1).all())).tolist()
        if all_valid:
            return _AttnMask(None, True, default_pos, None, True, pos_host)
        piece = pos_host is not None and input_shape[1] > 1
        dead_rows = bool(ops.ATTN_LEFT_PAD and not col0 and (each_any or piece))
        ok = bool(col0) or dead_rows
        return _AttnMask(attention_mask, ok and past_len == 0, default_pos,
                         lambda: self._prepare_decoder_attention_mask(attention_mask, input_shape, inputs_embeds, past_len),
                         ok, pos_host, dead_rows=dead_rows)

    def _ssm_left_pad(self, attention_mask, x, past_key_values, pixel_values, output_att):
        """The SSM layers' mask slot: None - they read no mask, as in the reference, so the pads of a left-padded row run
        through conv and scan - or, with ops.SSM_LEFT_PAD, a _SsmStarts for a LEFT-PADDED PREFILL, which then gives every row
        what it gets alone (SelectiveLinearAttention.forward).  Only for: inference (eval, no autograd) on the GPU, a
        selective_ssm model, no incoming past_key_values, no image prefix (the conv would have to reach over the pads between
        image and text), no absolute position embeddings (a row alone would be positioned from 0), no output_attentions; a
        mask [B, L] whose rows are all 0...0 1...1 (ops.left_pad_starts) with at least ssm_conv_kernel - 1 valid tokens each,
        so that the cached conv window holds real inputs only, and with a pad somewhere.  Anything else: None, today's path.
        Two host reads, per prefill."""
        cfg = self.config
        if not (ops.SSM_LEFT_PAD and attention_mask is not None and x.is_cuda and not self.training
                and not torch.is_grad_enabled() and cfg.attention_type == "selective_ssm" and past_key_values is None
                and pixel_values is None and cfg.position_embedding_type != "absolute" and not output_att
                and tuple(attention_mask.shape) == tuple(x.shape[:2])):
            return None
        start = ops.left_pad_starts(attention_mask)
        if start is None:
            return None
        longest_pad = int(start.max())
        if longest_pad == 0 or x.shape[1] - longest_pad < cfg.ssm_conv_kernel - 1:
            return None
        return _SsmStarts(start.to(x.device))

    @_on_input_device
    def forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None,
                inputs_embeds=None, pixel_values=None, use_cache=None, output_attentions=None,
                output_hidden_states=None, return_dict=None, document_ids=None, _packed_kv=None):
        """document_ids: int64 [B, L], non-decreasing along L - PACKED rows (standard_mha, or selective_ssm on a ROCm device
        under ops.SSM_PACKED; no cache): a run of equal ids is one document, a token attends within its document only (an SSM
        layer's conv and state stop at its start) and, with position_ids = None, is positioned within it (the pad tail of a
        row is a document of its own, so no attention_mask goes with it); _packed_layout has the rules.
        _packed_kv (internal: ApertisForCausalLM.prefill_packed, which has made sure that the layers take the document
        kernels): the length of the row's longest document, a host integer.  The packed forward then keeps every layer's
        post-RoPE (k, v) [B, L, W] and returns them in slot 3, and that length - not the row's - is what the rotary table must
        hold.  Only the use_cache refusal of _packed_layout is skipped; every other check of it applies.
        past_key_values: a prefill's tuple of per-layer pairs (plain tensors in, plain tensors out), or for standard_mha an
        ops.KVCache: a single-token step then appends to it IN PLACE on the decode kernels and hands the same object back
        (position_ids = None: the step's position is the cache's length); a cache with `multi_token` set takes a forward of
        several tokens the same way, on the chunk kernels; a call the kernels do not take runs the stock branch on the
        cache's views and hands back plain tensors."""
        cfg = self.config
        use_c = cfg.use_cache if use_cache is None else use_cache
        if document_ids is not None:
            use_c = bool(use_cache)               # (a packed forward keeps no cache: the configuration's default does not apply)
        out_att = cfg.output_attentions if output_attentions is None else output_attentions
        out_hs = cfg.output_hidden_states if output_hidden_states is None else output_hidden_states
        if input_ids is not None and inputs_embeds is not None:
            raise ValueError("Specify one of input_ids or inputs_embeds.")
        if inputs_embeds is None:
            if input_ids is None:
                raise ValueError("input_ids required if inputs_embeds is None.")
            inputs_embeds = self.token_embeddings(input_ids)
        B, Lq = inputs_embeds.shape[:2]
        ssm = cfg.attention_type != "standard_mha"
        past_len = 0
        kv_cache = past_key_values if isinstance(past_key_values, ops.KVCache) else None
        dev_step = kv_cache is not None and (kv_cache.step_active or kv_cache.slot_active)
        if dev_step and (Lq != 1 or position_ids is not None or attention_mask is not None):
            raise ops.ApertisHipError("a KVCache whose device step state is active, or one in slot mode, takes one token per "
                                      "step, with its own positions and key validity (no position_ids, no attention_mask)")
        if kv_cache is not None:
            past_len = kv_cache.length            # (stale under a device step state: nothing below may depend on it then)
        elif past_key_values is not None and past_key_values[0] is not None and not ssm:
            past_len = past_key_values[0][0].shape[1]
        pos = position_ids
        layout = None
        if document_ids is not None:
            layout = self._packed_layout(document_ids, (B, Lq), attention_mask, past_key_values, use_c, pixel_values,
                                         inputs_embeds.device)
            attention_mask = None
            if pos is None:
                pos = layout.positions
            if _packed_kv is not None:
                if ssm or position_ids is not None:
                    raise ValueError("_packed_kv: standard_mha with the layout's own positions only (prefill_packed)")
                use_c = True
        if dev_step:
            if cfg.position_embedding_type == "absolute" and self.abs_pos_embeddings is not None:
                raise ops.ApertisHipError("absolute position embeddings need the step's position on the host: not with a "
                                          "KVCache device step state")
        elif pos is None:
            pos = torch.arange(past_len, past_len + Lq, device=inputs_embeds.device).unsqueeze(0).expand(B, -1)
        if not dev_step and cfg.position_embedding_type == "absolute" and self.abs_pos_embeddings is not None:
            inputs_embeds = inputs_embeds + self.abs_pos_embeddings(pos)
        x, pos_layers = inputs_embeds, pos
        if cfg.multimodal and pixel_values is not None and past_len == 0:              # core.py:1207-1227
            img = self.vision_projection_forward(self.multimodal_encoder(pixel_values))
            n_img = img.shape[1]
            x = torch.cat([img.to(inputs_embeds.dtype), inputs_embeds], dim=1)
            img_pos = torch.arange(n_img, device=x.device).unsqueeze(0).expand(B, -1)
            pos_layers = torch.cat([img_pos, pos + n_img], dim=1)
            if attention_mask is not None and attention_mask.shape[1] == Lq:
                attention_mask = torch.cat([attention_mask.new_ones(B, n_img), attention_mask], dim=1)
            elif attention_mask is None:
                attention_mask = torch.ones(B, n_img + Lq, dtype=torch.long, device=x.device)
        elif cfg.multimodal and pixel_values is not None:
            logger.warning("pixel_values provided with past_key_values: image ignored for this step")
        x = self.embed_dropout(x)
        own_pos = position_ids is None and pos_layers is pos
        if layout is not None and ssm:
            if out_att:
                raise ValueError("document_ids: a packed selective_ssm forward returns no attention weights (output_attentions)")
            mask = _SsmDocs(layout)
        elif layout is not None:
            window = _active_window(cfg)
            if window is not None and x.shape[1] > window:        # the documents' bounds clipped to the window, once per forward
                layout = ops.window_layout(layout, window)
            # (layout_pos as an integer: the bound of the positions, rope_qk's in_range - the longest document of prefill_packed)
            mask = _AttnMask(None, True, False, lambda: self._document_additive_mask(layout, x.dtype), layout=layout,
                             layout_pos=int(_packed_kv) if own_pos and _packed_kv is not None else own_pos)
        elif ssm:
            # (the SSM layers read no mask, as in the reference - under ops.SSM_LEFT_PAD the starts of a left-padded prefill)
            mask = self._ssm_left_pad(attention_mask, x, past_key_values, pixel_values, out_att)
        else:
            mask = self._attention_mask(attention_mask, (B, x.shape[1]), x, past_len, own_pos,
                                        past_len if own_pos and kv_cache is not None
                                        and (x.shape[1] == 1 or kv_cache.multi_token) else None,
                                        kv_cache if dev_step else None)
            mask.window = _active_window(cfg)

        all_hs, all_att, all_cache = [], [], []
        lbs, rzs = [], []
        prepass = isinstance(past_key_values, _StackedPast) and x.shape[1] == 1 and use_c and not out_att and not torch.is_grad_enabled()
        pre_all = self._decode_prepass(past_key_values) if prepass else None
        for i, layer in enumerate(self.layers):
            if out_hs:
                all_hs.append(x)
            past = past_key_values[i] if past_key_values and i < len(past_key_values) else None
            if pre_all is not None:
                # (the pre-pass has advanced every state in place: its row rides on a view made for this call, so none can go stale)
                past = _SsmLayerPast(past.conv, past.state, pre_all[i], past.inplace)
            if self.gradient_checkpointing and self.training and not use_c:             # core.py:1258
                x, att_w, cache, lb, rz = torch.utils.checkpoint.checkpoint(layer, x, mask, pos_layers, past, out_att,
                                                                            use_c, use_reentrant=False)
            else:
                # hidden states are only materialised at layer boundaries when somebody asked for them
                x, att_w, cache, lb, rz = layer(x, mask, pos_layers, past, out_att, use_c, defer=not out_hs)
            if out_att:
                all_att.append(att_w)
            if use_c:
                all_cache.append(cache)
            if cfg.use_expert_system:
                lbs.append(lb)
                rzs.append(rz)
        x, _ = _enter_block(self.final_post_norm, x)
        if out_hs:
            all_hs.append(x)
        if cfg.use_expert_system:
            # one reduction over the layers instead of two scalar adds per layer (core.py:1283-1287 sums as it goes)
            lb_tot = torch.stack(lbs).sum() if lbs else _zero_scalar(x.device, x.dtype)
            rz_tot = torch.stack(rzs).sum() if rzs else _zero_scalar(x.device, x.dtype)
        if kv_cache is not None and all_cache and all(c is kv_cache for c in all_cache):
            new_past = kv_cache                   # every layer appended in place (the decode kernels): the same object goes back
        else:
            new_past = tuple(all_cache) if use_c and all_cache else None
        return (x, tuple(all_hs) if out_hs and all_hs else None, tuple(all_att) if out_att and all_att else None,
                new_past,
                lb_tot if cfg.use_expert_system else None, rz_tot if cfg.use_expert_system else None)

    def _decode_prepass(self, st):
        """The cache-only half of a single-token step for ALL layers in three launches (csrc/decode_step.hip): the reference keeps
        the FIRST conv output of [cached window | new xp] (core.py:369-373), which sees window[0] only, so conv output,
        x_param_proj, dt projection and state update of a token step do not depend on the token.  Returns pre [NL,B,Dn] fp32 =
        C s + D xc per layer (the states in `st.state_all` are updated in place), or None when the stack is not uniform."""
        impls = [l.attention.attention_mechanism_impl for l in self.layers]
        m0 = impls[0]
        NL = len(impls)
        if (NL == 0 or any(not isinstance(m, SelectiveLinearAttention) for m in impls) or st.conv_all.shape[0] != NL
                or not st.conv_all.is_cuda or m0.conv_kernel_size < 2 or m0.conv_kernel_size > 16
                or st.conv_all.dtype not in (torch.float32, torch.bfloat16)):
            return None
        Dn, R, h, N = m0.d_inner, m0.dt_rank, m0.num_heads, m0.d_state
        if any((m.d_inner, m.dt_rank, m.num_heads, m.d_state, m.conv_kernel_size) != (Dn, R, h, N, m0.conv_kernel_size) for m in impls):
            return None
        # (the layers' decode branch must take what is computed here - the states are updated in place, once: the caches have to be
        #  exactly what that branch accepts as a window)
        if (tuple(st.conv_all.shape[2:]) != (Dn, m0.conv_kernel_size - 1) or tuple(st.state_all.shape[1:]) != (st.conv_all.shape[1], Dn)
                or st.state_all.dtype != torch.float32 or not (1 <= R <= 64 and 1 <= h <= 16)):    # (ops.tiny_linear_supported: dt inside the state kernel)
            return None
        B = st.conv_all.shape[1]
        if any((m.dt_proj_head.bias is None) != (m0.dt_proj_head.bias is None) or m.conv1d.bias is None for m in impls):
            return None
        srcs = tuple(t for m in impls for t in (m.conv1d.weight, m.conv1d.bias, m.x_param_proj.weight, m.dt_proj_head.weight,
                                               m.dt_proj_head.bias, m.A_log, m.D) if t is not None)

        def make():
            pads = [m._padded_param_weight() for m in impls]
            return (torch.stack([m.conv1d.weight.detach().float().reshape(Dn, -1) for m in impls]).contiguous(),
                    torch.stack([m.conv1d.bias.detach().float() for m in impls]).contiguous(),
                    torch.stack([p[0].detach().float() for p in pads]).contiguous(),
                    torch.stack([m.dt_proj_head.weight.detach().float() for m in impls]).contiguous(),
                    (None if impls[0].dt_proj_head.bias is None else
                     torch.stack([m.dt_proj_head.bias.detach().float() for m in impls]).contiguous()),
                    torch.stack([m.A_log.detach().float() for m in impls]).contiguous(),
                    torch.stack([m.D.detach().float() for m in impls]).contiguous(), pads[0][1], pads[0][2])

        conv_w, conv_b, wp, w_dt, b_dt, a_log, d_all, Wb, Wr = ops.cached_prep(("decode_stack", id(self)), srcs, make)
        xc_all = ops.decode_pre_conv(st.conv_all, conv_w, conv_b)
        offs = st.offsets(NL, B)
        p_all = ops.grouped_linear(xc_all.reshape(NL * B, Dn), wp, None, offs, NL * B, compute_dtype=xc_all.dtype)
        return ops.decode_pre_state(p_all, 0, Wb, 2 * Wb, w_dt, b_dt, a_log, d_all, xc_all, st.state_all)

    def vision_projection_forward(self, feats):
        """Linear(vision_embed_dim -> hidden) on the MFMA GEMM tile (core.py:1035,1209)."""
        if isinstance(self.vision_projection, nn.Identity):
            return feats
        return ops.linear_mfma(feats, self.vision_projection.weight, self.vision_projection.bias,
                               compute_dtype=_compute_dtype(feats))


def _select_tokens(logits, alive, eos, pad, drawn=None):
    """One decode step's selection: the argmax of the fp32 `logits` - or `drawn`, the tokens the stock sampling block drew
    from them - with `pad` for a finished sequence (alive 0), and the alive flags after the step: a sequence that emits one
    of the `eos` ids is finished.  Returns (tokens, new alive flags); `alive` itself is not written."""
    nxt = torch.argmax(logits, dim=-1) if drawn is None else drawn
    nxt = nxt * alive + pad * (1 - alive)
    for e_ in eos:
        if e_ is not None:
            alive = alive.masked_fill((nxt == e_) & (alive == 1), 0)
    return nxt, alive


class ApertisForCausalLM(nn.Module):
    def __init__(self, config: ApertisConfig):
        super().__init__()
        self.config = config
        self.model = ApertisModel(config)
        self.lm_head = nn.Linear(config.hidden_size, config.vocab_size, bias=False)
        if config.tie_word_embeddings:
            self.lm_head.weight = self.model.token_embeddings.weight
        else:
            self.lm_head.weight.data.normal_(0.0, config.initializer_range)
        # training-loop opt-in: loss straight from the hidden states, logits never materialised (forward returns
        # None in their slot).  Off by default: the reference's callers may read outputs[1].
        self.fused_lm_head_loss = False

    def load_state_dict(self, state_dict, strict=True):
        return super().load_state_dict(state_dict, strict=strict)

    def save_pretrained(self, save_directory):
        os.makedirs(save_directory, exist_ok=True)
        torch.save(self.state_dict(), os.path.join(save_directory, "pytorch_model.bin"))
        self.config.save_pretrained(save_directory)

    def get_output_embeddings(self):
        return self.lm_head

    def set_output_embeddings(self, new_lm_head):
        self.lm_head = new_lm_head

    def get_input_embeddings(self):
        return self.model.token_embeddings

    def gradient_checkpointing_enable(self):
        self.model.gradient_checkpointing_enable()

    def resize_token_embeddings(self, new_num_tokens: int) -> nn.Linear:
        self.model.resize_token_embeddings(new_num_tokens)
        if self.config.tie_word_embeddings and self.lm_head.weight.shape[0] == new_num_tokens:
            pass
        if self.config.tie_word_embeddings:
            self.lm_head.weight = self.model.token_embeddings.weight
            self.lm_head.out_features = new_num_tokens
        else:
            old = self.lm_head
            self.lm_head = nn.Linear(self.config.hidden_size, new_num_tokens, bias=False, device=old.weight.device,
                                     dtype=old.weight.dtype)
            self.lm_head.weight.data.normal_(0.0, self.config.initializer_range)
            n = min(old.out_features, new_num_tokens)
            self.lm_head.weight.data[:n] = old.weight.data[:n]
        self.config.vocab_size = self.lm_head.out_features
        return self.lm_head

    @_on_input_device
    def forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None,
                inputs_embeds=None, pixel_values=None, labels=None, use_cache=None, output_attentions=None,
                output_hidden_states=None, document_ids=None):
        """Returns the reference's 7-tuple (loss, logits, hidden_states, attentions,
        past_key_values, lb_loss, rz_loss)  (core.py:1361-1472).
        document_ids (packed rows, ApertisModel.forward): the label of a document's first token at t >= 1 is ignored, so
        the shifted loss never asks the last token of one document for the first of the next; the loss stays the mean over
        the remaining targets."""
        outs = self.model(input_ids=input_ids, attention_mask=attention_mask, position_ids=position_ids,
                          past_key_values=past_key_values, inputs_embeds=inputs_embeds, pixel_values=pixel_values,
                          use_cache=use_cache, output_attentions=output_attentions,
                          output_hidden_states=output_hidden_states, document_ids=document_ids)
        if document_ids is not None and labels is not None:
            first = torch.zeros_like(document_ids, dtype=torch.bool)
            first[:, 1:] = document_ids[:, 1:] != document_ids[:, :-1]
            labels = labels.masked_fill(first, -100)
        hs = outs[0]
        if self.config.multimodal and pixel_values is not None and past_key_values is None and input_ids is not None:
            start = hs.shape[1] - input_ids.shape[1]                     # text positions are last, core.py:1399-1406
            if start >= 0:
                hs = hs[:, start:]
        if (labels is not None and self.fused_lm_head_loss and self.training and
                ops.linear_cross_entropy_supported(hs, self.lm_head.weight, labels)):
            # LM head + shifted cross entropy one sequence at a time (core.py:1412-1450): no [B, L, V] logits tensor, the
            # tuple's logits slot is None.  Opt-in (TrainStep / ApertisTrainer set it: they only read the loss).
            loss = ops.linear_cross_entropy(hs, self.lm_head.weight, labels, ignore_index=-100, compute_dtype=_compute_dtype(hs))
            if outs[4] is not None:
                loss = loss + outs[4]
            if outs[5] is not None:
                loss = loss + outs[5]
            return (loss, None) + outs[1:]
        logits = self.lm_head(hs)
        loss = None
        if labels is not None:
            sl, tl = logits[..., :-1, :], labels[..., 1:]
            n = min(sl.shape[1], tl.shape[1])
            if n == 0:
                loss = torch.zeros((), device=logits.device, requires_grad=self.training)
            elif ops.shifted_cross_entropy_supported(logits, labels):
                loss = ops.shifted_cross_entropy(logits, labels, ignore_index=-100)     # core.py:1407-1416, one pass
            else:
                loss = F.cross_entropy(sl[:, :n].reshape(-1, sl.shape[-1]).float(), tl[:, :n].reshape(-1),
                                       ignore_index=-100)
            if outs[4] is not None:
                loss = loss + outs[4]
            if outs[5] is not None:
                loss = loss + outs[5]
        return (loss, logits) + outs[1:]

    def prepare_inputs_for_generation(self, input_ids, past_key_values=None, attention_mask=None,
                                      position_ids_override=None, **kwargs):
        B, L = input_ids.shape
        if past_key_values is not None:
            ids = input_ids[:, -1:]
            pos = torch.full((B, 1), attention_mask.shape[1] - 1, dtype=torch.long, device=input_ids.device)
        else:
            ids = input_ids
            pos = torch.arange(L, device=input_ids.device).unsqueeze(0).expand(B, -1)
        if position_ids_override is not None:
            pos = position_ids_override
        inputs = {"input_ids": ids, "past_key_values": past_key_values, "attention_mask": attention_mask,
                  "position_ids": pos, "use_cache": kwargs.get("use_cache", True)}
        if past_key_values is None and "pixel_values" in kwargs:
            inputs["pixel_values"] = kwargs["pixel_values"]
        return inputs

    @torch.no_grad()
    def generate(self, input_ids=None, attention_mask=None, position_ids=None, pixel_values=None,
                 max_new_tokens: Optional[int] = 20, min_new_tokens: Optional[int] = 0, do_sample: Optional[bool] = False,
                 temperature: Optional[float] = 1.0, top_k: Optional[int] = 50, top_p: Optional[float] = 1.0,
                 repetition_penalty: Optional[float] = 1.0, eos_token_id=None, pad_token_id=None,
                 use_cache: bool = True, past_key_values=None, prefill_chunk: Optional[int] = None, **kwargs):
        """Greedy / top-k / top-p / repetition-penalty decoding loop (reference core.py:1520-1644).  The prepared copies of
        the weights (stacked / padded / cast) are reused from token to token inside the call (ops.prep_cache_scope).

        past_key_values (standard_mha on the GPU): a `multi_token` ops.KVCache (new_kv_cache) the caller keeps between calls.
        It holds n = cache.length <= P - 1 rows, and the caller promises that they are the keys and values of
        input_ids[:, :n] under attention_mask[:, :n].  Only positions >= n are forwarded: the rest of the prompt goes into
        the cache on the chunk kernels in steps of at most `prefill_chunk` tokens (None: one step), then the usual loop runs
        on the same cache.  On return cache.length == output.shape[1] - 1: the next turn passes the output plus its new
        tokens and the same cache.  A cache that cannot be continued raises (_generate_cache_check); nothing is prefilled
        again silently."""
        if input_ids is None:
            raise ValueError("input_ids must be provided.")
        if kwargs.get("document_ids") is not None:
            raise ValueError("generate(): packed rows (document_ids) are a training form; generate one sequence per row")
        if past_key_values is not None:
            self._generate_cache_check(past_key_values, input_ids, position_ids, pixel_values, max_new_tokens, use_cache,
                                       prefill_chunk)
        elif prefill_chunk is not None:
            raise ValueError("generate(): prefill_chunk pieces a prompt into a KVCache passed as past_key_values")
        with ops.prep_cache_scope():
            return self._generate(input_ids, attention_mask, position_ids, pixel_values, max_new_tokens, min_new_tokens,
                                  do_sample, temperature, top_k, top_p, repetition_penalty, eos_token_id, pad_token_id,
                                  use_cache, past_key_values, prefill_chunk)

    def new_kv_cache(self, batch_size, capacity, dtype=None, device=None):
        """An empty `multi_token` ops.KVCache for this model (standard_mha): one [batch_size, capacity, hidden_size] k and v
        buffer per layer.  dtype: the autocast dtype if autocast is enabled, else the projection weights' (what the
        projections will produce: _mha_graph_ok's rule); device: the weights'."""
        cfg = self.config
        if cfg.attention_type != "standard_mha":
            raise ops.ApertisHipError(f"new_kv_cache: a KVCache serves standard_mha, not attention_type {cfg.attention_type!r}")
        w = self.model.layers[0].attention.q_proj.weight
        if dtype is None:
            dtype = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else w.dtype
        return ops.KVCache.empty(cfg.num_hidden_layers, batch_size, capacity, cfg.hidden_size, dtype,
                                 w.device if device is None else device, multi_token=True)

    def _generate_cache_check(self, cache, input_ids, position_ids, pixel_values, max_new_tokens, use_cache, prefill_chunk):
        """Everything generate(past_key_values=cache) needs of the cache and the call, checked before the first forward: a
        call that cannot continue the cache in place raises here rather than prefill again or leave the kernels."""
        cfg, err = self.config, ops.ApertisHipError
        if not isinstance(cache, ops.KVCache):
            raise err(f"generate(): past_key_values takes an ops.KVCache (new_kv_cache), not {type(cache).__name__}")
        if cfg.attention_type != "standard_mha":
            raise err(f"generate(): a KVCache serves standard_mha, not attention_type {cfg.attention_type!r}")
        if not cache.multi_token:
            raise err("generate(): the KVCache must be multi_token (new_kv_cache, or KVCache.empty(..., multi_token=True))")
        if not use_cache:
            raise err("generate(): past_key_values with use_cache=False")
        if pixel_values is not None:
            raise err("generate(): pixel_values together with a KVCache (the image rows are not part of input_ids)")
        if position_ids is not None:
            raise err("generate(): a KVCache takes the model's own positions (position_ids=None)")
        if not (ops.ATTN_FUSED and ops.ATTN_DECODE_FUSED) or self.training or cfg.output_attentions:
            raise err("generate(): a KVCache needs ops.ATTN_FUSED and ops.ATTN_DECODE_FUSED, eval mode and no output_attentions")
        if cache.step_active or len(set(cache.lengths)) != 1 or len(cache) != len(self.model.layers):
            raise err(f"generate(): the KVCache is mid-step or not this model's ({len(cache)} layers, lengths {cache.lengths})")
        attn = self.model.layers[0].attention
        want = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else attn.q_proj.weight.dtype
        B, P = input_ids.shape
        if tuple(cache.k[0].shape) != (B, cache.capacity, cfg.hidden_size) or cache.dtype != want:
            raise err(f"generate(): a KVCache of {tuple(cache.k[0].shape)} {cache.dtype} for {B} sequences of width "
                      f"{cfg.hidden_size} in {want}")
        if not ops.attention_decode_supported(cache.k[0], attn.num_attention_heads):
            raise err("generate(): the KV-cache kernels take head dims 64 and 128 in fp32 or bf16")
        n = cache.length
        if n > P - 1:
            raise err(f"generate(): the KVCache holds {n} rows but the prompt has {P} tokens (at most {P - 1} may be cached)")
        if P + max_new_tokens - 1 > cache.capacity:
            raise err(f"generate(): {P} prompt tokens and {max_new_tokens} new ones need {P + max_new_tokens - 1} rows, the "
                      f"KVCache has {cache.capacity}")
        if prefill_chunk is not None and prefill_chunk < 1:
            raise ValueError(f"generate(): prefill_chunk {prefill_chunk} < 1")
        if not input_ids.is_cuda or not cache.k[0].is_cuda:
            raise err("generate(): a KVCache needs the model and its inputs on the GPU (there is no CPU path)")

    def _generate(self, input_ids, attention_mask, position_ids, pixel_values, max_new_tokens, min_new_tokens, do_sample,
                  temperature, top_k, top_p, repetition_penalty, eos_token_id, pad_token_id, use_cache, cache=None,
                  prefill_chunk=None):
        B, prompt_len = input_ids.shape
        temp = max(temperature, 1e-6) if do_sample else 1.0
        eos = self.config.eos_token_id if eos_token_id is None else eos_token_id
        eos = [] if eos is None else (eos if isinstance(eos, list) else [eos])
        pad = pad_token_id if pad_token_id is not None else self.config.pad_token_id
        pad = 0 if pad is None else pad
        mask = torch.ones_like(input_ids) if attention_mask is None else attention_mask
        pos = position_ids
        if pos is None:
            pos = torch.arange(prompt_len, device=input_ids.device).unsqueeze(0).expand(B, -1)
        px = pixel_values
        if self.config.multimodal and px is not None:
            n_img = (self.config.image_size // self.config.vision_patch_size) ** 2 + 1
            mask = torch.cat([mask.new_ones(B, n_img), mask], dim=1)
            pos = torch.cat([torch.arange(n_img, device=input_ids.device).unsqueeze(0).expand(B, -1), pos + n_img], dim=1)
        tokens, past = input_ids, None
        rest = None
        if cache is not None and max_new_tokens > 0:
            # the caller's cache holds the first n positions: the rest of the prompt goes into it in pieces, all but the last
            # here (their logits select nothing); the loop's first forward takes the last piece instead of a prefill
            past, n = cache, cache.length
            step = prompt_len - n if prefill_chunk is None else prefill_chunk
            while prompt_len - n > step:
                self._cache_forward(cache, input_ids[:, n:n + step], mask[:, :n + step])
                n += step
            rest = input_ids[:, n:]
        alive = torch.ones(B, dtype=torch.long, device=input_ids.device)
        # sampling or a repetition penalty on the GPU: one kernel per step selects the token (ops.sample_next); the stock block
        # below stays for CPU tensors, vocabularies the kernel does not take and SAMPLE_FUSED = False
        fused = ops.SAMPLE_FUSED and input_ids.is_cuda and (do_sample or repetition_penalty != 1.0)
        sampler = None
        for _ in range(max_new_tokens):
            inp = self.prepare_inputs_for_generation(tokens if past is None else tokens[:, -1:], past_key_values=past,
                                                     attention_mask=mask,
                                                     position_ids_override=pos if past is None else None,
                                                     pixel_values=px, use_cache=use_cache)
            px = None
            # (a step against a KVCache takes its position from the cache's length, a host integer - the value
            #  prepare_inputs_for_generation puts into every row, mask.shape[1] - 1 - so the decode kernels need no read-back)
            if rest is not None:
                out, rest = self._cache_forward(cache, rest, mask), None
            else:
                out = self(input_ids=inp["input_ids"], attention_mask=inp["attention_mask"],
                           position_ids=None if isinstance(past, ops.KVCache) else inp["position_ids"],
                           past_key_values=inp["past_key_values"],
                           pixel_values=inp.get("pixel_values"), use_cache=inp["use_cache"])
            prefill = past is None
            past = out[4] if use_cache else None
            if cache is not None and past is not cache:
                raise ops.ApertisHipError("generate(): a token step left the KVCache (the decode kernels did not take it); "
                                          "the cache passed as past_key_values can no longer be continued")
            if prefill and past is not None and self._kv_cache_ok(past, tokens, max_new_tokens):
                # standard_mha: the prefill's (k, v) move into preallocated buffers once; every later step appends in place
                past = ops.KVCache.from_prefill(past, mask.shape[1] + max_new_tokens)
            if fused and sampler is None:
                fused = ops.sample_supported(out[1][:, -1, :])
                if fused:
                    sampler = ops.Sampler(out[1][:, -1, :], tokens, do_sample=do_sample, temperature=temperature, top_k=top_k,
                                          top_p=top_p, repetition_penalty=repetition_penalty, eos=eos, pad=pad)
            if sampler is not None:
                nxt, new_alive = sampler.step(out[1][:, -1, :], alive, tokens.shape[1] - prompt_len)
            else:
                nxt_logits, drawn = out[1][:, -1, :].float(), None
                if repetition_penalty != 1.0:
                    for b in range(B):
                        if alive[b]:
                            seen = tokens[b][tokens[b] < nxt_logits.shape[-1]]
                            for t_ in seen.tolist():                    # divides once per occurrence, like the reference
                                nxt_logits[b, t_] /= repetition_penalty
                if do_sample:
                    if temp != 1.0:
                        nxt_logits = nxt_logits / temp
                    if top_k > 0:
                        kth = torch.topk(nxt_logits, top_k).values[:, -1:]
                        nxt_logits = nxt_logits.masked_fill(nxt_logits < kth, float("-inf"))
                    if top_p < 1.0:
                        srt, order = torch.sort(nxt_logits, descending=True)
                        drop = torch.cumsum(F.softmax(srt, dim=-1), dim=-1) > top_p
                        drop[..., 1:] = drop[..., :-1].clone()
                        drop[..., 0] = False
                        nxt_logits = nxt_logits.masked_fill(torch.zeros_like(drop).scatter_(-1, order, drop), float("-inf"))
                    drawn = torch.multinomial(F.softmax(nxt_logits, dim=-1), 1).squeeze(1)
                nxt, new_alive = _select_tokens(nxt_logits, alive, eos, pad, drawn)
            tokens = torch.cat([tokens, nxt.unsqueeze(-1)], dim=-1)
            mask = torch.cat([mask, alive.unsqueeze(-1).to(mask.dtype)], dim=1)     # (the flags the token was selected under)
            alive = new_alive
            if sampler is None:
                stop = bool(alive.max() == 0)
            else:                                                       # (the sampler's error word rides in the step's one read)
                any_alive, code = torch.cat((alive.max().reshape(1), sampler.err.to(alive.dtype))).tolist()
                sampler.check(code)
                stop = any_alive == 0
            if stop and tokens.shape[1] - prompt_len >= min_new_tokens:
                break
            left = max_new_tokens - (tokens.shape[1] - prompt_len)
            if (past is not None and left >= DECODE_GRAPH_MIN_STEPS
                    and self._decode_graph_ok(tokens, do_sample, repetition_penalty, sampler, past, left, mask)):
                # the remaining single-token steps as ONE captured HIP graph replayed `left` times (same kernels, same tokens)
                return self._generate_graph_tail(tokens, past, alive, left, prompt_len, min_new_tokens, eos, pad,
                                                 sampler=sampler, mask=mask)
        return tokens

    def _cache_forward(self, cache, ids, mask):
        """One forward of `ids` (the positions after the rows `cache` holds) that must extend the caller's cache in place: a
        forward the KV-cache kernels did not take (it hands plain tensors back and leaves the cache behind) raises."""
        out = self(input_ids=ids, attention_mask=mask, position_ids=None, past_key_values=cache, use_cache=True)
        if out[4] is not cache:
            raise ops.ApertisHipError(f"generate(): a forward of {ids.shape[1]} tokens against the KVCache did not run on the "
                                      "KV-cache kernels (key 0 of a sequence masked without APERTIS_MHA_LEFT_PAD=1, a sequence "
                                      "with no valid key, or the attention mask does not cover the prompt): there is no "
                                      "fallback that keeps the cache")
        return out

    def _kv_cache_ok(self, past, tokens, max_new_tokens):
        """Whether generate() carries this prefill's cache as an ops.KVCache (the decode kernels then take every step that
        qualifies, ApertisAttention._decode_ok): standard_mha on the GPU, both switches on, fp32 or bf16 with D 64 or 128."""
        cfg = self.config
        return (cfg.attention_type == "standard_mha" and ops.ATTN_FUSED and ops.ATTN_DECODE_FUSED and tokens.is_cuda
                and max_new_tokens > 1 and not self.training and not torch.is_grad_enabled()
                and isinstance(past[0], tuple) and len(past[0]) == 2 and past[0][0].dim() == 3
                and ops.attention_decode_supported(past[0][0], cfg.num_attention_heads))

    def _decode_graph_ok(self, tokens, do_sample, repetition_penalty, sampler=None, past=None, left=0, mask=None, slots=False):
        """slots: generate_many()'s step over KV-cache slots - device-state by construction, so the standard_mha conditions of
        generate()'s tail (_mha_graph_ok, ops.ATTN_DECODE_GRAPH) do not apply."""
        cfg = self.config
        # (sampling and the penalty replay too when the fused sampler selects the tokens: its kernel reads the step counter
        #  and the occurrence table from device buffers)
        ok = (DECODE_GRAPH and tokens.is_cuda and (sampler is not None or (not do_sample and repetition_penalty == 1.0))
              and not torch.is_grad_enabled() and cfg.position_embedding_type != "absolute" and not self.training)
        if cfg.attention_type != "standard_mha" or slots:
            return ok
        return ok and self._mha_graph_ok(tokens, past, left, mask)

    def _mha_graph_ok(self, tokens, past, left, mask):
        """Whether the remaining `left` token steps of a standard_mha model replay as a graph (opt-in: ops.ATTN_DECODE_GRAPH):
        every precondition of ApertisAttention._decode_ok that does not change from step to step, checked ONCE - the past is
        an ops.KVCache in the dtype the projections produce, with room for every remaining row; the rotary table reaches the
        last position; key 0 of every sequence is valid, or with ops.ATTN_LEFT_PAD some key of every sequence (one host read
        here; the columns so far do not change afterwards).  Anything
        else stays on the eager loop, which raises where it always did when a position runs off the table."""
        if not (ops.ATTN_DECODE_GRAPH and ops.ATTN_FUSED and ops.ATTN_DECODE_FUSED and isinstance(past, ops.KVCache)
                and not past.step_active and len(set(past.lengths)) == 1 and not self.config.output_attentions):
            return False
        attn = self.model.layers[0].attention
        n, (B, cap, _) = past.length, past.k[0].shape
        window = _active_window(self.config)
        if window is not None and n + left > window and not ops.ATTN_WINDOW_CACHE:
            return False                         # (opt-in: the replayed step's window form, KVCache.step_state_begin(window=))
        want = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else attn.q_proj.weight.dtype
        if not (n == tokens.shape[1] - 1 and B == tokens.shape[0] and n + left <= cap and past.dtype == want
                and len(past) == len(self.model.layers) and ops.attention_decode_supported(past.k[0], attn.num_attention_heads)
                and (attn.rope is None or n + left <= attn.rope.cos_cached.shape[0])):
            return False
        if mask is None or tuple(mask.shape) != (B, n + 1):
            return mask is None
        return bool(mask.bool().any(1).all() if ops.ATTN_LEFT_PAD else mask[:, 0].all())

    def _generate_graph_tail(self, tokens, past, alive, left, prompt_len, min_new_tokens, eos, pad, sampler=None, mask=None):
        """Decoding of `left` more tokens through a captured HIP graph of the single-token step (reference core.py:1578-1644:
        the same forward through the cache, then the eager loop's selection, _select_tokens - attention mask and position ids
        do not enter an SSM model's step).  An eager token step is ~2 600 small launches, 18 ms of mostly host time at 44
        layers; the replay is 10 ms (tools/decode_graph_try.py).  Token, cache, alive flags, the step counter and the outputs
        live in static buffers that the graph updates in place; the host looks at the alive flags every 16 steps only.
        With a `sampler` (ops.Sampler: sampling or a repetition penalty) its kernel replaces the argmax and the pad / eos
        updates; its occurrence table and error word are static buffers too, and its draw counter is the step index.
        standard_mha (`past` an ops.KVCache, `mask` the key validity so far): the cache itself is the static state.  Its device
        step state (length, key validity, error word) is activated here; the step's kernels read row, position and key count
        from it, on a grid fixed for the whole tail; after the forward the body writes the validity column of the token about
        to be selected (the alive flags it is selected under - the column the eager loop appends) and ends with
        `dev_len += 1`.  No KV buffer is cloned: the rows the warm-up writes are at or beyond the starting length, and the
        replay rewrites them."""
        B, dev = tokens.shape[0], tokens.device
        cache = past if isinstance(past, ops.KVCache) else None
        s_tok = tokens[:, -1:].clone()
        s_alive = alive.clone()
        s_idx = torch.zeros(1, dtype=torch.long, device=dev)
        s_out = torch.full((B, left), pad, dtype=tokens.dtype, device=dev)
        s_any = torch.ones(left, dtype=alive.dtype, device=dev)          # max over the batch of `alive` after each step
        # what the body updates in place: saved before the warm-up, restored after it and after the capture
        state = [s_tok, s_alive]
        s_nxt = torch.empty(B, dtype=torch.long, device=dev)            # (the sampler's tokens)
        off = tokens.shape[1] - prompt_len                      # (steps already decoded: the draw counter goes on from there)
        if sampler is not None:
            state += [t for t in (sampler.counts, sampler.err) if t is not None]
        start, cap, err_word = 0, 0, None
        if cache is None:
            # (contiguous copies: the prefill hands the conv window over as a transposed view, and a cache that is not contiguous
            #  is copied in and out of every token step instead of being updated in place - two launches per layer: `inplace`)
            s_past = [_SsmLayerPast(c.clone(memory_format=torch.contiguous_format), st.clone(memory_format=torch.contiguous_format),
                                    inplace=True) for (c, st) in past]
            if (DECODE_PREPASS and len(s_past) > 0 and all(c.dim() == 3 and st.dim() == 3 and st.dtype == torch.float32 and
                                                           c.shape == s_past[0][0].shape and st.shape == s_past[0][1].shape
                                                           and c.dtype == s_past[0][0].dtype for c, st in s_past)):
                # one tensor per kind, the per-layer caches as views: the cache-only half of every layer's step runs at once
                conv_all = torch.stack([c for c, _ in s_past]).contiguous()
                state_all = torch.stack([st.reshape(st.shape[0], -1) for _, st in s_past]).contiguous()
                s_past = _StackedPast(conv_all, state_all, s_past[0][1].shape[1], s_past[0][1].shape[2], inplace=True)
            state += [t for pair in s_past for t in pair]
        else:
            s_past, start, cap = cache, cache.length, cache.capacity
            # one split count for the whole tail, from the length it ends at (which end to size for)
            # (a window reaches the replayed step only under ops.ATTN_WINDOW_CACHE: without it _mha_graph_ok let no tail past the
            #  window in, and the launches stay the ones they were)
            window = _active_window(self.config) if ops.ATTN_WINDOW_CACHE else None
            cache.step_state_begin(self.config.num_attention_heads, mask, L_end=start + left, window=window)
            state += [cache.dev_len, cache.dev_valid, cache.dev_err]
            err_word = cache.dev_err

        def body():
            out = self(input_ids=s_tok, past_key_values=s_past, use_cache=True)
            if cache is not None:
                # the new token's validity column (row dev_len + 1: the step above filled row dev_len), once per step, with the
                # flags the token is selected under; the clamp keeps a length that ran away (the error word says so) inside the buffer
                cache.dev_valid.scatter_(1, (cache.dev_len + 1).clamp_(max=cap - 1).expand(B, 1), s_alive.unsqueeze(1))
            if sampler is None:
                nxt, al = _select_tokens(out[1][:, -1, :].float(), s_alive, eos, pad)
                s_alive.copy_(al)
            else:
                sampler.step(out[1][:, -1, :], s_alive, off, step=s_idx, alive_out=s_alive, out=s_nxt)
                nxt = s_nxt
            s_out.scatter_(1, s_idx.expand(B, 1), nxt.unsqueeze(1).to(s_out.dtype))
            s_any.scatter_(0, s_idx, s_alive.max().reshape(1))
            s_idx.add_(1)
            s_tok.copy_(nxt.unsqueeze(1))
            if cache is not None:
                cache.dev_len.add_(1)
            else:
                for (sc, ss), (nc, ns) in zip(s_past, out[4]):
                    if nc.data_ptr() != sc.data_ptr():     # (both updated in place by the step: the views say `inplace`)
                        sc.copy_(nc)
                    if ns.data_ptr() != ss.data_ptr():
                        ss.copy_(ns)

        kept = 0
        try:
            out = self._generate_graph_run(body, state, (s_idx, s_out, s_any), tokens, left, prompt_len, min_new_tokens, pad,
                                           sampler=sampler, err_word=err_word)
            kept = out.shape[1] - tokens.shape[1]
            return out
        finally:
            if cache is not None:
                cache.step_state_end(start + kept)       # (the replay may have run up to 15 steps past the last token kept)

    def _generate_graph_run(self, body, state, outputs, tokens, left, prompt_len, min_new_tokens, pad, sampler=None, err_word=None):
        """Warm-up, capture and replay of `body` for `left` steps.  `state`: the tensors the body updates in place (token, alive
        flags, caches, the sampler's occurrence table and error word, a KVCache's step state); `outputs`: the step counter,
        the tokens and the per-step alive maximum, which start from zero / pad / one."""
        s_idx, s_out, s_any = outputs
        keep = [t.clone() for t in state]

        def restore():
            for t, k in zip(state, keep):
                t.copy_(k)
            s_idx.zero_()
            s_out.fill_(pad)
            s_any.fill_(1)

        graph = self._capture_step(body, restore, tokens.device)
        done = left
        for i in range(left):
            graph.replay()
            if (i + 1) % 16 == 0 or i + 1 == left:
                if err_word is None:
                    flags = s_any[:i + 1].tolist()                     # the only host sync: every 16 steps
                else:                                                  # (the KV cache's error word rides in the same read)
                    *flags, code = torch.cat((s_any[:i + 1], err_word.to(s_any.dtype))).tolist()
                    if code:
                        raise ops.ApertisHipError("generate(): a replayed KV-cache step ran past the cache or the rotary table "
                                                  f"(error word {code}); nothing was written by that step")
                if sampler is not None:
                    sampler.check()
                stop = next((j for j, a in enumerate(flags)
                             if a == 0 and tokens.shape[1] - prompt_len + j + 1 >= min_new_tokens), None)
                if stop is not None:
                    done = stop + 1
                    break
        return torch.cat([tokens, s_out[:, :done]], dim=-1)

    @staticmethod
    def _capture_step(body, restore, dev):
        """`body` as a captured graph: warm-up on a side stream (lazy bindings, prepared-weight cache, allocator), `restore()`
        of the state it advanced, the capture, `restore()` again."""
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(2):
                body()
        torch.cuda.current_stream(dev).wait_stream(side)
        restore()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):    # (another thread's GPU work - a trainer thread beside chat - must not fail on this capture)
            body()
        restore()
        return graph

    _NO_PACKED_SSM_PREFILL = ("a selective_ssm model has no packed prefill: the packed scan returns no per-document end state "
                              "and no conv window; that needs kernel work and is not offered")

    def _packed_prefill_refusals(self, what):
        """What keeps a packed prefill off the document kernels, each a ValueError naming the condition, before any GPU
        work: there is no stock fallback (ApertisAttention._fused_ok would quietly take one)."""
        cfg, attn = self.config, self.model.layers[0].attention
        if cfg.attention_type != "standard_mha":
            raise ValueError(f"{what}: {self._NO_PACKED_SSM_PREFILL}")
        if self.lm_head.weight.device.type != "cuda":
            raise ValueError(f"{what}: the model is not on a GPU (there is no CPU path)")
        if self.training:
            raise ValueError(f"{what}: the model is in training mode (call .eval())")
        if cfg.output_attentions:
            raise ValueError(f"{what}: output_attentions (the document kernels return no attention weights)")
        if not ops.ATTN_FUSED:
            raise ValueError(f"{what}: ops.ATTN_FUSED is off (a packed prefill runs on the document kernels only)")
        if attn.attention_head_size not in (64, 128) or cfg.hidden_size != attn.attention_head_size * attn.num_attention_heads:
            raise ValueError(f"{what}: head dim {attn.attention_head_size} (the document kernels take 64 or 128)")
        if self._mha_slot_dtype() not in (torch.float32, torch.bfloat16):
            raise ValueError(f"{what}: dtype {self._mha_slot_dtype()} (the document kernels take fp32 or bf16)")

    @torch.no_grad()
    def prefill_packed(self, prompts):
        """The prefill of n >= 1 prompts of a standard_mha model as ONE forward over a packed row [1, sum L_i]: the prompts
        are the row's documents 0 ... n-1 in list order (ApertisModel.forward(document_ids=...)), so a token attends within
        its prompt only and is positioned within it, the attention runs on the document kernels (ops.document_attention:
        key tiles in front of a query's document are skipped) and no padding is computed.  A token's K and V rows depend on
        its own document alone, so slicing every layer's post-RoPE (k, v) of the row by document gives each prompt the
        prefill cache it gets in a row of its own - up to the rounding of projections run at another row count.

        prompts: 1-D int64 tensors on the model's GPU, or lists of ids, each of at least one token and no longer than the
        rotary table (the row may be longer than the table: the longest prompt is what it must hold).
        Returns (logits, pasts): logits [n, V], the LM head on the n last-token rows of the final hidden states (gathered
        before the head: the [sum L_i, V] logits are never formed); pasts[i], a tuple per layer of (k, v), each [1, L_i, W] -
        VIEWS of the packed row's tensors, not copies, in the form KVCache.slot_install and KVCache.from_prefill take (both
        copy).  One host read, ops.document_layout's.

        Eval mode, on the GPU, no autograd.  There is no stock fallback: ops.ATTN_FUSED off, a head dim other than 64 / 128,
        a dtype other than fp32 / bf16, output_attentions, training mode, a CPU model or a selective_ssm model raise
        ValueError before any GPU work (_packed_prefill_refusals), as do an empty list, an empty prompt and a prompt longer
        than the rotary table.  The public forward(document_ids=..., use_cache=True) keeps raising: only this method keeps
        a packed row's (k, v).

        MoE models: the expert capacity limit applies in training mode only (AdaptiveExpertSystem.forward), so in eval mode
        routing is per token and a packed row changes no document's routing."""
        self._packed_prefill_refusals("prefill_packed()")
        cfg, dev = self.config, self.lm_head.weight.device
        prompts = list(prompts)
        if not prompts:
            raise ValueError("prefill_packed(): no prompts")
        rope = self.model.layers[0].attention.rope
        max_pos = rope.cos_cached.shape[0] if rope is not None else cfg.max_position_embeddings
        for i, p in enumerate(prompts):
            if isinstance(p, torch.Tensor) and (p.device != dev or p.dim() != 1 or p.dtype != torch.int64):
                raise ValueError(f"prefill_packed(): prompt {i} is a {p.dtype} tensor of shape {tuple(p.shape)} on {p.device}, "
                                 "expected 1-D int64 on the model's GPU")
            if len(p) == 0:
                raise ValueError(f"prefill_packed(): prompt {i} is empty")
            if len(p) > max_pos:
                raise ValueError(f"prefill_packed(): prompt {i} of {len(p)} tokens runs past the rotary table ({max_pos} "
                                 "positions)")
        lens = [len(p) for p in prompts]
        ends = list(itertools.accumulate(lens))
        with ops.prep_cache_scope(), ops.device_guard(self.lm_head.weight):
            ids = [p if isinstance(p, torch.Tensor) else torch.tensor(list(p), dtype=torch.int64, device=dev) for p in prompts]
            docs = torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens)).to(dev)
            outs = self.model(input_ids=torch.cat(ids)[None], document_ids=docs[None], _packed_kv=max(lens))
            last = torch.tensor([e - 1 for e in ends], dtype=torch.int64).to(dev)
            logits = self.lm_head(outs[0][0].index_select(0, last))
        pasts = [tuple((k[:, a:b], v[:, a:b]) for k, v in outs[3]) for a, b in zip([0] + ends, ends)]
        return logits, pasts

    @torch.no_grad()
    def generate_many(self, prompts, max_new_tokens=20, slots: int = 16, do_sample: bool = False, temperature: float = 1.0,
                      top_k: int = 50, top_p: float = 1.0, repetition_penalty: float = 1.0, eos_token_id=None,
                      pad_token_id=None, return_stats: bool = False, pixel_values=None, prefill_tokens: Optional[int] = None):
        """generate() for many prompts of a selective_ssm model on ONE decode batch of `slots` rows whose finished rows are
        refilled: a prompt is prefilled alone (the call generate() makes for it), its conv windows and SSM states are copied
        into a free row of the static decode state, and the token step - the graph-replayed one where generate() would
        replay - runs over all rows until nothing waits and no row is live.  No padding is computed, prompts need not be
        equally long, and a row that ends early makes room for the next prompt.

        prompts: 1-D int64 tensors on the model's GPU, or lists of ids, of any lengths >= 1; max_new_tokens: one integer or
        one per prompt; slots: 1...16 (the row bound of the small-step kernels).  Returns a list of 1-D int64 tensors in the
        order of `prompts`: the prompt and its new tokens, up to and with its first eos or `max_new_tokens` of them, never
        padded - what generate(prompts[i][None], max_new_tokens=m_i, ...) returns for it alone, cut after the first eos.
        Greedy decoding (with or without a repetition penalty) is token-equal to those alone runs.  With do_sample=True every
        row is drawn from the distribution it would be drawn from alone, but with the draw counter of this call's one
        ops.Sampler - (seed, slot row, step of the call) - so a sampled run is NOT token-equal to the alone run under the
        same torch seed.  There is no min_new_tokens (in generate() it is a condition on the batch, not a per-row rule).

        A prompt shorter than ssm_conv_kernel - 1 tokens has no full conv window to install: it runs through generate()
        alone when its turn comes.  standard_mha models, absolute position embeddings, pixel_values, output_attentions,
        training mode and CPU tensors raise ValueError before any GPU work.

        standard_mha under ops.ATTN_SLOTS (opt-in, APERTIS_MHA_SLOTS=1): the same call on KV-cache slots - one ops.KVCache of
        `slots` rows in slot mode, a length per row.  A prompt of any length >= 1 is prefilled alone
        and installed; there is no fallback, `stats["fallbacks"]` stays empty.  The step replays as a graph under
        DECODE_GRAPH / DECODE_GRAPH_MIN_STEPS exactly like the SSM slots (ops.ATTN_DECODE_GRAPH is generate()'s switch and
        is not consulted).  Refused on top of the list above, before any GPU work (_mha_slots_refusals): a head dim other
        than 64 / 128 or a dtype other than fp32 / bf16, an active sliding window, ops.ATTN_FUSED or ops.ATTN_DECODE_FUSED
        off, a prompt whose length + budget - 1 exceeds the rotary table.

        prefill_tokens (standard_mha under ops.ATTN_SLOTS only; None, the default: every prompt is prefilled alone, as
        above): an integer >= 1 makes a refill ROUND of the waiting prompts - in arrival order one per free slot, until the
        next one would bring the round's prompt tokens past `prefill_tokens`, at least one (serving.prefill_round).  A round
        of two or more prompts is ONE prefill_packed() call, whose per-document (k, v) views slot_install copies; a round of
        one prompt is the batch-1 forward of the default.  Every prompt's first token is selected by the calls the default
        makes for it (the sampled draw has the prompt's prefill ordinal as its counter, so it does not depend on the knob),
        with one host read per round instead of one per prompt; a prompt that ends at its first token leaves its slot free
        for the next round.  Greedy runs are token-equal to the alone runs as long as no step's top-2 logits tie within the
        rounding of projections run at another row count.  Anything but an integer >= 1 (bools included) and a selective_ssm
        model (its packed scan returns no per-document end state and no conv window) raise ValueError before any forward.

        return_stats=True: (outputs, stats) with stats = {"steps": token steps run, "replays": of them graph replays,
        "graphs": graphs captured, "prefills": prompts prefilled into slots, "live_slot_steps": sum over steps of the rows
        whose token was kept, "slot_steps": steps * slots, "fallbacks": indices of the prompts that ran through
        generate()} - and, only when prefill_tokens is not None, "prefill_forwards": the prefill forwards run (batch-1
        ones plus packed ones)."""
        cfg = self.config
        mha = cfg.attention_type == "standard_mha"
        if mha and not ops.ATTN_SLOTS:
            raise ValueError("generate_many(): slots serve selective_ssm models; a standard_mha model batches through "
                             "generate(past_key_values=...) with a KVCache, or one left-padded generate() batch (KV-cache "
                             "slots are opt-in: ops.ATTN_SLOTS / APERTIS_MHA_SLOTS=1)")
        if prefill_tokens is not None:
            if isinstance(prefill_tokens, bool) or not isinstance(prefill_tokens, int) or prefill_tokens < 1:
                raise ValueError(f"generate_many(): prefill_tokens must be None or an integer >= 1, got {prefill_tokens!r}")
            if not mha:
                raise ValueError(f"generate_many(prefill_tokens=...): {self._NO_PACKED_SSM_PREFILL}")
        if cfg.position_embedding_type == "absolute":
            raise ValueError("generate_many(): absolute position embeddings (a slot's position would differ per row)")
        if pixel_values is not None:
            raise ValueError("generate_many(): pixel_values (an image prefix is not part of a slot's state)")
        if self.training:
            raise ValueError("generate_many(): the model is in training mode (call .eval())")
        if cfg.output_attentions:
            raise ValueError("generate_many(): output_attentions")
        if not mha and cfg.ssm_conv_kernel < 2:
            raise ValueError("generate_many(): ssm_conv_kernel < 2 (the single-token step needs a conv window)")
        if not 1 <= slots <= GENERATE_MANY_MAX_SLOTS:
            raise ValueError(f"generate_many(): slots = {slots}, the small-step kernels take 1...{GENERATE_MANY_MAX_SLOTS} rows")
        prompts = list(prompts)
        budgets = [max_new_tokens] * len(prompts) if isinstance(max_new_tokens, int) else [int(m) for m in max_new_tokens]
        if len(budgets) != len(prompts):
            raise ValueError(f"generate_many(): {len(budgets)} max_new_tokens for {len(prompts)} prompts")
        dev = self.lm_head.weight.device
        if dev.type != "cuda":
            raise ValueError("generate_many(): the model is not on a GPU (there is no CPU path)")
        for i, p in enumerate(prompts):
            if isinstance(p, torch.Tensor) and (not p.is_cuda or p.dim() != 1 or p.dtype != torch.int64):
                raise ValueError(f"generate_many(): prompt {i} is a {p.dtype} tensor of shape {tuple(p.shape)} on {p.device}, "
                                 "expected 1-D int64 on the model's GPU")
            if len(p) == 0:
                raise ValueError(f"generate_many(): prompt {i} is empty")
        if mha:
            self._mha_slots_refusals([len(p) for p in prompts], budgets)
        ids = [p if isinstance(p, torch.Tensor) else torch.tensor(list(p), dtype=torch.int64, device=dev) for p in prompts]
        with ops.prep_cache_scope(), ops.device_guard(self.lm_head.weight):
            outs, stats = self._generate_many(ids, budgets, slots, do_sample, temperature, top_k, top_p, repetition_penalty,
                                              eos_token_id, pad_token_id, prefill_tokens)
        return (outs, stats) if return_stats else outs

    def _mha_slot_dtype(self):
        """The dtype the projections produce, and with it a prefill's (k, v) and the slot cache (_mha_graph_ok's rule)."""
        return (torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda")
                else self.model.layers[0].attention.q_proj.weight.dtype)

    def _mha_slots_refusals(self, lens, budgets):
        """What generate_many() refuses of a standard_mha model under ops.ATTN_SLOTS beyond the common list, before any
        forward (each a ValueError): a head dim or dtype the decode kernels do not take; an active sliding window (the window
        form of the device-length attention measures its window from the ONE length it reads, which is wrong for every row
        but the longest); ops.ATTN_FUSED or ops.ATTN_DECODE_FUSED off (there is no stock step over slots); a prompt whose
        last step would be positioned beyond the rotary table (serving.mha_slot_overrun)."""
        from .serving import mha_slot_overrun
        cfg, attn = self.config, self.model.layers[0].attention
        if attn.attention_head_size not in (64, 128) or cfg.hidden_size != attn.attention_head_size * attn.num_attention_heads:
            raise ValueError(f"generate_many(): head dim {attn.attention_head_size} (the KV-cache decode kernels take 64 or 128)")
        if self._mha_slot_dtype() not in (torch.float32, torch.bfloat16):
            raise ValueError(f"generate_many(): dtype {self._mha_slot_dtype()} (the KV-cache decode kernels take fp32 or bf16)")
        if _active_window(cfg) is not None:
            raise ValueError("generate_many(): sliding_window under ops.ATTN_WINDOW (a slot's window would be measured from "
                             "the longest slot's length)")
        if not (ops.ATTN_FUSED and ops.ATTN_DECODE_FUSED):
            raise ValueError("generate_many(): KV-cache slots run on the decode kernels (ops.ATTN_FUSED and "
                             "ops.ATTN_DECODE_FUSED); there is no stock step over slots")
        if attn.rope is not None:
            max_pos = attn.rope.cos_cached.shape[0]
            i = mha_slot_overrun(lens, budgets, max_pos)
            if i is not None:
                raise ValueError(f"generate_many(): prompt {i} of {lens[i]} tokens with {budgets[i]} new ones runs past the "
                                 f"rotary table ({max_pos} positions)")

    def _slot_state(self, past, S):
        """Zeroed decode state for S rows, shaped after one prefill's per-layer (conv window [1, Dn, k-1], state [1, h, N]): the
        stacked form the graph tail builds (_StackedPast: the cache-only half of a step runs for all layers at once) under
        its condition, else one pair of buffers per layer.  Returns (state, the tensors a step updates in place)."""
        c0, st0 = past[0]
        if (DECODE_PREPASS and all(c.dim() == 3 and st.dim() == 3 and st.dtype == torch.float32 and c.shape == c0.shape
                                   and st.shape == st0.shape and c.dtype == c0.dtype for c, st in past)):
            conv_all = torch.zeros((len(past), S) + tuple(c0.shape[1:]), dtype=c0.dtype, device=c0.device)
            state_all = torch.zeros(len(past), S, st0.shape[1] * st0.shape[2], dtype=torch.float32, device=c0.device)
            return _StackedPast(conv_all, state_all, st0.shape[1], st0.shape[2], inplace=True), [conv_all, state_all]
        state = [_SsmLayerPast(torch.zeros((S,) + tuple(c.shape[1:]), dtype=c.dtype, device=c.device),
                               torch.zeros((S,) + tuple(st.shape[1:]), dtype=st.dtype, device=st.device), inplace=True)
                 for c, st in past]
        return state, [t for pair in state for t in pair]

    def _generate_many(self, ids, budgets, S, do_sample, temperature, top_k, top_p, repetition_penalty, eos_token_id,
                       pad_token_id, prefill_tokens=None):
        """generate_many()'s loop.  The slot state is the SSM layers' conv windows and states (_slot_state), or - standard_mha
        under ops.ATTN_SLOTS - ONE ops.KVCache in slot mode with serving.mha_slot_capacity rows per slot, allocated once per
        call: a prompt's batch-1 prefill is installed with KVCache.slot_install, a freed row is emptied with slot_free where
        the alive flags are rewritten, the step body is bracketed by slots_step_begin / slots_step_end, and the cache's error
        word rides in the burst's host read.  Everything else - the schedule, the burst rule, the sampler's handling, the
        capture - is one code for both.  `prefill_tokens` (standard_mha only, checked by the caller): refill rounds whose
        two or more prompts are one prefill_packed() forward; a prompt's first token and install are `settle` either way."""
        from .serving import SlotSchedule, mha_slot_capacity, prefill_round
        cfg, dev = self.config, self.lm_head.weight.device
        mha = cfg.attention_type == "standard_mha"
        eos = cfg.eos_token_id if eos_token_id is None else eos_token_id
        eos = [] if eos is None else (eos if isinstance(eos, list) else [eos])
        eos_set = frozenset(int(e) for e in eos if e is not None)
        pad = pad_token_id if pad_token_id is not None else cfg.pad_token_id
        pad = 0 if pad is None else pad
        window = 0 if mha else cfg.ssm_conv_kernel - 1        # (any prompt fits a KV-cache slot: no fallback there)
        sched = SlotSchedule(len(ids), budgets, S)
        stats = {"steps": 0, "replays": 0, "graphs": 0, "prefills": 0, "live_slot_steps": 0, "slot_steps": 0, "fallbacks": []}
        if prefill_tokens is not None:
            stats["prefill_forwards"] = 0
        s_tok = torch.full((S, 1), pad, dtype=torch.long, device=dev)
        s_alive = torch.zeros(S, dtype=torch.long, device=dev)
        s_idx = torch.zeros(1, dtype=torch.long, device=dev)            # column of s_out: zeroed before every burst
        s_step = torch.zeros(1, dtype=torch.long, device=dev)           # steps of the whole call: the sampler's draw counter
        burst = max(int(GENERATE_MANY_BURST), 1)
        s_out = torch.full((S, max(burst, 2)), pad, dtype=torch.long, device=dev)      # (the capture's warm-up runs two steps)
        s_nxt = torch.empty(S, dtype=torch.long, device=dev)
        s_ones = torch.ones(S, dtype=torch.long, device=dev)            # the alive flags of a refill round's rows
        s_one = s_ones[:1]                                              # an install's one-row alive flag, and where its
        s_end = torch.empty(1, dtype=torch.long, device=dev)            # kernel puts the flag after the token (the host decides)
        want_sampler = do_sample or repetition_penalty != 1.0
        sampler = state = graph = None
        in_place = [s_tok, s_alive, s_idx, s_step, s_out]               # what a step writes: restored around the capture
        cache = None
        if mha:
            # (no KV buffer is cloned around the capture, as in _generate_graph_tail: the warm-up writes rows at or beyond
            #  each slot's length, and a replayed step rewrites a row before its validity column is set)
            cap = mha_slot_capacity([len(p) for p in ids], budgets)
            cache = state = ops.KVCache.empty(cfg.num_hidden_layers, S, cap, cfg.hidden_size, self._mha_slot_dtype(), dev)
            cache.slots_begin(cfg.num_attention_heads, L_end=cap)
            in_place.extend([cache.dev_lens, cache.dev_len, cache.dev_valid, cache.dev_err])

        def install(i, b):
            """Prompt i's batch-1 prefill; its first token and caches as a round of one (settle)."""
            out = self(input_ids=ids[i][None], use_cache=True)
            settle([(i, b)], out[1][:, -1, :], [out[4]])

        def settle(taken, logits, pasts):
            """The end of a refill round: `taken`, its (prompt, free slot) pairs in arrival order; `logits` [n, V], their
            last-position rows; `pasts[j]`, the j-th prompt's batch-1 caches (prefill_packed's views are such).  Every
            first token is selected on the device as a prompt prefilled alone selects it, ONE host read brings them back
            (with the sampler's error word), and a prompt's caches go into its row if the slot then is live."""
            nonlocal sampler, state
            ordinal = stats["prefills"] + 1                # (of the round's first prompt: prompts prefilled so far, plus one)
            stats["prefills"] += len(taken)
            if state is None:
                state, bufs = self._slot_state(pasts[0], S)
                in_place.extend(bufs)
            if want_sampler and sampler is None:
                if not (ops.SAMPLE_FUSED and ops.sample_supported(logits)):
                    raise ops.ApertisHipError("generate_many(): sampling and the repetition penalty run on the fused sampler "
                                              f"(ops.SAMPLE_FUSED, logits {tuple(logits.shape)} {logits.dtype}); there is no "
                                              "stock path over slots")
                # (ids >= V are skipped by the occurrence table: it starts at zero, a row is rebuilt when a prompt moves in)
                none = torch.full((S, 1), logits.shape[-1], dtype=torch.long, device=dev)
                sampler = ops.Sampler(logits[:1].expand(S, -1), none, do_sample=do_sample, temperature=temperature, top_k=top_k,
                                      top_p=top_p, repetition_penalty=repetition_penalty, eos=eos, pad=pad)
                if sampler.uniforms is not None:
                    raise ops.ApertisHipError("generate_many(): ops.sample.SAMPLE_UNIFORMS is generate()'s test hook")
                in_place.extend(t for t in (sampler.counts, sampler.err) if t is not None)
            if sampler is None:
                # (an argmax per row: the rows of a round select what each selects as the one row of its own call)
                nxt, _ = _select_tokens(logits.float(), s_ones[:len(taken)], eos, pad)
                firsts = nxt.tolist()
            else:
                for j, (i, b) in enumerate(taken):
                    counts = None
                    if sampler.counts is not None:
                        sampler.counts[b].copy_(ops.token_counts(ids[i][None], logits.shape[-1], sampler.err)[0])
                        counts = sampler.counts[b:b + 1]
                    # (the kernel sees row 0 here: the draw counters of the installs - the prompt's prefill ordinal, whatever
                    #  the round it came in - lie above every step of the call)
                    ops.sample_next(logits[j:j + 1], s_one, sampler.err, do_sample=sampler.do_sample, temperature=sampler.temp,
                                    top_k=sampler.top_k, top_p=sampler.top_p, repetition_penalty=sampler.penalty,
                                    counts=counts, eos=sampler.eos, pad=sampler.pad, seed=sampler.seed,
                                    step=sampler.zero_step, step_off=(1 << 40) + ordinal + j,
                                    alive_out=s_end, out=s_nxt[b:b + 1])
                nxt = s_nxt[b:b + 1] if len(taken) == 1 else torch.cat([s_nxt[b:b + 1] for _, b in taken])
                *firsts, code = torch.cat((nxt, sampler.err.to(nxt.dtype))).tolist()
                sampler.check(code)
            for j, ((i, b), first, past) in enumerate(zip(taken, firsts, pasts)):
                if sched.place(b, first, eos_set):
                    moved.append(b)
                    s_tok[b].copy_(nxt[j:j + 1])
                    if cache is not None:
                        cache.slot_install(b, past)
                    elif isinstance(state, _StackedPast):
                        state.conv_all[:, b].copy_(torch.stack([c[0] for c, _ in past]))
                        state.state_all[:, b].copy_(torch.stack([st[0].reshape(-1) for _, st in past]))
                    else:
                        for (sc, ss), (c, st) in zip(state, past):
                            sc[b].copy_(c[0])
                            ss[b].copy_(st[0])

        def body():
            if cache is not None:
                cache.slots_step_begin()
            out = self(input_ids=s_tok, past_key_values=state, use_cache=True)
            if sampler is None:
                nxt, al = _select_tokens(out[1][:, -1, :].float(), s_alive, eos, pad)
                s_alive.copy_(al)
            else:
                sampler.step(out[1][:, -1, :], s_alive, 0, step=s_step, alive_out=s_alive, out=s_nxt)
                nxt = s_nxt
            s_out.scatter_(1, s_idx.expand(S, 1), nxt.unsqueeze(1))
            s_idx.add_(1)
            s_step.add_(1)
            s_tok.copy_(nxt.unsqueeze(1))
            if cache is not None:
                if out[4] is not cache:
                    raise ops.ApertisHipError("generate_many(): a token step left the slot cache (the decode kernels did not "
                                              "take it)")
                cache.slots_step_end(s_alive)
                return
            for (sc, ss), (nc, ns) in zip(state, out[4]):
                if nc.data_ptr() != sc.data_ptr():         # (both updated in place by the step: the views say `inplace`)
                    sc.copy_(nc)
                if ns.data_ptr() != ss.data_ptr():
                    ss.copy_(ns)

        slotted = [m for p, m in zip(ids, budgets) if len(p) >= window]
        want_graph = DECODE_GRAPH and bool(slotted) and max(slotted) - 1 >= DECODE_GRAPH_MIN_STEPS
        moved = [None]                 # slots filled or freed since s_alive was last written (None: not written yet)
        while not sched.finished():
            # prefill_tokens: refill rounds - the waiting prompts one per free slot up to the token cap (prefill_round), two
            # or more of them as one packed forward; a prompt that ends at its first token frees its slot for the next round
            while prefill_tokens is not None and sched.head() is not None and sched.free():
                free = sched.free()
                wait = sched.waiting(len(free))
                taken = [(wait[j], free[j]) for j in prefill_round([len(ids[i]) for i in wait], len(free), prefill_tokens)]
                if len(taken) == 1:                        # (the alone call: the knob never makes a lone prefill slower)
                    install(*taken[0])
                else:
                    settle(taken, *self.prefill_packed([ids[i] for i, _ in taken]))
                stats["prefill_forwards"] += 1
            # every free slot takes the next prompts in arrival order until one stays (or none waits)
            for b in sched.free():
                while sched.head() is not None and sched.slot[b] is None:
                    i = sched.head()
                    if len(ids[i]) < window:
                        # (its prefill hands back a shorter window, which no token step takes in place: generate()'s own loop)
                        alone = self.generate(input_ids=ids[i][None], max_new_tokens=budgets[i], do_sample=do_sample,
                                              temperature=temperature, top_k=top_k, top_p=top_p,
                                              repetition_penalty=repetition_penalty, eos_token_id=eos_token_id,
                                              pad_token_id=pad_token_id)
                        sched.complete(alone[0, len(ids[i]):].tolist(), eos_set)
                        stats["fallbacks"].append(i)
                    else:
                        install(i, b)
            live = sched.live()
            if not live:
                continue
            if moved:
                # (a row that ran out of budget is still alive on the device, one refilled after its eos is not)
                s_alive.copy_(torch.tensor([int(b in live) for b in range(S)], dtype=torch.long))
                if cache is not None:
                    for b in moved:
                        if b is not None and b not in live:
                            cache.slot_free(b)
                del moved[:]
            # (the slot step of a standard_mha model is device-state by construction: generate()'s ops.ATTN_DECODE_GRAPH and
            #  _mha_graph_ok are not consulted)
            if want_graph and graph is None and self._decode_graph_ok(s_tok, do_sample, repetition_penalty, sampler, slots=mha):
                keep = [t.clone() for t in in_place]
                graph = self._capture_step(body, lambda: [t.copy_(k) for t, k in zip(in_place, keep)], dev)
                stats["graphs"] += 1
            n = sched.burst(burst if graph is not None else 1)
            s_idx.zero_()
            for _ in range(n):
                if graph is not None:
                    graph.replay()
                else:
                    body()
            stats["steps"] += n
            stats["replays"] += n if graph is not None else 0
            stats["slot_steps"] += n * S
            # the one host read of the burst: its tokens, with the sampler's and the slot cache's error words
            errs = [t for t in (sampler.err if sampler is not None else None, cache.dev_err if cache is not None else None)
                    if t is not None]
            if not errs:
                got = s_out[:, :n].tolist()
            else:
                flat = torch.cat([s_out[:, :n].reshape(-1)] + [e.to(s_out.dtype) for e in errs]).tolist()
                if cache is not None and flat.pop():
                    raise ops.ApertisHipError("generate_many(): a KV-cache slot step ran past its slot or the rotary table; "
                                              "nothing was written by that step")
                if sampler is not None:
                    sampler.check(flat.pop())
                got = [flat[b * n:(b + 1) * n] for b in range(S)]
            moved.extend(sched.feed(got, eos_set))
        stats["live_slot_steps"] = sched.fed
        new = torch.tensor([t for row in sched.tokens for t in row], dtype=torch.long, device=dev)
        new = torch.split(new, [len(row) for row in sched.tokens])
        return [torch.cat((p, t)) for p, t in zip(ids, new)], stats


# ----------------------------------------------------------------------------------------------
# Model sizing  (reference core.py:1709-2105)
# ----------------------------------------------------------------------------------------------
def parse_param_count(param_str: Union[str, int]) -> int:
    """'10M' / '1.5B' / '350k' / int -> integer parameter count (core.py:1709-1739)."""
    if isinstance(param_str, int):
        return param_str
    s = str(param_str).strip().upper()
    if not s:
        raise ValueError("Parameter string cannot be empty.")
    mult = {"K": 1_000, "M": 1_000_000, "B": 1_000_000_000}.get(s[-1], 1)
    if mult != 1:
        s = s[:-1]
    try:
        return int(float(s) * mult)
    except ValueError:
        raise ValueError(f"Invalid numeric value in parameter string: '{param_str}'")


def _calculate_params_for_dims(vocab_size, hidden_size, num_layers, intermediate_size, tie_word_embeddings=True,
                               use_expert_system=False, num_experts=0) -> int:
    """The reference's MHA-shaped estimator (4h^2 attention), used for sizing even for SSM models
    (core.py:1741-1769)."""
    h, I = hidden_size, intermediate_size
    p = vocab_size * h * (1 if tie_word_embeddings else 2)
    p += num_layers * 4 * h * h
    if use_expert_system and num_experts > 0:
        p += num_layers * (num_experts * 2 * h * I + h * num_experts)
    else:
        p += num_layers * 2 * h * I
    return p + (2 * num_layers + 1) * 2 * h


def calculate_model_dimensions(target_params_str, vocab_size, use_expert_system=False, num_experts_target=8,
                               min_hidden_size=256, max_hidden_size=8192, min_layers=2, max_layers=128,
                               head_dim_preference=64, intermediate_multiple_of=256, intermediate_ratio=4.0,
                               tie_word_embeddings=True) -> Dict[str, Any]:
    """Grid search (layers in steps of 2, hidden a multiple of the head dim with a growing step,
    I = 4h rounded up to 256) for the closest estimated parameter count; reproduces the
    reference's choices exactly (core.py:1771-1893; golden table in tests/golden)."""
    target = parse_param_count(target_params_str)
    hd = head_dim_preference
    best, best_diff = None, float("inf")

    def dims_for(h):
        heads = max(1, h // hd)
        I = max(intermediate_multiple_of, -(-int(h * intermediate_ratio) // intermediate_multiple_of) * intermediate_multiple_of)
        return heads, I

    for layers in range(min_layers, max_layers + 1, 2):
        cur = min_hidden_size
        while cur <= max_hidden_size:
            h = cur if cur % hd == 0 else (cur // hd + 1) * hd
            h = h or hd
            if h > max_hidden_size:
                break
            heads, I = dims_for(h)
            params = _calculate_params_for_dims(vocab_size, h, layers, I, tie_word_embeddings, use_expert_system,
                                                num_experts_target if use_expert_system else 0)
            diff = abs(params - target)
            if diff < best_diff:
                best_diff = diff
                best = {"hidden_size": h, "num_hidden_layers": layers, "num_attention_heads": heads,
                        "intermediate_size": I, "calculated_params": params, "target_params": target,
                        "param_diff": diff}
            if params > target and diff > best_diff:
                break
            cur += max(hd, h // 16)
            if cur > max_hidden_size and best is None:
                cur = max_hidden_size
    if best is None:
        h = min_hidden_size
        heads, I = dims_for(h)
        params = _calculate_params_for_dims(vocab_size, h, min_layers, I, tie_word_embeddings, use_expert_system,
                                            num_experts_target if use_expert_system else 0)
        return {"hidden_size": h, "num_hidden_layers": min_layers, "num_attention_heads": heads,
                "intermediate_size": I, "calculated_params": params, "target_params": target,
                "param_diff": abs(params - target), "備考": "Fallback configuration"}
    return best


def estimate_model_parameters(config: ApertisConfig) -> int:
    """Parameter estimate from a config (core.py:1895-1965): embeddings (+ untied head), 4h^2
    attention, dense or E-expert FFN (+ router), 2L+1 norms, absolute positions, vision projection."""
    h, I, L = config.hidden_size, config.intermediate_size, config.num_hidden_layers
    total = config.vocab_size * h * (1 if config.tie_word_embeddings else 2)
    ffn = 2 * h * I
    if config.use_expert_system and config.num_experts > 0:
        ffn = config.num_experts * 2 * h * I + h * config.num_experts
    total += L * (4 * h * h + ffn) + (2 * L + 1) * 2 * h
    if config.position_embedding_type == "absolute":
        total += config.max_position_embeddings * h
    if config.multimodal and config.vision_embed_dim != h:
        total += config.vision_embed_dim * h
    return total


def create_apertis_model(target_param_count: Union[str, int] = "125M", vocab_size_override: Optional[int] = None,
                         multimodal: bool = False, use_flash_attention: bool = False, use_expert_system: bool = False,
                         num_experts_target_override: Optional[int] = None,
                         experts_per_token_target_override: Optional[int] = None,
                         attention_type_override: Optional[str] = None, ssm_d_inner: Optional[int] = None,
                         ssm_d_state: int = 16, ssm_dt_rank: Union[int, str] = "auto", ssm_conv_kernel: int = 4,
                         config_overrides: Optional[Dict[str, Any]] = None) -> ApertisForCausalLM:
    """Size a model for a parameter budget and build it (reference core.py:1969-2105)."""
    vocab = vocab_size_override if vocab_size_override is not None else ApertisConfig(**(config_overrides or {})).vocab_size
    dims = calculate_model_dimensions(target_param_count, vocab, use_expert_system=use_expert_system,
                                      num_experts_target=8 if num_experts_target_override is None else num_experts_target_override)
    cfg = {k: dims[k] for k in ("hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size")}
    cfg["vocab_size"] = vocab
    cfg["attention_type"] = attention_type_override or "standard_mha"
    cfg.update(multimodal=multimodal, use_flash_attention=use_flash_attention, use_expert_system=use_expert_system,
               ssm_d_inner=ssm_d_inner, ssm_d_state=ssm_d_state, ssm_dt_rank=ssm_dt_rank, ssm_conv_kernel=ssm_conv_kernel)
    if use_expert_system:
        cfg["num_experts"] = 8 if num_experts_target_override is None else num_experts_target_override
        cfg["experts_per_token"] = 2 if experts_per_token_target_override is None else experts_per_token_target_override
    if config_overrides:
        cfg.update(config_overrides)
    h, heads = cfg["hidden_size"], cfg["num_attention_heads"]
    if h % heads != 0:
        head_dim = h // heads if heads > 0 else 64
        if head_dim > 0 and h % head_dim == 0:
            cfg["num_attention_heads"] = h // head_dim
        else:
            cfg["num_attention_heads"] = next((i for i in range(min(heads, h), 0, -1) if h % i == 0), 1)
    config = ApertisConfig(**cfg)
    logger.info("Model configured with H=%d L=%d A=%d I=%d V=%d (~%.2fM params by the reference estimator)",
                config.hidden_size, config.num_hidden_layers, config.num_attention_heads, config.intermediate_size,
                config.vocab_size, estimate_model_parameters(config) / 1e6)
    return ApertisForCausalLM(config)
