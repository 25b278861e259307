"""UnifiedMultimodalEncoder mirror (reference src/multimodal/module.py:10-161).

Patch embedding runs as a GEMM on the MFMA tile: stride == kernel, so Conv2d(3, Dv, p, p) is
`patches[B*gh*gw, 3*p*p] @ weight.view(Dv, -1).T + bias` with K index c*p*p + ky*p + kx
(module.py:35-40,102-103).

The ViT body (~98.7 % of the encoder FLOPs) has two paths over the SAME parameters - `vision_layers` is a ModuleList of
stock nn.TransformerEncoderLayer either way, so state-dict keys, shapes, init and checkpoints do not depend on the path:
  * stock (the default): the layers' own forward, op by op, with torch's inference fast path switched off around it;
  * fused (`ops.VIT_FUSED`, APERTIS_VIT_FUSED=1, and `fused_supported`): per layer the LayerNorm / residual boundaries of
    the text model (ops.layer_norm, ops.dropout_add_layer_norm), the MFMA GEMMs with their bias (ops.linear_mfma), the
    bidirectional flash attention on the packed in-projection (ops.full_attention_qkv) and Linear -> GELU -> dropout ->
    Linear on the expert-MLP pair (ops.expert_mlp as one group).  Its train-mode dropout masks come from the library's
    counter hash, not from torch's Philox stream.  A tower that does not qualify runs the stock path.
"""
import threading
from typing import List

import torch
import torch.nn as nn

from . import ops
from .ops._base import _compute_dtype


_fp_lock = threading.Lock()
_fp_depth = 0
_fp_saved = True


def _fastpath_enter():
    global _fp_depth, _fp_saved
    with _fp_lock:
        if _fp_depth == 0:
            _fp_saved = torch.backends.mha.get_fastpath_enabled()
            torch.backends.mha.set_fastpath_enabled(False)
        _fp_depth += 1


def _fastpath_exit():
    global _fp_depth
    with _fp_lock:
        _fp_depth -= 1
        if _fp_depth == 0:
            torch.backends.mha.set_fastpath_enabled(_fp_saved)


class UnifiedMultimodalEncoder(nn.Module):
    """Vision tower: patch embed -> [cls] + learned positions -> pre-norm transformer -> LayerNorm."""

    _MEAN = (0.485, 0.456, 0.406)
    _STD = (0.229, 0.224, 0.225)

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.image_size = config.image_size
        self.vision_embed_dim = config.vision_embed_dim
        self.vision_patch_size = config.vision_patch_size
        # nn.Conv2d only holds the parameters (checkpoint names/shapes); forward() is a GEMM
        self.patch_embed = nn.Conv2d(3, self.vision_embed_dim, kernel_size=self.vision_patch_size,
                                     stride=self.vision_patch_size)
        self.num_patches = (self.image_size // self.vision_patch_size) ** 2
        self.vision_pos_embed = nn.Parameter(torch.zeros(1, self.num_patches + 1, self.vision_embed_dim))
        self.cls_token = nn.Parameter(torch.zeros(1, 1, self.vision_embed_dim))
        heads = getattr(config, "vision_heads", 12)
        layers = getattr(config, "vision_layers", 12)
        self.vision_layers = nn.ModuleList([
            nn.TransformerEncoderLayer(d_model=self.vision_embed_dim, nhead=heads,
                                       dim_feedforward=self.vision_embed_dim * 4, dropout=0.1, activation="gelu",
                                       batch_first=True, norm_first=True)
            for _ in range(layers)])
        self.vision_ln = nn.LayerNorm(self.vision_embed_dim)
        nn.init.normal_(self.vision_pos_embed, std=0.02)
        nn.init.normal_(self.cls_token, std=0.02)
        nn.init.normal_(self.patch_embed.weight, std=0.02)
        nn.init.zeros_(self.patch_embed.bias)

    def patchify(self, pixel_values: torch.Tensor) -> torch.Tensor:
        """[B,3,Hi,Wi] -> [B, gh*gw, 3*p*p]; row = py*gw + px, column = c*p*p + ky*p + kx."""
        B, C, Hi, Wi = pixel_values.shape
        p = self.vision_patch_size
        gh, gw = Hi // p, Wi // p
        x = pixel_values[:, :, :gh * p, :gw * p].reshape(B, C, gh, p, gw, p).permute(0, 2, 4, 1, 3, 5)
        return x.reshape(B, gh * gw, C * p * p)

    def embed_patches(self, pixel_values: torch.Tensor) -> torch.Tensor:
        """Patch-embed stage of forward() (module.py:102-103) -> [B, num_patches, Dv]."""
        with ops.device_guard(pixel_values):
            return self._embed_patches(pixel_values)

    def _embed_patches(self, pixel_values: torch.Tensor) -> torch.Tensor:
        cols = self.patchify(pixel_values)
        cd = cols.dtype
        if torch.is_autocast_enabled():
            cd = torch.bfloat16
        w = self.patch_embed.weight.reshape(self.vision_embed_dim, -1)
        return ops.linear_mfma(cols, w, self.patch_embed.bias, compute_dtype=cd)

    def forward(self, pixel_values: torch.Tensor) -> torch.Tensor:
        B = pixel_values.shape[0]
        patches = self.embed_patches(pixel_values).to(self.vision_pos_embed.dtype)
        x = torch.cat([self.cls_token.expand(B, -1, -1), patches], dim=1) + self.vision_pos_embed   # module.py:106-110
        if self.fused_supported(x):                       # ops.VIT_FUSED: layers and vision_ln on the project's kernels
            with ops.device_guard(x):
                return self._fused_body(x)
        # torch's fused inference "fast path" for TransformerEncoderLayer loses ~1e-4 on ROCm (measured: 1.4e-4 vs 3e-7
        # abs error against fp64 for one layer); parity with the reference's fp32 CPU path needs the op-by-op path.
        # The switch is process-global and the reference runs training in daemon threads (interface.py:1188): it is
        # flipped under a lock that counts the forwards inside, restored when the last one leaves.
        _fastpath_enter()
        try:
            for layer in self.vision_layers:                                                          # module.py:113-114
                x = layer(x)
        finally:
            _fastpath_exit()
        return self.vision_ln(x)                                                                      # module.py:117

    # -- the body on the project's kernels (ops.VIT_FUSED) ------------------------------------------
    def _fused_geometry(self) -> bool:
        """Whether the tower is one the fused body can run, whatever the input: head dim 64 or 128, 16-byte rows, and
        layers as the constructor builds them (pre-norm, GELU, batch-first, one packed in-projection, every bias)."""
        Dv = self.vision_embed_dim
        if len(self.vision_layers) == 0 or Dv % 8 or Dv > 4096:
            return False
        for layer in self.vision_layers:
            if not isinstance(layer, nn.TransformerEncoderLayer):
                return False
            at = layer.self_attn
            heads = at.num_heads
            if (not layer.norm_first or getattr(layer, "activation_relu_or_gelu", 0) != 2 or not at.batch_first
                    or not at._qkv_same_embed_dim or at.in_proj_bias is None or at.out_proj.bias is None
                    or at.bias_k is not None or at.add_zero_attn or at.embed_dim != Dv
                    or Dv % heads or Dv // heads not in (64, 128)
                    or layer.linear1.bias is None or layer.linear2.bias is None
                    or layer.linear1.in_features != Dv or layer.linear2.out_features != Dv
                    or layer.linear1.out_features % 8
                    or any(n.weight is None or n.bias is None or tuple(n.normalized_shape) != (Dv,)
                           for n in (layer.norm1, layer.norm2))):
                return False
        return self.vision_ln.weight is not None and self.vision_ln.bias is not None

    def fused_supported(self, x: torch.Tensor) -> bool:
        """Whether forward() runs the fused body for the residual stream x [B, L, Dv]: the switch is on, x is on the GPU in
        the parameters' dtype (fp32, or bf16 when that is the compute dtype too), the geometry qualifies and the grid of
        the attention kernels can hold B * heads."""
        if not ops.VIT_FUSED or not x.is_cuda or x.dim() != 3 or x.shape[0] < 1 or not self._fused_geometry():
            return False
        if x.dtype not in (torch.float32, torch.bfloat16) or (x.dtype != torch.float32 and _compute_dtype(x) != x.dtype):
            return False
        return x.shape[0] * max(layer.self_attn.num_heads for layer in self.vision_layers) <= 65535

    def _fused_body(self, x: torch.Tensor) -> torch.Tensor:
        """The layers and the final LayerNorm (module.py:113-117).  The residual stream x stays in the parameters' dtype;
        block outputs are in the compute dtype (bf16 under autocast).  Every `x + dropout(block)` and the LayerNorm behind
        it are one kernel each way; the last boundary's normalised output IS vision_ln(x)."""
        B, L, Dv = x.shape
        rows = B * L
        cd = _compute_dtype(x)
        layers = list(self.vision_layers)
        n0 = layers[0].norm1
        h = ops.layer_norm(x, n0.weight, n0.bias, n0.eps, out_dtype=cd)
        for i, layer in enumerate(layers):
            at, train = layer.self_attn, layer.training
            qkv = ops.linear_mfma(h, at.in_proj_weight, at.in_proj_bias, compute_dtype=cd)
            ctx = ops.full_attention_qkv(qkv, at.num_heads, at.dropout, train)
            o = ops.linear_mfma(ctx, at.out_proj.weight, at.out_proj.bias, compute_dtype=cd)
            x, h2 = ops.dropout_add_layer_norm(o, x, layer.norm2.weight, layer.norm2.bias, layer.norm2.eps, layer.dropout1.p,
                                               train, out_dtype=cd)
            p_drop = layer.dropout.p if train else 0.0
            seed = int(torch.empty((), dtype=torch.int64).random_().item()) if p_drop > 0 else 0
            f = ops.expert_mlp(h2.reshape(rows, Dv), layer.linear1.weight.unsqueeze(0), layer.linear1.bias.unsqueeze(0),
                               layer.linear2.weight.unsqueeze(0), layer.linear2.bias.unsqueeze(0),
                               ops.dense_offsets(rows, x.device), rows, act="gelu", drop_p=p_drop, seed=seed,
                               compute_dtype=cd).reshape(B, L, Dv)
            last = i + 1 == len(layers)
            nxt = self.vision_ln if last else layers[i + 1].norm1
            x, h = ops.dropout_add_layer_norm(f, x, nxt.weight, nxt.bias, nxt.eps, layer.dropout2.p, train,
                                              out_dtype=x.dtype if last else cd)
        return h

    # -- PIL helpers (module.py:121-161) without the torchvision dependency ----------------------
    def process_image(self, image_path: str) -> torch.Tensor:
        try:
            import numpy as np
            from PIL import Image
            img = Image.open(image_path).convert("RGB").resize((self.image_size, self.image_size), Image.BILINEAR)
            t = torch.from_numpy(np.asarray(img, dtype=np.float32) / 255.0).permute(2, 0, 1)
            mean = torch.tensor(self._MEAN).view(3, 1, 1)
            std = torch.tensor(self._STD).view(3, 1, 1)
            return ((t - mean) / std).unsqueeze(0)
        except Exception as e:  # same contract as the reference: blank image on failure
            print(f"Error processing image {image_path}: {e}")
            return torch.zeros(1, 3, self.image_size, self.image_size)

    def process_batch(self, image_paths: List[str]) -> torch.Tensor:
        return torch.stack([self.process_image(p).squeeze(0) for p in image_paths])
