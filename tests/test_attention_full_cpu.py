"""Bidirectional attention and the fused vision tower without a GPU: the library exports the two entry points under ABI 4.12,
the header declares them and the binding takes as many arguments, both refuse bad arguments before any launch with the codes
of the causal pair, the switch is off by default and forwarded, the tower's predicate says no off the GPU and for the head
dims of the committed vision fixtures, and the tower's state dict is that of stock nn.TransformerEncoderLayers."""
import ctypes
import json
import os
import re

import torch
import torch.nn as nn

from conftest import load_golden

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -2
F32, BF16 = 0, 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("apertis_attention_full_fwd", "apertis_attention_full_bwd")


def _lib():
    from apertis_llm_amd import _lib
    return _lib.load()


def _header():
    with open(os.path.join(ROOT, "include", "apertis_hip.h")) as f:
        return f.read()


def test_library_exports_header_declares_and_binding_matches():
    from apertis_llm_amd import _lib
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    hdr = _header()
    for name, causal in zip(NAMES, ("apertis_attention_fwd", "apertis_attention_bwd")):
        assert hasattr(cdll, name), name
        m = re.search(r"\bint " + name + r"\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/apertis_hip.h"
        params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(params), (name, params)
        # the argument list of the causal entry point, name by name and type by type
        mc = re.search(r"\bint " + causal + r"\(([^)]*)\)\s*;", hdr)
        assert params == [re.sub(r"\s+", " ", p.strip()) for p in mc.group(1).split(",")]
        assert list(argtypes) == list(_lib.SIGNATURES[causal][1])


def test_abi_version_is_still_4_12():
    from apertis_llm_amd import _lib
    assert _lib.ABI_VERSION == (4 << 16) | 12
    assert int(_lib.load().apertis_abi_version()) == (4 << 16) | 12
    assert re.search(r"#define APERTIS_ABI_VERSION \(\(4 << 16\) \| 12\)", _header())


# non-null, 16-byte aligned stand-ins: validation happens before any launch, nothing is dereferenced
P = 0x1000
FWD_PTRS = ("q", "k", "v", "out", "lse")
BWD_PTRS = ("q", "k", "v", "out", "dout", "lse", "ws", "dq", "dk", "dv")


def _fwd(name, **kw):
    a = {**dict(q=P, k=P, v=P, kv=None, out=P, lse=P, q_rs=192, k_rs=192, v_rs=192, o_rs=192, B=2, L=5, H=3, D=64, p=0.0,
                seed=0, dt=BF16), **kw}
    return getattr(_lib(), name)(a["q"], a["q_rs"], a["k"], a["k_rs"], a["v"], a["v_rs"], a["kv"], a["out"], a["o_rs"], a["lse"],
                                 a["B"], a["L"], a["H"], a["D"], a["p"], a["seed"], a["dt"], None)


def _bwd(name, **kw):
    a = {**dict(q=P, k=P, v=P, out=P, dout=P, lse=P, kv=None, ws=P, dq=P, dk=P, dv=P, q_rs=192, k_rs=192, v_rs=192, o_rs=192,
                do_rs=192, d_rs=192, B=2, L=5, H=3, D=64, p=0.0, seed=0, dt=BF16), **kw}
    return getattr(_lib(), name)(a["q"], a["q_rs"], a["k"], a["k_rs"], a["v"], a["v_rs"], a["out"], a["o_rs"], a["dout"], a["do_rs"],
                                 a["lse"], a["kv"], a["ws"], a["dq"], a["dk"], a["dv"], a["d_rs"], a["B"], a["L"], a["H"], a["D"],
                                 a["p"], a["seed"], a["dt"], None)


def _refusals(call, ptrs, strides):
    """(what, code) of every bad argument the issue lists, for one entry point."""
    got = [(f"null {n}", call(**{n: None})) for n in ptrs]
    got += [(f"p {p}", call(p=p)) for p in (-0.1, 1.0, 1.5, float("nan"))]
    got += [("D 48", call(D=48, q_rs=144, k_rs=144, v_rs=144, o_rs=144, **({"do_rs": 144, "d_rs": 144} if "d_rs" in strides else {})))]
    got += [("B*H 65536", call(B=16384, H=4, D=64, **{s: 256 for s in strides}))]
    got += [(f"misaligned {s}", call(**{s: 196})) for s in strides]            # bf16: 392-byte rows
    got += [(f"misaligned {n}", call(**{n: P + 8})) for n in ptrs]
    return dict(got)


def test_full_entry_points_refuse_what_the_causal_ones_refuse_with_the_same_codes():
    fs, bs = ("q_rs", "k_rs", "v_rs", "o_rs"), ("q_rs", "k_rs", "v_rs", "o_rs", "do_rs", "d_rs")
    for full, causal, call, ptrs, strides in ((NAMES[0], "apertis_attention_fwd", _fwd, FWD_PTRS, fs),
                                              (NAMES[1], "apertis_attention_bwd", _bwd, BWD_PTRS, bs)):
        got = _refusals(lambda **kw: call(full, **kw), ptrs, strides)
        want = _refusals(lambda **kw: call(causal, **kw), ptrs, strides)
        assert got == want, (full, got, want)
        assert all(rc in (ERR_ARG, ERR_UNSUPPORTED) for rc in got.values()), got
        assert all(got[f"null {n}"] == ERR_ARG for n in ptrs)
        assert all(got[k] == ERR_ARG for k in got if k.startswith("p "))
        assert got["D 48"] == ERR_UNSUPPORTED and got["B*H 65536"] == ERR_UNSUPPORTED
        assert all(got[f"misaligned {s}"] == ERR_UNSUPPORTED for s in strides)
        # the largest grid that is accepted, with nothing to do: not an error, but the arguments are still looked at
        assert call(full, B=0) == OK and call(full, L=0) == OK and call(full, L=0, B=21845, H=3) == OK
        assert call(full, L=0, q=None) == ERR_ARG and call(full, L=0, D=48) == ERR_UNSUPPORTED


def _encoder(Dv, heads, layers=2, image=32, patch=8):
    import apertis_llm_amd as A
    cfg = A.ApertisConfig(hidden_size=48, num_attention_heads=3, multimodal=True, image_size=image, vision_embed_dim=Dv,
                          vision_patch_size=patch, vision_layers=layers, vision_heads=heads)
    return A.UnifiedMultimodalEncoder(cfg)


def test_switch_is_off_by_default_and_forwarded(monkeypatch):
    from apertis_llm_amd import ops
    # read once, at import: off unless APERTIS_VIT_FUSED=1 (the suite runs with it unset)
    assert ops.VIT_FUSED is (os.environ.get("APERTIS_VIT_FUSED", "0") == "1")
    if "APERTIS_VIT_FUSED" not in os.environ:
        assert ops.VIT_FUSED is False
    assert "VIT_FUSED" in ops._FORWARDED and ops._FORWARDED["VIT_FUSED"] is ops.attention
    monkeypatch.setattr(ops, "VIT_FUSED", True)
    assert ops.attention.VIT_FUSED is True                     # the package forwards the write to the owner
    for name in ("full_attention", "full_attention_qkv", "full_attention_supported"):
        assert callable(getattr(ops, name)), name


def test_tower_predicate(monkeypatch):
    from apertis_llm_amd import ops
    good = _encoder(128, 2)
    x = torch.zeros(2, 17, 128)
    assert good._fused_geometry() and not good.fused_supported(x)          # the switch is off
    monkeypatch.setattr(ops, "VIT_FUSED", True)
    assert not good.fused_supported(x)                                      # a CPU tensor
    # the committed vision fixtures: head dims 16 (vision) and 12 (model_ssm_moe_mm)
    g = load_golden("vision")
    assert g["sd"]["vision_layers.0.self_attn.in_proj_weight"].shape[1] // 2 == 16
    cfg = json.loads(str(load_golden("model_ssm_moe_mm")["config_json"]))
    assert cfg["vision_embed_dim"] // cfg["vision_heads"] == 12
    for Dv, heads in ((32, 2), (cfg["vision_embed_dim"], cfg["vision_heads"])):
        enc = _encoder(Dv, heads)
        assert not enc._fused_geometry() and not enc.fused_supported(torch.zeros(2, 17, Dv))
    assert _encoder(256, 2)._fused_geometry() and _encoder(256, 4)._fused_geometry()
    assert not _encoder(256, 8)._fused_geometry() and not _encoder(512, 2)._fused_geometry()      # head dims 32, 256
    # layers other than the ones the constructor builds
    for change in (dict(norm_first=False), dict(activation="relu"), dict(batch_first=False)):
        enc = _encoder(128, 2)
        kw = {**dict(d_model=128, nhead=2, dim_feedforward=512, dropout=0.1, activation="gelu", batch_first=True, norm_first=True),
              **change}
        enc.vision_layers[1] = nn.TransformerEncoderLayer(**kw)
        assert not enc._fused_geometry(), change
    # the op-level predicate: the grid bound on top of attention_supported's conditions
    assert ops.full_attention_supported(torch.empty(2, 5, 192), 3) and not ops.full_attention_supported(torch.empty(2, 5, 192), 4)
    assert ops.full_attention_supported(torch.empty(2, 5, 576), 3, packed=True)
    assert not ops.full_attention_supported(torch.empty(2, 5, 576), 3)
    assert not ops.full_attention_supported(torch.empty(2, 5, 192, dtype=torch.float16), 3)
    assert ops.full_attention_supported(torch.empty(65535, 0, 64), 1) and not ops.full_attention_supported(torch.empty(65536, 0, 64), 1)
    for fn in (lambda: ops.full_attention(x, x, x, 2), lambda: ops.full_attention_qkv(torch.zeros(2, 17, 384), 2)):
        try:
            fn()
        except ops.ApertisHipError as e:
            assert "ROCm device only" in str(e)
        else:
            raise AssertionError("a CPU tensor was accepted")


def test_state_dict_is_the_stock_layers():
    enc = _encoder(128, 2, layers=3)
    stock = nn.ModuleList([nn.TransformerEncoderLayer(d_model=128, nhead=2, dim_feedforward=512, dropout=0.1, activation="gelu",
                                                      batch_first=True, norm_first=True) for _ in range(3)])
    want = {f"vision_layers.{k}": tuple(v.shape) for k, v in stock.state_dict().items()}
    want.update({"patch_embed.weight": (128, 3, 8, 8), "patch_embed.bias": (128,), "vision_pos_embed": (1, 17, 128),
                 "cls_token": (1, 1, 128), "vision_ln.weight": (128,), "vision_ln.bias": (128,)})
    got = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    assert got == want
    assert all(type(layer) is nn.TransformerEncoderLayer for layer in enc.vision_layers)
