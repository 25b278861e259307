"""SwiGLU without a GPU: the library exports the two entry points under ABI 4.12, the header declares them and the binding
takes as many arguments, both refuse bad arguments before any launch, ops.swiglu_supported says no off the GPU and with the
switch off, and a use_swiglu model on the CPU is the stock formula bit for bit whatever the switch says."""
import ctypes
import os
import re

import pytest
import torch

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -2
F32, BF16 = 0, 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("apertis_swiglu_fwd", "apertis_swiglu_bwd")


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
    for name in NAMES:
        assert hasattr(cdll, name), name
        m = re.search(r"\bint " + name + r"\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/apertis_hip.h"
        params = [p.strip() for p in m.group(1).split(",")]
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(params), (name, params)
        assert params[-1] == "void *stream" and argtypes[-1] is ctypes.c_void_p
        # pointers are void pointers, sizes int64, the dtype a plain int - position by position
        for p, a in zip(params, argtypes):
            want = ctypes.c_void_p if "*" in p else ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_int
            assert a is want, (name, p, a)
    assert len(_lib.SIGNATURES["apertis_swiglu_fwd"][1]) == 6 and len(_lib.SIGNATURES["apertis_swiglu_bwd"][1]) == 8


def test_abi_version_is_still_4_12():
    from apertis_llm_amd import _lib
    assert _lib.ABI_VERSION == (4 << 16) | 12
    assert int(_lib.load().apertis_abi_version()) == (4 << 16) | 12
    assert re.search(r"#define APERTIS_ABI_VERSION \(\(4 << 16\) \| 12\)", _header())


# non-null, 16-byte aligned stand-ins: validation happens before any launch, nothing is dereferenced
P = 0x1000


def _fwd(**kw):
    a = {**dict(gu=P, h=P, rows=3, F=64, dt=BF16, st=None), **kw}
    return _lib().apertis_swiglu_fwd(a["gu"], a["h"], a["rows"], a["F"], a["dt"], a["st"])


def _bwd(**kw):
    a = {**dict(dh=P, gu=P, dgu=P, h=P, rows=3, F=64, dt=BF16, st=None), **kw}
    return _lib().apertis_swiglu_bwd(a["dh"], a["gu"], a["dgu"], a["h"], a["rows"], a["F"], a["dt"], a["st"])


def test_swiglu_fwd_validates_before_any_launch():
    for name in ("gu", "h"):
        assert _fwd(**{name: None}) == ERR_ARG, name
    assert _fwd(rows=-1) == ERR_ARG and _fwd(F=0) == ERR_ARG and _fwd(F=-8) == ERR_ARG
    assert _fwd(dt=2) == ERR_ARG and _fwd(dt=-1) == ERR_ARG
    for F in (4, 12, 63, 65, 260):                       # bf16 wants F % 8 == 0
        assert _fwd(F=F) == ERR_UNSUPPORTED, F
    for F in (2, 6, 63, 65):                             # fp32 wants F % 4 == 0
        assert _fwd(F=F, dt=F32) == ERR_UNSUPPORTED, F
    for name in ("gu", "h"):
        for off in (2, 4, 8):
            assert _fwd(**{name: P + off}) == ERR_UNSUPPORTED, (name, off)
            assert _fwd(**{name: P + off}, dt=F32) == ERR_UNSUPPORTED, (name, off)
    # nothing to do is not an error - but the arguments are still looked at
    assert _fwd(rows=0) == OK and _fwd(rows=0, F=4, dt=F32) == OK and _fwd(rows=0, F=8) == OK
    assert _fwd(rows=0, gu=None) == ERR_ARG and _fwd(rows=0, F=4) == ERR_UNSUPPORTED and _fwd(rows=0, h=P + 8) == ERR_UNSUPPORTED


def test_swiglu_bwd_validates_before_any_launch():
    for name in ("dh", "gu", "dgu"):
        assert _bwd(**{name: None}) == ERR_ARG, name
    assert _bwd(rows=-1) == ERR_ARG and _bwd(F=0) == ERR_ARG and _bwd(F=-4) == ERR_ARG
    assert _bwd(dt=2) == ERR_ARG and _bwd(dt=-1) == ERR_ARG
    for F in (4, 12, 63, 260):
        assert _bwd(F=F) == ERR_UNSUPPORTED, F
    for F in (2, 6, 63):
        assert _bwd(F=F, dt=F32) == ERR_UNSUPPORTED, F
    for name in ("dh", "gu", "dgu", "h"):
        assert _bwd(**{name: P + 8}) == ERR_UNSUPPORTED, name
    # h_out is optional
    assert _bwd(rows=0) == OK and _bwd(rows=0, h=None) == OK and _bwd(rows=0, F=4, dt=F32, h=None) == OK
    assert _bwd(rows=0, dgu=None) == ERR_ARG and _bwd(rows=0, F=12) == ERR_UNSUPPORTED


class _FakeGpuTensor:
    """What ops.swiglu_supported looks at, of a tensor that claims to live on the GPU."""
    is_cuda = True

    def __init__(self, shape, dtype=torch.float32):
        self.shape, self.dtype = tuple(shape), dtype

    def dim(self):
        return len(self.shape)

    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n


def test_swiglu_supported_predicate(monkeypatch):
    from apertis_llm_amd import ops
    assert ops.SWIGLU_FUSED is True                           # the shipped default (APERTIS_SWIGLU_FUSED unset)
    assert "SWIGLU_FUSED" in ops._FORWARDED and ops.swiglu in ops._MODULES
    assert not ops.swiglu_supported(torch.randn(2, 5, 32), 256)            # a CPU tensor
    gpu = _FakeGpuTensor((2, 5, 32))
    assert ops.swiglu_supported(gpu, 256)
    assert ops.swiglu_supported(_FakeGpuTensor((1, 32), torch.bfloat16), 8)
    assert not ops.swiglu_supported(_FakeGpuTensor((2, 5, 32), torch.float64), 256)
    assert not ops.swiglu_supported(_FakeGpuTensor((2, 5, 32), torch.float16), 256)
    assert not ops.swiglu_supported(_FakeGpuTensor((2, 5, 36)), 256)        # H % 8
    assert not ops.swiglu_supported(gpu, 260)                               # F % 8
    assert not ops.swiglu_supported(_FakeGpuTensor((0, 32)), 256)           # no row
    monkeypatch.setattr(ops, "SWIGLU_FUSED", False)
    assert ops.swiglu.SWIGLU_FUSED is False                                 # the package forwards the write to the owner
    assert not ops.swiglu_supported(gpu, 256)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_cpu_model_is_the_stock_formula_bit_for_bit(dt, monkeypatch):
    """use_swiglu (with the expert settings left in: SwiGLU wins over MoE) on the CPU, the switch on: every SwiGLUFFN output is
    w_down(silu(w_gate x) * w_up x) of its input, bit for bit, and ops.swiglu_mlp is never called."""
    import torch.nn.functional as F
    import apertis_llm_amd as A
    from apertis_llm_amd import model as M, ops
    assert ops.SWIGLU_FUSED
    torch.manual_seed(3)
    cfg = A.ApertisConfig(vocab_size=96, hidden_size=32, num_hidden_layers=2, num_attention_heads=2, intermediate_size=64,
                          attention_type="standard_mha", use_rmsnorm=True, use_swiglu=True, use_expert_system=True, num_experts=4,
                          experts_per_token=2)
    model = A.ApertisForCausalLM(cfg).to(dt).eval()
    ffns = [m for m in model.modules() if isinstance(m, M.SwiGLUFFN)]
    assert len(ffns) == 2 and all(f.ffn_dim == 256 for f in ffns)
    assert not any(type(m).__name__ == "AdaptiveExpertSystem" for m in model.modules())
    assert sorted(k.split("ffn.")[1] for k in model.state_dict() if ".ffn." in k and "layers.0." in k) == \
        ["w_down.weight", "w_gate.weight", "w_up.weight"]
    monkeypatch.setattr(ops, "swiglu_mlp", lambda *a, **k: pytest.fail("ops.swiglu_mlp on a CPU tensor"))
    seen = []
    hooks = [f.register_forward_hook(lambda mod, args, out: seen.append((mod, args[0], out))) for f in ffns]
    ids = torch.randint(4, 96, (2, 12), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        out = model(input_ids=ids, labels=ids, use_cache=False)
    for h in hooks:
        h.remove()
    assert len(seen) == 2 and torch.isfinite(out[0])
    for mod, x, y in seen:
        assert y.dtype == dt and torch.equal(y, mod.w_down(F.silu(mod.w_gate(x)) * mod.w_up(x)))
