"""Left-padded selective_ssm prefills (ops.ssm.SSM_LEFT_PAD), what needs no GPU:

  1. ops.left_pad_starts: which masks qualify and what it returns
  2. the switch: off by default, read from APERTIS_SSM_LEFT_PAD=1 at import, forwarded by the ops package, not re-exported
  3. apertis_dwconv_silu_start_fwd: exported under ABI 4.12, declared in the header, bound with as many arguments, and every
     bad argument class refused before any launch
  4. ops.dwconv_silu(start=...) refuses a CPU tensor and autograd
  5. off the GPU the switch changes nothing: ApertisModel._ssm_left_pad answers None, a CPU model's logits are the same bits
     with the switch on and off, and the start form is never reached (a selective_ssm block has no CPU path at all: it raises
     the same "no CPU fallback" error either way)
"""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -2
F32, BF16 = 0, 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "apertis_dwconv_silu_start_fwd"


@pytest.fixture
def switch():
    from apertis_llm_amd import ops
    prev = ops.SSM_LEFT_PAD
    yield ops
    ops.SSM_LEFT_PAD = prev


# ---------------------------------------------------------------------------------------------------------------------------
# 1. left_pad_starts
def test_left_pad_starts_on_every_mask_form():
    from apertis_llm_amd import ops
    ones = torch.ones(3, 7, dtype=torch.long)
    s = ops.left_pad_starts(ones)
    assert s.dtype == torch.int32 and s.tolist() == [0, 0, 0]
    assert ops.left_pad_starts(torch.ones(1, 1, dtype=torch.bool)).tolist() == [0]
    left = ones.clone()
    left[1, :5] = 0
    left[2, :6] = 0                                    # a single valid token, the last
    s = ops.left_pad_starts(left)
    assert s.dtype == torch.int32 and tuple(s.shape) == (3,) and s.tolist() == [0, 5, 6]
    for dt in (torch.bool, torch.int32, torch.float32):     # the mask's dtype does not matter, only zero / non-zero
        assert ops.left_pad_starts(left.to(dt)).tolist() == [0, 5, 6]
    right = ones.clone()
    right[1, 4:] = 0
    assert ops.left_pad_starts(right) is None
    both = left.clone()
    both[1, 6] = 0                                     # left AND right padded
    assert ops.left_pad_starts(both) is None
    hole = left.clone()
    hole[0, 3] = 0
    assert ops.left_pad_starts(hole) is None
    hole_in_pad = left.clone()
    hole_in_pad[1, 2] = 1                              # 0 0 1 0 0 1 1
    assert ops.left_pad_starts(hole_in_pad) is None
    empty_row = left.clone()
    empty_row[0] = 0
    assert ops.left_pad_starts(empty_row) is None
    assert ops.left_pad_starts(None) is None
    assert ops.left_pad_starts(torch.ones(7)) is None and ops.left_pad_starts(torch.ones(2, 1, 1, 7)) is None
    assert ops.left_pad_starts(torch.ones(2, 0)) is None


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the switch
def test_switch_is_off_by_default_forwarded_and_not_reexported(switch):
    ops = switch
    if os.environ.get("APERTIS_SSM_LEFT_PAD") is None:
        assert ops.SSM_LEFT_PAD is False and ops.ssm.SSM_LEFT_PAD is False
    assert "SSM_LEFT_PAD" not in vars(ops) and ops._FORWARDED["SSM_LEFT_PAD"] is ops.ssm
    ops.SSM_LEFT_PAD = True
    assert ops.ssm.SSM_LEFT_PAD is True and "SSM_LEFT_PAD" not in vars(ops)
    ops.SSM_LEFT_PAD = False
    assert ops.ssm.SSM_LEFT_PAD is False


def test_switch_is_read_from_the_environment_at_import():
    code = ("import os, sys, importlib; sys.path.insert(0, %r); from apertis_llm_amd.ops import ssm; out = []\n"
            "for v in (None, '1', '0', '', 'true'):\n"
            "    os.environ.pop('APERTIS_SSM_LEFT_PAD', None)\n"
            "    if v is not None: os.environ['APERTIS_SSM_LEFT_PAD'] = v\n"
            "    out.append(importlib.reload(ssm).SSM_LEFT_PAD)\n"
            "print(out)" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().splitlines()[-1] == "[False, True, False, False, False]"      # only "1" turns it on


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the entry point
def _header():
    with open(os.path.join(ROOT, "include", "apertis_hip.h")) as f:
        return f.read()


def test_library_exports_header_declares_and_binding_matches():
    from apertis_llm_amd import _lib
    assert _lib.ABI_VERSION == (4 << 16) | 12 and int(_lib.load().apertis_abi_version()) == _lib.ABI_VERSION
    assert re.search(r"#define APERTIS_ABI_VERSION \(\(4 << 16\) \| 12\)", _header())
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)                             # noqa: E731
    m = re.search(r"\bint " + NAME + r"\(([^)]*)\)\s*;", strip(_header()))
    assert m, f"{NAME} is not declared in include/apertis_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    plain = re.search(r"\bint apertis_dwconv_silu_fwd\(([^)]*)\)\s*;", strip(_header()))
    plain = [" ".join(p.split()) for p in plain.group(1).split(",")]
    # the plain forward's argument list with `start` after `bias`
    assert params == plain[:4] + ["const int32_t *start"] + plain[4:]
    restype, argtypes = _lib.SIGNATURES[NAME]
    assert restype is ctypes.c_int and len(argtypes) == len(params) == 13
    for p, a in zip(params, argtypes):
        want = ctypes.c_void_p if "*" in p else ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_int
        assert a is want, (p, a)


@pytest.fixture(scope="module")
def mem():
    """Host memory with a 64-byte aligned start: the entry point only looks at the addresses (every case below is refused
    before a launch, or has nothing to launch)."""
    buf = ctypes.create_string_buffer(4096 + 64)
    return buf, (ctypes.addressof(buf) + 63) // 64 * 64


def _call(p, **kw):
    from apertis_llm_amd import _lib
    a = dict(x=p, x_rs=64, w=p, bias=p, start=p, out=p, out_rs=64, B=2, L=5, Dn=64, k=4, dtype=F32, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return _lib.load().apertis_dwconv_silu_start_fwd(*a.values())


def test_entry_point_validates_before_any_launch(mem):
    _, p = mem
    for name in ("x", "w", "bias", "start", "out"):
        assert _call(p, **{name: None}) == ERR_ARG, name
    assert _call(p, B=-1) == ERR_ARG and _call(p, L=-1) == ERR_ARG
    assert _call(p, dtype=2) == ERR_ARG and _call(p, dtype=-1) == ERR_ARG
    for k in (0, 1, 17, -3):
        assert _call(p, k=k) == ERR_UNSUPPORTED, k
        assert _call(p, k=k, dtype=BF16) == ERR_UNSUPPORTED, k
        assert _call(p, k=k, B=0) == ERR_UNSUPPORTED, k          # nothing to do, but the arguments are still looked at
    for Dn in (0, -4, 6, 63, 4 * 4096 + 4):
        assert _call(p, Dn=Dn, x_rs=4 * 4100, out_rs=4 * 4100) == ERR_UNSUPPORTED, Dn
    assert _call(p, x_rs=66) == ERR_UNSUPPORTED and _call(p, out_rs=62) == ERR_UNSUPPORTED   # strides of whole 4-channel chunks
    assert _call(p, x_rs=60) == ERR_UNSUPPORTED and _call(p, out_rs=60) == ERR_UNSUPPORTED   # a row stride below Dn
    for name in ("x", "out"):
        assert _call(p, **{name: p + 8}) == ERR_UNSUPPORTED            # fp32 chunks are 16 bytes
        assert _call(p, **{name: p + 4}, dtype=BF16) == ERR_UNSUPPORTED   # bf16 chunks are 8
    for k in (2, 4, 16):
        assert _call(p, k=k, B=0) == OK and _call(p, k=k, L=0, dtype=BF16) == OK
    assert _call(p, B=0, x=None) == ERR_ARG


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the op
def test_dwconv_silu_start_refuses_cpu_tensors_and_autograd():
    from apertis_llm_amd import ops
    x, w, b = torch.randn(2, 6, 8), torch.randn(8, 1, 4), torch.randn(8)
    start = torch.tensor([0, 2], dtype=torch.int32)
    with torch.no_grad(), pytest.raises(ops.ApertisHipError, match="no CPU fallback"):
        ops.dwconv_silu(x, w, b, start=start)
    with pytest.raises(ops.ApertisHipError, match="forward only"):
        ops.dwconv_silu(x.requires_grad_(), w, b, start=start)
    with pytest.raises(ops.ApertisHipError, match="forward only"):
        ops.dwconv_silu(x.detach(), torch.nn.Parameter(w), b, start=start)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. off the GPU nothing changes
def _left_padded(B=3, L=12):
    mask = torch.ones(B, L, dtype=torch.long)
    mask[1, :5] = 0
    mask[2, :9] = 0
    return mask


def test_ssm_left_pad_answers_none_off_the_gpu_and_with_the_switch_off(switch, monkeypatch):
    import apertis_llm_amd as A
    ops = switch
    cfg = A.ApertisConfig(vocab_size=64, hidden_size=64, num_hidden_layers=1, num_attention_heads=4, intermediate_size=64,
                          attention_type="selective_ssm", max_position_embeddings=64)
    model = A.ApertisModel(cfg).eval()
    mask, x = _left_padded(), torch.zeros(3, 12, 64)
    monkeypatch.setattr(ops.ssm, "left_pad_starts", lambda m: pytest.fail("the mask was read"))
    monkeypatch.setattr(ops, "left_pad_starts", lambda m: pytest.fail("the mask was read"))
    with torch.no_grad():
        for on in (False, True):
            ops.SSM_LEFT_PAD = on
            assert model._ssm_left_pad(mask, x, None, None, False) is None           # a CPU tensor
            assert model._ssm_left_pad(None, x, None, None, False) is None


@pytest.mark.parametrize("attention_type", ["standard_mha", "selective_ssm"])
def test_cpu_model_is_untouched_by_the_switch(switch, monkeypatch, attention_type):
    """standard_mha runs its stock CPU branch: the same logits, bit for bit, with the switch on and off.  A selective_ssm block
    has no CPU path - its conv raises - and raises the same error with the switch on and off; neither reaches the start form."""
    import apertis_llm_amd as A
    ops = switch
    torch.manual_seed(5)
    cfg = A.ApertisConfig(vocab_size=64, hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=64,
                          attention_type=attention_type, max_position_embeddings=64)
    model = A.ApertisForCausalLM(cfg).eval()
    monkeypatch.setattr(ops.ssm, "_dwconv_silu_start", lambda *a: pytest.fail("the start form off the GPU"))
    mask = _left_padded()
    ids = torch.randint(4, 64, mask.shape, generator=torch.Generator().manual_seed(1))
    got = []
    with torch.no_grad():
        for on in (False, True, False):
            ops.SSM_LEFT_PAD = on
            if attention_type == "selective_ssm":
                with pytest.raises(ops.ApertisHipError, match="no CPU fallback"):
                    model(input_ids=ids, attention_mask=mask, use_cache=True)
            else:
                got.append(model(input_ids=ids, attention_mask=mask, use_cache=True)[1])
    for g in got[1:]:
        assert torch.equal(g, got[0])
