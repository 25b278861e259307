"""The host side of the padded-vocabulary LM head + loss (ops/loss.py, LCE_PAD_VOCAB), no GPU: the Vp arithmetic, the
vocabulary term of linear_cross_entropy_supported under both switch states, and the switch itself (off by default, read
from APERTIS_LCE_PAD_VOCAB at import like the other APERTIS_LCE_* switches, forwarded by the ops package)."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, F32 = torch.bfloat16, torch.float32


@pytest.mark.parametrize("V,vp_bf16,vp_f32", [(1, 8, 4), (7, 8, 8), (8, 8, 8), (9, 16, 12), (50257, 50264, 50260)])
def test_padded_width(V, vp_bf16, vp_f32):
    from apertis_llm_amd.ops import loss
    assert loss._lce_padded_vocab(V, BF16) == vp_bf16 and loss._lce_padded_vocab(V, F32) == vp_f32
    for dt, vn in ((BF16, 8), (F32, 4)):
        vp = loss._lce_padded_vocab(V, dt)
        assert vp % vn == 0 and 0 <= vp - V < vn
        assert loss._lce_padded_vocab(vp, dt) == vp                       # an aligned width is its own


def test_vocabulary_term_under_both_switch_states(monkeypatch):
    from apertis_llm_amd.ops import loss
    monkeypatch.setattr(loss, "LCE_PAD_VOCAB", False)
    assert [loss._lce_vocab_ok(V, BF16) for V in (1, 7, 8, 9, 50257, 50264)] == [False, False, True, False, False, True]
    assert [loss._lce_vocab_ok(V, F32) for V in (1, 4, 7, 8, 9, 50257, 50260)] == [False, True, False, True, False, False, True]
    monkeypatch.setattr(loss, "LCE_PAD_VOCAB", True)
    for dt in (BF16, F32):
        assert all(loss._lce_vocab_ok(V, dt) for V in (1, 7, 8, 9, 50257)) and not loss._lce_vocab_ok(0, dt)


class _FakeGpuTensor:
    """What ops.linear_cross_entropy_supported looks at, of a tensor that claims to live on the GPU."""
    is_cuda = True

    def __init__(self, shape, dtype=torch.float32):
        self.shape, self.dtype = tuple(shape), dtype

    def dim(self):
        return len(self.shape)


@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "f32"])
def test_supported_predicate(monkeypatch, dt):
    """Only the vocabulary term moves with the switch; every other term stays."""
    from apertis_llm_amd import ops
    h, lab = _FakeGpuTensor((2, 9, 32), dt), _FakeGpuTensor((2, 11), torch.int64)

    def W(V):
        return _FakeGpuTensor((V, 32))
    monkeypatch.setattr(ops, "LCE_PAD_VOCAB", False)
    assert ops.linear_cross_entropy_supported(h, W(1000), lab) and not ops.linear_cross_entropy_supported(h, W(1001), lab)
    monkeypatch.setattr(ops, "LCE_PAD_VOCAB", True)
    assert ops.loss.LCE_PAD_VOCAB is True                                  # the package forwards the write to the owner
    assert ops.linear_cross_entropy_supported(h, W(1000), lab) and ops.linear_cross_entropy_supported(h, W(1001), lab)
    assert ops.linear_cross_entropy_supported(h, W(1), lab) and ops.linear_cross_entropy_supported(h, W(50257), lab)
    assert not ops.linear_cross_entropy_supported(torch.zeros(2, 9, 32, dtype=dt), W(1001), lab)            # a CPU tensor
    assert not ops.linear_cross_entropy_supported(_FakeGpuTensor((2, 1, 32), dt), W(1001), lab)             # L < 2
    assert not ops.linear_cross_entropy_supported(_FakeGpuTensor((2, 9, 32), torch.float16), W(1001), lab)  # dtype
    assert not ops.linear_cross_entropy_supported(h, W(1001), _FakeGpuTensor((3, 11), torch.int64))         # batch
    assert not ops.linear_cross_entropy_supported(h, W(1001), _FakeGpuTensor((2, 11), torch.int32))         # label dtype
    # materialised logits keep their alignment rule
    assert not ops.shifted_cross_entropy_supported(_FakeGpuTensor((2, 9, 1001), dt), lab)
    assert ops.shifted_cross_entropy_supported(_FakeGpuTensor((2, 9, 1000), dt), lab)


def test_switch_is_off_by_default_and_reads_its_environment_variable():
    from apertis_llm_amd import ops
    assert ops.LCE_PAD_VOCAB is (os.environ.get("APERTIS_LCE_PAD_VOCAB", "0") == "1")        # read once, at import
    assert "LCE_PAD_VOCAB" not in vars(ops) and ops._FORWARDED["LCE_PAD_VOCAB"] is ops.loss
    env = dict(os.environ, APERTIS_LCE_PAD_VOCAB="1", APERTIS_LCE_FUSED_CE="0")
    code = "from apertis_llm_amd import ops; print(ops.LCE_PAD_VOCAB, ops.loss.LCE_PAD_VOCAB, ops.loss.LCE_FUSED_CE, ops.loss.LCE_OWN_WGRAD)"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True).stdout
    assert out.split() == ["True", "True", "False", "True"]
    env["APERTIS_LCE_PAD_VOCAB"] = "0"
    code = "from apertis_llm_amd import ops; print(ops.LCE_PAD_VOCAB)"
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True).stdout.split() == ["False"]
