"""The device-length forms of the standard_mha decode step, what needs no GPU:

  1. apertis_rope_kv_append_at / apertis_attention_decode_at refuse every bad argument class before any launch
  2. ApertisForCausalLM._decode_graph_ok keeps a standard_mha model off the graph tail with the switch off, with a
     plain-tuple past and with absolute position embeddings
"""
import ctypes

import pytest
import torch

ERR_ARG, ERR_UNSUPPORTED = -1, -2
F32, BF16 = 0, 1


@pytest.fixture(scope="module")
def lib():
    from apertis_llm_amd import _lib
    assert _lib.F32 == F32 and _lib.BF16 == BF16
    return _lib.load()


@pytest.fixture(scope="module")
def mem():
    """Host memory with a 64-byte aligned start: the entry points only look at the addresses (every case below is refused
    before a launch)."""
    buf = ctypes.create_string_buffer(4096 + 64)
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    return buf, base


def _append_args(p, **kw):
    B, W, cap, max_pos = 2, 256, 320, 512
    a = dict(q=p, q_rs=W, k=p, k_rs=W, v=p, v_rs=W, cos=p, sin=p, max_pos=max_pos, len=p, pos_offset=0, err=p, q_out=p,
             q_out_rs=W, k_cache=p, kc_rs=W, kc_bs=cap * W, v_cache=p, vc_rs=W, vc_bs=cap * W, cap=cap, B=B, W=W, dtype=F32,
             stream=None)
    a.update(kw)
    return tuple(a.values())


@pytest.mark.parametrize("kw,want", [
    (dict(q=None), ERR_ARG), (dict(k=None), ERR_ARG), (dict(v=None), ERR_ARG), (dict(q_out=None), ERR_ARG),
    (dict(k_cache=None), ERR_ARG), (dict(v_cache=None), ERR_ARG),
    (dict(len=None), ERR_ARG), (dict(err=None), ERR_ARG),                  # the device length and the error word are required
    (dict(cos=None), ERR_ARG), (dict(sin=None), ERR_ARG),                  # the tables come together
    (dict(q_rs=255), ERR_ARG), (dict(k_rs=255), ERR_ARG), (dict(v_rs=255), ERR_ARG), (dict(q_out_rs=255), ERR_ARG),
    (dict(kc_rs=255), ERR_ARG), (dict(vc_rs=255), ERR_ARG), (dict(kc_bs=320 * 256 - 1), ERR_ARG), (dict(vc_bs=1), ERR_ARG),
    (dict(W=255, q_rs=512), ERR_ARG), (dict(W=0), ERR_ARG), (dict(cap=0), ERR_ARG), (dict(B=-1), ERR_ARG),
    (dict(dtype=7), ERR_ARG), (dict(max_pos=0), ERR_ARG),
    (dict(pos_offset=512), ERR_ARG), (dict(pos_offset=-512 - 320), ERR_ARG),   # no row of the cache lands in the table
])
def test_append_at_refuses_bad_arguments_before_any_launch(lib, mem, kw, want):
    _, p = mem
    assert lib.apertis_rope_kv_append_at(*_append_args(p, **kw)) == want


def _attn_args(p, **kw):
    B, H, D, cap = 2, 4, 64, 320
    W = H * D
    a = dict(q=p, q_rs=W, k=p, k_rs=W, k_bs=cap * W, v=p, v_rs=W, v_bs=cap * W, cap=cap, len=p, key_valid=p, kv_rs=cap, out=p,
             out_rs=W, ws=p, B=B, H=H, D=D, splits=4, dtype=F32, stream=None)
    a.update(kw)
    return tuple(a.values())


@pytest.mark.parametrize("kw,want", [
    (dict(q=None), ERR_ARG), (dict(k=None), ERR_ARG), (dict(v=None), ERR_ARG), (dict(out=None), ERR_ARG),
    (dict(len=None), ERR_ARG),
    (dict(q_rs=255), ERR_ARG), (dict(out_rs=255), ERR_ARG), (dict(k_rs=255), ERR_ARG), (dict(v_rs=255), ERR_ARG),
    (dict(k_bs=320 * 256 - 4), ERR_ARG), (dict(v_bs=4), ERR_ARG),
    (dict(kv_rs=319), ERR_ARG),                                            # the validity buffer covers the capacity
    (dict(dtype=7), ERR_ARG), (dict(cap=0), ERR_ARG), (dict(B=-1), ERR_ARG), (dict(H=0), ERR_ARG),
    (dict(D=48, q_rs=256), ERR_UNSUPPORTED), (dict(D=256, H=1), ERR_UNSUPPORTED), (dict(B=65536), ERR_UNSUPPORTED),
    (dict(splits=0), ERR_ARG), (dict(splits=-1), ERR_ARG), (dict(splits=65), ERR_ARG),     # required, 1..MAX_SPLITS
    (dict(ws=None), ERR_ARG),                                              # splits > 1 needs the workspace
    (dict(q_rs=257), ERR_UNSUPPORTED), (dict(k_rs=258, k_bs=320 * 258), ERR_UNSUPPORTED),  # 16-byte rows
    (dict(v_rs=260, v_bs=320 * 260 + 1), ERR_UNSUPPORTED), (dict(dtype=BF16, q_rs=260), ERR_UNSUPPORTED),
])
def test_attention_at_refuses_bad_arguments_before_any_launch(lib, mem, kw, want):
    _, p = mem
    assert lib.apertis_attention_decode_at(*_attn_args(p, **kw)) == want


def test_attention_at_refuses_misaligned_pointers(lib, mem):
    _, p = mem
    for name in ("q", "k", "v"):
        assert lib.apertis_attention_decode_at(*_attn_args(p, **{name: p + 4})) == ERR_UNSUPPORTED


def test_split_count_is_not_bounded_by_the_key_count(lib, mem):
    """The by-value form refuses more pieces than keys (Lk 2, 8 pieces); the device-length form has no host Lk to refuse by:
    with B = 0 (nothing to launch) every split count in range is accepted."""
    _, p = mem
    by_value = (p, 256, p, 256, 320 * 256, p, 256, 320 * 256, 320, p, 320, p, 256, p, 0, 2, 4, 64, 8, F32, None)
    assert lib.apertis_attention_decode(*by_value) == ERR_ARG
    for n in (1, 8, 64):
        assert lib.apertis_attention_decode_at(*_attn_args(p, B=0, splits=n)) == 0


def test_decode_graph_ok_keeps_standard_mha_off_the_tail_without_a_gpu(monkeypatch):
    import apertis_llm_amd as A
    from apertis_llm_amd import ops

    def model(**kw):
        cfg = dict(vocab_size=64, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=128,
                   attention_type="standard_mha", max_position_embeddings=64)
        cfg.update(kw)
        return A.ApertisForCausalLM(A.ApertisConfig(**cfg)).eval()
    assert ops.ATTN_DECODE_GRAPH is False                    # off unless APERTIS_MHA_DECODE_GRAPH=1
    toks = torch.zeros(1, 5, dtype=torch.long)
    plain = ((torch.zeros(1, 4, 128), torch.zeros(1, 4, 128)),)
    cache = ops.KVCache([torch.zeros(1, 40, 128)], [torch.zeros(1, 40, 128)], length=4)
    mask = torch.ones(1, 5, dtype=torch.long)
    with torch.no_grad():
        m = model()
        assert not m._decode_graph_ok(toks, False, 1.0, None, cache, 30, mask)            # the switch is off
        assert not m._mha_graph_ok(toks, cache, 30, mask)
        monkeypatch.setattr(ops, "ATTN_DECODE_GRAPH", True)
        assert ops.attention.ATTN_DECODE_GRAPH is True
        assert not m._mha_graph_ok(toks, plain, 30, mask)                                 # a plain-tuple past
        assert not m._decode_graph_ok(toks, False, 1.0, None, plain, 30, mask)
        assert not m._decode_graph_ok(toks, False, 1.0, None, cache, 30, mask)            # CPU tokens
        assert not m._mha_graph_ok(toks, cache, 37, mask)                                 # no room for 37 more rows
        assert not model(max_position_embeddings=20)._mha_graph_ok(toks, cache, 30, mask)   # the rotary table ends first
        absm = model(position_embedding_type="absolute")
        assert not absm._decode_graph_ok(toks, False, 1.0, None, cache, 30, mask)         # absolute position embeddings
        # the same questions with everything else in place: only the device keeps the first from being yes
        assert m._mha_graph_ok(toks, cache, 30, mask)
        left_padded = mask.clone()
        left_padded[0, 0] = 0
        assert not m._mha_graph_ok(toks, cache, 30, left_padded)

