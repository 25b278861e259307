"""Left-padded standard_mha batches on the HIP kernels (ops.ATTN_LEFT_PAD), what needs no GPU:

  1. the library exports apertis_attention_dead_rows under ABI 4.12 and refuses every bad argument class before any launch
  2. the switch is off by default and forwarded by the ops package
  3. ApertisModel._attention_mask: the (fused_ok, decode_ok, dead_rows) triple per mask form, switch off (the rule before
     the switch existed) and on
  4. ApertisForCausalLM._mha_graph_ok takes a left-padded mask only with both switches on
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
    """Host memory with a 64-byte aligned start: the entry point only looks at the addresses (every case below is refused
    before a launch, or has nothing to launch)."""
    buf = ctypes.create_string_buffer(4096 + 64)
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    return buf, base


@pytest.fixture
def left_pad():
    from apertis_llm_amd import ops
    prev = ops.ATTN_LEFT_PAD, ops.ATTN_DECODE_GRAPH
    yield ops
    ops.ATTN_LEFT_PAD, ops.ATTN_DECODE_GRAPH = prev


def _args(p, **kw):
    B, W, n, Lq, cap = 2, 256, 7, 5, 40
    a = dict(v=p, v_rs=W, v_bs=cap * W, key_valid=p, kv_rs=n + Lq, out=p, out_rs=W, out_bs=Lq * W, B=B, Lq=Lq, n=n, W=W,
             dtype=F32, stream=None)
    a.update(kw)
    return tuple(a.values())


def test_library_exports_the_fill_under_the_same_abi(lib):
    from apertis_llm_amd import _lib
    assert _lib.ABI_VERSION == (4 << 16) | 12 and int(lib.apertis_abi_version()) == _lib.ABI_VERSION
    assert "apertis_attention_dead_rows" in _lib.SIGNATURES
    assert lib.apertis_attention_dead_rows is not None


@pytest.mark.parametrize("kw,want", [
    (dict(v=None), ERR_ARG), (dict(key_valid=None), ERR_ARG), (dict(out=None), ERR_ARG),
    (dict(W=0), ERR_ARG), (dict(W=-256), ERR_ARG), (dict(Lq=0), ERR_ARG), (dict(n=-1), ERR_ARG), (dict(B=-1), ERR_ARG),
    (dict(dtype=7), ERR_ARG),
    (dict(v_rs=255), ERR_ARG), (dict(out_rs=252), ERR_ARG),                # a row stride below W
    (dict(v_bs=12 * 256 - 4), ERR_ARG), (dict(out_bs=5 * 256 - 4), ERR_ARG),   # a batch stride below the rows it spans
    (dict(kv_rs=11), ERR_ARG), (dict(n=8), ERR_ARG),                       # kv_rs < n + Lq
    (dict(v_rs=257, v_bs=40 * 257 + 3), ERR_UNSUPPORTED), (dict(out_rs=258, out_bs=5 * 258 + 2), ERR_UNSUPPORTED),
    (dict(v_bs=40 * 256 + 1), ERR_UNSUPPORTED), (dict(out_bs=5 * 256 + 2), ERR_UNSUPPORTED),
    (dict(dtype=BF16, v_rs=260, v_bs=40 * 260), ERR_UNSUPPORTED),          # 520-byte rows
    (dict(W=254), ERR_UNSUPPORTED), (dict(dtype=BF16, W=252), ERR_UNSUPPORTED),   # no whole 16-byte vectors
    (dict(B=65536), ERR_UNSUPPORTED),
    (dict(B=0), 0),                                                        # nothing to launch
])
def test_fill_refuses_bad_arguments_before_any_launch(lib, mem, kw, want):
    _, p = mem
    assert lib.apertis_attention_dead_rows(*_args(p, **kw)) == want


def test_fill_refuses_misaligned_pointers(lib, mem):
    _, p = mem
    for name in ("v", "out"):
        for off in (4, 8):
            assert lib.apertis_attention_dead_rows(*_args(p, **{name: p + off})) == ERR_UNSUPPORTED


def test_switch_is_off_by_default_and_forwarded(left_pad):
    ops = left_pad
    assert ops.ATTN_LEFT_PAD is False and ops.attention.ATTN_LEFT_PAD is False   # off unless APERTIS_MHA_LEFT_PAD=1
    ops.ATTN_LEFT_PAD = True
    assert ops.attention.ATTN_LEFT_PAD is True and "ATTN_LEFT_PAD" not in vars(ops)
    ops.ATTN_LEFT_PAD = False
    assert ops.attention.ATTN_LEFT_PAD is False


def _masks():
    B, L = 3, 12
    all_valid = torch.ones(B, L, dtype=torch.long)
    right = all_valid.clone()
    right[1, 7:] = 0
    left = all_valid.clone()
    left[1, :5] = 0
    holes = all_valid.clone()
    holes[2, 0] = holes[2, 4] = holes[2, 9] = 0
    dead = left.clone()
    dead[0] = 0
    return dict(all_valid=all_valid, right_padded=right, left_padded=left, key0_and_holes=holes, one_fully_masked=dead)


# (fused_ok, decode_ok, dead_rows) of a forward without a past; with a past, fused_ok is False and the others stay
OFF = dict(all_valid=(True, True, False), right_padded=(True, True, False), left_padded=(False, False, False),
           key0_and_holes=(False, False, False), one_fully_masked=(False, False, False))
ON = dict(OFF, left_padded=(True, True, True), key0_and_holes=(True, True, True))


@pytest.mark.parametrize("name", list(OFF))
@pytest.mark.parametrize("switch", [False, True])
def test_attention_mask_triples(left_pad, name, switch):
    import apertis_llm_amd as A
    ops = left_pad
    cfg = A.ApertisConfig(vocab_size=64, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=128,
                          attention_type="standard_mha", max_position_embeddings=64)
    model = A.ApertisModel(cfg).eval()
    mask = _masks()[name]
    B, L = mask.shape
    x = torch.zeros(B, L, 128)
    ops.ATTN_LEFT_PAD = switch
    want = (ON if switch else OFF)[name]
    m = model._attention_mask(mask, (B, L), x, 0, True)
    assert (m.fused_ok, m.decode_ok, m.dead_rows) == want
    assert (m.key_valid is None) == (name == "all_valid")
    # a single-token step against L - 1 cached keys: the same decision, and never the prefill's kernels
    m = model._attention_mask(mask, (B, 1), x[:, :1], L - 1, True, L - 1)
    assert (m.fused_ok, m.decode_ok, m.dead_rows) == ((name == "all_valid"),) + want[1:]
    # a multi-token piece going into a KVCache may lie wholly inside a sequence's padding (the valid keys come later)
    m = model._attention_mask(mask, (B, 4), x[:, :4], L - 4, True, L - 4)
    piece = (True, True) if switch and name == "one_fully_masked" else want[1:]
    assert (m.fused_ok, m.decode_ok, m.dead_rows) == ((name == "all_valid"),) + piece
    # no mask at all, and a device step state: untouched by the switch
    m = model._attention_mask(None, (B, L), x, 0, True)
    assert (m.fused_ok, m.decode_ok, m.dead_rows) == (True, True, False)


def test_mha_graph_ok_takes_a_left_padded_mask_only_with_both_switches(left_pad):
    import apertis_llm_amd as A
    ops = left_pad
    cfg = A.ApertisConfig(vocab_size=64, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=128,
                          attention_type="standard_mha", max_position_embeddings=64)
    m = A.ApertisForCausalLM(cfg).eval()
    toks = torch.zeros(2, 5, dtype=torch.long)
    cache = ops.KVCache([torch.zeros(2, 40, 128)], [torch.zeros(2, 40, 128)], length=4)
    mask = torch.ones(2, 5, dtype=torch.long)
    left_padded = mask.clone()
    left_padded[0, :2] = 0
    fully = left_padded.clone()
    fully[1] = 0
    with torch.no_grad():
        for graph in (False, True):
            for pad in (False, True):
                ops.ATTN_DECODE_GRAPH, ops.ATTN_LEFT_PAD = graph, pad
                assert m._mha_graph_ok(toks, cache, 30, mask) == graph
                assert m._mha_graph_ok(toks, cache, 30, left_padded) == (graph and pad)
                assert not m._mha_graph_ok(toks, cache, 30, fully)               # a sequence without a valid key
                assert not m._mha_graph_ok(toks, cache, 30, left_padded[:, :4])  # the mask does not cover the step
