"""standard_mha KV-cache decode without a GPU (csrc/attention_decode.hip, ops/attention.py): the entry points refuse bad
arguments before any launch, the split heuristic and its workspace at a table of shapes, the host logic of ops.KVCache."""
import pytest
import torch

F32, BF16 = 0, 1
P = 4096            # a 16-byte aligned stand-in for a device pointer: nothing is dereferenced before the checks pass


def _lib():
    from apertis_llm_amd import _lib
    return _lib.load()


def _decode(lib, q=P, q_rs=256, k=P, k_rs=256, k_bs=None, v=P, v_rs=256, v_bs=None, cap=32, kv=None, kv_rs=0, out=P, out_rs=256,
            ws=None, B=2, Lk=8, H=4, D=64, splits=1, dtype=F32):
    k_bs = cap * k_rs if k_bs is None else k_bs
    v_bs = cap * v_rs if v_bs is None else v_bs
    return lib.apertis_attention_decode(q, q_rs, k, k_rs, k_bs, v, v_rs, v_bs, cap, kv, kv_rs, out, out_rs, ws, B, Lk, H, D, splits,
                                        dtype, None)


def _append(lib, q=P, q_rs=256, k=P, k_rs=256, v=P, v_rs=256, cos=P, sin=P, max_pos=64, t=3, qo=P, qo_rs=256, kc=P, kc_rs=256,
            kc_bs=None, vc=P, vc_rs=256, vc_bs=None, cap=32, t_cache=3, B=2, W=256, dtype=F32):
    kc_bs = cap * kc_rs if kc_bs is None else kc_bs
    vc_bs = cap * vc_rs if vc_bs is None else vc_bs
    return lib.apertis_rope_kv_append(q, q_rs, k, k_rs, v, v_rs, cos, sin, max_pos, t, qo, qo_rs, kc, kc_rs, kc_bs, vc, vc_rs, vc_bs,
                                      cap, t_cache, B, W, dtype, None)


def test_attention_decode_validates_before_any_launch():
    lib = _lib()
    assert _decode(lib, B=0) == 0                                         # the baseline call is well-formed: nothing to do
    assert _decode(lib, q=None) == -1 and _decode(lib, k=None) == -1 and _decode(lib, v=None) == -1 and _decode(lib, out=None) == -1
    assert _decode(lib, Lk=0) == -1 and _decode(lib, Lk=-3) == -1         # Lk < 1
    assert _decode(lib, Lk=33) == -1                                      # Lk > cap
    assert _decode(lib, H=0) == -1 and _decode(lib, dtype=2) == -1
    assert _decode(lib, q_rs=255) == -1 and _decode(lib, k_rs=128) == -1 and _decode(lib, k_bs=31 * 256) == -1
    assert _decode(lib, kv=P, kv_rs=7) == -1                              # a mask row shorter than Lk
    assert _decode(lib, splits=-1) == -1 and _decode(lib, splits=9) == -1 and _decode(lib, Lk=32, splits=2, ws=None, B=1) == -1
    assert _decode(lib, cap=4096, Lk=4096, splits=65, ws=P) == -1         # above APERTIS_ATTN_DECODE_MAX_SPLITS
    # shapes the kernels are not built for: D = 48, rows off the 16-byte grid
    assert _decode(lib, D=48, H=4, q_rs=192, k_rs=192, v_rs=192, out_rs=192) == -2
    assert _decode(lib, k_rs=258) == -2 and _decode(lib, v_rs=257) == -2 and _decode(lib, dtype=BF16, k_rs=260) == -2
    assert _decode(lib, q=P + 4) == -2 and _decode(lib, k=P + 8) == -2
    assert _decode(lib, B=65536) == -2


def test_rope_kv_append_validates_before_any_launch():
    lib = _lib()
    assert _append(lib, B=0) == 0
    for name in ("q", "k", "v", "qo", "kc", "vc"):
        assert _append(lib, **{name: None}) == -1, name
    assert _append(lib, cos=None) == -1 and _append(lib, sin=None) == -1  # they come together ...
    assert _append(lib, cos=None, sin=None, B=0) == 0                     # ... or not at all: a plain append
    assert _append(lib, t_cache=32) == -1 and _append(lib, t_cache=40) == -1 and _append(lib, t_cache=-1) == -1    # t_cache >= cap
    assert _append(lib, t=64) == -1 and _append(lib, t=-65) == -1 and _append(lib, t=-64, B=0) == 0 and _append(lib, t=63, B=0) == 0
    assert _append(lib, cos=None, sin=None, t=10 ** 6, B=0) == 0          # no table, no range
    assert _append(lib, W=255) == -1 and _append(lib, W=0) == -1 and _append(lib, dtype=2) == -1
    assert _append(lib, kc_rs=128) == -1 and _append(lib, vc_bs=31 * 256) == -1 and _append(lib, qo_rs=100) == -1
    assert _append(lib, cap=0, t_cache=0) == -1


def test_splits_and_workspace_at_a_table_of_shapes():
    """splits = min(256 // (B*H), Lk // 128, 64), at least 1: a pure function of the shape, never more than Lk."""
    lib = _lib()
    table = {(1, 14, 1, 64): 1, (1, 14, 127, 64): 1, (1, 14, 128, 64): 1, (1, 14, 256, 64): 2, (1, 14, 2048, 64): 16,
             (1, 14, 4096, 64): 18, (1, 14, 8191, 64): 18, (16, 14, 2048, 64): 1, (16, 12, 8191, 128): 1, (1, 1, 8191, 128): 63,
             (4, 14, 2047, 64): 4,
             (1, 1, 16384, 64): 64, (64, 12, 4096, 64): 1, (1, 8, 512, 128): 4, (3, 4, 40, 64): 1}
    for (B, H, Lk, D), want in table.items():
        got = lib.apertis_attention_decode_splits(B, H, Lk, D)
        assert got == want == lib.apertis_attention_decode_splits(B, H, Lk, D), (B, H, Lk, D, got)
        assert 1 <= got <= min(Lk, 64)
        assert lib.apertis_attention_decode_workspace_bytes(B, H, D, got) == (0 if got == 1 else B * H * got * (D + 2) * 4)
    assert lib.apertis_attention_decode_splits(0, 4, 8, 64) == -1 and lib.apertis_attention_decode_splits(1, 4, 0, 64) == -1
    assert lib.apertis_attention_decode_workspace_bytes(2, 4, 64, 0) == -1
    assert lib.apertis_attention_decode_workspace_bytes(2, 4, 64, 65) == -1
    assert lib.apertis_attention_decode_workspace_bytes(2, 4, 64, 64) == 2 * 4 * 64 * 66 * 4


def test_kv_cache_host_logic():
    from apertis_llm_amd import ops
    B, L, W, NL = 2, 5, 128, 3
    past = tuple((torch.randn(B, L, W), torch.randn(B, L, W)) for _ in range(NL))
    with pytest.raises(ops.ApertisHipError):
        ops.KVCache.from_prefill(past, L - 1)                             # capacity below the prefill
    c = ops.KVCache.from_prefill(past, 9)
    assert len(c) == NL and c.capacity == 9 and c.length == L and c.lengths == [L] * NL and c.dtype == torch.float32
    assert bool(c)
    # the indexing contract of the tuple it replaces: cache[i][0].shape[1] is the past length, [0] / [1] are views
    for i in range(NL):
        k, v = c[i]
        assert len(c[i]) == 2 and c[i][0].shape == (B, L, W) and torch.equal(k, past[i][0]) and torch.equal(v, past[i][1])
        assert k.data_ptr() == c.k[i].data_ptr() and c[i][1].data_ptr() == c.v[i].data_ptr()
        assert k.stride() == (9 * W, W, 1)
    assert torch.equal(c[-1][0], past[-1][0])
    with pytest.raises(IndexError):
        c[NL]
    with pytest.raises(IndexError):
        c[0][2]
    assert all(torch.equal(layer[0], p[0]) and torch.equal(layer[1], p[1]) for layer, p in zip(c, past))
    # lengths are per layer: layer 0 growing does not move what layer 1 shows
    c.lengths[0] += 1
    assert c[0][0].shape[1] == L + 1 and c[1][0].shape[1] == L and c.length == L + 1
    c.lengths = [9] * NL
    assert c[2][1].shape[1] == 9
    e = ops.KVCache.empty(2, 3, 16, 64, torch.bfloat16)
    assert e.length == 0 and e[0][0].shape == (3, 0, 64) and e.dtype == torch.bfloat16 and e.capacity == 16
    with pytest.raises(ops.ApertisHipError):
        ops.KVCache([torch.zeros(2, 4, 8)], [torch.zeros(2, 4, 9)])
    with pytest.raises(ops.ApertisHipError):
        ops.KVCache([torch.zeros(2, 4, 8)], [torch.zeros(2, 4, 8)], length=5)
    with pytest.raises(ops.ApertisHipError):
        ops.KVCache.empty(1, 1, 0, 64)


def test_decode_ops_refuse_cpu_tensors_and_the_switch_is_forwarded():
    from apertis_llm_amd import ops
    c = ops.KVCache.empty(1, 2, 8, 128)
    x = torch.randn(2, 128)
    with pytest.raises(ops.ApertisHipError):
        ops.kv_append_rope(x, x, x, c, 0)
    with pytest.raises(ops.ApertisHipError):
        ops.attention_decode(x, c, 0, 2)
    assert c.lengths == [0]
    assert ops.attention_decode_supported(x, 2) and ops.attention_decode_supported(x, 1)
    assert not ops.attention_decode_supported(torch.randn(2, 192), 4) and not ops.attention_decode_supported(x.half(), 2)
    prev = ops.ATTN_DECODE_FUSED
    try:
        ops.ATTN_DECODE_FUSED = False
        assert ops.attention.ATTN_DECODE_FUSED is False and ops.ATTN_DECODE_FUSED is False
    finally:
        ops.ATTN_DECODE_FUSED = prev
    assert ops.attention.ATTN_DECODE_FUSED is prev


def test_cpu_model_with_a_kv_cache_runs_the_stock_branch_and_returns_plain_tensors():
    """A KVCache handed to a CPU model: the kernels do not run there; the stock branch reads the cache's views and hands
    back plain tensors, the same bits as with the plain tuple."""
    import apertis_llm_amd as A
    from apertis_llm_amd import ops
    torch.manual_seed(0)
    cfg = A.ApertisConfig(vocab_size=64, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128,
                          attention_type="standard_mha", max_position_embeddings=64)
    model = A.ApertisForCausalLM(cfg).eval()
    ids = torch.randint(4, 64, (2, 7))
    with torch.no_grad():
        past = model(input_ids=ids[:, :-1], use_cache=True)[4]
        a = model(input_ids=ids[:, -1:], past_key_values=past, use_cache=True)
        cache = ops.KVCache.from_prefill(past, 16)
        b = model(input_ids=ids[:, -1:], past_key_values=cache, use_cache=True)
    assert torch.equal(a[1], b[1]) and isinstance(b[4], tuple) and cache.lengths == [6, 6]
    assert all(torch.equal(x, y) for pa, pb in zip(a[4], b[4]) for x, y in zip(pa, pb))
