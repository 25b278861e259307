"""standard_mha multi-token KV-cache steps without a GPU (csrc/attention_decode.hip, ops/attention.py, model.py): the entry
points refuse bad arguments before any launch, the split rule and its workspace at a table of shapes, the `multi_token` flag
of ops.KVCache, and every refusal of generate(past_key_values=...)."""
import pytest
import torch

F32, BF16 = 0, 1
P = 4096            # a 16-byte aligned stand-in for a device pointer: nothing is dereferenced before the checks pass


def _lib():
    from apertis_llm_amd import _lib
    return _lib.load()


def _chunk(lib, q=P, q_rs=256, k=P, k_rs=256, k_bs=None, v=P, v_rs=256, v_bs=None, cap=64, kv=None, kv_rs=0, out=P, out_rs=256,
           ws=None, B=2, Lq=8, n=20, H=4, D=64, splits=1, dtype=F32):
    k_bs = cap * k_rs if k_bs is None else k_bs
    v_bs = cap * v_rs if v_bs is None else v_bs
    return lib.apertis_attention_chunk(q, q_rs, k, k_rs, k_bs, v, v_rs, v_bs, cap, kv, kv_rs, out, out_rs, ws, B, Lq, n, H, D,
                                       splits, dtype, None)


def _append(lib, q=P, q_rs=256, q_bs=None, k=P, k_rs=256, k_bs=None, v=P, v_rs=256, v_bs=None, cos=P, sin=P, max_pos=64, t0=3,
            qo=P, kc=P, kc_rs=256, kc_bs=None, vc=P, vc_rs=256, vc_bs=None, cap=32, t_cache0=3, B=2, Lq=8, W=256, dtype=F32):
    q_bs = Lq * q_rs if q_bs is None else q_bs
    k_bs = Lq * k_rs if k_bs is None else k_bs
    v_bs = Lq * v_rs if v_bs is None else v_bs
    kc_bs = cap * kc_rs if kc_bs is None else kc_bs
    vc_bs = cap * vc_rs if vc_bs is None else vc_bs
    return lib.apertis_rope_kv_append_chunk(q, q_rs, q_bs, k, k_rs, k_bs, v, v_rs, v_bs, cos, sin, max_pos, t0, qo, kc, kc_rs, kc_bs,
                                            vc, vc_rs, vc_bs, cap, t_cache0, B, Lq, W, dtype, None)


def test_abi_version_is_4_12():
    from apertis_llm_amd import _lib
    assert _lib.ABI_VERSION == (4 << 16) | 12 == _lib.load().apertis_abi_version()


def test_attention_chunk_validates_before_any_launch():
    lib = _lib()
    assert _chunk(lib, B=0) == 0                                          # the baseline call is well-formed: nothing to do
    assert _chunk(lib, q=None) == -1 and _chunk(lib, k=None) == -1 and _chunk(lib, v=None) == -1 and _chunk(lib, out=None) == -1
    assert _chunk(lib, Lq=0) == -1 and _chunk(lib, n=-1) == -1
    assert _chunk(lib, n=57) == -1 and _chunk(lib, n=56, B=0) == 0        # n + Lq > cap
    assert _chunk(lib, n=2 ** 62, Lq=2 ** 62) == -1                       # (no overflow in that sum)
    assert _chunk(lib, H=0) == -1 and _chunk(lib, dtype=2) == -1
    assert _chunk(lib, q_rs=255) == -1 and _chunk(lib, out_rs=128) == -1 and _chunk(lib, k_rs=128) == -1
    assert _chunk(lib, k_bs=63 * 256) == -1 and _chunk(lib, v_bs=63 * 256) == -1
    assert _chunk(lib, kv=P, kv_rs=27) == -1 and _chunk(lib, kv=P, kv_rs=28, B=0) == 0       # a mask row shorter than n + Lq
    assert _chunk(lib, splits=-1) == -1 and _chunk(lib, splits=65, ws=P) == -1               # outside [1, 64] (0: the rule)
    assert _chunk(lib, splits=2, ws=None) == -1                           # a missing workspace
    assert _chunk(lib, splits=0, ws=None, B=1, H=1, n=4000, Lq=8, cap=4096) == -1            # ... which the rule's count needs too
    # shapes the kernels are not built for: D = 48, rows off the 16-byte grid
    assert _chunk(lib, D=48, H=4, q_rs=192, k_rs=192, v_rs=192, out_rs=192) == -2
    assert _chunk(lib, k_rs=258) == -2 and _chunk(lib, v_rs=257) == -2 and _chunk(lib, dtype=BF16, k_rs=260) == -2
    assert _chunk(lib, q=P + 4) == -2 and _chunk(lib, k=P + 8) == -2 and _chunk(lib, out=P + 4) == -2
    assert _chunk(lib, B=16384) == -2                                     # B * H > 65535


def test_rope_kv_append_chunk_validates_before_any_launch():
    lib = _lib()
    assert _append(lib, B=0) == 0 and _append(lib, Lq=0) == 0
    for name in ("q", "k", "v", "qo", "kc", "vc"):
        assert _append(lib, **{name: None}) == -1, name
    assert _append(lib, cos=None) == -1 and _append(lib, sin=None) == -1  # they come together ...
    assert _append(lib, cos=None, sin=None, B=0) == 0                     # ... or not at all: a plain append
    assert _append(lib, t_cache0=25) == -1 and _append(lib, t_cache0=24, B=0) == 0           # t_cache0 + Lq > cap
    assert _append(lib, t_cache0=-1) == -1 and _append(lib, t_cache0=40) == -1 and _append(lib, Lq=-1) == -1
    assert _append(lib, t_cache0=2 ** 62, Lq=2 ** 62) == -1
    assert _append(lib, t0=57) == -1 and _append(lib, t0=56, B=0) == 0    # positions off the table: t0 + Lq > max_pos
    assert _append(lib, t0=-65) == -1 and _append(lib, t0=-64, B=0) == 0 and _append(lib, t0=64) == -1
    assert _append(lib, cos=None, sin=None, t0=10 ** 6, B=0) == 0         # no table, no range
    assert _append(lib, W=255) == -1 and _append(lib, W=0) == -1 and _append(lib, dtype=2) == -1
    assert _append(lib, q_rs=128) == -1 and _append(lib, kc_rs=128) == -1 and _append(lib, vc_bs=31 * 256) == -1
    assert _append(lib, k_bs=7 * 256) == -1 and _append(lib, cap=0, t_cache0=0) == -1


def test_chunk_splits_and_workspace_at_a_table_of_shapes():
    """splits = min(2048 // (B * H * ceil(Lq / 16)), Lk // 64, 64), at least 1: the decode rule's form counted in waves of 16
    query rows, a pure function of the shape."""
    lib = _lib()
    table = {(1, 14, 64, 1984, 64): 31, (1, 14, 16, 1936, 64): 30, (1, 14, 65, 4096, 64): 29, (1, 14, 256, 2176, 64): 9,
             (1, 14, 1024, 2944, 64): 2, (16, 14, 64, 1984, 64): 2, (16, 14, 16, 1936, 64): 9, (16, 14, 256, 2176, 64): 1,
             (1, 8, 64, 1984, 128): 31, (1, 8, 16, 528, 128): 8, (1, 1, 3, 16384, 64): 64, (2, 3, 130, 630, 64): 9,
             (2, 3, 3, 260, 128): 4, (1, 1, 7, 7, 64): 1, (1, 14, 16, 16, 64): 1, (4, 14, 64, 8192, 64): 9}
    for (B, H, Lq, Lk, D), want in table.items():
        got = lib.apertis_attention_chunk_splits(B, H, Lq, Lk, D)
        assert got == want == max(1, min(2048 // (B * H * -(-Lq // 16)), Lk // 64, 64)), (B, H, Lq, Lk, D, got)
        assert lib.apertis_attention_chunk_workspace_bytes(B, H, Lq, D, got) == (0 if got == 1 else B * Lq * H * got * (D + 2) * 4)
    assert lib.apertis_attention_chunk_splits(0, 4, 8, 8, 64) == -1 and lib.apertis_attention_chunk_splits(1, 4, 0, 8, 64) == -1
    assert lib.apertis_attention_chunk_splits(1, 4, 9, 8, 64) == -1                        # Lk < Lq
    assert lib.apertis_attention_chunk_workspace_bytes(2, 4, 8, 64, 0) == -1
    assert lib.apertis_attention_chunk_workspace_bytes(2, 4, 8, 64, 65) == -1
    assert lib.apertis_attention_chunk_workspace_bytes(2, 4, 8, 64, 64) == 2 * 8 * 4 * 64 * 66 * 4


def test_multi_token_flag_defaults_to_false_in_all_three_constructors():
    from apertis_llm_amd import ops
    k, v = [torch.zeros(2, 4, 8)], [torch.zeros(2, 4, 8)]
    past = ((torch.randn(2, 3, 8), torch.randn(2, 3, 8)),)
    assert ops.KVCache(k, v).multi_token is False
    assert ops.KVCache.empty(1, 2, 4, 8).multi_token is False
    assert ops.KVCache.from_prefill(past, 5).multi_token is False
    assert ops.KVCache(k, v, 0, True).multi_token is True and ops.KVCache(k, v, multi_token=True).multi_token is True
    assert ops.KVCache.empty(1, 2, 4, 8, multi_token=True).multi_token is True
    c = ops.KVCache.from_prefill(past, 5, multi_token=True)
    assert c.multi_token is True and c.length == 3 and torch.equal(c[0][0], past[0][0])
    assert "a forward of several tokens extends this cache in place on the chunk kernels" in " ".join(ops.KVCache.__doc__.split())


def test_chunk_ops_refuse_cpu_tensors():
    from apertis_llm_amd import ops
    c = ops.KVCache.empty(1, 2, 8, 128, multi_token=True)
    x = torch.randn(2, 3, 128)
    with pytest.raises(ops.ApertisHipError):
        ops.kv_append_rope_chunk(x, x, x, c, 0)
    c.lengths = [3]
    with pytest.raises(ops.ApertisHipError):
        ops.attention_chunk(x, c, 0, 2)
    assert c.lengths == [3]


def _cpu_model(**kw):
    import apertis_llm_amd as A
    torch.manual_seed(0)
    base = dict(vocab_size=64, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128,
                attention_type="standard_mha", max_position_embeddings=64)
    base.update(kw)
    return A.ApertisForCausalLM(A.ApertisConfig(**base)).eval()


def test_new_kv_cache_is_sized_from_the_config():
    from apertis_llm_amd import ops
    model = _cpu_model()
    c = model.new_kv_cache(3, 20)
    assert isinstance(c, ops.KVCache) and c.multi_token and len(c) == 2 and c.capacity == 20 and c.length == 0
    assert tuple(c.k[0].shape) == (3, 20, 128) and c.dtype == torch.float32 and c.k[0].device.type == "cpu"
    assert model.new_kv_cache(1, 4, dtype=torch.bfloat16).dtype == torch.bfloat16
    with pytest.raises(ops.ApertisHipError):
        _cpu_model(attention_type="selective_ssm").new_kv_cache(1, 4)


def test_cpu_multi_token_forward_with_a_flagged_cache_runs_the_stock_branch():
    """The chunk kernels do not run on the CPU: a forward of several tokens against a multi_token cache there is the stock
    branch on its views - plain tensors back, the cache untouched, the bits of the plain-tuple past."""
    from apertis_llm_amd import ops
    model = _cpu_model()
    ids = torch.randint(4, 64, (2, 9))
    with torch.no_grad():
        past = model(input_ids=ids[:, :5], use_cache=True)[4]
        a = model(input_ids=ids[:, 5:], past_key_values=past, use_cache=True)
        cache = ops.KVCache.from_prefill(past, 16, multi_token=True)
        b = model(input_ids=ids[:, 5:], past_key_values=cache, use_cache=True)
    assert torch.equal(a[1], b[1]) and isinstance(b[4], tuple) and cache.lengths == [5, 5]


def test_generate_refuses_a_cache_it_cannot_continue():
    """Every refusal of generate(past_key_values=...): raised before any forward, never a silent prefill or fall-back."""
    from apertis_llm_amd import ops
    model = _cpu_model()
    ids = torch.randint(4, 64, (2, 6))
    forwards = []
    model.forward = lambda *a, **k: forwards.append(1)
    ok = model.new_kv_cache(2, 32)

    def refused(why, cache=ok, m=model, exc=ops.ApertisHipError, **kw):
        args = dict(input_ids=ids, max_new_tokens=4, past_key_values=cache)
        args.update(kw)
        with pytest.raises(exc, match=why):
            m.generate(**args)
    refused("no CPU path")                                                # CPU tensors, everything else in order
    refused("must be multi_token", cache=ops.KVCache.empty(2, 2, 32, 128))
    refused("takes an ops.KVCache", cache=tuple((torch.zeros(2, 0, 128), torch.zeros(2, 0, 128)) for _ in range(2)))
    refused("for 2 sequences", cache=model.new_kv_cache(3, 32))           # batch
    refused("in torch.float32", cache=model.new_kv_cache(2, 32, dtype=torch.bfloat16))          # dtype
    refused("not this model's", cache=ops.KVCache.empty(3, 2, 32, 128, multi_token=True))       # another layer count
    full = model.new_kv_cache(2, 32)
    full.lengths = [6, 6]
    refused("at most 5 may be cached", cache=full)                        # n > P - 1
    refused("need 9 rows", cache=model.new_kv_cache(2, 8))                # 6 + 4 - 1 = 9 rows needed
    refused("pixel_values", pixel_values=torch.zeros(2, 3, 8, 8))
    refused("use_cache=False", use_cache=False)
    refused("position_ids=None", position_ids=torch.arange(6).unsqueeze(0).expand(2, -1))
    refused("prefill_chunk 0", prefill_chunk=0, exc=ValueError)
    ssm = _cpu_model(attention_type="selective_ssm")
    ssm.forward = model.forward
    refused("serves standard_mha", m=ssm)                                 # not standard_mha
    with pytest.raises(ValueError):
        model.generate(input_ids=ids, max_new_tokens=4, prefill_chunk=4)  # pieces go into a cache: none given
    assert forwards == [] and ok.lengths == [0, 0] and full.lengths == [6, 6]
