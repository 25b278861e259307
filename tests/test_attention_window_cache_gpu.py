"""The sliding-window forms of the KV-cache kernels (csrc/attention_decode.hip: attn_decode_k / attn_chunk_k with WIN;
apertis_attention_decode_window_at, apertis_attention_chunk_window of include/apertis_hip_ext.h), through ops:

  1. decode at a device-held length under a window: the bits of ops.attention_decode(window=, splits=) on the same rows; with
     more pieces than keys, the by-value bars of test_attention_at_with_empty_pieces_holds_the_by_value_bars
  2. nothing outside the window is read: K / V rows before `begin` and from Lk on are NaN, their validity columns say "attend"
  3. ONE captured step {append at dev_len, windowed attention, dev_len += 1} replayed across the window edge
  4. the chunk kernel under a window at one split: the bits ops.window_attention gives rows [n:] of the whole sequence
  5. other split counts at the fp64 / stock-SDPA bars, determinism, splits=0 is the rule's count at min(Lk, W + Lq) keys
  6. nothing in front of the chunk's window is read
  7. dead rows are filled as ops.window_attention(dead_rows=True) fills them

Shapes: B 2, H 2, D 64 and 128, fp32 and bf16."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_error_report

pytestmark = pytest.mark.gpu

NAN = float("nan")
B, H = 2, 2
CAP = 300
WINDOWS = [1, 5, 33, 130, 300, 1000]
TYPES = [(64, torch.float32), (128, torch.float32), (64, torch.bfloat16), (128, torch.bfloat16)]
TYPE_IDS = ["D64-fp32", "D128-fp32", "D64-bf16", "D128-bf16"]


def _lks(W):
    return sorted({Lk for Lk in (1, W - 1, W, W + 1, 257, 300) if 1 <= Lk <= CAP})


def _name(dtype):
    return str(dtype).split(".")[-1]


# ------------------------------------------------------------------------------------------------ 1.-3. decode
def _decode_case(ops, dev, D, Lk, W, dtype, masked, poison_outside=False):
    """q [B, H*D]; a one-layer cache of CAP rows that holds Lk, rows >= Lk NaN; the step state under window W with the device
    length at Lk - 1 (the step's own row is in).  masked: every third key of sequence B-1 blanked, the newest key kept (holes
    INSIDE the window wherever it is wider than two keys), the blanked rows NaN.  poison_outside: K / V rows before begin =
    max(Lk - W, 0) are NaN too and every validity column before `begin` and from Lk on says "attend"."""
    Wd = H * D
    gen = torch.Generator(device=dev).manual_seed(1000 * Lk + 7 * min(W, 999) + D + (3 if masked else 0))
    q = torch.randn(B, Wd, device=dev, generator=gen).to(dtype)
    k = torch.full((B, CAP, Wd), NAN, device=dev, dtype=dtype)
    v = torch.full((B, CAP, Wd), NAN, device=dev, dtype=dtype)
    k[:, :Lk] = torch.randn(B, Lk, Wd, device=dev, generator=gen).to(dtype)
    v[:, :Lk] = torch.randn(B, Lk, Wd, device=dev, generator=gen).to(dtype)
    valid = torch.ones(B, Lk, dtype=torch.bool, device=dev)
    if masked:
        valid[B - 1] = torch.arange(Lk, device=dev) % 3 != 1
        valid[:, Lk - 1] = True
        k[:, :Lk][~valid] = NAN
        v[:, :Lk][~valid] = NAN
    cache = ops.KVCache([k], [v], length=Lk)
    cache.step_state_begin(H, valid.long() if masked else None, window=W)
    assert cache.step_window == W and cache.dev_valid.shape == (B, CAP) and bool((cache.dev_valid[:, Lk:] == 1).all())
    cache.dev_len.fill_(Lk - 1)
    begin = max(Lk - W, 0)
    if poison_outside:
        k[:, :begin] = NAN
        v[:, :begin] = NAN
        cache.dev_valid[:, :begin] = 1
    return q, cache, (valid.long() if masked else None), valid, begin


def _decode_ref64(q, cache, Lk, begin, valid):
    """fp64 explicit softmax over the window's keys [begin, Lk) (masked rows' poison replaced by zeros), and those rows."""
    k, v = cache.k[0][:, begin:Lk].clone(), cache.v[0][:, begin:Lk].clone()
    ok = valid[:, begin:Lk]
    k[~ok] = 0
    v[~ok] = 0
    n, D = Lk - begin, q.shape[1] // H
    qh, kh, vh = q.double().view(B, H, D), k.double().view(B, n, H, D), v.double().view(B, n, H, D)
    s = torch.einsum("bhd,bjhd->bhj", qh, kh) * (1.0 / float(np.sqrt(np.float32(D))))
    s = s.masked_fill(~ok[:, None, :], float("-inf"))
    return torch.einsum("bhj,bjhd->bhd", torch.softmax(s, dim=-1), vh).reshape(B, H * D), k, v, ok


def _decode_sdpa(q, k, v, ok):
    n, D = k.shape[1], q.shape[1] // H
    qh = q.view(B, 1, H, D).transpose(1, 2)
    kh, vh = k.view(B, n, H, D).transpose(1, 2), v.view(B, n, H, D).transpose(1, 2)
    return F.scaled_dot_product_attention(qh, kh, vh, attn_mask=ok[:, None, None, :]).transpose(1, 2).reshape(B, H * D)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("D,dtype", TYPES, ids=TYPE_IDS)
def test_decode_window_at_gives_the_by_value_window_bits(dev, D, dtype, masked):
    """For the same Lk, window and split count: torch.equal with ops.attention_decode(window=W, splits=n), the same kernel on
    pointers offset by begin.  More pieces than keys in the window (the by-value form refuses the count): finite and at the
    by-value bars - fp32 against an fp64 softmax over the window at rtol 1e-4, bf16 within twice stock bf16 SDPA's error
    plus 1e-6 of the reference's magnitude."""
    from apertis_llm_amd import ops
    n_equal = n_bars = 0
    for W in WINDOWS:
        for Lk in _lks(W):
            q, cache, kv, valid, begin = _decode_case(ops, dev, D, Lk, W, dtype, masked)
            for n in (1, 3, 8):
                got = ops.attention_decode_at(q, cache, 0, H, splits=n)
                assert got.shape == q.shape and got.dtype == dtype and torch.isfinite(got).all(), (W, Lk, n)
                if n <= min(Lk, W):
                    want = ops.attention_decode(q, cache, 0, H, kv, splits=n, window=W)
                    assert torch.equal(got, want), (W, Lk, n)
                    n_equal += 1
                    continue
                with pytest.raises(ops.ApertisHipError):
                    ops.attention_decode(q, cache, 0, H, kv, splits=n, window=W)
                ref, k, v, ok = _decode_ref64(q, cache, Lk, begin, valid)
                tag = f"attention_decode_window_at empty pieces {_name(dtype)} D{D} W{W} Lk{Lk} splits{n} mask{int(masked)}"
                if dtype == torch.float32:
                    rel_error_report(tag, got, ref, rtol=1e-4)
                else:
                    rep = rel_error_report(tag, got, ref, check=False)
                    srep = rel_error_report("stock SDPA " + tag, _decode_sdpa(q, k, v, ok), ref, check=False)
                    assert rep["max_abs"] <= 2 * srep["max_abs"] + 1e-6 * rep["ref_absmax"], (rep, srep)
                n_bars += 1
            assert cache.lengths == [Lk]
            cache.step_state_end(Lk)
            assert cache.step_window is None and not cache.step_active
    assert n_equal > 60 and n_bars >= 10, (n_equal, n_bars)


@pytest.mark.parametrize("D,dtype", TYPES, ids=TYPE_IDS)
def test_decode_window_at_reads_nothing_outside_the_window(dev, D, dtype):
    """K / V rows [0, begin) and [Lk, cap) are NaN and every validity column there says "attend": the output is finite and has
    the bits of the run on a cache whose rows before `begin` are ordinary numbers."""
    from apertis_llm_amd import ops
    checked = 0
    for W in WINDOWS:
        for Lk in _lks(W):
            for masked in (False, True):
                q, clean, _, _, begin = _decode_case(ops, dev, D, Lk, W, dtype, masked)
                q2, dirty, _, _, _ = _decode_case(ops, dev, D, Lk, W, dtype, masked, poison_outside=True)
                assert torch.equal(q, q2)
                if begin:
                    assert torch.isnan(dirty.k[0][:, :begin]).all() and torch.isnan(dirty.v[0][:, :begin]).all()
                    assert bool((dirty.dev_valid[:, :begin] == 1).all()) and torch.isfinite(clean.k[0][0, :begin]).all()
                for n in (1, 3, 8):
                    got = ops.attention_decode_at(q, dirty, 0, H, splits=n)
                    assert torch.isfinite(got).all(), (W, Lk, n, masked)
                    assert torch.equal(got, ops.attention_decode_at(q, clean, 0, H, splits=n)), (W, Lk, n, masked)
                    checked += begin > 0
    assert checked >= 60, checked


@pytest.mark.parametrize("D,dtype", TYPES, ids=TYPE_IDS)
def test_one_captured_windowed_step_replays_across_the_window_edge(dev, D, dtype):
    """ONE graph of {kv_append_rope_at, attention_decode_at under W 33 with 4 pieces, dev_len += 1} on one stream, captured and
    then replayed from dev_len = 29 for 8 steps (Lk 30 .. 37: begin leaves 0 at the fifth): every step's output is the bits of
    the eager by-value append + attention_decode(window=33, splits=4) on a second cache fed the same rows."""
    import apertis_llm_amd as A
    from apertis_llm_amd import ops
    Wd, n0, steps, W = H * D, 29, 8, 33
    rope = A.model.RotaryEmbedding(Wd, 512).to(dev)
    cos, sin = rope.cos_cached, rope.sin_cached
    gen = torch.Generator(device=dev).manual_seed(33 + D)
    rows = torch.randn(2, B, n0, Wd, device=dev, generator=gen).to(dtype)

    def cache():
        k = torch.full((B, CAP, Wd), NAN, device=dev, dtype=dtype)
        v = torch.full((B, CAP, Wd), NAN, device=dev, dtype=dtype)
        k[:, :n0], v[:, :n0] = rows[0], rows[1]
        return ops.KVCache([k], [v], length=n0)
    a, b = cache(), cache()
    mask = torch.ones(B, CAP, dtype=torch.long, device=dev)
    mask[B - 1, 1:CAP:3] = 0                                        # (holes inside every window of the run)
    a.step_state_begin(H, mask, splits=4, window=W)
    s_q, s_k, s_v = (torch.zeros(B, Wd, device=dev, dtype=dtype) for _ in range(3))
    s_out = torch.zeros(B, Wd, device=dev, dtype=dtype)

    def step():
        qr = ops.kv_append_rope_at(s_q, s_k, s_v, a, 0, cos, sin)
        s_out.copy_(ops.attention_decode_at(qr, a, 0, H))
        a.dev_len.add_(1)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        step()                                                      # warm-up (row 29 is rewritten by the first replay)
    torch.cuda.current_stream(dev).wait_stream(side)
    a.dev_len.fill_(n0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    a.dev_len.fill_(n0)
    for i in range(steps):
        qkv = torch.randn(3, B, Wd, device=dev, generator=gen).to(dtype)
        s_q.copy_(qkv[0]), s_k.copy_(qkv[1]), s_v.copy_(qkv[2])
        graph.replay()
        qr = ops.kv_append_rope(qkv[0], qkv[1], qkv[2], b, 0, n0 + i, cos, sin)
        want = ops.attention_decode(qr, b, 0, H, mask, splits=4, window=W)
        assert torch.isfinite(s_out).all() and torch.equal(s_out, want), i
    assert int(a.dev_err) == 0 and int(a.dev_len) == 37 == b.length
    assert torch.equal(a.k[0][:, :37], b.k[0][:, :37]) and torch.equal(a.v[0][:, :37], b.v[0][:, :37])


# ------------------------------------------------------------------------------------------------ 4.-7. chunk
CHUNKS = [(0, 70, 40), (35, 21, 40), (100, 5, 33), (100, 70, 1), (64, 64, 32), (37, 130, 64), (56, 8, 64), (200, 17, 1000)]


@functools.lru_cache(maxsize=None)
def _chunk_case(D, n, Lq, W, dtype, masked):
    """The whole sequence q, k, v [B, n + Lq, H*D] (what window_attention takes), a cache of n + Lq + 5 rows that holds them
    (rows past n + Lq and the rows of masked keys NaN, mask columns past n + Lq nonzero garbage), the key mask with about 30 %
    scattered zeros (key 0 valid), the fp64 explicit softmax of the chunk's rows under the window - a row without any allowed
    key is zeros, as the kernels leave it - and the allow mask.  Built once per case and shared, never written to."""
    dev = torch.device("cuda:0")
    Wd, Lk = H * D, n + Lq
    cap = Lk + 5
    gen = torch.Generator(device=dev).manual_seed(1000 * n + 10 * Lq + D + min(W, 999) + (5 if masked else 0))
    q, k, v = (torch.randn(B, Lk, Wd, device=dev, generator=gen).to(dtype) for _ in range(3))
    kc = torch.full((B, cap, Wd), NAN, device=dev, dtype=dtype)
    vc = torch.full((B, cap, Wd), NAN, device=dev, dtype=dtype)
    kc[:, :Lk], vc[:, :Lk] = k, v
    kv = valid = None
    if masked:
        valid = torch.rand(B, Lk, device=dev, generator=gen) >= 0.3
        valid[:, 0] = True
        kv = torch.full((B, cap), 77, dtype=torch.long, device=dev)
        kv[:, :Lk] = valid.long()
        kc[:, :Lk][~valid] = NAN
        vc[:, :Lk][~valid] = NAN
    pos, key = (n + torch.arange(Lq, device=dev))[:, None], torch.arange(Lk, device=dev)[None, :]
    allow = ((key <= pos) & (pos - key < W))[None, None].expand(B, 1, Lq, Lk)
    if valid is not None:
        allow = allow & valid[:, None, None, :]
    live = allow.any(-1)                                                     # [B, 1, Lq]
    kz, vz = (k, v) if valid is None else (k.masked_fill(~valid[:, :, None], 0), v.masked_fill(~valid[:, :, None], 0))
    qh = q[:, n:].double().view(B, Lq, H, D)
    kh, vh = kz.double().view(B, Lk, H, D), vz.double().view(B, Lk, H, D)
    s = torch.einsum("bihd,bjhd->bhij", qh, kh) * (1.0 / float(np.sqrt(np.float32(D))))
    s = s.masked_fill(~allow, float("-inf")).masked_fill(~live[..., None], 0.0)
    ref = torch.einsum("bhij,bjhd->bihd", torch.softmax(s, dim=-1), vh) * live.transpose(1, 2)[..., None]
    hd = lambda t: t.view(B, t.shape[1], H, D).transpose(1, 2)      # noqa: E731
    sdpa = F.scaled_dot_product_attention(hd(q[:, n:]), hd(kz), hd(vz), attn_mask=allow | ~live[..., None])
    sdpa = (sdpa * live[..., None]).transpose(1, 2).reshape(B, Lq, Wd)
    return dict(q=q, k=k, v=v, kc=kc, vc=vc, kv=kv, valid=valid, ref=ref.reshape(B, Lq, Wd), sdpa=sdpa)


def _cache(ops, c, n, Lq, kc=None, vc=None):
    return ops.KVCache([c["kc"] if kc is None else kc], [c["vc"] if vc is None else vc], length=n + Lq)


def _launches(ops, fn):
    timer = ops.KernelTimer(("apertis_attention_chunk", "apertis_attention_chunk_window"))
    ops.set_kernel_timer(timer)
    try:
        out = fn()
    finally:
        ops.set_kernel_timer(None)
    return out, [r[0] for r in timer.records]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("D,dtype", TYPES, ids=TYPE_IDS)
def test_chunk_window_at_one_split_gives_the_bits_of_window_attention(dev, D, dtype, masked):
    """Tiles are aligned at multiples of 32 from key 0 in both kernels and a tile with no key valid for a row is a no-op for
    that row: row i of the chunk has the bits ops.window_attention gives row n + i of the whole sequence.  With W >= n + Lq
    the call is the plain ops.attention_chunk, launch and bits."""
    from apertis_llm_amd import ops
    for n, Lq, W in CHUNKS:
        c = _chunk_case(D, n, Lq, W, dtype, masked)
        q = c["q"][:, n:]
        got, names = _launches(ops, lambda: ops.attention_chunk(q, _cache(ops, c, n, Lq), 0, H, c["kv"], splits=1, window=W))
        assert got.shape == q.shape and got.dtype == dtype and torch.isfinite(got).all(), (n, Lq, W)
        whole = ops.window_attention(c["q"], c["k"], c["v"], H, W, None if c["valid"] is None else c["valid"].long())
        assert torch.equal(got, whole[:, n:]), (n, Lq, W)
        if W >= n + Lq:
            assert names == ["apertis_attention_chunk"]
            assert torch.equal(got, ops.attention_chunk(q, _cache(ops, c, n, Lq), 0, H, c["kv"], splits=1)), (n, Lq, W)
            # ... and the window entry point itself, handed a window that wide, has those bits too
            direct = _chunk_window_direct(ops, q, _cache(ops, c, n, Lq), c["kv"], W, 1)
            assert torch.equal(got, direct), (n, Lq, W)
        else:
            assert names == ["apertis_attention_chunk_window"]


def _chunk_window_direct(ops, q, cache, kv, W, splits):
    """apertis_attention_chunk_window through the binding, whatever the window (ops.attention_chunk takes the plain call when
    the window covers every key)."""
    from apertis_llm_amd import _lib
    kc, vc = cache.k[0], cache.v[0]
    Bq, Lq, Wd = q.shape
    q = q.contiguous()
    out = torch.empty_like(q)
    nbytes = ops.attention_chunk_workspace_bytes(Bq, H, Lq, Wd // H, splits)
    ws = torch.empty(max(nbytes, 16) // 4, dtype=torch.float32, device=q.device)
    rc = _lib.load().apertis_attention_chunk_window(
        q.data_ptr(), Wd, kc.data_ptr(), kc.stride(1), kc.stride(0), vc.data_ptr(), vc.stride(1), vc.stride(0), kc.shape[1],
        None if kv is None else kv.data_ptr(), 0 if kv is None else kv.stride(0), out.data_ptr(), Wd, ws.data_ptr(), Bq, Lq,
        cache.length - Lq, W, H, Wd // H, splits, ops.dtype_code(q), ops.stream_ptr())
    assert rc == 0
    return out


@pytest.mark.parametrize("D,dtype", TYPES, ids=TYPE_IDS)
def test_chunk_window_other_split_counts_hold_the_bars_and_repeat(dev, D, dtype):
    """2, 5 and 64 runs of every wave's tiles [first, last] (most of 64 are empty): fp32 against the fp64 softmax under the
    window at rtol 1e-4, bf16 within twice stock bf16 SDPA's error plus 1e-6 of the reference's magnitude; the same bits on a
    second call; splits=0 is the rule's count at min(n + Lq, W + Lq) keys."""
    from apertis_llm_amd import ops
    rule_counts = set()
    for n, Lq, W in CHUNKS:
        for masked in (False, True):
            c = _chunk_case(D, n, Lq, W, dtype, masked)
            q, ref = c["q"][:, n:], c["ref"]
            sbase = rel_error_report(f"stock SDPA chunk window {_name(dtype)} D{D} n{n} Lq{Lq} W{W}", c["sdpa"], ref, check=False)
            for s_ in (2, 5, ops.ATTN_DECODE_MAX_SPLITS):
                cache = _cache(ops, c, n, Lq)
                a = ops.attention_chunk(q, cache, 0, H, c["kv"], splits=s_, window=W)
                b = ops.attention_chunk(q, cache, 0, H, c["kv"], splits=s_, window=W)
                assert torch.isfinite(a).all() and torch.equal(a, b), (n, Lq, W, s_)
                tag = f"attention_chunk window splits {s_} {_name(dtype)} D{D} n{n} Lq{Lq} W{W} mask{int(masked)}"
                if dtype == torch.float32:
                    rel_error_report(tag, a, ref, rtol=1e-4)
                else:
                    rep = rel_error_report(tag, a, ref, check=False)
                    assert rep["max_abs"] <= 2 * sbase["max_abs"] + 1e-6 * rep["ref_absmax"], (tag, rep, sbase)
            rule = ops.attention_chunk_splits(B, H, Lq, min(n + Lq, W + Lq), D)
            assert rule == max(1, min(2048 // (B * H * -(-Lq // 16)), min(n + Lq, W + Lq) // 64, 64))
            rule_counts.add(rule)
            auto = ops.attention_chunk(q, _cache(ops, c, n, Lq), 0, H, c["kv"], window=W)
            assert torch.equal(auto, ops.attention_chunk(q, _cache(ops, c, n, Lq), 0, H, c["kv"], splits=rule, window=W)), (n, Lq, W)
    assert len(rule_counts) > 1, rule_counts                                 # the rule's count is not always one here
    with pytest.raises(ValueError):
        ops.attention_chunk(q, _cache(ops, c, n, Lq), 0, H, c["kv"], window=0)


@pytest.mark.parametrize("D,dtype", TYPES, ids=TYPE_IDS)
def test_chunk_window_reads_nothing_in_front_of_the_window(dev, D, dtype):
    """The shapes with n >= W: K / V rows [0, n - W + 1) - in front of the first key the chunk's first row sees - are NaN and
    key_valid says "attend" there: the output is finite and has the bits of the unpoisoned run, at one split and at five."""
    from apertis_llm_amd import ops
    shapes = [(n, Lq, W) for n, Lq, W in CHUNKS if n >= W]
    assert len(shapes) == 3
    for n, Lq, W in shapes:
        for masked in (False, True):
            c = _chunk_case(D, n, Lq, W, dtype, masked)
            q, front = c["q"][:, n:], n - W + 1
            kc, vc = c["kc"].clone(), c["vc"].clone()
            kc[:, :front] = NAN
            vc[:, :front] = NAN
            kv = torch.ones(B, n + Lq + 5, dtype=torch.long, device=dev) if c["kv"] is None else c["kv"].clone()
            kv[:, :front] = 1
            for s_ in (1, 5):
                want = ops.attention_chunk(q, _cache(ops, c, n, Lq), 0, H, c["kv"], splits=s_, window=W)
                got = ops.attention_chunk(q, _cache(ops, c, n, Lq, kc, vc), 0, H, kv, splits=s_, window=W)
                assert torch.isfinite(got).all() and torch.equal(got, want), (n, Lq, W, masked, s_)


@pytest.mark.parametrize("D,dtype", TYPES, ids=TYPE_IDS)
def test_chunk_window_fills_dead_rows_as_window_attention_does(dev, D, dtype):
    """Left padding that reaches into the chunk (n 35, Lq 21, W 40, row 0 padded by 40 keys): rows 35 .. 39 of sequence 0 have
    no valid key at or before them and get attention_dead_rows over [0, n + Lq), the bits of window_attention(dead_rows=True)."""
    from apertis_llm_amd import ops
    n, Lq, W = 35, 21, 40
    c = _chunk_case(D, n, Lq, W, dtype, False)
    kv = torch.ones(B, n + Lq, dtype=torch.long, device=dev)
    kv[0, :40] = 0
    got = ops.attention_chunk(c["q"][:, n:], _cache(ops, c, n, Lq), 0, H, kv, splits=1, dead_rows=True, window=W)
    want = ops.window_attention(c["q"], c["k"], c["v"], H, W, kv, dead_rows=True)[:, n:]
    plain = ops.attention_chunk(c["q"][:, n:], _cache(ops, c, n, Lq), 0, H, kv, splits=1, window=W)
    assert torch.isfinite(got).all() and torch.equal(got, want)
    assert bool((plain[0, :5] == 0).all()) and bool((got[0, :5] != 0).any()) and torch.equal(got[0, 5:], plain[0, 5:])
