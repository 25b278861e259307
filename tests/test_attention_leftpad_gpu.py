"""Left-padded standard_mha batches on the HIP kernels (ops.ATTN_LEFT_PAD; csrc/attention_deadrows.hip,
ops.attention_dead_rows, the dead_rows flag of ops.causal_attention / ops.attention_chunk), everything through the C ABI via ops:

  1. the fill kernel alone: dead rows are the fp64 column mean of V, every other row keeps its bits, two runs agree
  2. causal_attention(dead_rows=True) against fp64 (masked softmax on live rows, column mean on dead ones)
  3. attention_chunk(dead_rows=True) against fp64, one run and three; the bits of causal_attention at n = 0 and one run
  4. a model forward: the kernels run; the valid rows' logits and cache are the GPU stock run's, and every row's, pad rows
     included, are those of the same weights' stock forward on the CPU (on the GPU torch's memory-efficient SDPA gives a
     dead row zeros, not the reference's average: the test's docstring)
  5. generate(), eager: every token step on the decode kernels, the stock run's tokens
  6. generate() through the graph tail
  7. generate() from the caller's KVCache in pieces of 8 tokens, one of them wholly inside a sequence's padding
  8. what stays on the stock path: autograd, train mode, a sequence without a valid key

A DEAD row is a query row with no valid key at or before its own position.  The reference adds finfo.min for the causal and
the padding mask, so all scores of such a row saturate to one value and its softmax is uniform over all Lk keys.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_error_report

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture
def ops():
    from apertis_llm_amd import ops
    prev = ops.ATTN_FUSED, ops.ATTN_DECODE_FUSED, ops.ATTN_DECODE_GRAPH, ops.ATTN_LEFT_PAD
    yield ops
    ops.ATTN_FUSED, ops.ATTN_DECODE_FUSED, ops.ATTN_DECODE_GRAPH, ops.ATTN_LEFT_PAD = prev


def _spy(monkeypatch, owner, name):
    """Count the calls of owner.<name> (the model looks its ops up on the package at call time; causal_attention and
    attention_chunk look attention_dead_rows up in ops.attention)."""
    calls = []
    real = getattr(owner, name)

    def spy(*a, **k):
        calls.append(tuple(a[0].shape))
        return real(*a, **k)
    monkeypatch.setattr(owner, name, spy)
    return calls


def _dead(valid, n, Lq):
    """[B, Lq] bool: row i (key position n + i) has no valid key j <= n + i."""
    seen = valid.bool().cumsum(1) > 0
    return ~seen[:, n:n + Lq]


# ------------------------------------------------------------------------------------------------ 1. the fill kernel
# first_valid of the padded sequence per (n, Lq): 5 left pads of a whole sequence; 9 = inside the chunk (7, 5), whose cached
# keys are then all masked; 45 = dead rows 0..4 of the chunk (40, 70)
NLQ_FILL = {(0, 37): 5, (0, 100): 5, (7, 5): 9, (40, 70): 45}


def _fill_mask(n, Lq, cap, dev):
    """One mask per sequence: nothing padded; left pads up to first_valid; keys [0, n + 3) and n + 4 masked with n + 3
    valid (dead rows 0..2 only); everything masked.  Columns >= n + Lq hold nonzero garbage: they are never read."""
    Lk = n + Lq
    kv = torch.full((4, cap + 2), 77, dtype=torch.long, device=dev)
    kv[:, :Lk] = 1
    kv[1, :NLQ_FILL[(n, Lq)]] = 0
    kv[2, :n + 3] = 0
    kv[2, n + 4] = 0
    kv[3, :Lk] = 0
    return kv


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n,Lq", list(NLQ_FILL))
@pytest.mark.parametrize("W", [128, 384])
def test_fill_kernel_alone(dev, ops, W, n, Lq, dtype):
    """V [4, cap, W] cut out of a larger buffer (batch stride (cap + 3) * W), its rows >= n + Lq NaN; values around 3 so that
    no column mean is zero to rounding and the fp32 bar is a plain elementwise rtol.  fp32: rtol 1e-5 against the fp64 mean
    (an fp32 sum of <= 110 terms of one sign is good to a few 1e-7).  bf16: within one bf16 ulp of the fp64 mean rounded to
    bf16 (the fp32 mean is rounded once; it can fall on the other side of a rounding boundary than the fp64 one)."""
    B, Lk = 4, n + Lq
    cap = Lk + 5
    gen = torch.Generator(device=dev).manual_seed(100 * n + Lq + W)
    vfull = torch.full((B, cap + 3, W), NAN, device=dev, dtype=dtype)
    v = vfull[:, :cap]
    v[:, :Lk] = (torch.randn(B, Lk, W, device=dev, generator=gen) + 3.0).to(dtype)
    assert v.stride(0) == (cap + 3) * W
    kv = _fill_mask(n, Lq, cap, dev)
    dead = _dead(kv[:, :Lk], n, Lq)
    assert dead[0].sum() == 0 and dead[1].sum() == NLQ_FILL[(n, Lq)] - n and dead[2].sum() == 3 and dead[3].all()
    poison = torch.randn(B, Lq, W, device=dev, generator=gen).to(dtype)
    out = poison.clone()
    assert ops.attention_dead_rows(out, v, kv, n) is out
    ref = v[:, :Lk].double().mean(1)[:, None, :].expand(B, Lq, W)
    assert torch.equal(out[~dead], poison[~dead])                         # every other row: untouched, bit for bit
    got, want = out[dead], ref[dead]
    assert torch.isfinite(got).all()
    if dtype == torch.float32:
        err = float(((got.double() - want).abs() / want.abs()).max())
        print(f"fill fp32 W{W} n{n} Lq{Lq}: max rel err {err:.3e}")
        assert err <= 1e-5
    else:
        want_bf = want.to(torch.bfloat16).double()
        ulp = torch.exp2(torch.floor(torch.log2(want_bf.abs())) - 7)
        err = float(((got.double() - want_bf).abs() / ulp).max())
        print(f"fill bf16 W{W} n{n} Lq{Lq}: max err {err:.2f} ulp, {int((got.double() != want_bf).sum())} of {got.numel()} differ")
        assert err <= 1.0
    again = poison.clone()
    ops.attention_dead_rows(again, v, kv, n)
    assert torch.equal(again, out)


def test_fill_checks_its_arguments(dev, ops):
    v = torch.zeros(2, 12, 128, device=dev)
    out = torch.zeros(2, 5, 128, device=dev)
    kv = torch.ones(2, 12, dtype=torch.long, device=dev)
    ops.attention_dead_rows(out, v, kv, 7)
    for bad in (lambda: ops.attention_dead_rows(out, v, kv, 8),                          # v and mask end before n + Lq
                lambda: ops.attention_dead_rows(out, v, kv[:, :11], 7),
                lambda: ops.attention_dead_rows(out, v, None, 7),
                lambda: ops.attention_dead_rows(out, v.bfloat16(), kv, 7),
                lambda: ops.attention_dead_rows(out, v[:, :, :64], kv, 7),
                lambda: ops.attention_dead_rows(torch.zeros(2, 5, 256, device=dev)[:, :, ::2], v, kv, 7),   # not writable in place
                lambda: ops.attention_dead_rows(out.cpu(), v.cpu(), kv.cpu(), 7)):
        with pytest.raises(ops.ApertisHipError):
            bad()


# ------------------------------------------------------------------------------------------------ 2. causal_attention
def _ref_fp64(q, k, v, H, valid, n):
    """The reference's semantics in fp64: finfo.min (not -inf) where the causal or the padding mask forbids, so a dead row's
    softmax is uniform over all keys.  q: the chunk's rows [B, Lq, W]; k, v: [B, n + Lq, W]."""
    B, Lq, W = q.shape
    Lk, D = k.shape[1], W // H
    qh = q.double().view(B, Lq, H, D)
    kh, vh = k.double().view(B, Lk, H, D), v.double().view(B, Lk, H, D)
    s = torch.einsum("bihd,bjhd->bhij", qh, kh) * (1.0 / float(np.sqrt(np.float32(D))))
    allow = (torch.arange(Lk, device=q.device)[None, :] <= (n + torch.arange(Lq, device=q.device))[:, None])[None, None]
    allow = allow & valid.bool()[:, None, None, :]
    s = s.masked_fill(~allow, torch.finfo(torch.float64).min)
    return torch.einsum("bhij,bjhd->bihd", torch.softmax(s, dim=-1), vh).reshape(B, Lq, W), allow


def _stock_sdpa(q, k, v, H, allow):
    """Stock SDPA as the model's stock branch calls it: the additive mask of _prepare_decoder_attention_mask."""
    B, Lq, W = q.shape
    D = W // H
    hd = lambda t: t.view(B, t.shape[1], H, D).transpose(1, 2)      # noqa: E731
    add = (1.0 - allow.to(q.dtype)) * torch.finfo(q.dtype).min
    return F.scaled_dot_product_attention(hd(q), hd(k), hd(v), attn_mask=add).transpose(1, 2).reshape(B, Lq, W)


def _hold(name, got, ref, stock, dtype):
    """fp32: test_attention_fp32_matches_fp64's bar.  bf16: test_attention_bf16_within_twice_stock_sdpa_error's rule."""
    if dtype == torch.float32:
        rel_error_report(name, got, ref, rtol=1e-4)
    else:
        rep = rel_error_report(name, got, ref, check=False)
        srep = rel_error_report("stock SDPA " + name, stock(), ref, check=False)
        assert rep["max_abs"] <= 2 * srep["max_abs"] + 1e-6 * rep["ref_absmax"], (rep, srep)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,L,H,D", [(3, 100, 2, 64), (3, 37, 3, 128)])
def test_causal_attention_dead_rows_match_fp64(dev, ops, B, L, H, D, dtype):
    """Pads 0, 5 and 70 (a whole 64-row work-group of dead rows at L = 100; the whole sequence at L = 37)."""
    gen = torch.Generator(device=dev).manual_seed(L + D)
    q, k, v = (torch.randn(B, L, H * D, device=dev, generator=gen).to(dtype) for _ in range(3))
    kv = torch.ones(B, L, dtype=torch.long, device=dev)
    for b, pad in enumerate((0, 5, 70)):
        kv[b, :pad] = 0
    dead = _dead(kv, 0, L)
    assert dead.sum() == 5 + min(70, L)
    ref, allow = _ref_fp64(q, k, v, H, kv, 0)
    assert torch.allclose(ref[dead], v.double().mean(1)[:, None].expand(B, L, H * D)[dead], rtol=1e-12, atol=1e-14)
    got = ops.causal_attention(q, k, v, H, kv, dead_rows=True)
    tag = f"causal_attention dead_rows {str(dtype).split('.')[-1]} L{L} D{D}"
    _hold(tag, got, ref, lambda: _stock_sdpa(q, k, v, H, allow), dtype)
    _hold(tag + " (dead rows only)", got[dead], ref[dead], lambda: _stock_sdpa(q, k, v, H, allow)[dead], dtype)
    # without the flag: the same kernel, zeros on the dead rows, the same bits elsewhere
    plain = ops.causal_attention(q, k, v, H, kv)
    assert bool((plain[dead] == 0).all()) and torch.equal(plain[~dead], got[~dead])
    assert torch.equal(ops.causal_attention(q, k, v, H, kv, dead_rows=True), got)
    # inference only
    for i in range(3):
        ts = [t.clone().requires_grad_(j == i) for j, t in enumerate((q, k, v))]
        with pytest.raises(ops.ApertisHipError):
            ops.causal_attention(*ts, H, kv, dead_rows=True)
        with torch.no_grad():
            assert torch.equal(ops.causal_attention(*ts, H, kv, dead_rows=True), got)
    with pytest.raises(ops.ApertisHipError):
        ops.causal_attention(q, k, v, H, kv, 0.1, training=True, dead_rows=True)


# ------------------------------------------------------------------------------------------------ 3. attention_chunk
@functools.lru_cache(maxsize=None)
def _chunk_case(n, Lq, dtype):
    """B 3, H 2, D 64: the whole sequence q, k, v [B, n + Lq, W], the cache buffers cut out of larger ones (batch stride
    (cap + 3) * W, rows >= n + Lq NaN, the k rows of masked keys NaN), the mask [B, cap + 2] (garbage beyond n + Lq) and the
    fp64 reference of the chunk's rows.  Left pads 0, n + 3 (dead rows 0..2 of the chunk) and 3 (dead rows only at n = 0).
    Built once per case and shared, never written to."""
    dev = torch.device("cuda:0")
    B, H, D = 3, 2, 64
    W, Lk = H * D, n + Lq
    cap = Lk + 5
    gen = torch.Generator(device=dev).manual_seed(1000 * n + Lq)
    q, k, v = (torch.randn(B, Lk, W, device=dev, generator=gen).to(dtype) for _ in range(3))
    valid = torch.ones(B, Lk, dtype=torch.bool, device=dev)
    valid[1, :n + 3] = False
    valid[2, :3] = False
    kfull = torch.full((B, cap + 3, W), NAN, device=dev, dtype=dtype)
    vfull = torch.full((B, cap + 3, W), NAN, device=dev, dtype=dtype)
    kc, vc = kfull[:, :cap], vfull[:, :cap]
    kc[:, :Lk], vc[:, :Lk] = k, v
    kc[:, :Lk][~valid] = NAN
    kv = torch.full((B, cap + 2), 77, dtype=torch.long, device=dev)
    kv[:, :Lk] = valid.long()
    ref, allow = _ref_fp64(q[:, n:], k, v, H, valid, n)
    return dict(q=q, k=k, v=v, kc=kc, vc=vc, kv=kv, valid=valid, ref=ref, allow=allow, dead=_dead(valid, n, Lq), H=H)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("Lq", [5, 70])
@pytest.mark.parametrize("n", [0, 7, 40])
def test_attention_chunk_dead_rows_match_fp64(dev, ops, n, Lq, splits, dtype):
    c = _chunk_case(n, Lq, dtype)
    H, dead = c["H"], c["dead"]
    assert dead[0].sum() == 0 and dead[1].sum() == 3 and dead[2].sum() == (3 if n == 0 else 0)
    q = c["q"][:, n:]
    cache = lambda: ops.KVCache([c["kc"]], [c["vc"]], length=n + Lq)      # noqa: E731
    got = ops.attention_chunk(q, cache(), 0, H, c["kv"], splits=splits, dead_rows=True)
    assert torch.isfinite(got).all()
    tag = f"attention_chunk dead_rows {str(dtype).split('.')[-1]} n{n} Lq{Lq} splits{splits}"
    stock = lambda: _stock_sdpa(q, c["k"], c["v"], H, c["allow"])          # noqa: E731
    _hold(tag, got, c["ref"], stock, dtype)
    _hold(tag + " (dead rows only)", got[dead], c["ref"][dead], lambda: stock()[dead], dtype)
    plain = ops.attention_chunk(q, cache(), 0, H, c["kv"], splits=splits)
    assert bool((plain[dead] == 0).all()) and torch.equal(plain[~dead], got[~dead])
    assert torch.equal(ops.attention_chunk(q, cache(), 0, H, c["kv"], splits=splits, dead_rows=True), got)
    if splits == 1:
        # one run: the bits of the forward over the whole sequence on the chunk's rows, dead ones included
        whole = ops.causal_attention(c["q"], c["k"], c["v"], H, c["valid"].long(), dead_rows=n == 0)
        rows = torch.ones_like(dead) if n == 0 else ~dead
        assert torch.equal(got[rows], whole[:, n:][rows])
    with pytest.raises(ops.ApertisHipError):
        ops.attention_chunk(q.clone().requires_grad_(), cache(), 0, H, c["kv"], splits=splits, dead_rows=True)


# ------------------------------------------------------------------------------------------------ 4.-8. the model
LAYERS, P = 2, 40
SEED = 5       # every top-2 gap of the stock runs below is above 1e-2 with this seed (asserted at 1e-3 where it matters)


@functools.lru_cache(maxsize=None)
def _model_and_ids():
    """2 layers, hidden 256, 4 x 64 heads, fp32, eval; ids [2, 40].  Initialised on the CPU: the same weights everywhere."""
    import apertis_llm_amd as A
    torch.manual_seed(SEED)
    cfg = A.ApertisConfig(vocab_size=512, hidden_size=256, num_hidden_layers=LAYERS, num_attention_heads=4,
                          intermediate_size=512, attention_type="standard_mha", max_position_embeddings=512)
    model = A.ApertisForCausalLM(cfg).eval()
    ids = torch.randint(4, 512, (2, P))
    dev = torch.device("cuda:0")
    return model.to(dev), ids.to(dev)


def _mask(ids, pads):
    mask = torch.ones_like(ids)
    for b, pad in enumerate(pads):
        mask[b, :pad] = 0
    return mask


def _spy_logits(monkeypatch, model):
    """Record the last-position logits of every forward of `model`."""
    steps = []
    fwd = model.forward

    def spy(*a, **k):
        out = fwd(*a, **k)
        steps.append(out[1][:, -1, :].detach().float().clone())
        return out
    monkeypatch.setattr(model, "forward", spy)
    return steps


def _min_top2_gap(steps):
    top2 = torch.topk(torch.stack(steps, 1), 2, dim=-1).values
    return float((top2[..., 0] - top2[..., 1]).min())


def _forward_both_ways(ops, monkeypatch):
    """ids [2, 40], mask[0, :5] = 0, use_cache, no_grad: (logits, past) with the switch off and on; with it on, one
    causal_attention and one fill per layer, with it off none."""
    model, ids = _model_and_ids()
    mask = _mask(ids, (5, 0))
    fused, fills = _spy(monkeypatch, ops, "causal_attention"), _spy(monkeypatch, ops.attention, "attention_dead_rows")

    def run():
        with torch.no_grad():
            out = model(input_ids=ids, attention_mask=mask, use_cache=True)
        return out[1], out[4]
    ops.ATTN_LEFT_PAD = False
    off = run()
    assert fused == [] and fills == []
    ops.ATTN_LEFT_PAD = True
    on = run()
    assert fused == [(2, P, 256)] * LAYERS and fills == [(2, P, 256)] * LAYERS
    return model, ids, mask, off, on


def test_model_forward_runs_the_kernels_and_matches_the_stock_path(dev, ops, monkeypatch):
    """With the switch on one causal_attention and one fill per layer, and at test_prefill_cache_is_the_stock_cache's bars
    (rtol 1e-4, atol 1e-5):
      - the logits and the returned (k, v) of the rows of VALID tokens are the switch-off (stock) run's on the GPU;
      - the logits and the returned (k, v) of ALL rows, pad rows included, are those of the same weights' stock forward on
        the CPU.  Zeros on the pad rows would miss them: those rows go through out_proj, the FFN and the LM head.
    Why the pad rows are not held to the GPU's switch-off run: the premise that the stock path gives a dead row the
    reference's average holds on the CPU (and for torch's math SDPA kernel) but not on the MI355X, where
    F.scaled_dot_product_attention picks the memory-efficient kernel for an additive mask and that kernel returns exact zeros
    for a row whose mask is finfo.min everywhere.  The reference itself computes softmax(scores + mask) explicitly: the
    average.  So the reference for every row is the CPU run; the GPU stock run's pad rows (printed below: up to 1.14 from
    the switch-on run's at a largest logit of 1.49, the other rows within 1.1e-6) are reported, not asserted."""
    import apertis_llm_amd as A
    model, ids, mask, (logits_off, past_off), (logits_on, past_on) = _forward_both_ways(ops, monkeypatch)
    live = mask.bool()
    rel_error_report("left-padded forward against the GPU stock run, pad rows (reported only)", logits_on[~live],
                     logits_off[~live], check=False)
    rel_error_report("left-padded forward against the GPU stock run, valid rows", logits_on[live], logits_off[live],
                     check=False)
    torch.testing.assert_close(logits_on[live], logits_off[live], rtol=1e-4, atol=1e-5)
    assert len(past_on) == len(past_off) == LAYERS
    for (ka, va), (kb, vb) in zip(past_on, past_off):
        torch.testing.assert_close(ka[live], kb[live], rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(va[live], vb[live], rtol=1e-4, atol=1e-5)
    cpu_model = A.ApertisForCausalLM(model.config).eval()
    cpu_model.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    with torch.no_grad():
        out = cpu_model(input_ids=ids.cpu(), attention_mask=mask.cpu(), use_cache=True)
    rel_error_report("left-padded forward against the CPU stock run, pad rows", logits_on[~live], out[1][~live.cpu()],
                     check=False)
    torch.testing.assert_close(logits_on.cpu(), out[1], rtol=1e-4, atol=1e-5)
    assert len(out[4]) == LAYERS
    for (ka, va), (kb, vb) in zip(past_on, out[4]):
        torch.testing.assert_close(ka.cpu(), kb, rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(va.cpu(), vb, rtol=1e-4, atol=1e-5)


def _generate(model, ids, mask, new, **kw):
    return model.generate(input_ids=ids, attention_mask=mask, max_new_tokens=new, do_sample=False, eos_token_id=-1,
                          pad_token_id=0, **kw)


def test_generate_eager_runs_every_step_on_the_decode_kernels(dev, ops, monkeypatch):
    """Greedy, 10 new tokens.  The switch-off (stock) run's top-2 gap is above 1e-3 in every selecting row of every step - a
    condition on the stock run - so the switch-on run, fp32 at the 1e-4 bar, must select the same tokens; it takes
    layers * (NEW - 1) calls of each decode kernel (append + RoPE, attention) where the stock run takes none."""
    NEW = 10
    model, ids = _model_and_ids()
    mask = _mask(ids, (5, 0))
    dec, app = _spy(monkeypatch, ops, "attention_decode"), _spy(monkeypatch, ops, "kv_append_rope")
    fused = _spy(monkeypatch, ops, "causal_attention")
    ops.ATTN_LEFT_PAD = False
    with monkeypatch.context() as mp:
        steps = _spy_logits(mp, model)
        off = _generate(model, ids, mask, NEW)
    gap = _min_top2_gap(steps)
    print(f"stock left-padded generate: smallest top-2 gap {gap:.3e} over {len(steps)} steps")
    assert len(steps) == NEW and gap > 1e-3 and dec == [] and app == [] and fused == []
    ops.ATTN_LEFT_PAD = True
    on = _generate(model, ids, mask, NEW)
    assert len(dec) == LAYERS * (NEW - 1) and len(app) == LAYERS * (NEW - 1) and len(fused) == LAYERS
    assert torch.equal(on, off)


def test_generate_through_the_graph_tail(dev, ops, monkeypatch):
    """Both switches on, 40 new tokens: one graph tail, the tokens of the eager switch-on run (the same kernels on the same
    bits; the tail's fixed split count is the heuristic's own, 1, at these lengths)."""
    import apertis_llm_amd as A
    NEW = 40
    assert NEW - 1 >= A.model.DECODE_GRAPH_MIN_STEPS
    model, ids = _model_and_ids()
    mask = _mask(ids, (5, 0))
    ops.ATTN_LEFT_PAD = True
    ops.ATTN_DECODE_GRAPH = False
    eager = _generate(model, ids, mask, NEW)
    tails, replays = [], []
    tail, replay = A.model.ApertisForCausalLM._generate_graph_tail, torch.cuda.CUDAGraph.replay

    def tail_spy(self, *a, **k):
        tails.append(1)
        return tail(self, *a, **k)

    def replay_spy(g):
        replays.append(1)
        return replay(g)
    monkeypatch.setattr(A.model.ApertisForCausalLM, "_generate_graph_tail", tail_spy)
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", replay_spy)
    dec, dec_at = _spy(monkeypatch, ops, "attention_decode"), _spy(monkeypatch, ops, "attention_decode_at")
    ops.ATTN_DECODE_GRAPH = True
    got = _generate(model, ids, mask, NEW)
    assert len(tails) == 1 and len(replays) >= (NEW - 1) // 16 * 16 and len(dec) <= 2 * LAYERS and len(dec_at) > 0
    assert torch.equal(got, eager)
    # with the padding switch off the same call stays on the eager stock loop
    del tails[:], replays[:], dec[:], dec_at[:]
    ops.ATTN_LEFT_PAD = False
    _generate(model, ids, mask, NEW)
    assert tails == [] and replays == [] and dec == [] and dec_at == []


def test_generate_from_a_kv_cache_in_pieces_of_eight(dev, ops, monkeypatch):
    """Pads 0 and 11, prefill_chunk = 8: the first piece of sequence 1 is wholly dead, the second has dead rows 0..2.  With
    the switch on the call completes on the chunk kernels (5 pieces x 2 layers, a fill after each) and returns the tokens of
    the plain switch-on generate(): the FFN is dense, so no valid row ever reads a pad row.  (The stock run's top-2 gaps are
    above 1e-3.)  With the switch off the same call raises, as before."""
    NEW = 10
    model, ids = _model_and_ids()
    mask = _mask(ids, (0, 11))
    ops.ATTN_LEFT_PAD = False
    with monkeypatch.context() as mp:
        steps = _spy_logits(mp, model)
        stock = _generate(model, ids, mask, NEW)
    gap = _min_top2_gap(steps)
    print(f"stock left-padded generate (pads 0, 11): smallest top-2 gap {gap:.3e}")
    assert gap > 1e-3
    with pytest.raises(ops.ApertisHipError):
        _generate(model, ids, mask, NEW, past_key_values=model.new_kv_cache(2, P + NEW), prefill_chunk=8)
    ops.ATTN_LEFT_PAD = True
    plain = _generate(model, ids, mask, NEW)
    assert torch.equal(plain, stock)
    chunks = _spy(monkeypatch, ops, "attention_chunk")
    fills = _spy(monkeypatch, ops.attention, "attention_dead_rows")
    dec, app = _spy(monkeypatch, ops, "attention_decode"), _spy(monkeypatch, ops, "kv_append_rope")
    app_chunk = _spy(monkeypatch, ops, "kv_append_rope_chunk")
    cache = model.new_kv_cache(2, P + NEW)
    got = _generate(model, ids, mask, NEW, past_key_values=cache, prefill_chunk=8)
    assert chunks == [(2, 8, 256)] * (LAYERS * P // 8) and fills == chunks and app_chunk == chunks
    assert len(dec) == LAYERS * (NEW - 1) and len(app) == LAYERS * (NEW - 1)
    assert cache.length == P + NEW - 1
    assert torch.equal(got, plain)


@pytest.mark.parametrize("case", ["autograd", "train_mode", "fully_masked"])
def test_stays_on_the_stock_path(dev, ops, monkeypatch, case):
    """Switch on, but autograd enabled, train mode, or a sequence without a valid key: no fused, decode or fill call, and the
    outputs are the switch-off run's bit for bit.  (No generate() for the fully masked sequence: its first new token is a
    valid key, so the token steps qualify again.)"""
    import apertis_llm_amd as A
    model, ids = _model_and_ids()
    mask = _mask(ids, (5, 0))
    if case == "fully_masked":
        mask[1] = 0
    if case == "train_mode":
        # (a model of its own: train() on the shared one would leak into the other tests if this one failed half-way)
        torch.manual_seed(SEED)
        cfg = A.ApertisConfig(vocab_size=512, hidden_size=256, num_hidden_layers=LAYERS, num_attention_heads=4,
                              intermediate_size=512, attention_type="standard_mha", max_position_embeddings=512,
                              hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
        model = A.ApertisForCausalLM(cfg).to(dev).train()
    spies = [_spy(monkeypatch, ops, n) for n in ("causal_attention", "attention_decode", "attention_chunk")]
    spies.append(_spy(monkeypatch, ops.attention, "attention_dead_rows"))

    def run():
        with torch.set_grad_enabled(case == "autograd"):
            out = model(input_ids=ids, attention_mask=mask, use_cache=True)
            res = [out[1].detach(), *(t.detach() for pair in out[4] for t in pair)]
            if case == "train_mode":
                with torch.no_grad():
                    res.append(_generate(model, ids, mask, 4))
        return res
    ops.ATTN_LEFT_PAD = False
    off = run()
    ops.ATTN_LEFT_PAD = True
    on = run()
    assert all(s == [] for s in spies)
    assert len(on) == len(off) and all(torch.equal(a, b) for a, b in zip(on, off))
