"""`config.sliding_window` through a standard_mha model on the GPU, under ops.ATTN_WINDOW: training on ops.window_attention
against the stock branch with its band, packed rows on the document kernels with a clipped layout, generate() with every
token step reading at most W cache rows, left-padded batches, the graph replay declining - and nothing at all with the
switch off.  The tiny model: hidden 128, 2 x 64 heads, 2 layers, vocabulary 64, fp32."""
import functools

import pytest
import torch

from conftest import rel_error_report

pytestmark = pytest.mark.gpu

LAYERS = 2
SEED = 5       # every top-2 gap of the CPU stock-branch runs of the generate() cases below is above 1e-1 with this seed
WINDOW_LAUNCHES = ("apertis_attention_window_fwd", "apertis_attention_window_bwd")


@pytest.fixture
def ops():
    from apertis_llm_amd import ops
    prev = ops.ATTN_WINDOW, ops.ATTN_FUSED, ops.ATTN_LEFT_PAD, ops.ATTN_DECODE_GRAPH
    ops.ATTN_WINDOW = True
    yield ops
    ops.ATTN_WINDOW, ops.ATTN_FUSED, ops.ATTN_LEFT_PAD, ops.ATTN_DECODE_GRAPH = prev


def _model(dev, window, **kw):
    import apertis_llm_amd as A
    base = dict(vocab_size=64, hidden_size=128, num_hidden_layers=LAYERS, num_attention_heads=2, intermediate_size=256,
                attention_type="standard_mha", position_embedding_type="rotary", max_position_embeddings=128,
                hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, sliding_window=window)
    base.update(kw)
    torch.manual_seed(SEED)
    return A.ApertisForCausalLM(A.ApertisConfig(**base)).to(dev)


def _ids(dev, B, L, seed=3):
    return torch.randint(4, 64, (B, L), generator=torch.Generator().manual_seed(seed)).to(dev)


def _timed(ops, names, fn):
    """(what fn returns, the launches of `names` it made, by name)."""
    timer = ops.KernelTimer(names)
    ops.set_kernel_timer(timer)
    try:
        out = fn()
    finally:
        ops.set_kernel_timer(None)
    return out, [r[0] for r in timer.records]


def _spy(monkeypatch, owner, name, record):
    real = getattr(owner, name)

    def spy(*a, **k):
        record(a, k)
        return real(*a, **k)
    monkeypatch.setattr(owner, name, spy)


# ------------------------------------------------------------------------------------------------------------- training
def _grads(model, ids):
    model.zero_grad(set_to_none=True)
    torch.manual_seed(42)
    loss, logits = model(input_ids=ids, labels=ids)[:2]
    loss.backward()
    return float(loss.detach()), logits.detach(), {n: p.grad.detach().float().clone() for n, p in model.named_parameters() if p.grad is not None}


def test_training_matches_the_stock_branch_with_the_band(dev, ops):
    """L 96, W 40, fp32: one window launch pair per layer; logits and every parameter gradient at the model-parity bar of
    tests/test_attention_gpu.py (rel_error_report, rtol 1e-4) against the same model with ops.ATTN_FUSED off, whose stock
    branch applies the band.  The band matters: the W = None model's logits differ."""
    model, ids = _model(dev, 40).train(), _ids(dev, 2, 96)
    (lf, of, gf), names = _timed(ops, WINDOW_LAUNCHES + ("apertis_attention_fwd",), lambda: _grads(model, ids))
    assert sorted(names) == ["apertis_attention_window_bwd"] * LAYERS + ["apertis_attention_window_fwd"] * LAYERS
    ops.ATTN_FUSED = False
    (ls, os_, gs), names = _timed(ops, WINDOW_LAUNCHES + ("apertis_attention_fwd",), lambda: _grads(model, ids))
    assert names == [] and gf.keys() == gs.keys() and len(gs) > 0
    assert abs(lf - ls) <= 1e-5 * abs(ls)
    rel_error_report("window model train logits fp32", of, os_, rtol=1e-4)
    for n in gs:
        rel_error_report(f"window model train grad fp32 {n}", gf[n], gs[n], rtol=1e-4)
    ops.ATTN_FUSED = True
    with torch.no_grad():
        assert not torch.allclose(_model(dev, None).train()(input_ids=ids)[1], of, rtol=1e-3, atol=1e-3)
    # gradient checkpointing with attention dropout: the recompute draws the same seed
    drop = _model(dev, 40, attention_probs_dropout_prob=0.1).train()
    grads = []
    for ckpt in (False, True):
        drop.model.gradient_checkpointing = ckpt
        grads.append(_grads(drop, ids)[2])
    for n in grads[0]:
        torch.testing.assert_close(grads[1][n], grads[0][n], rtol=1e-5, atol=1e-7, msg=n)


def test_one_bf16_autocast_step_has_a_finite_loss(dev, ops):
    model, ids = _model(dev, 40).train(), _ids(dev, 2, 96)

    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = model(input_ids=ids, labels=ids)[0]
        loss.backward()
        return loss
    loss, names = _timed(ops, WINDOW_LAUNCHES, step)
    assert sorted(names) == ["apertis_attention_window_bwd"] * LAYERS + ["apertis_attention_window_fwd"] * LAYERS
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None)


def test_a_row_no_longer_than_the_window_takes_the_causal_call(dev, ops):
    """Key length <= W: ops.causal_attention with today's bits (the W = None model's logits, torch.equal)."""
    ids = _ids(dev, 2, 40)
    with torch.no_grad():
        got, names = _timed(ops, WINDOW_LAUNCHES + ("apertis_attention_fwd",), lambda: _model(dev, 40).eval()(input_ids=ids)[1])
        assert names == ["apertis_attention_fwd"] * LAYERS
        assert torch.equal(got, _model(dev, None).eval()(input_ids=ids)[1])


# ---------------------------------------------------------------------------------------------------------- packed rows
def test_packed_rows_run_the_document_kernels_on_the_clipped_layout(dev, ops, monkeypatch):
    """Three documents (50, 13, 33 tokens), W 24: every document's logits are those of the document run alone under the
    window (rtol 1e-4), ops.document_attention ran once per layer on ops.window_layout's clipped arrays, and no window or
    plain causal launch happened."""
    lens, W = (50, 13, 33), 24
    model, ids = _model(dev, W).eval(), _ids(dev, 1, 96)
    docs = torch.repeat_interleave(torch.arange(3), torch.tensor(lens))[None].to(dev)
    layouts = []
    _spy(monkeypatch, ops, "document_attention", lambda a, k: layouts.append(a[4]))
    with torch.no_grad():
        logits, names = _timed(ops, WINDOW_LAUNCHES + ("apertis_attention_fwd", "apertis_attention_doc_fwd"),
                               lambda: model(input_ids=ids, document_ids=docs)[1])
        assert names == ["apertis_attention_doc_fwd"] * LAYERS and len(layouts) == LAYERS
        want = ops.window_layout(ops.document_layout(docs), W)
        idx = torch.arange(96, device=dev)
        assert torch.equal(want.start[0].long(), torch.maximum(ops.document_layout(docs).start[0].long(), idx - W + 1))
        for lay in layouts:
            assert torch.equal(lay.start, want.start) and torch.equal(lay.end, want.end) and lay.pairs == want.pairs
        at = 0
        for n in lens:
            alone = model(input_ids=ids[:, at:at + n])[1]
            rel_error_report(f"packed windowed logits tokens {at}..{at + n - 1}", logits[0, at:at + n], alone[0], rtol=1e-4)
            at += n
        ops.ATTN_WINDOW = False
        assert not torch.allclose(model(input_ids=ids, document_ids=docs)[1], logits, rtol=1e-3, atol=1e-3)


# ------------------------------------------------------------------------------------------------------------ switch off
def test_switch_off_is_the_model_without_a_window(dev, ops):
    ops.ATTN_WINDOW = False
    ids = _ids(dev, 2, 96)
    with torch.no_grad():
        got, names = _timed(ops, WINDOW_LAUNCHES + ("apertis_attention_fwd",), lambda: _model(dev, 40).eval()(input_ids=ids)[1])
        assert names == ["apertis_attention_fwd"] * LAYERS
        assert torch.equal(got, _model(dev, None).eval()(input_ids=ids)[1])
        toks, names = _timed(ops, WINDOW_LAUNCHES, lambda: _generate(_model(dev, 40).eval(), ids[:, :50], None, 8))
        assert names == [] and torch.equal(toks, _generate(_model(dev, None).eval(), ids[:, :50], None, 8))


# -------------------------------------------------------------------------------------------------------------- generate
P, W, NEW = 50, 40, 24


def _generate(model, ids, mask, new, **kw):
    return model.generate(input_ids=ids, attention_mask=mask, max_new_tokens=new, do_sample=False, eos_token_id=-1,
                          pad_token_id=0, **kw)


def _spy_logits(monkeypatch, model):
    steps = []
    fwd = model.forward

    def spy(*a, **k):
        out = fwd(*a, **k)
        steps.append(out[1][:, -1, :].detach().float().clone())
        return out
    monkeypatch.setattr(model, "forward", spy)
    return steps


def _recompute_loop(model, ids, new):
    """Greedy decoding that runs the full windowed forward over everything so far for every token: (tokens, step logits)."""
    toks, steps = ids, []
    with torch.no_grad():
        for _ in range(new):
            steps.append(model(input_ids=toks)[1][:, -1, :].float())
            toks = torch.cat([toks, steps[-1].argmax(-1, keepdim=True)], dim=1)
    return toks, steps


def _min_top2_gap(steps):
    top2 = torch.topk(torch.stack(steps, 1), 2, dim=-1).values
    return float((top2[..., 0] - top2[..., 1]).min())


@functools.lru_cache(maxsize=None)
def _reference_run():
    """The recompute loop of the windowed model, once for the tests below: (model, ids, tokens, step logits)."""
    dev = torch.device("cuda:0")
    model, ids = _model(dev, W).eval(), _ids(dev, 2, P)
    toks, steps = _recompute_loop(model, ids, NEW)
    return model, ids, toks, tuple(steps)


def test_generate_reads_at_most_the_window_from_the_cache(dev, ops, monkeypatch):
    """Greedy, prompt 50, W 40, 24 new tokens, B 2: the tokens of a loop that recomputes the full windowed forward for every
    token (that loop's top-2 gaps are above 1e-3, a condition on the reference run), the step logits within 1e-4 of its, and
    every apertis_attention_decode launch - layers * (NEW - 1) of them - saw Lk <= W, in fact Lk = W."""
    model, ids, want, ref_steps = _reference_run()
    gap = _min_top2_gap(list(ref_steps))
    print(f"recompute loop under the window: smallest top-2 gap {gap:.3e} over {NEW} steps")
    assert gap > 1e-3
    seen = []
    _spy(monkeypatch, ops.attention, "_launch", lambda a, k: seen.append(a[2][15]) if a[0] == "apertis_attention_decode" else None)
    with monkeypatch.context() as mp:
        steps = _spy_logits(mp, model)
        got = _generate(model, ids, None, NEW)
    assert torch.equal(got, want)
    assert seen == [W] * (LAYERS * (NEW - 1))
    assert len(steps) == NEW
    for s_, (a, b) in enumerate(zip(steps, ref_steps)):
        rel_error_report(f"windowed generate step {s_}", a, b, rtol=1e-4)
    # the window matters for these tokens' logits: the full-attention model's first step differs
    with torch.no_grad():
        full = _model(dev, None).eval()(input_ids=ids)[1][:, -1].float()
    assert not torch.allclose(full, ref_steps[0], rtol=1e-3, atol=1e-3)


def test_generate_left_padded_rows_yield_what_they_yield_alone(dev, ops, monkeypatch):
    """ops.ATTN_LEFT_PAD: row 0 left-padded by 9 next to a full row.  Each row's new tokens are those of the row generated
    alone without its padding (whose top-2 gaps are above 1e-3), and every decode launch saw Lk <= W."""
    ops.ATTN_LEFT_PAD = True
    model, ids, _, _ = _reference_run()
    pad = 9
    mask = torch.ones_like(ids)
    mask[0, :pad] = 0
    seen = []
    _spy(monkeypatch, ops.attention, "_launch", lambda a, k: seen.append(a[2][15]) if a[0] == "apertis_attention_decode" else None)
    got = _generate(model, ids, mask, NEW)
    assert seen and max(seen) <= W
    for b, prompt in enumerate((ids[:1, pad:], ids[1:])):
        with monkeypatch.context() as mp:
            steps = _spy_logits(mp, model)
            alone = _generate(model, prompt, None, NEW)
        assert _min_top2_gap(steps) > 1e-3
        assert torch.equal(got[b, P:], alone[0, prompt.shape[1]:]), b


def test_the_graph_replay_declines_past_the_window(dev, ops, monkeypatch):
    """ops.ATTN_DECODE_GRAPH, prompt 10 and 40 new tokens (39 steps left after the first: enough for a graph tail).  W 40 <
    10 + 40: no graph tail, the eager loop's decode launches, the tokens of the run with the graph switch off.  W 64: the
    band never matters, and the tail replays as it does without a window."""
    import apertis_llm_amd as A
    new = 40
    model, ids, _, _ = _reference_run()
    ids = ids[:, :10]
    want = _generate(model, ids, None, new)
    ops.ATTN_DECODE_GRAPH = True
    tails = []
    _spy(monkeypatch, A.model.ApertisForCausalLM, "_generate_graph_tail", lambda a, k: tails.append(1))
    got, names = _timed(ops, ("apertis_attention_decode", "apertis_attention_decode_at"), lambda: _generate(model, ids, None, new))
    assert tails == [] and names == ["apertis_attention_decode"] * (LAYERS * (new - 1))
    assert torch.equal(got, want)
    wide = _model(dev, 64).eval()
    replayed = _generate(wide, ids, None, new)
    assert len(tails) == 1
    ops.ATTN_DECODE_GRAPH = False
    assert torch.equal(replayed, _generate(wide, ids, None, new))


def test_a_multi_token_cache_step_declines_the_chunk_kernels_past_the_window(dev, ops):
    """generate(past_key_values=cache): a piece that would reach past W rows raises with the existing message (the chunk
    kernels have no window predicate); one that stays inside W runs on them."""
    model, ids, _, _ = _reference_run()
    with pytest.raises(ops.ApertisHipError, match="did not run on the KV-cache kernels"):
        _generate(model, ids, None, 4, past_key_values=model.new_kv_cache(2, P + 4), prefill_chunk=16)
    inside = _generate(model, ids[:, :20], None, 4, past_key_values=model.new_kv_cache(2, 24), prefill_chunk=8)
    assert torch.equal(inside, _generate(model, ids[:, :20], None, 4))
