"""generate() of a windowed standard_mha model past its window on the KV-cache kernels, under ops.ATTN_WINDOW and
ops.ATTN_WINDOW_CACHE: the graph replay of the token step (apertis_attention_decode_window_at), chunked prefill into a cache the
caller keeps and a second chat turn on it (apertis_attention_chunk_window) - and, with the second switch off, today's declines.
The tiny model of tests/test_window_model_gpu.py: hidden 128, 2 x 64 heads, 2 layers, vocabulary 64, fp32, seed 5; ids from seed 3;
W 40.  Every greedy comparison is conditioned on its reference run's smallest top-2 logit gap, printed and held above 1e-3."""
import pytest
import torch

from conftest import rel_error_report

pytestmark = pytest.mark.gpu

LAYERS, SEED, W = 2, 5, 40
DECODE = ("apertis_attention_decode", "apertis_attention_decode_at", "apertis_attention_decode_window_at")
CHUNK = ("apertis_attention_chunk", "apertis_attention_chunk_window")
NEW_NAMES = ("apertis_attention_decode_window_at", "apertis_attention_chunk_window")


@pytest.fixture
def ops():
    from apertis_llm_amd import ops
    prev = ops.ATTN_WINDOW, ops.ATTN_WINDOW_CACHE, ops.ATTN_FUSED, ops.ATTN_LEFT_PAD, ops.ATTN_DECODE_GRAPH
    ops.ATTN_WINDOW = ops.ATTN_WINDOW_CACHE = True
    yield ops
    ops.ATTN_WINDOW, ops.ATTN_WINDOW_CACHE, ops.ATTN_FUSED, ops.ATTN_LEFT_PAD, ops.ATTN_DECODE_GRAPH = prev


def _model(dev, window):
    import apertis_llm_amd as A
    cfg = dict(vocab_size=64, hidden_size=128, num_hidden_layers=LAYERS, num_attention_heads=2, intermediate_size=256,
               attention_type="standard_mha", position_embedding_type="rotary", max_position_embeddings=128,
               hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, sliding_window=window)
    torch.manual_seed(SEED)
    return A.ApertisForCausalLM(A.ApertisConfig(**cfg)).to(dev).eval()


def _ids(dev, B, L, seed=3):
    return torch.randint(4, 64, (B, L), generator=torch.Generator().manual_seed(seed)).to(dev)


def _generate(model, ids, mask, new, **kw):
    return model.generate(input_ids=ids, attention_mask=mask, max_new_tokens=new, do_sample=False, eos_token_id=-1,
                          pad_token_id=0, **kw)


def _record_launches(monkeypatch, ops, names):
    """The names of the library calls ops.attention makes from here on, in order (no events: a capture is in flight)."""
    seen, real = [], ops.attention._launch

    def spy(name, *a, **k):
        if name in names:
            seen.append(name)
        return real(name, *a, **k)
    monkeypatch.setattr(ops.attention, "_launch", spy)
    return seen


def _spy_logits(monkeypatch, model):
    steps, fwd = [], model.forward

    def spy(*a, **k):
        out = fwd(*a, **k)
        steps.append(out[1][:, -1, :].detach().float().clone())
        return out
    monkeypatch.setattr(model, "forward", spy)
    return steps


def _min_top2_gap(steps):
    top2 = torch.topk(torch.stack(steps, 1), 2, dim=-1).values
    return float((top2[..., 0] - top2[..., 1]).min())


def _reference(monkeypatch, what, model, ids, mask, new):
    """A greedy reference run and the condition on it: (tokens, step logits); the smallest top-2 gap printed, above 1e-3."""
    with monkeypatch.context() as mp:
        steps = _spy_logits(mp, model)
        toks = _generate(model, ids, mask, new)
    gap = _min_top2_gap(steps)
    print(f"{what}: smallest top-2 gap {gap:.3e} over {len(steps)} steps")
    assert len(steps) == new and gap > 1e-3, (what, gap)
    return toks, steps


def _recompute_loop(model, ids, new):
    """Greedy decoding that runs the full windowed forward over everything so far for every token: (tokens, step logits)."""
    toks, steps = ids, []
    with torch.no_grad():
        for _ in range(new):
            steps.append(model(input_ids=toks)[1][:, -1, :].float())
            toks = torch.cat([toks, steps[-1].argmax(-1, keepdim=True)], dim=1)
    return toks, steps


def _spy_tails(monkeypatch):
    import apertis_llm_amd as A
    tails, real = [], A.model.ApertisForCausalLM._generate_graph_tail

    def spy(self, *a, **k):
        tails.append(1)
        return real(self, *a, **k)
    monkeypatch.setattr(A.model.ApertisForCausalLM, "_generate_graph_tail", spy)
    return tails


# --------------------------------------------------------------------------------------------------------- graph replay
def test_the_graph_replay_runs_past_the_window(dev, ops, monkeypatch):
    """ops.ATTN_DECODE_GRAPH, prompt 10 and 40 new tokens, W 40 < 50: exactly one graph tail, its attention launches are
    apertis_attention_decode_window_at, no by-value decode launch once it has started, and the tokens are those of the eager
    loop with the graph switch off."""
    model, ids = _model(dev, W), _ids(dev, 2, 50)[:, :10]
    want, _ = _reference(monkeypatch, "eager loop, prompt 10 + 40 new", model, ids, None, 40)
    ops.ATTN_DECODE_GRAPH = True
    tails, seen = _spy_tails(monkeypatch), _record_launches(monkeypatch, ops, DECODE)
    got = _generate(model, ids, None, 40)
    assert len(tails) == 1
    assert "apertis_attention_decode_window_at" in seen and "apertis_attention_decode_at" not in seen
    first = seen.index("apertis_attention_decode_window_at")
    assert set(seen[first:]) == {"apertis_attention_decode_window_at"} and set(seen[:first]) <= {"apertis_attention_decode"}
    assert len(seen[first:]) % LAYERS == 0
    assert torch.equal(got, want)


@pytest.mark.parametrize("new", [24, 30])
def test_left_padded_rows_under_the_graph_switch_yield_what_they_yield_alone(dev, ops, monkeypatch, new):
    """ops.ATTN_LEFT_PAD and ops.ATTN_DECODE_GRAPH: row 0 left-padded by 9 next to a full row, prompt 50 (the cases of
    test_generate_left_padded_rows_yield_what_they_yield_alone).  Each row's new tokens are those of the row generated alone
    without its padding on the eager loop.  24 new tokens leave 23 steps after the first, one short of a graph tail; 30 new
    ones replay 29 steps, the padded validity columns riding in the cache's device state."""
    ops.ATTN_LEFT_PAD = True
    model, ids = _model(dev, W), _ids(dev, 2, 50)
    pad = 9
    mask = torch.ones_like(ids)
    mask[0, :pad] = 0
    alone = [_reference(monkeypatch, f"row {b} alone, {new} new", model, prompt, None, new)[0]
             for b, prompt in enumerate((ids[:1, pad:], ids[1:]))]
    ops.ATTN_DECODE_GRAPH = True
    tails, seen = _spy_tails(monkeypatch), _record_launches(monkeypatch, ops, DECODE)
    got = _generate(model, ids, mask, new)
    assert len(tails) == (1 if new - 1 >= 24 else 0)
    assert ("apertis_attention_decode_window_at" in seen) == bool(tails) and "apertis_attention_decode_at" not in seen
    for b, prompt in enumerate((ids[:1, pad:], ids[1:])):
        assert torch.equal(got[b, 50:], alone[b][0, prompt.shape[1]:]), b


# ------------------------------------------------------------------------------------------------------ chunked prefill
def test_chunked_prefill_into_a_cache_runs_past_the_window(dev, ops, monkeypatch):
    """generate(ids[:, :50], 8 new, past_key_values=new_kv_cache(2, 58), prefill_chunk=16): pieces [0, 16), [16, 32) stay inside
    W 40 (the plain chunk launch), [32, 48) and [48, 50) reach past it (apertis_attention_chunk_window); the tokens are those
    of generate without a cache, the step logits within rtol 1e-4 of the loop that recomputes the full windowed forward."""
    model, ids = _model(dev, W), _ids(dev, 2, 50)
    want, _ = _reference(monkeypatch, "no cache, prompt 50 + 8 new", model, ids, None, 8)
    ref_toks, ref_steps = _recompute_loop(model, ids, 8)
    gap = _min_top2_gap(ref_steps)
    print(f"recompute loop, prompt 50 + 8 new: smallest top-2 gap {gap:.3e}")
    assert gap > 1e-3 and torch.equal(ref_toks, want)
    seen = _record_launches(monkeypatch, ops, CHUNK)
    cache = model.new_kv_cache(2, 58)
    with monkeypatch.context() as mp:
        steps = _spy_logits(mp, model)
        got = _generate(model, ids, None, 8, past_key_values=cache, prefill_chunk=16)
    assert seen == ["apertis_attention_chunk"] * (2 * LAYERS) + ["apertis_attention_chunk_window"] * (2 * LAYERS)
    assert torch.equal(got, want) and cache.length == 57
    assert len(steps) == 3 + 8                                      # three pieces whose logits select nothing, then the steps
    for i, (a, b) in enumerate(zip(steps[3:], ref_steps)):
        rel_error_report(f"chunked windowed prefill step {i}", a, b, rtol=1e-4)


def test_a_second_turn_on_the_same_cache_crosses_the_window(dev, ops, monkeypatch):
    """Turn 1: prompt ids[:, :30], 6 new, into a multi_token cache.  Turn 2: the output plus ids[:, 30:50] - 56 tokens, 35 of
    them cached, the 21 new ones one windowed chunk - and 6 new, on the same cache: the tokens of the 56-token prompt from
    scratch.  The window matters there: the unwindowed model's last-position logits on that prompt differ."""
    model, ids = _model(dev, W), _ids(dev, 2, 50)
    want1, _ = _reference(monkeypatch, "no cache, prompt 30 + 6 new", model, ids[:, :30], None, 6)
    cache = model.new_kv_cache(2, 64)
    seen = _record_launches(monkeypatch, ops, CHUNK)
    out1 = _generate(model, ids[:, :30], None, 6, past_key_values=cache)
    assert torch.equal(out1, want1) and cache.length == 35 and seen == ["apertis_attention_chunk"] * LAYERS
    turn2 = torch.cat([out1, ids[:, 30:50]], dim=1)
    assert turn2.shape[1] == 56
    want2, steps2 = _reference(monkeypatch, "no cache, the 56-token second turn + 6 new", model, turn2, None, 6)
    del seen[:]
    out2 = _generate(model, turn2, None, 6, past_key_values=cache)
    assert seen == ["apertis_attention_chunk_window"] * LAYERS
    assert torch.equal(out2, want2) and cache.length == 61
    with torch.no_grad():
        full = _model(dev, None)(input_ids=turn2)[1][:, -1].float()
    diff = float((full - steps2[0]).abs().max())
    print(f"windowed against unwindowed last-position logits on the 56-token prompt: max difference {diff:.3e}")
    assert diff > 1e-3


# ------------------------------------------------------------------------------------------------------------ switch off
def test_with_the_cache_switch_off_nothing_new_is_launched(dev, ops, monkeypatch):
    """ops.ATTN_WINDOW alone: the same calls make no launch of the two new entry points - the graph replay declines past the
    window, the chunked call raises as it does today, a second turn that crosses the window raises too."""
    ops.ATTN_WINDOW_CACHE = False
    model, ids = _model(dev, W), _ids(dev, 2, 50)
    ops.ATTN_DECODE_GRAPH = True
    tails, seen = _spy_tails(monkeypatch), _record_launches(monkeypatch, ops, DECODE + CHUNK)
    _generate(model, ids[:, :10], None, 40)
    assert tails == [] and seen == ["apertis_attention_decode"] * (LAYERS * 39)
    with pytest.raises(ops.ApertisHipError, match="did not run on the KV-cache kernels"):
        _generate(model, ids, None, 8, past_key_values=model.new_kv_cache(2, 58), prefill_chunk=16)
    cache = model.new_kv_cache(2, 64)
    out1 = _generate(model, ids[:, :30], None, 6, past_key_values=cache)
    with pytest.raises(ops.ApertisHipError, match="did not run on the KV-cache kernels"):
        _generate(model, torch.cat([out1, ids[:, 30:50]], dim=1), None, 6, past_key_values=cache)
    assert not set(seen) & set(NEW_NAMES)
