"""KV-cache slots with a length per row (ops.ATTN_SLOTS): the two slot ops against the single-row calls they stand for, the
step helpers, and ApertisForCausalLM.generate_many on a standard_mha model - every prompt gets the tokens generate() gives it
alone, cut after its first eos, while the rows of one decode batch are refilled as they finish.

Model recipe of tests/test_generate_many_gpu.py with a head dim the decode kernels take: 2 layers, hidden 128, 2 heads (D 64),
intermediate 256, vocab 64, 128 rotary positions, fp32, oracle.seeded's weights with a gain.  Seven prompts of 1, 2, 5, 9, 17,
33 and 40 tokens in 3 slots, 30 new tokens.  The alone runs come from batch-1 generate() on the eager loop; before any token is
compared the smallest top-2 logit gap over all their steps must exceed 1e-3 of the largest logit (a condition on the inputs:
the slots run the projections at another batch size, which is not the alone step's arithmetic to the last bit).
"""
import functools

import pytest
import torch

from conftest import rel_error_report

pytestmark = pytest.mark.gpu

NAN = float("nan")
LENS, NEW, VOCAB, SLOTS = [1, 2, 5, 9, 17, 33, 40], 30, 64, 3
NO_EOS = -1
# Gain and prompt seed: searched on the CPU (the stock branch computes the same model) so that the precondition holds with
# room, plain and under the repetition penalty (there: gaps 3.2e-3 plain, 1.4e-3 with the penalty; most seeds leave a gap
# below 1e-3 somewhere in the 210 steps of the seven alone runs); the GPU run's own assert is what counts, and it prints the gap
GAIN = 16.0
PROMPT_SEED = 24


@pytest.fixture
def ops():
    from apertis_llm_amd import ops
    return ops


@pytest.fixture
def slots_on(ops, monkeypatch):
    monkeypatch.setattr(ops, "ATTN_SLOTS", True)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ------------------------------------------------------------------------------------------------------------- the two ops
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_slot_append_carries_the_alone_calls_bits(dev, ops, dtype):
    import apertis_llm_amd as A
    S, cap, W, heads, lens = 3, 40, 128, 2, [0, 7, 39]
    rope = A.model.RotaryEmbedding(W, 64, 10000.0).to(dev)
    cos, sin = rope.cos_cached, rope.sin_cached
    assert tuple(cos.shape) == (64, W // 2)
    gen = torch.Generator(device=dev).manual_seed(5)
    q, k, v = (torch.randn(S, W, device=dev, generator=gen).to(dtype) for _ in range(3))
    cache = ops.KVCache.empty(1, S, cap, W, dtype, dev)
    cache.k[0].fill_(NAN)
    cache.v[0].fill_(NAN)
    cache.slots_begin(heads)
    cache.dev_lens.copy_(torch.tensor(lens))
    qo = ops.kv_append_rope_slots(q, k, v, cache, 0, cos, sin)
    assert tuple(qo.shape) == (S, W) and qo.dtype == dtype
    assert int(cache.dev_err) == 0 and cache.dev_lens.tolist() == lens          # (the op moves no length)
    for b, t in enumerate(lens):
        alone = ops.KVCache([torch.full((1, cap, W), NAN, device=dev, dtype=dtype)],
                            [torch.full((1, cap, W), NAN, device=dev, dtype=dtype)], length=t)
        qa = ops.kv_append_rope(q[b:b + 1], k[b:b + 1], v[b:b + 1], alone, 0, None, cos, sin)
        assert torch.equal(_bits(qo[b]), _bits(qa[0])), b
        assert torch.equal(_bits(cache.k[0][b, t]), _bits(alone.k[0][0, t])), b
        assert torch.equal(_bits(cache.v[0][b, t]), _bits(alone.v[0][0, t])), b
        assert not bool(torch.isnan(cache.k[0][b, t]).any() | torch.isnan(cache.v[0][b, t]).any())
        others = torch.ones(cap, dtype=torch.bool, device=dev)
        others[t] = False
        assert bool(torch.isnan(cache.k[0][b, others]).all() & torch.isnan(cache.v[0][b, others]).all()), b


@functools.lru_cache(maxsize=None)
def _attention_case(D):
    """S = 4 slots of 300 rows holding 1, 37, 129 and 300 keys (dev_lens 0, 36, 128, 299: the step's own key included), every
    row beyond a slot's keys NaN; the validity as slot_install and slots_step_begin leave it; the fp64 softmax over each
    row's own keys, computed once."""
    from apertis_llm_amd import ops
    dev = torch.device("cuda:0")
    S, H, cap, lens = 4, 2, 300, [0, 36, 128, 299]
    W = H * D
    gen = torch.Generator(device=dev).manual_seed(11 + D)
    q = torch.randn(S, W, device=dev, generator=gen)
    cache = ops.KVCache.empty(1, S, cap, W, torch.float32, dev)
    cache.k[0].copy_(torch.randn(S, cap, W, device=dev, generator=gen))
    cache.v[0].copy_(torch.randn(S, cap, W, device=dev, generator=gen))
    cache.slots_begin(H)
    ref = torch.empty(S, W, dtype=torch.float64, device=dev)
    for b, n in enumerate(lens):
        cache.k[0][b, n + 1:] = NAN
        cache.v[0][b, n + 1:] = NAN
        cache.dev_lens[b] = n
        cache.dev_valid[b].copy_(torch.arange(cap, device=dev) < n)
        kh = cache.k[0][b, :n + 1].double().view(n + 1, H, D)
        vh = cache.v[0][b, :n + 1].double().view(n + 1, H, D)
        s = torch.einsum("hd,jhd->hj", q[b].double().view(H, D), kh) / float(torch.tensor(float(D)).sqrt())
        ref[b] = torch.einsum("hj,jhd->hd", torch.softmax(s, dim=-1), vh).reshape(W)
    cache.slots_step_begin()
    assert cache.dev_len.tolist() == [299]
    want = torch.arange(cap, device=dev)[None, :] <= torch.tensor(lens, device=dev)[:, None]
    assert torch.equal(cache.dev_valid != 0, want)
    return q, cache, lens, ref


@pytest.mark.parametrize("D", [64, 128])
def test_slot_attention_at_one_split_is_the_alone_call(dev, ops, D):
    q, cache, lens, ref = _attention_case(D)
    got = ops.attention_decode_slots(q, cache, 0, 2, splits=1)
    assert not bool(torch.isnan(got).any())
    for b, n in enumerate(lens):
        alone = ops.KVCache([cache.k[0][b:b + 1]], [cache.v[0][b:b + 1]], length=n + 1)
        one = ops.attention_decode(q[b:b + 1], alone, 0, 2, splits=1)
        assert torch.equal(_bits(got[b]), _bits(one[0])), (b, n)
    rel_error_report(f"attention_decode_slots fp32 D{D} splits1", got, ref, rtol=1e-4)


@pytest.mark.parametrize("splits", [2, 5])
@pytest.mark.parametrize("D", [64, 128])
def test_slot_attention_forced_splits_read_no_row_past_a_slots_end(dev, ops, D, splits):
    q, cache, lens, ref = _attention_case(D)
    got = ops.attention_decode_slots(q, cache, 0, 2, splits=splits)
    assert not bool(torch.isnan(got).any())
    rel_error_report(f"attention_decode_slots fp32 D{D} splits{splits}", got, ref, rtol=1e-4)


def test_step_helpers_validity_maximum_and_clamp(dev, ops):
    S, cap, W = 3, 8, 128
    cache = ops.KVCache.empty(1, S, cap, W, torch.float32, dev)
    cache.slots_begin(2)
    assert cache.dev_valid.dtype == torch.int64 and not bool(cache.dev_valid.any()) and cache.dev_lens.tolist() == [0] * S
    cache.dev_lens.copy_(torch.tensor([0, 5, cap - 1]))
    alive = torch.tensor([1, 0, 1], device=dev)
    want = torch.zeros(S, cap, dtype=torch.bool)
    cache.slots_step_begin()
    want[0, 0] = want[1, 5] = want[2, cap - 1] = True
    assert torch.equal((cache.dev_valid != 0).cpu(), want) and cache.dev_len.tolist() == [cap - 1]
    cache.slots_step_end(alive)
    assert cache.dev_lens.tolist() == [1, 5, cap - 1]                 # (row 1 is not alive; row 2 is clamped)
    cache.slots_step_begin()
    want[0, 1] = True
    assert torch.equal((cache.dev_valid != 0).cpu(), want) and cache.dev_len.tolist() == [cap - 1]
    cache.slots_step_end(alive)
    assert cache.dev_lens.tolist() == [2, 5, cap - 1] and int(cache.dev_err) == 0


def test_slot_mode_checks(dev, ops):
    S, cap, W, layers = 2, 8, 128, 2
    cache = ops.KVCache.empty(layers, S, cap, W, torch.float32, dev)
    cache.step_state_begin(2)
    with pytest.raises(ops.ApertisHipError, match="step state is active"):
        cache.slots_begin(2)
    cache.step_state_end(0)
    with pytest.raises(ops.ApertisHipError, match="not in slot mode"):
        cache.slot_free(0)
    cache.slots_begin(2)
    with pytest.raises(ops.ApertisHipError, match="slot mode"):
        cache.step_state_begin(2)
    past = lambda L, dtype=torch.float32, n=layers: tuple(                                  # noqa: E731
        (torch.ones(1, L, W, device=dev, dtype=dtype), torch.ones(1, L, W, device=dev, dtype=dtype)) for _ in range(n))
    with pytest.raises(ops.ApertisHipError, match="do not fit"):
        cache.slot_install(0, past(cap + 1))
    with pytest.raises(ops.ApertisHipError, match="slot_install"):
        cache.slot_install(0, past(3, torch.bfloat16))
    with pytest.raises(ops.ApertisHipError, match="layers"):
        cache.slot_install(0, past(3, n=1))
    with pytest.raises(ops.ApertisHipError, match="outside"):
        cache.slot_install(S, past(3))
    assert not bool(cache.dev_valid.any()) and cache.dev_lens.tolist() == [0, 0]          # (a refused install wrote nothing)
    cache.slot_install(1, past(cap))
    cache.slot_install(0, past(3))
    assert cache.dev_lens.tolist() == [3, cap] and cache.dev_valid.sum(1).tolist() == [3, cap]
    assert bool((cache.k[1][0, :3] == 1).all())
    cache.slot_free(1)
    assert cache.dev_lens.tolist() == [3, 0] and cache.dev_valid.sum(1).tolist() == [3, 0]
    cache.slots_end()
    assert not cache.slot_active
    with pytest.raises(ops.ApertisHipError, match="not in slot mode"):
        ops.attention_decode_slots(torch.zeros(S, W, device=dev), cache, 0, 2)


# ------------------------------------------------------------------------------------------------------------ model level
@functools.lru_cache(maxsize=None)
def _model(kind="mha"):
    import apertis_llm_amd as A
    from oracle import seeded
    kw = dict(hidden_size=128, num_attention_heads=2, intermediate_size=256)
    kw.update({"mha": {}, "window": dict(sliding_window=8), "d16": dict(hidden_size=64, num_attention_heads=4),
               "absolute": dict(position_embedding_type="absolute")}[kind])
    cfg = A.ApertisConfig(vocab_size=VOCAB, num_hidden_layers=2, max_position_embeddings=128, attention_type="standard_mha",
                          **kw)
    model = A.ApertisForCausalLM(cfg).eval()
    model.load_state_dict(seeded.fill_state_dict(model.state_dict(), gain=GAIN))
    return model.to(torch.device("cuda:0"))


@functools.lru_cache(maxsize=None)
def _prompts():
    g = torch.Generator().manual_seed(PROMPT_SEED)
    return [torch.randint(4, VOCAB, (n,), generator=g).to("cuda:0") for n in LENS]


def _spy_forward(model, calls):
    """Every model.forward call as its keyword arguments (generate() and generate_many() pass keywords only)."""
    fwd = model.forward

    def spy(*a, **k):
        assert not a
        calls.append(k)
        return fwd(**k)
    model.forward = spy


@functools.lru_cache(maxsize=None)
def _alone(penalty=1.0):
    """Every prompt alone through batch-1 generate() on the eager loop, NEW tokens, no eos: (new tokens per prompt, the
    smallest top-2 gap over all steps as a share of the largest logit - of the logits the token is selected from: each
    divided by the penalty once per earlier occurrence of its token)."""
    import apertis_llm_amd as A
    model = _model()
    toks, gap = [], float("inf")
    graph, A.model.DECODE_GRAPH = A.model.DECODE_GRAPH, False
    fwd = model.forward
    try:
        for p in _prompts():
            steps, seen = [], torch.zeros(VOCAB, device=p.device)

            def spy(*a, **k):
                out = fwd(*a, **k)
                seen.add_(torch.bincount(k["input_ids"][0], minlength=VOCAB))
                steps.append(out[1].detach().float()[0, -1] / penalty ** seen)
                return out
            model.forward = spy
            out = model.generate(input_ids=p[None], max_new_tokens=NEW, do_sample=False, repetition_penalty=penalty,
                                 eos_token_id=NO_EOS, pad_token_id=0)
            assert tuple(out.shape) == (1, len(p) + NEW) and len(steps) == NEW
            toks.append(out[0, len(p):].clone())
            last = torch.stack(steps)
            top2 = torch.topk(last, 2, dim=-1).values
            gap = min(gap, float(((top2[:, 0] - top2[:, 1]) / last.abs().amax(-1)).min()))
    finally:
        del model.forward
        A.model.DECODE_GRAPH = graph
    return toks, gap


def _cut(t, eos, budget=NEW):
    t = t[:budget]
    hit = (t == eos).nonzero()
    return t[:int(hit[0]) + 1] if len(hit) else t


def _want(eos=NO_EOS, budgets=None, penalty=1.0):
    toks, gap = _alone(penalty)
    print(f"alone runs (standard_mha, penalty {penalty}): smallest top-2 gap {gap:.3e} of the largest logit")
    assert gap > 1e-3, "a near-tie in an alone run: pick other weights (GAIN) or prompts (PROMPT_SEED)"
    budgets = [NEW] * len(LENS) if budgets is None else budgets
    return [torch.cat((p, _cut(t, eos, m))) for p, t, m in zip(_prompts(), toks, budgets)]


def _same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == torch.int64 and g.dim() == 1 and g.is_cuda
        assert torch.equal(g, w), (i, g.tolist(), w.tolist())


def _early_eos(toks):
    """A token some prompt emits at its step 5 - so that its row ends there at the latest, while others are mid-run - such
    that at least two other prompts never emit it."""
    for t in toks:
        eos = int(t[5])
        if sum(1 for o in toks if not bool((o == eos).any())) >= 2:
            return eos
    raise AssertionError("no step-5 token leaves two rows running to the end: pick other prompts")


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_greedy_every_prompt_gets_its_alone_run(dev, slots_on, monkeypatch, graph):
    import apertis_llm_amd as A
    assert NEW - 1 >= A.model.DECODE_GRAPH_MIN_STEPS
    monkeypatch.setattr(A.model, "DECODE_GRAPH", graph)
    got, stats = _model().generate_many(_prompts(), max_new_tokens=NEW, slots=SLOTS, eos_token_id=NO_EOS, pad_token_id=0,
                                        return_stats=True)
    _same(got, _want())
    assert set(stats) == {"steps", "replays", "graphs", "prefills", "live_slot_steps", "slot_steps", "fallbacks"}
    assert stats["prefills"] == len(LENS) and stats["fallbacks"] == [] and stats["graphs"] == int(graph)
    assert stats["live_slot_steps"] == len(LENS) * (NEW - 1) and stats["slot_steps"] == SLOTS * stats["steps"]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_an_eos_frees_rows_that_are_refilled(dev, slots_on, monkeypatch, graph):
    import apertis_llm_amd as A
    model = _model()
    toks, _ = _alone()
    eos = _early_eos(toks)
    want = _want(eos)
    assert min(len(w) - n for w, n in zip(want, LENS)) <= 6 and sum(len(w) - n == NEW for w, n in zip(want, LENS)) >= 2
    monkeypatch.setattr(A.model, "DECODE_GRAPH", graph)
    replays, real = [], torch.cuda.CUDAGraph.replay
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", lambda self: (replays.append(id(self)), real(self))[1])
    got, stats = model.generate_many(_prompts(), max_new_tokens=NEW, slots=SLOTS, eos_token_id=eos, pad_token_id=0,
                                     return_stats=True)
    _same(got, want)
    assert stats["prefills"] == len(LENS) and stats["fallbacks"] == []
    if graph:
        assert stats["graphs"] == 1 and len(set(replays)) == 1          # one graph captured for the whole call
        assert stats["replays"] == stats["steps"] == len(replays) > 0
    else:
        assert stats["graphs"] == 0 and stats["replays"] == 0 and replays == [] and stats["steps"] > 0


def test_repetition_penalty(dev, slots_on):
    model, prompts = _model(), _prompts()
    want = _want(penalty=1.3)
    assert any(not torch.equal(w, g) for w, g in zip(want, _want())), "the penalty changes no token: it shows nothing"
    _same(model.generate_many(prompts, max_new_tokens=NEW, slots=SLOTS, repetition_penalty=1.3, eos_token_id=NO_EOS,
                              pad_token_id=0), want)


def test_per_prompt_budgets_with_one_and_zero(dev, slots_on):
    budgets = [1, 0, 7, 30, 30, 16, 3]
    want = _want(budgets=budgets)
    got, stats = _model().generate_many(_prompts(), max_new_tokens=budgets, slots=SLOTS, eos_token_id=NO_EOS, pad_token_id=0,
                                        return_stats=True)
    assert [len(g) for g in got] == [n + m for n, m in zip(LENS, budgets)]
    _same(got, want)
    assert stats["prefills"] == sum(1 for m in budgets if m > 0) and stats["fallbacks"] == []
    assert stats["live_slot_steps"] == sum(m - 1 for m in budgets if m > 0)


def test_one_slot(dev, slots_on):
    got, stats = _model().generate_many(_prompts(), max_new_tokens=NEW, slots=1, eos_token_id=NO_EOS, pad_token_id=0,
                                        return_stats=True)
    _same(got, _want())
    assert stats["prefills"] == len(LENS) and stats["live_slot_steps"] == stats["slot_steps"] == len(LENS) * (NEW - 1)


def test_a_sampled_run_repeats_under_its_seed(dev, slots_on):
    model, prompts = _model(), _prompts()
    runs = []
    for _ in range(2):
        torch.manual_seed(3)
        runs.append(model.generate_many(prompts, max_new_tokens=NEW, slots=SLOTS, do_sample=True, temperature=0.7, top_k=50,
                                        top_p=0.9, eos_token_id=NO_EOS, pad_token_id=0))
    _same(runs[0], runs[1])
    for g, p in zip(runs[0], prompts):
        assert len(g) == len(p) + NEW and torch.equal(g[:len(p)], p)
        assert 0 <= int(g.min()) and int(g.max()) < VOCAB


def test_install_is_the_alone_prefill_and_a_step_is_one_forward(dev, ops, slots_on):
    model, prompts = _model(), _prompts()
    calls = []
    _spy_forward(model, calls)
    try:
        got, stats = model.generate_many(prompts, max_new_tokens=NEW, slots=SLOTS, eos_token_id=NO_EOS, pad_token_id=0,
                                         return_stats=True)
    finally:
        del model.forward
    prefills = [k for k in calls if k.get("past_key_values") is None]
    assert len(prefills) == len(prompts)
    for k, p in zip(prefills, prompts):                       # one batch-1 prefill per prompt, in arrival order
        assert torch.equal(k["input_ids"], p[None]) and k["use_cache"] is True
        assert k.get("attention_mask") is None and k.get("position_ids") is None and k.get("pixel_values") is None
    steps = [k for k in calls if k.get("past_key_values") is not None]
    caches = {id(k["past_key_values"]) for k in steps}
    assert steps and len(caches) == 1                         # one slot cache for the whole call
    for k in steps:
        cache = k["past_key_values"]
        assert isinstance(cache, ops.KVCache) and tuple(cache.k[0].shape)[0] == SLOTS and k["use_cache"] is True
        assert tuple(k["input_ids"].shape) == (SLOTS, 1) and k.get("attention_mask") is None
    # (one forward per eager step, plus the three of the capture: two warm-up runs and the captured one)
    assert len(steps) == stats["steps"] - stats["replays"] + 3 * stats["graphs"]
    _same(got, _want())


@pytest.mark.parametrize("case", ["window", "head_dim", "absolute", "rotary_table", "decode_fused_off"])
def test_refusals_under_the_switch_launch_no_forward(dev, ops, slots_on, monkeypatch, case):
    model = _model({"window": "window", "head_dim": "d16", "absolute": "absolute"}.get(case, "mha"))
    prompts = list(_prompts()[:3]) + [_prompts()[-1]]
    kw = dict(max_new_tokens=4, slots=2, eos_token_id=NO_EOS, pad_token_id=0)
    if case == "window":
        monkeypatch.setattr(ops, "ATTN_WINDOW", True)
        match = "sliding_window"
    elif case == "head_dim":
        match = "head dim 16"
    elif case == "absolute":
        match = "absolute position"
    elif case == "rotary_table":
        kw["max_new_tokens"] = [4, 4, 4, 90]                 # 40 + 90 - 1 = 129 > 128 positions
        match = r"prompt 3 of 40 tokens with 90 new ones runs past the rotary table \(128 positions\)"
    else:
        monkeypatch.setattr(ops, "ATTN_DECODE_FUSED", False)
        match = "ATTN_DECODE_FUSED"
    calls = []
    _spy_forward(model, calls)
    try:
        with pytest.raises(ValueError, match=match):
            model.generate_many(prompts, **kw)
        if case == "rotary_table":                           # the bound itself is taken: 40 + 89 - 1 = 128
            kw["max_new_tokens"] = [1, 1, 1, 89]
            assert calls == []
            got = model.generate_many(prompts, **kw)
            assert len(got[3]) == 40 + 89 and calls
            calls.clear()
    finally:
        del model.forward
    assert calls == []


def test_switch_off_keeps_todays_refusal(dev, ops, monkeypatch):
    monkeypatch.setattr(ops, "ATTN_SLOTS", False)
    model, calls = _model(), []
    _spy_forward(model, calls)
    try:
        with pytest.raises(ValueError, match=r"generate\(past_key_values=.*left-padded"):
            model.generate_many(list(_prompts()[:3]), max_new_tokens=4, slots=2)
    finally:
        del model.forward
    assert calls == []
